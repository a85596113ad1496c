"""Host checks of tests/copy_cases.py: that the gather_copy case set reaches
every loop of k_gather_copy / d_copy_bytes_part (a condition on the inputs,
so it is proved here, without a GPU, with the grid taken from the library's
own gather_copy_blocks), and that the models and layouts keep the buffer
discipline the GPU tests rely on."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_cases as cc  # noqa: E402
from ucc_amd import core  # noqa: E402

CASES = cc.gather_cases()
BY_NAME = {c.name: c for c in CASES}


def grid_of(case):
    return core().ec_gather_copy_blocks(case.lens)


def test_grid_binding_needs_no_device_and_checks_n():
    c = core()
    assert c.ec_gather_copy_blocks([0]) == 1
    assert c.ec_gather_copy_blocks([16 * 256]) == 1
    assert c.ec_gather_copy_blocks([16 * 256 + 16]) == 2
    assert c.ec_gather_copy_blocks([1 << 40]) == 2048
    for bad in ([], [1] * (cc.MAX_SRCS + 1)):
        with pytest.raises(RuntimeError):
            c.ec_gather_copy_blocks(bad)
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(0, [0, 0], [0], [0, 0])
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(0, [], [], [])
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(0, [0] * 9, [0] * 9, [0] * 9)


def test_case_set_reaches_every_path_class():
    reached = {k: [] for k in cc.PATH_CLASSES}
    for case in CASES:
        for k in cc.path_classes(case, grid_of(case)):
            reached[k].append(case.name)
    missing = [k for k, v in reached.items() if not v]
    assert not missing, f"no case reaches: {missing}"


def test_named_cases_take_the_paths_they_are_named_for():
    """the shapes of the required cases, worked from the library's grid"""
    def pm(name):
        c = BY_NAME[name]
        g = grid_of(c)
        return g, cc.path_model(c.n, c.lens, c.aligns, g)

    g, p = pm("batched_uniform")
    assert g == 73 and p[0]["branch"] == "part16"
    assert (p[0]["batched_first"], p[0]["batched_last"], p[0]["single"],
            p[0]["tail"]) == (2, 2, 100, 9)
    g, p = pm("batched_divergent")
    assert g == 64 and (p[0]["batched_first"], p[0]["batched_last"]) == \
        (2, 1)
    g, p = pm("looped_long")
    assert g == 5 and all(r["branch"] == "looped" for r in p)
    assert p[0]["batched_first"] >= 1 and p[0]["single"] > 0
    g, p = pm("looped_divergent")
    assert g < 8 and (p[0]["batched_first"], p[0]["batched_last"]) == (1, 0)
    g, p = pm("looped_tiny")
    assert g == 1 and max(BY_NAME["looped_tiny"].lens) <= 200
    g, p = pm("mixed")
    assert [r["branch"] for r in p] == ["part16", "partbyte", "part16",
                                        "part16"]
    g, p = pm("descending_looped")
    assert g < 4
    g, p = pm("descending_partitioned")
    assert g >= 4
    for name in ("descending_looped", "descending_partitioned"):
        offs = BY_NAME[name].offs
        assert offs == sorted(offs, reverse=True)
        gaps = {offs[i] - offs[i + 1] - BY_NAME[name].lens[i + 1]
                for i in range(3)}
        assert len(gaps) == 3


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_layout_discipline(case):
    """alignments as asked, guards everywhere, sources and fill disjoint
    in value, and the model writes the moves and nothing else"""
    regions = sorted(zip(case.offs, case.lens))
    assert regions[0][0] >= cc.GUARD
    for (o0, l0), (o1, _) in zip(regions, regions[1:]):
        assert o1 - (o0 + l0) >= cc.GUARD
    assert case.dst_size - (regions[-1][0] + regions[-1][1]) >= cc.GUARD
    for i in range(case.n):
        assert case.offs[i] % 16 == case.aligns[i][0]
        assert case.src_offs[i] % 16 == case.aligns[i][1]
        assert case.src_offs[i] + case.lens[i] <= case.src_size
    arena, init = case.arena(), case.dst_initial()
    assert arena.max(initial=0) < 128 and init.min() >= 128
    exp = case.expected()
    written = np.zeros(case.dst_size, dtype=bool)
    for src, off, ln in case.moves():
        assert not written[off:off + ln].any()
        written[off:off + ln] = True
        assert np.array_equal(exp[off:off + ln], src)
    assert np.array_equal(exp[~written], init[~written])
    assert int(written.sum()) == sum(case.lens)


def test_streams_are_not_periodic():
    a = cc.src_bytes(5, 70000)
    for period in (1, 2, 4, 16, 64, 256, 1024, 4096, 16 * 256, 65536):
        assert not np.array_equal(a[period:], a[:-period])


def test_v_layouts():
    for n in (2, 3, 4, 8):
        for es in (1, 2, 8):
            g = 2048 // es
            counts = cc.v_counts(n, g, 0)
            assert 0 in counts and max(counts) > 2 * g
            assert any(0 < c < g for c in cc.v_counts(n, g, 2) + counts)
            displs, total = cc.v_displs(counts, es)
            regs = sorted(zip(displs, counts))
            assert regs[0][0] * es >= cc.GUARD
            for (d0, c0), (d1, _) in zip(regs, regs[1:]):
                assert (d1 - d0 - c0) * es >= cc.GUARD
            assert (total - regs[-1][0] - regs[-1][1]) * es >= cc.GUARD
            if n >= 3:
                assert displs != sorted(displs)
                assert displs != sorted(displs, reverse=True)


def test_coll_models_on_a_tiny_example():
    """3 ranks, 1-byte elements, worked by hand"""
    n, es = 3, 1
    contrib = [np.full(4, 10 * (r + 1), dtype=np.uint8) for r in range(n)]
    dst = np.full(20, 200, dtype=np.uint8)
    mv = cc.coll_moves("allgatherv", n, 1, counts=[1, 2, 0],
                       displs=[5, 1, 9])
    got = cc.coll_expected(dst, 2, es, mv, contrib)
    want = dst.copy()
    want[7] = 10
    want[3:5] = 20
    assert np.array_equal(got, want)
    mv = cc.coll_moves("allgatherv", n, 1, counts=[1, 2, 0],
                       displs=[5, 1, 9], inplace=True)
    assert mv == [(0, 0, 5, 1), (2, 0, 9, 0)]
    sc = [[1, 2, 1], [0, 1, 3], [2, 2, 0]]
    sd = [[0, 1, 3], [0, 0, 1], [0, 2, 0]]
    rd = [[0, 9, 4], [6, 0, 2], [1, 5, 0]]
    mv = cc.coll_moves("alltoallv", n, 2, scounts=sc, sdispls=sd,
                       rdispls=rd)
    assert mv == [(0, 3, 1, 1), (1, 1, 5, 3), (2, 0, 0, 0)]
    assert cc.coll_moves("gather", n, 0, root=1, counts=[2] * 3,
                         displs=[0, 2, 4]) == []
    assert cc.coll_moves("gather", n, 1, root=1, counts=[2] * 3,
                         displs=[0, 2, 4], inplace=True) == \
        [(0, 0, 0, 2), (2, 0, 4, 2)]
    assert cc.coll_moves("scatterv", n, 2, root=0, counts=[1, 0, 3],
                         displs=[7, 0, 2]) == [(0, 2, 0, 3)]
    assert cc.coll_moves("scatter", n, 0, root=0, counts=[2] * 3,
                         displs=[0, 2, 4], inplace=True) == []
    assert cc.coll_moves("bcast", n, 2, root=2, counts=[4]) == []
    assert cc.coll_moves("bcast", n, 0, root=2, counts=[4]) == \
        [(2, 0, 0, 4)]
