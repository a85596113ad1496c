"""The fused one-kernel allgatherv / reduce_scatterv / alltoallv of tl/cdna4
(UCC_TL_CDNA4_FUSED_COLLS=1): tests/fused_vcolls_worker.py runs seeded
exact-integer cases and compares every destination bit for bit. Four
torchrun launches in total (ranks share cuda:0), shared by all tests of this
file; the worker's docstring lists the modes.

Selection is read from the UCC_COLL_TRACE lines: every rank writes down for
every request of the three types whether it must trace cdna4/fused, and the
multiset of trace lines must match. Which kernel served a post is read from
the debug lines, one per post: k_fused_coll, k_fused_coll_graph or
k_fused_a2av, and for an alltoallv whose vote failed the fallback line."""

import collections
import glob
import os
import re
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_zc_fused_gpu import _torchrun  # noqa: E402

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "fused_vcolls_worker.py")

HOST_KERNEL = "host-sequenced kernel (k_fused_coll)"
GRAPH_KERNEL = "graph kernel (k_fused_coll_graph)"
A2AV_KERNEL = "cdna4 fused alltoallv: host-sequenced kernel (k_fused_a2av)"
A2AV_FALLBACK = re.compile(
    r"cdna4 fused alltoallv: a pair exceeds the (\d+)-byte cell, "
    r"served by (\w+)")
THREE = ("allgatherv", "reduce_scatterv", "alltoallv")

ENV = {
    "UCC_TL_CDNA4_FUSED_COLLS": "1",
    "UCC_TL_CDNA4_FUSED_COLLS_MAX": "524288",
    "UCC_COLL_TRACE": "1",
    "UCC_LOG_LEVEL": "debug",
}
ENV_OFF = {"UCC_TL_CDNA4_FUSED_COLLS": "0", "UCC_COLL_TRACE": "1",
           "UCC_LOG_LEVEL": "debug"}

TRACE = re.compile(r"coll (\w+) mem \w+ size (\d+) -> (\w+)/(\w+) ")
REQ = re.compile(r"^FV_REQ (\w+) (\d+) ([FO])$", re.M)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for mode, nproc, env in (("all", 2, ENV), ("three", 3, ENV),
                             ("trig", 2, ENV), ("off", 2, ENV_OFF)):
        d = tmp_path_factory.mktemp(mode)
        proc = _torchrun([WORKER, str(d), mode], timeout=240, env_extra=env,
                         nproc=nproc)
        proc.notes = "".join(open(f).read() for f in
                             sorted(glob.glob(os.path.join(str(d), "*.txt"))))
        sys.stdout.write(f"--- {mode}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-1500:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln and " INFO " not in ln)[-3000:])
        out[mode] = proc
    return out


def _traced(proc):
    """(coll, msgsize, traced cdna4/fused) of every trace line of the three
    types."""
    got = collections.Counter()
    for coll, size, tl, alg in TRACE.findall(proc.stderr):
        if coll in THREE:
            got[(coll, int(size), (tl, alg) == ("cdna4", "fused"))] += 1
    return got


def _announced(proc):
    return collections.Counter(
        (coll, int(size), f == "F")
        for coll, size, f in REQ.findall(proc.notes))


def _ok(proc, nranks):
    assert proc.returncode == 0
    assert proc.stdout.count("FV_OK") == nranks


def _sum(proc, key):
    return sum(int(x) for x in
               re.findall(r"^FV_%s (\d+)$" % key, proc.notes, re.M))


@pytest.mark.parametrize("mode,nranks,cell", [("all", 2, 262128),
                                              ("three", 3, 174752)])
def test_results_and_selection(runs, mode, nranks, cell):
    """Every case is bitwise right, gaps and bands intact (asserted in the
    worker). Every alltoallv and every in-bound allgatherv and
    reduce_scatterv traced cdna4/fused, every request over the bound
    something else. Every alltoallv post ran k_fused_a2av; every post with
    one oversized pair fell back on every rank, also on a rank whose own
    row and column fit (rank 2 of the 3-rank launch)."""
    proc = runs[mode]
    _ok(proc, nranks)
    want = _announced(proc)
    assert want == _traced(proc)
    for coll in THREE:
        assert any(f for (c, _, f) in want if c == coll), coll
    for coll in ("allgatherv", "reduce_scatterv"):
        assert any(not f for (c, _, f) in want if c == coll), coll
    assert proc.stderr.count(HOST_KERNEL) == _sum(proc, "COLL") > 0
    assert GRAPH_KERNEL not in proc.stderr
    assert proc.stderr.count(A2AV_KERNEL) == _sum(proc, "A2AV") > 0
    # the cell is the same on every rank and post; the requests with a
    # pair of one cell (more than 128 KiB) ran on more than one block
    grids = re.findall(r"\(k_fused_a2av\), (\d+) blocks, cell (\d+) bytes",
                       proc.stderr)
    assert {c for _, c in grids} == {str(cell)}
    assert min(int(b) for b, _ in grids) == 1
    assert max(int(b) for b, _ in grids) > 1
    fell = A2AV_FALLBACK.findall(proc.stderr)
    # one line per rank and post: the same number on every rank
    assert len(fell) == _sum(proc, "FALLBACK") > 0
    assert len(fell) % nranks == 0
    assert set(fell) == {(str(cell), "gated_pipeline")}


def test_triggered_and_graph_replay(runs):
    proc = runs["trig"]
    _ok(proc, 2)
    want = _announced(proc)
    assert want == _traced(proc)
    assert all(f for (_, _, f) in want)
    # 2 allgatherv, 2 reduce_scatterv and the alltoallv, on 2 ranks
    assert sum(want.values()) == 2 * 5
    # three eager posts and one capture per request, none host-sequenced;
    # the alltoallv's triggered post launched nothing of its own
    assert proc.stderr.count(GRAPH_KERNEL) == _sum(proc, "GRAPH") == 2 * 4 * 4
    assert HOST_KERNEL not in proc.stderr
    assert "k_fused_a2av" not in proc.stderr
    assert not A2AV_FALLBACK.search(proc.stderr)


def test_knob_unset_keeps_selection(runs):
    proc = runs["off"]
    _ok(proc, 2)
    got = _traced(proc)
    assert got == _announced(proc)
    assert sum(got.values()) == 2 * len(THREE)
    algs = {coll: alg for coll, _, _, alg in TRACE.findall(proc.stderr)
            if coll in THREE}
    assert algs == dict.fromkeys(THREE, "gated_pipeline")
    # the score map printed at team creation has no fused entry for them
    assert not re.search(r"^(%s):\w+:\S*@cdna4/fused" % "|".join(THREE),
                         proc.stderr, re.M)
    assert "alltoallv:cuda:" in proc.stderr
    assert "cdna4 fused" not in proc.stderr
