"""k_gather_copy (and d_copy_bytes_part under it) byte for byte: every case
of tests/copy_cases.py in one launch through the ec_gather_copy hook,
compared over the whole destination allocation, guards included, with the
numpy model "these bytes of these sources land at these offsets and nothing
else changes". No tolerance anywhere.

That the case set reaches every loop of the kernel is proved on the CPU, in
tests/test_copy_cases.py; here each launch also reports the grid it used,
which must be the one that proof was made with."""

import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import copy_cases as cc  # noqa: E402
from ucc_amd import core  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cc.gather_cases()


def _dev(a):
    t = torch.from_numpy(a).cuda()
    assert t.data_ptr() % 16 == 0
    return t


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_gather_copy(case):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = core()
    arena_h = case.arena()
    arena, dst = _dev(arena_h), _dev(case.dst_initial())
    srcs = [arena.data_ptr() + so for so in case.src_offs]
    for i in range(case.n):
        assert (dst.data_ptr() + case.offs[i]) % 16 == case.aligns[i][0]
        assert srcs[i] % 16 == case.aligns[i][1]
        # in bounds, before anything is launched
        assert case.offs[i] + case.lens[i] <= case.dst_size - cc.GUARD
        assert case.src_offs[i] + case.lens[i] <= case.src_size
    torch.cuda.synchronize()
    blocks = c.ec_gather_copy(dst.data_ptr(), srcs, case.offs, case.lens)
    assert blocks == c.ec_gather_copy_blocks(case.lens)
    got = dst.cpu().numpy()
    at = cc.first_diff(got, case.expected())
    assert at is None, (
        f"{case.name}: first differing byte at {at} of {case.dst_size}, "
        f"got {got[at]}, regions {list(zip(case.offs, case.lens))}, "
        f"{blocks} blocks")
    assert np.array_equal(arena.cpu().numpy(), arena_h), "source changed"


def test_gather_copy_rejects_bad_n():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = core()
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(p, [], [], [])
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(p, [p] * 9, [0] * 9, [0] * 9)
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(p, [p, p], [0], [1, 1])
    with pytest.raises(RuntimeError):
        c.ec_gather_copy(p, [0], [0], [16])
    assert bool((buf == 0).all())
