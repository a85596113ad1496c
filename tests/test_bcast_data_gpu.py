"""The data phase of the gated bcast (bcast_phase), run alone and in-process
through the probe kernel k_bcast_data (core().ec_bcast_data) and compared
byte for byte with the source slice.

Grid: blocks=2, threads=256, so one grid stride is 512 packs of 16 bytes
and one batch of the 4-deep loop is 2,048 packs = 32 KiB. Slice lengths sit
on the loop boundaries: 15 B (byte tail only); one batch; one batch + one
pack (batched loop, then the per-pack loop); three batches; five batches +
511 packs + 3 B (batched loop, per-pack loop, byte tail).

Destinations: one (the zc_write = 0 form, my_out) and 2, 3, 5, 8 (the push
form) with no entry skipped and with one skipped at the first, the middle
and the last position. Every destination carries 64 sentinel bytes on both
sides of the slice, which must keep their fill, and a skipped destination
must keep all of it."""

import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ucc_amd import core  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS, THREADS, DEPTH = 2, 256, 4
BATCH = DEPTH * BLOCKS * THREADS * 16  # bytes
GUARD = 64
FILL = 0xA5

LENGTHS = [15, BATCH, BATCH + 16, 3 * BATCH, 5 * BATCH + 511 * 16 + 3]

CASES = [(1, None)]
for _n in (2, 3, 5, 8):
    for _s in dict.fromkeys((None, 0, _n // 2, _n - 1)):
        CASES.append((_n, _s))


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)


def run_probe(ndst, skip, length, sl_b=0, seed=0):
    g = torch.Generator().manual_seed(seed)
    src = torch.randint(0, 256, (sl_b + length + GUARD,), generator=g,
                        dtype=torch.uint8)
    dsrc = src.cuda()
    dsts = [torch.full((GUARD + length + GUARD,), FILL, dtype=torch.uint8,
                       device="cuda") for _ in range(ndst)]
    ptrs = [0 if j == skip else d.data_ptr() + GUARD
            for j, d in enumerate(dsts)]
    torch.cuda.synchronize()
    ms = core().ec_bcast_data(dsrc.data_ptr(), ptrs, sl_b, sl_b + length,
                              blocks=BLOCKS, threads=THREADS, reps=1)
    torch.cuda.synchronize()
    assert ms >= 0.0
    want = src[sl_b:sl_b + length].numpy()
    for j, d in enumerate(dsts):
        got = d.cpu().numpy()
        what = f"ndst={ndst} skip={skip} len={length} dst{j}"
        if j == skip:
            assert (got == FILL).all(), what + " (skipped)"
            continue
        assert np.array_equal(got[GUARD:GUARD + length], want), what
        assert (got[:GUARD] == FILL).all(), what + " front band"
        assert (got[GUARD + length:] == FILL).all(), what + " back band"
    # the source is only read
    assert np.array_equal(dsrc.cpu().numpy(), src.numpy())


@pytest.mark.parametrize("ndst,skip", CASES,
                         ids=[f"n{n}-skip{s}" for n, s in CASES])
def test_lengths(ndst, skip):
    for li, length in enumerate(LENGTHS):
        print(f"ndst={ndst} skip={skip} len={length}")
        run_probe(ndst, skip, length, seed=100 * ndst + li)


@pytest.mark.parametrize("ndst,skip", [(1, None), (3, 1)])
def test_slice_offset(ndst, skip):
    """sl_b != 0, a multiple of 256 bytes as the host produces: the source
    is a base, destinations are already offset by the slice start."""
    run_probe(ndst, skip, LENGTHS[-1], sl_b=3 * 256, seed=7)


def test_bad_arguments():
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    c = core()
    with pytest.raises(RuntimeError):  # no destination
        c.ec_bcast_data(p, [], 0, 256, blocks=2)
    with pytest.raises(RuntimeError):  # the only destination is skipped
        c.ec_bcast_data(p, [0], 0, 256, blocks=2)
    with pytest.raises(RuntimeError):  # sl_e < sl_b
        c.ec_bcast_data(p, [p + 1024], 512, 256, blocks=2)
    with pytest.raises(RuntimeError):  # threads the kernel is not built for
        c.ec_bcast_data(p, [p + 1024], 0, 256, blocks=2, threads=512)
    for src, dsts, sl_b in ((p + 8, [p + 1024], 0), (p, [p + 1028], 0),
                            (p, [p + 1024], 8), (p, [0, p + 1032], 0)):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            c.ec_bcast_data(src, dsts, sl_b, 256, blocks=2)
