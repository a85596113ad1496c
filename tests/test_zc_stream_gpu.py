"""The streamed (non-temporal) data phase of the fused zero-copy allreduce.

Probe: k_zc_data with stream=1 (core().ec_zc_data) at n = 2, blocks = 2,
threads = 256, every kind and every count of tests/test_zc_data_gpu.py.
Those counts are the loop boundaries of depth U = 4 — scalar tail only,
one batch, one batch + 1 pack, two batches, three batches, five batches +
511 packs + 3 elements — the smallest shapes at which a wrong load or store
form can show. The result must equal that file's CPU model and the
stream=0 run bit for bit, guards intact; the same for zc_write = 0, in
place and at sl_b = 768. stream=1 at a rank count without a streamed
instantiation raises.

Real path: tests/zc_fused_worker.py, unchanged, in the environment of
tests/test_zc_fused_gpu.py, once with UCC_TL_CDNA4_ZC_STREAM=0 and once
with =1 (2 ranks): every dst bitwise equal between the runs, the policy
line logged once per one-kernel line with =1 and never with =0. A third
run at 4 ranks (depth 2: no streamed instantiation) with =1 completes and
logs the plain fallback."""

import glob
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_zc_data_gpu import (BLOCKS, GUARD, KINDS, THREADS,  # noqa: E402
                              check, counts_for, expected, fill_value,
                              inputs, raw)
from test_zc_fused_gpu import (CASES, ENV, ONE_KERNEL, WORKER,  # noqa: E402
                               _torchrun)
from ucc_amd import core, dtypes  # noqa: E402

pytestmark = pytest.mark.gpu

STREAMING = "zc data phase: streaming"
NO_INSTANCE = "zc data phase: plain (no streamed instantiation)"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert "UCC_EC_REDUCE_DEPTH" not in os.environ, (
        "UCC_EC_REDUCE_DEPTH overrides the depths these counts are built on")
    torch.cuda.set_device(0)


def run_probe(x, ucc_dt, op, stream, zc_write=1, sl_b=0, inplace=False):
    """run_probe of tests/test_zc_data_gpu.py with the stream keyword."""
    n, count = x.shape
    tdt = x.dtype
    es = x.element_size()
    first = sl_b // es
    m = count - first
    srcs = [x[r].clone().cuda() for r in range(n)]
    dsts = [torch.full((m + GUARD,), fill_value(tdt), dtype=tdt,
                       device="cuda") for _ in range(n if zc_write else 1)]
    dptr = [d.data_ptr() for d in dsts]
    if inplace:
        dptr[0] = srcs[0].data_ptr() + sl_b
    alpha = 1.0 / n if op == dtypes.OP_AVG else 1.0
    torch.cuda.synchronize()
    core().ec_zc_data([s.data_ptr() for s in srcs], dptr, sl_b, count * es,
                      ucc_dt, op, zc_write, alpha, blocks=BLOCKS,
                      threads=THREADS, reps=1, stream=stream)
    torch.cuda.synchronize()
    if inplace:
        dsts[0] = torch.cat([srcs[0][first:],
                             torch.full((GUARD,), fill_value(tdt),
                                        dtype=tdt, device="cuda")])
    return dsts


def both(x, ucc_dt, op, exp, what, **kw):
    """stream=1 against the CPU model (guards included) and against
    stream=0, whole buffers."""
    s1 = run_probe(x, ucc_dt, op, 1, **kw)
    s0 = run_probe(x, ucc_dt, op, 0, **kw)
    check(s1, exp, x.dtype, what + " stream=1")
    assert len(s0) == len(s1)
    for j, (a, b) in enumerate(zip(s0, s1)):
        assert np.array_equal(raw(a), raw(b)), f"{what} dst{j}: 0 vs 1"


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_counts(kind):
    tdt, ucc_dt, op = KINDS[kind]
    for ci, count in enumerate(counts_for(2, tdt)):
        x = inputs(2, count, tdt, 7000 + ci)
        both(x, ucc_dt, op, expected(x, op), f"{kind} count={count}")


def test_single_dst():
    """zc_write = 0: the nt stores go to my_out."""
    tdt, ucc_dt, op = KINDS["bf16_sum"]
    for ci, count in enumerate(counts_for(2, tdt)):
        x = inputs(2, count, tdt, 7100 + ci)
        both(x, ucc_dt, op, expected(x, op), f"zc_write=0 count={count}",
             zc_write=0)


def test_inplace():
    tdt, ucc_dt, op = KINDS["bf16_sum"]
    for ci, count in enumerate(counts_for(2, tdt)):
        x = inputs(2, count, tdt, 7200 + ci)
        both(x, ucc_dt, op, expected(x, op), f"inplace count={count}",
             inplace=True)


def test_slice_offset():
    tdt, ucc_dt, op = KINDS["bf16_avg"]
    sl_b = 768
    first = sl_b // 2
    for ci, c in enumerate(counts_for(2, tdt)):
        x = inputs(2, first + c, tdt, 7300 + ci)
        both(x, ucc_dt, op, expected(x, op)[first:], f"sl_b=768 count={c}",
             sl_b=sl_b)


def test_no_streamed_instantiation_raises():
    """n = 3 runs at depth 2, which has no streamed instantiation."""
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(RuntimeError, match="Not supported"):
        core().ec_zc_data([p, p, p], [p, p, p], 0, 256, dtypes.FLOAT32,
                          dtypes.OP_SUM, 1, 1.0, blocks=2, stream=1)
    # and the same call is served plain
    core().ec_zc_data([p, p, p], [p + 1024, p + 2048, p + 3072], 0, 256,
                      dtypes.FLOAT32, dtypes.OP_SUM, 1, 1.0, blocks=2,
                      stream=0)
    torch.cuda.synchronize()


# ------------------------------------------------------------- real path
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    out = {}
    for tag, knob, nproc, extra in (("plain", "0", 2, []),
                                    ("stream", "1", 2, []),
                                    ("stream4", "1", 4, ["repost"])):
        d = tmp_path_factory.mktemp(tag)
        proc = _torchrun([WORKER, str(d)] + extra, timeout=240,
                         env_extra={**ENV, "UCC_TL_CDNA4_ZC_STREAM": knob},
                         nproc=nproc)
        sys.stdout.write(f"--- {tag}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-2000:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln)[-3000:])
        out[tag] = (proc, str(d))
    return out


def test_real_path_bitwise_equal(runs):
    (p0, d0), (p1, d1) = runs["plain"], runs["stream"]
    assert p0.returncode == 0 and p1.returncode == 0
    assert p0.stdout.count("ZCF_OK") == 2
    assert p1.stdout.count("ZCF_OK") == 2
    names = sorted(os.path.basename(p)
                   for p in glob.glob(os.path.join(d0, "*.npy")))
    assert names == sorted(f"{c}_rank{r}.npy" for c in CASES
                           for r in range(2))
    for n in names:
        a = np.load(os.path.join(d0, n))
        b = np.load(os.path.join(d1, n))
        assert a.shape == b.shape, n
        assert np.array_equal(a, b), n


def test_real_path_policy_logged(runs):
    p0, p1 = runs["plain"][0], runs["stream"][0]
    assert p1.stderr.count(ONE_KERNEL) == 2 * 9
    assert p1.stderr.count(STREAMING) == p1.stderr.count(ONE_KERNEL)
    assert p0.stderr.count(ONE_KERNEL) == 2 * 9
    assert STREAMING not in p0.stderr


def test_four_ranks_fall_back_to_plain(runs):
    proc, _ = runs["stream4"]
    assert proc.returncode == 0
    assert proc.stdout.count("ZCF_OK") == 4
    assert proc.stderr.count(ONE_KERNEL) == 4
    assert proc.stderr.count(NO_INSTANCE) == 4
    assert STREAMING not in proc.stderr
