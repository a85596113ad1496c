"""The data phase of the fused zero-copy allreduce (zc_data_phase), run
alone and in-process through the probe kernel k_zc_data (core().ec_zc_data)
and compared BITWISE with a CPU model of the kernel's order: convert every
rank's element to the accumulate type (fp32 for bf16/fp16/fp32, int32 for
int32), reduce ranks 0..n-1 in that order, scale once by alpha, round once
to the element type.

Grid: blocks=2, threads=256, so one grid stride is 512 packs of 16 bytes
and one batch of the pipelined loop is U * 512 packs. The depth follows
the rank count as in the real launcher: n=2 -> U=4, n=3,4 -> U=2,
n=5,8 -> U=1 (no pipelined loop). "Peers" are separate local tensors.

Counts, in packs, for the U of each case: less than one pack (scalar tail
only); one batch; one batch + 1 pack; two batches (the "two left"
epilogue); three batches (steady loop once, "one left" epilogue); five
batches + 511 packs + 3 elements (steady loop twice, per-pack loop, scalar
tail).

Inputs: bf16 and fp16 draw from k/2, k in [-8, 8], so every sum of up to 8
ranks (|k| <= 64, 7 significant bits) is exact in fp32 and in bf16/fp16,
and AVG is exact where alpha is a power of two; AVG therefore runs at
n = 2, 4, 8 (U = 4, 2, 1) and the expected values do not depend on any
rounding helper. AVG at n = 3 and 5 is NOT covered (1/3 and 1/5 are not
exact), and zc_write = 0 and the in-place case run bf16 SUM only. fp32
SUM uses seeded normals: sequential IEEE fp32 adds on the CPU are the
kernel's adds. int32 MAX uses seeded integers.

The depth table below is the launcher's default selection. With
UCC_EC_REDUCE_DEPTH set the launcher would run another depth and the
counts would no longer sit on its loop boundaries, so the module fails
at set-up if that variable is in the environment.

Every dst carries 64 guard elements behind the slice, which must keep
their fill value.

One more case runs seeded bf16 normals through a real 2-process allreduce
on the three-kernel path (UCC_TL_CDNA4_ZC_FUSED=0: k_staged_reduce) and
requires the probe to reproduce both ranks' slices of that dst bit for
bit."""

import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_zc_fused_gpu import REPO, _torchrun  # noqa: E402
from ucc_amd import core, dtypes  # noqa: E402

pytestmark = pytest.mark.gpu

BLOCKS, THREADS = 2, 256
STRIDE = BLOCKS * THREADS  # packs per grid stride
GUARD = 64

DEPTH = {2: 4, 3: 2, 4: 2, 5: 1, 8: 1}

# name -> (torch dtype, ucc dtype, op)
KINDS = {
    "bf16_sum": (torch.bfloat16, dtypes.BFLOAT16, dtypes.OP_SUM),
    "bf16_avg": (torch.bfloat16, dtypes.BFLOAT16, dtypes.OP_AVG),
    "fp32_sum": (torch.float32, dtypes.FLOAT32, dtypes.OP_SUM),
    "int32_max": (torch.int32, dtypes.INT32, dtypes.OP_MAX),
    "fp16_sum": (torch.float16, dtypes.FLOAT16, dtypes.OP_SUM),
}

CASES = [(n, k) for n in sorted(DEPTH) for k in KINDS
         if k != "bf16_avg" or n in (2, 4, 8)]


def counts_for(n, tdt):
    """Element counts at which the loop structure of depth U changes."""
    vec = 16 // torch.empty(0, dtype=tdt).element_size()
    batch = DEPTH[n] * STRIDE  # packs
    return [vec - 1, batch * vec, (batch + 1) * vec, 2 * batch * vec,
            3 * batch * vec, (5 * batch + 511) * vec + 3]


def inputs(n, count, tdt, seed):
    g = torch.Generator().manual_seed(seed)
    if tdt == torch.int32:
        return torch.randint(-1_000_000, 1_000_000, (n, count), generator=g,
                             dtype=torch.int32)
    if tdt == torch.float32:
        return torch.randn(n, count, generator=g)
    k = torch.randint(-8, 9, (n, count), generator=g)
    return (k.float() / 2).to(tdt)


def expected(x, op):
    """The kernel's order on the CPU."""
    n = x.shape[0]
    if x.dtype == torch.int32:
        assert op == dtypes.OP_MAX
        acc = x[0].clone()
        for r in range(1, n):
            acc = torch.maximum(acc, x[r])
        return acc
    acc = x[0].float()
    for r in range(1, n):
        acc = acc + x[r].float()
    if op == dtypes.OP_AVG:
        acc = acc * torch.tensor(1.0 / n, dtype=torch.float32)
    return acc.to(x.dtype)


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


def fill_value(tdt):
    return 77 if tdt == torch.int32 else 7.5


def run_probe(x, ucc_dt, op, zc_write=1, sl_b=0, inplace=False):
    """One k_zc_data launch over elements [sl_b/es, count) of x[r]; returns
    the dst tensors (slice + guard each)."""
    n, count = x.shape
    tdt = x.dtype
    es = x.element_size()
    first = sl_b // es
    m = count - first
    srcs = [x[r].clone().cuda() for r in range(n)]
    ndst = n if zc_write else 1
    dsts = [torch.full((m + GUARD,), fill_value(tdt), dtype=tdt,
                       device="cuda") for _ in range(ndst)]
    dptr = [d.data_ptr() for d in dsts]
    if inplace:
        dptr[0] = srcs[0].data_ptr() + sl_b
    alpha = 1.0 / n if op == dtypes.OP_AVG else 1.0
    torch.cuda.synchronize()
    ms = core().ec_zc_data([s.data_ptr() for s in srcs], dptr, sl_b,
                           count * es, ucc_dt, op, zc_write, alpha,
                           blocks=BLOCKS, threads=THREADS, reps=1)
    torch.cuda.synchronize()
    assert ms >= 0.0
    if inplace:
        dsts[0] = torch.cat([srcs[0][first:],
                             torch.full((GUARD,), fill_value(tdt),
                                        dtype=tdt, device="cuda")])
    return dsts


def check(dsts, exp, tdt, what):
    m = exp.numel()
    guard = raw(torch.full((GUARD,), fill_value(tdt), dtype=tdt))
    for j, d in enumerate(dsts):
        got = raw(d)
        es = d.element_size()
        print(f"{what} dst{j}: {m} elements")
        assert np.array_equal(got[:m * es], raw(exp)), f"{what} dst{j}"
        assert np.array_equal(got[m * es:], guard), f"{what} dst{j} guard"


@pytest.fixture(scope="module", autouse=True)
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert "UCC_EC_REDUCE_DEPTH" not in os.environ, (
        "UCC_EC_REDUCE_DEPTH overrides the depths these counts are built on")
    torch.cuda.set_device(0)


@pytest.mark.parametrize("n,kind", CASES,
                         ids=[f"n{n}-{k}" for n, k in CASES])
def test_counts(n, kind):
    """zc_write = 1 into n dsts at every count of the list."""
    tdt, ucc_dt, op = KINDS[kind]
    for ci, count in enumerate(counts_for(n, tdt)):
        x = inputs(n, count, tdt, 1000 * n + ci)
        dsts = run_probe(x, ucc_dt, op)
        assert len(dsts) == n
        check(dsts, expected(x, op), tdt, f"{kind} n={n} count={count}")


@pytest.mark.parametrize("n", [2, 3, 5])
def test_single_dst(n):
    """zc_write = 0 (reduce_scatter): my_out only, U = 4, 2, 1."""
    tdt, ucc_dt, op = KINDS["bf16_sum"]
    for ci, count in enumerate(counts_for(n, tdt)):
        x = inputs(n, count, tdt, 2000 * n + ci)
        dsts = run_probe(x, ucc_dt, op, zc_write=0)
        assert len(dsts) == 1
        check(dsts, expected(x, op), tdt, f"zc_write=0 n={n} count={count}")


def test_inplace():
    """dst0 is src0: batches touch disjoint elements."""
    tdt, ucc_dt, op = KINDS["bf16_sum"]
    count = counts_for(2, tdt)[-1]
    x = inputs(2, count, tdt, 31)
    dsts = run_probe(x, ucc_dt, op, inplace=True)
    check(dsts, expected(x, op), tdt, "inplace")


@pytest.mark.parametrize("n", [2, 4, 8])
def test_slice_offset(n):
    """sl_b != 0, a multiple of 256 bytes as the host produces; srcs are
    bases, dsts are already offset by the slice start."""
    tdt, ucc_dt, op = KINDS["bf16_avg"]
    sl_b = 3 * 256
    first = sl_b // 2
    count = first + counts_for(n, tdt)[-1]
    x = inputs(n, count, tdt, 41 + n)
    dsts = run_probe(x, ucc_dt, op, sl_b=sl_b)
    check(dsts, expected(x, op)[first:], tdt, f"sl_b={sl_b} n={n}")


def test_bad_arguments():
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    c = core()
    with pytest.raises(RuntimeError):  # one rank
        c.ec_zc_data([p], [p], 0, 256, dtypes.FLOAT32, dtypes.OP_SUM, 1, 1.0,
                     blocks=2)
    with pytest.raises(RuntimeError):  # dst count does not match zc_write
        c.ec_zc_data([p, p], [p], 0, 256, dtypes.FLOAT32, dtypes.OP_SUM, 1,
                     1.0, blocks=2)
    with pytest.raises(RuntimeError):  # sl_e < sl_b
        c.ec_zc_data([p, p], [p, p], 512, 256, dtypes.FLOAT32,
                     dtypes.OP_SUM, 1, 1.0, blocks=2)
    with pytest.raises(RuntimeError):  # threads the kernel is not built for
        c.ec_zc_data([p, p], [p, p], 0, 256, dtypes.FLOAT32, dtypes.OP_SUM,
                     1, 1.0, blocks=2, threads=512)
    for srcs, dsts, sl_b in (([p, p + 8], [p, p], 0), ([p, p], [p + 4, p], 0),
                             ([p, p], [p, p], 8), ([p, 0], [p, p], 0)):
        with pytest.raises(RuntimeError, match="16-byte aligned"):
            c.ec_zc_data(srcs, dsts, sl_b, 256, dtypes.FLOAT32,
                         dtypes.OP_SUM, 1, 1.0, blocks=2)
    with pytest.raises(RuntimeError, match="Not supported"):
        c.ec_zc_data([p, p], [p, p], 0, 256, dtypes.FLOAT32, dtypes.OP_BAND,
                     1, 1.0, blocks=2)


def test_normals_match_three_kernel_path(tmp_path):
    """Seeded bf16 normals: both ranks' slices of a real 2-process
    allreduce on the three-kernel path, reproduced by the probe."""
    seed, count = 515, 100_003
    proc = _torchrun(
        [os.path.join(REPO, "tests", "zc_data_worker.py"), str(tmp_path),
         str(seed), str(count)], timeout=240,
        env_extra={"UCC_TL_CDNA4_FUSED_MAX": "64",
                   "UCC_TL_CDNA4_GATED_BLOCKS": "8",
                   "UCC_TL_CDNA4_ZC_FUSED": "0",
                   "UCC_LOG_LEVEL": "debug"})
    sys.stdout.write(proc.stdout[-2000:])
    sys.stderr.write("\n".join(ln for ln in proc.stderr.splitlines()
                               if " DEBUG " not in ln)[-3000:])
    assert proc.returncode == 0
    assert proc.stdout.count("ZCD_OK") == 2
    assert "zero-copy three-kernel" in proc.stderr
    ref = [np.load(os.path.join(str(tmp_path), f"normals_rank{r}.npy"))
           for r in range(2)]
    assert np.array_equal(ref[0], ref[1])
    # inputs of tests/zc_fused_worker.py Job.inputs, slices of the host
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(2, count, generator=g).to(torch.bfloat16)
    total = count * 2
    per = (total // 2) & ~255
    for r, (b, e) in enumerate(((0, per), (per, total))):
        dsts = run_probe(x[:, :e // 2].contiguous(), dtypes.BFLOAT16,
                         dtypes.OP_SUM, sl_b=b)
        for j, d in enumerate(dsts):
            assert np.array_equal(raw(d)[:e - b], ref[0][b:e]), (r, j)
