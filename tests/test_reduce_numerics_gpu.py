"""Device reductions against the exact model of tests/numerics_cases.py,
bit for bit, through every kernel that has its own store site; all ranks
on cuda:0. The rule tested is the "Reduction numerics" section of
docs/USER_GUIDE.md.

 * in-process jig, allreduce at 3 ranks (every family) and 7 ranks (the AVG
   cases): staged-linear, the vector k_reduce with its scalar tail;
 * in-process jig, reduce to root 0 whose dst sits one element past a
   16-byte boundary: k_reduce_scalar (narrow floats, integer extremes);
 * tests/numerics_worker.py fused, 3 processes: k_fused_allreduce;
 * tests/numerics_worker.py gated, 3 processes, UCC_TL_CDNA4_FUSED_MAX
   below the smallest message: one-shot (k_staged_reduce) and persistent
   zero-copy (k_zc_allreduce) requests.
"""

import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numerics_cases as nc  # noqa: E402
from test_zc_fused_gpu import ONE_KERNEL, REPO, _torchrun  # noqa: E402
from ucc_amd import dtypes  # noqa: E402
from ucc_amd.testing import LocalJob  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "numerics_worker.py")
NPROC = 3
_JOBS = {}


def _job(n):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if n not in _JOBS:
        torch.cuda.set_device(0)
        _JOBS[n] = LocalJob(n)
    return _JOBS[n]


def _dev(raw):
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda()


@pytest.mark.parametrize("case", nc.cases(3) + nc.cases(7),
                         ids=lambda c: c.id)
def test_vector_kernel(case):
    job = _job(case.n)
    srcs = [_dev(x) for x in case.x]
    dsts = [torch.full_like(s, 0xA5) for s in srcs]
    # the fills run on torch's stream, the collective on the library's
    torch.cuda.synchronize()
    before = job.c.ec_reduce_scalar_launches()
    reqs = job.coll("allreduce", [
        dict(src=srcs[r].data_ptr(), dst=dsts[r].data_ptr(),
             count=case.count, dt=case.dt, op=case.op,
             mem_type=dtypes.MEM_CUDA)
        for r in range(case.n)
    ])
    job.run(reqs)
    torch.cuda.synchronize()
    # every reduce of it took the vector kernel
    assert job.c.ec_reduce_scalar_launches() == before
    for d in dsts:
        assert case.mismatch(d.cpu().numpy().tobytes()) is None


@pytest.mark.parametrize("case",
                         [c for c in nc.cases(3) if nc.is_scalar_family(c)],
                         ids=lambda c: c.id)
def test_scalar_kernel(case):
    job = _job(case.n)
    esz = dtypes.DT_SIZE[case.dt]
    srcs = [_dev(x) for x in case.x]
    # the allocation is 16-byte aligned; dst starts one element in and is
    # followed by guard bytes the kernel must leave alone
    room = torch.full((case.nbytes + esz + 16,), 0xA5, dtype=torch.uint8,
                      device="cuda")
    assert room.data_ptr() % 16 == 0 and esz < 16
    spare = [torch.full_like(s, 0xA5) for s in srcs]
    torch.cuda.synchronize()
    before = job.c.ec_reduce_scalar_launches()
    reqs = job.coll("reduce", [
        dict(src=srcs[r].data_ptr(),
             dst=room.data_ptr() + esz if r == 0 else spare[r].data_ptr(),
             count=case.count, dt=case.dt, op=case.op, root=0,
             mem_type=dtypes.MEM_CUDA)
        for r in range(case.n)
    ])
    job.run(reqs)
    torch.cuda.synchronize()
    # the root's reduce took k_reduce_scalar, not the vector kernel
    assert job.c.ec_reduce_scalar_launches() == before + 1
    got = room.cpu().numpy()
    assert case.mismatch(got[esz:esz + case.nbytes].tobytes()) is None
    assert (got[:esz] == 0xA5).all() and (got[esz + case.nbytes:] == 0xA5).all()


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    fused_max = str(nc.MIN_BYTES - 1)
    for mode, env in (("fused", {}),
                      ("gated", {"UCC_TL_CDNA4_FUSED_MAX": fused_max,
                                 "UCC_LOG_LEVEL": "debug"})):
        proc = _torchrun([WORKER, mode], timeout=240, env_extra=env,
                         nproc=NPROC)
        sys.stdout.write(f"--- {mode}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-8000:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln)[-3000:])
        out[mode] = proc
    return out


def _check(proc, mode):
    assert "NUM_BAD" not in proc.stdout
    assert proc.returncode == 0
    done = f"mode={mode} cases={len(nc.cases(NPROC))} bad=0"
    assert proc.stdout.count(done) == NPROC


def test_fused_kernel(runs):
    _check(runs["fused"], "fused")


def test_gated_kernels(runs):
    proc = runs["gated"]
    _check(proc, "gated")
    # the persistent request of every case named the one-kernel zero-copy
    # path at set-up, on every rank; the one-shot ones ran stage /
    # k_staged_reduce / gather
    assert proc.stderr.count(ONE_KERNEL) == NPROC * len(nc.cases(NPROC))
