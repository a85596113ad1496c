"""Every cell of the device reductions' dtype x op dispatch, through each
kernel family that has its own table, compared exactly (no tolerance) with
the host model in tests/dispatch_cases.py: 14 dtypes plus the two complex
types, every op op_supported() accepts, 2 ranks on cuda:0,
count = 3 * (16 / elem_size) + 3 (three 16-byte packs and a scalar tail).

 * in-process jig (LocalJob): same-process ranks are refused by the fused
   and the gated paths, so this message runs the staged-linear algorithm
   and its n-source k_reduce;
 * tests/dispatch_worker.py fused: cross-process, default thresholds,
   k_fused_allreduce;
 * tests/dispatch_worker.py gated: UCC_TL_CDNA4_FUSED_MAX below the
   smallest message, one-shot (k_staged_reduce) and persistent zero-copy
   (k_zc_allreduce) requests.

Unsupported (dtype, op) pairs must be refused at coll_init on every path.
"""

import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import dispatch_cases as dc  # noqa: E402
from test_zc_fused_gpu import ONE_KERNEL, REPO, _torchrun  # noqa: E402
from ucc_amd import dtypes  # noqa: E402
from ucc_amd.testing import LocalJob  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "dispatch_worker.py")


def test_table_shape():
    """14 dtypes x (SUM PROD MAX MIN) + 6 floats x AVG + 8 ints x 6
    logical/bitwise + 2 complex x (SUM AVG)"""
    assert len(dc.CELLS) == 14 * 4 + 6 + 8 * 6 + 2 * 2
    assert len(dc.CELLS) + len(dc.UNSUPPORTED) == 16 * 11


@pytest.fixture(scope="module")
def job():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    return LocalJob(2)


@pytest.mark.parametrize("cell", dc.CELLS, ids=dc.cell_id)
def test_reduce_kernel_cell(job, cell):
    dt, op = cell
    x = dc.inputs(dt, op)
    srcs = [dc.to_device(dt, x[r]) for r in range(2)]
    dsts = [torch.zeros_like(s) for s in srcs]
    reqs = job.coll("allreduce", [
        dict(src=srcs[r].data_ptr(), dst=dsts[r].data_ptr(),
             count=dc.count_for(dt), dt=dt, op=op,
             mem_type=dtypes.MEM_CUDA)
        for r in range(2)
    ])
    job.run(reqs)
    torch.cuda.synchronize()
    for d in dsts:
        assert dc.mismatch(dt, op, x, d) is None


def test_reduce_kernel_unsupported(job):
    buf = torch.zeros(256, dtype=torch.uint8, device="cuda")
    for dt, op in dc.UNSUPPORTED:
        with pytest.raises(RuntimeError, match="Not supported"):
            job.c.coll_init(job.teams[0], "allreduce", src=buf.data_ptr(),
                            dst=buf.data_ptr(), count=dc.count_for(dt),
                            dt=dt, op=op, mem_type=dtypes.MEM_CUDA)


@pytest.fixture(scope="module")
def runs():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for mode, env in (("fused", {}),
                      ("gated", {"UCC_TL_CDNA4_FUSED_MAX": "32",
                                 "UCC_LOG_LEVEL": "debug"})):
        proc = _torchrun([WORKER, mode], timeout=240, env_extra=env)
        sys.stdout.write(f"--- {mode}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-4000:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln)[-3000:])
        out[mode] = proc
    return out


def _check(proc, mode):
    assert "DISPATCH_BAD" not in proc.stdout
    assert proc.returncode == 0
    done = (f"mode={mode} cells={len(dc.CELLS)} "
            f"refused={len(dc.UNSUPPORTED)} bad=0")
    assert proc.stdout.count(done) == 2


def test_fused_kernel_table(runs):
    _check(runs["fused"], "fused")


def test_gated_kernel_tables(runs):
    proc = runs["gated"]
    _check(proc, "gated")
    # the persistent request of every cell named the one-kernel zero-copy
    # path at set-up, on both ranks; the one-shot ones stay below the
    # zero-copy threshold and ran stage / k_staged_reduce / gather
    assert proc.stderr.count(ONE_KERNEL) == 2 * len(dc.CELLS)
