"""The one-lane protocol edges of k_zc_allreduce under re-posting:
tests/zc_edges_worker.py re-posts persistent zero-copy bf16 allreduces 64
times (counts 100, 16 384, 2*(65 536 + 8*300 + 5), and 16 384 in place) and
a zero-copy reduce_scatter 16 times, 2 ranks on cuda:0, fresh exact inputs
before every post, dst compared bitwise with the exact sum after every
post. Once with the default cache policy (plain at these sizes) and once
with UCC_TL_CDNA4_ZC_STREAM=1."""

import os
import sys

import pytest

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_zc_fused_gpu import ENV, ONE_KERNEL, REPO, _torchrun  # noqa: E402

pytestmark = pytest.mark.gpu

WORKER = os.path.join(REPO, "tests", "zc_edges_worker.py")
STREAMING = "zc data phase: streaming"
NTASKS = 5  # four allreduce requests and the reduce_scatter


@pytest.mark.parametrize("stream", [None, "1"], ids=["default", "stream1"])
def test_reposts_exact(stream):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(ENV)
    if stream is not None:
        env["UCC_TL_CDNA4_ZC_STREAM"] = stream
    proc = _torchrun([WORKER], timeout=240, env_extra=env)
    sys.stdout.write(proc.stdout[-2000:])
    sys.stderr.write("\n".join(ln for ln in proc.stderr.splitlines()
                               if " DEBUG " not in ln)[-3000:])
    assert proc.returncode == 0
    assert proc.stdout.count("ZCE_OK") == 2
    assert "tiny+l1+batch+l1_inplace+rs" in proc.stdout
    assert proc.stderr.count(ONE_KERNEL) == 2 * NTASKS
    assert proc.stderr.count(STREAMING) == (2 * NTASKS if stream else 0)
