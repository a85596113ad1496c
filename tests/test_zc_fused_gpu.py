"""Fused zero-copy allreduce (k_zc_allreduce, one launch per post) against
the stage/reduce/gather launches it replaces: tests/zc_fused_worker.py
runs the same seeded cases with UCC_TL_CDNA4_ZC_FUSED=0 and =1 (2 ranks
on cuda:0) and every dst must match bit for bit; the lockstep re-post
case also runs at 4 ranks. Three torchrun launches in total, shared by
all tests of this file."""

import glob
import os
import subprocess
import sys
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "zc_fused_worker.py")

ONE_KERNEL = "zero-copy one-kernel (k_zc_allreduce) path"
THREE_KERNEL = "zero-copy three-kernel"

# small messages onto the gated zero-copy path, non-default grid
ENV = {
    "UCC_TL_CDNA4_FUSED_MAX": "64",
    "UCC_TL_CDNA4_GATED_BLOCKS": "8",
    "UCC_LOG_LEVEL": "debug",
}

CASES = ["bf16_sum_batches", "bf16_tiny", "fp32_sum", "bf16_avg",
         "int32_max", "bf16_inplace", "repost", "inter_ar0",
         "inter_rs_staged", "inter_ar1", "inter_a2a", "inter_ar2",
         "rs_zc0", "rs_zc1", "rs_zc2"]


def _torchrun(script_args, timeout=600, env_extra=None, nproc=2):
    """torchrun with a time-salted rendezvous port and one retry: the
    elastic agent occasionally fails its local TCPStore bind on a busy
    box, which is unrelated to the code under test."""
    print("ndev=", torch.cuda.device_count())
    last = None
    for attempt in range(3):
        port = 29000 + (int(time.time() * 7) + attempt * 131) % 2000
        env = dict(os.environ)
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if env_extra:
            env.update(env_extra)
        proc = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
             f"--nproc-per-node={nproc}", "--master-addr=127.0.0.1",
             f"--master-port={port}"] + script_args,
            cwd=REPO, env=env, capture_output=True, text=True,
            timeout=timeout)
        last = proc
        if proc.returncode == 0:
            return proc
    return last


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = {}
    for tag, fused, nproc, extra in (("three", "0", 2, []),
                                     ("fused", "1", 2, []),
                                     ("fused4", "1", 4, ["repost"])):
        d = tmp_path_factory.mktemp(tag)
        proc = _torchrun([WORKER, str(d)] + extra, timeout=240,
                         env_extra={**ENV, "UCC_TL_CDNA4_ZC_FUSED": fused},
                         nproc=nproc)
        sys.stdout.write(f"--- {tag}: rc={proc.returncode}\n")
        sys.stdout.write(proc.stdout[-2000:])
        sys.stderr.write("\n".join(
            ln for ln in proc.stderr.splitlines()
            if " DEBUG " not in ln)[-3000:])
        out[tag] = (proc, str(d))
    return out


def test_three_kernel_run(runs):
    proc, _ = runs["three"]
    assert proc.returncode == 0
    assert proc.stdout.count("ZCF_OK") == 2
    assert THREE_KERNEL in proc.stderr
    assert ONE_KERNEL not in proc.stderr


def test_fused_run(runs):
    proc, _ = runs["fused"]
    assert proc.returncode == 0
    assert proc.stdout.count("ZCF_OK") == 2


def test_one_kernel_path_ran(runs):
    """Every zero-copy task of the fused run names the one-kernel path at
    set-up: 8 allreduce requests and the zero-copy reduce_scatter, on
    each of the 2 ranks."""
    proc, _ = runs["fused"]
    assert proc.stderr.count(ONE_KERNEL) == 2 * 9
    assert THREE_KERNEL not in proc.stderr


def test_bitwise_equal_to_three_kernel(runs):
    _, d3 = runs["three"]
    _, d1 = runs["fused"]
    assert runs["three"][0].returncode == 0
    assert runs["fused"][0].returncode == 0
    names = sorted(os.path.basename(p)
                   for p in glob.glob(os.path.join(d3, "*.npy")))
    assert names == sorted(f"{c}_rank{r}.npy" for c in CASES
                           for r in range(2))
    for n in names:
        a = np.load(os.path.join(d3, n))
        b = np.load(os.path.join(d1, n))
        assert a.shape == b.shape, n
        assert np.array_equal(a, b), n


def test_repost_4_ranks(runs):
    proc, _ = runs["fused4"]
    assert proc.returncode == 0
    assert proc.stdout.count("ZCF_OK") == 4
    assert proc.stderr.count(ONE_KERNEL) == 4
