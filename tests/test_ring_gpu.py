"""tl/cdna4's opt-in multi-ring allreduce / reduce_scatter / allgather
(algorithm `ring`, UCC_TL_CDNA4_RING=1): tests/ring_worker.py in a fresh
child process per team size for the in-process jig, and under torchrun with
2 and 4 single-rank processes on cuda:0, plus the unchanged default.

Each worker launch happens once, under its own subprocess timeout, with no
retry; after a failed launch the later launches of this module are skipped.
The worker checks results bit for bit, that all ranks' allreduce outputs
are identical and that ec_ring_step_launches() grew by what the plan
predicts; here the trace (UCC_COLL_TRACE=1) is counted: `cdna4/ring` once
per request the worker initialised."""

import os
import re
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "ring_worker.py")

_launch_failed = []


def _launch(cmd, what, timeout):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _launch_failed:
        pytest.skip(f"earlier launch failed: {_launch_failed[0]}")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        proc = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True,
                              text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        _launch_failed.append(f"{what}: timeout")
        raise
    sys.stdout.write(proc.stdout[-3000:])
    other = [ln for ln in proc.stderr.splitlines() if " score " not in ln]
    sys.stderr.write("\n".join(other[-80:]) + "\n")
    if proc.returncode != 0:
        _launch_failed.append(f"{what}: exit {proc.returncode}")
    return proc


def _ring_trace(proc):
    return [ln for ln in proc.stderr.splitlines()
            if " mem cuda " in ln and "-> cdna4/ring " in ln]


def _sum(proc, tag, key):
    vals = re.findall(rf"{tag} [^\n]*?\b{key}=(\d+)", proc.stdout)
    return len(vals), sum(int(v) for v in vals)


@pytest.mark.parametrize("n", [2, 3, 4, 6, 8])
def test_ring_inprocess(n):
    """n ranks of one process, RING_NRINGS 1 and auto: every case of the
    worker passes and every ring request logged cdna4/ring exactly once;
    the reduce_scatterv went elsewhere."""
    proc = _launch([sys.executable, WORKER, "inproc", str(n)],
                   f"inproc {n}", 240)
    assert proc.returncode == 0
    passes, n_req = _sum(proc, "RING_INPROC_OK", "n_req")
    assert passes == 2 and n_req > 0
    assert len(_ring_trace(proc)) == n_req
    rsv = [ln for ln in proc.stderr.splitlines()
           if "coll reduce_scatterv mem cuda" in ln]
    assert len(rsv) == 2 * n and not any("/ring " in ln for ln in rsv)
    assert "timed out" not in proc.stderr


@pytest.mark.parametrize("nproc", [2, 4])
def test_ring_cross_process(nproc):
    """one rank per process on one GPU: left's outbox is read over the IPC
    mapping. bf16, the three collectives, 999 per rank and 3 fragments."""
    proc = _launch(
        [sys.executable, "-m", "torch.distributed.run", "--standalone",
         "--nnodes=1", f"--nproc-per-node={nproc}", WORKER, "xproc", "0"],
        f"xproc {nproc}", 300)
    assert proc.returncode == 0
    ranks, n_req = _sum(proc, "RING_XPROC_OK", "n_req")
    assert ranks == nproc and n_req == nproc * 12
    assert len(_ring_trace(proc)) == n_req
    assert "timed out" not in proc.stderr


def test_default_score_map_has_no_ring():
    """with no ring knob set the score map has no cdna4 ring entry (tl/tcp
    has host algorithms of its own whose names contain `ring`; they are not
    meant), and what the knob adds is those entries and nothing else"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    code = (
        "import sys, torch; sys.path.insert(0, %r); torch.cuda.set_device(0)\n"
        "from ucc_amd.testing import LocalJob\n"
        "job = LocalJob(2)\n"
        "print('SCORE_MAP_BEGIN'); print(job.c.score_map_str(job.teams[0]))\n"
        "print('SCORE_MAP_END')\n" % REPO)
    env = dict(os.environ)
    for k in ("UCC_TL_CDNA4_RING", "UCC_TL_CDNA4_RING_NRINGS", "UCC_TUNE"):
        env.pop(k, None)
    off = _launch_env(code, env)
    assert "cdna4/ring" not in off
    env["UCC_TL_CDNA4_RING"] = "1"
    on = _launch_env(code, env)
    added = [ln for ln in on.splitlines() if "@cdna4/ring:" in ln]
    assert len(added) == 6 and all(ln.endswith(":70") for ln in added)
    strip = [ln for ln in on.splitlines() if "@cdna4/ring:" not in ln]
    assert strip == off.splitlines()


def _launch_env(code, env):
    p = subprocess.run([sys.executable, "-c", code], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=120)
    sys.stderr.write(p.stderr[-2000:])
    assert p.returncode == 0
    return p.stdout.split("SCORE_MAP_BEGIN")[1].split("SCORE_MAP_END")[0]
