"""The collectives that only move bytes, byte for byte over whole guarded
allocations (tests/copy_colls_worker.py, models in tests/copy_cases.py):

 * staged_linear and its k_gather_copy launches: one fresh process per team
   size 2, 3 and 8, all ranks on cuda:0 through LocalJob; the selection
   trace must name cdna4/staged_linear once per request and nothing else;
 * the device-gated pipeline (k_staged_stage, k_staged_gather) across
   processes, one rank per process on cuda:0: 2 ranks with the default
   grid, 4 ranks with UCC_TL_CDNA4_GATED_BLOCKS=8, and the two grids smaller
   than the team, 4 ranks with 2 blocks and 3 ranks with 1 block, where
   k_staged_gather's blocks must loop over the sources.

Every worker is launched once, under its own `timeout -k`; a worker that has
started is never retried, and after a worker that aborted, crashed, ran
into its time limit or reported an illegal access nothing further is
started. The worker's docstring says what each case checks."""

import os
import re
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "copy_colls_worker.py")

# time limits in seconds: four times the first clean run on an MI355X. The
# three in-process workers took 7.7 s together and were not timed one by
# one, so each gets four times that sum; the cross-process runs took 8.4,
# 5.9, 6.2 and 5.8 s, torchrun's start-up included.
INPROC_LIMIT = {2: 32, 3: 32, 8: 32}
XPROC_LIMIT = {"n2_default": 34, "n4_blocks8": 24, "n4_blocks2": 25,
               "n3_blocks1": 24}

XENV = {
    "UCC_TL_CDNA4_CHUNK_SIZE": "65536",
    # below the smallest message: the allreduce is a gated one
    "UCC_TL_CDNA4_FUSED_MAX": "1",
    # a protocol error ends as a reported timeout within seconds (the value
    # of test_xproc_spin_timeout_recovery)
    "UCC_TL_CDNA4_SPIN_LIMIT": "3000000",
    "UCC_TL_CDNA4_GATED_ROOTED": "1",
    "UCC_COLL_TRACE": "1",
    # debug: the zero-copy launch pattern of a task is named at that level
    "UCC_LOG_LEVEL": "debug",
}
UNSET = ("UCC_TL_CDNA4_GATED_BLOCKS", "UCC_TUNE", "UCC_TL_CDNA4_RING",
         "UCC_TL_CDNA4_FUSED_COLLS", "UCC_TL_CDNA4_STAGE_SDMA",
         "UCC_TL_CDNA4_ZCOPY", "UCC_TL_CDNA4_GATED")

XRUNS = {
    "n2_default": (2, None),
    "n4_blocks8": (4, "8"),
    "n4_blocks2": (4, "2"),     # grid < ranks
    "n3_blocks1": (3, "1"),     # grid < ranks
}

_stopped = []
_cache = {}

TRACE = re.compile(r"coll (\w+) mem cuda size \d+ -> (\S+)")
DONE = re.compile(r"COPY_DONE mode=(\w+) n=(\d+) ranks=\[[\d, ]*\] "
                  r"cases=(\d+) n_req=(\d+) refused=(\d+) bad=(\d+)")


FAULT_CODES = (124, 137, 134, 139, -6, -9, -11)
FAULT_MARKS = ("illegal memory access", "Memory access fault", "SIGSEGV",
               "SIGABRT", "exitcode  : -")


def _launch(key, make_cmd, limit, nproc, env_extra=None):
    """one launch per key, cached; see the module docstring. make_cmd
    (attempt) gives the command line."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if key in _cache:
        return _cache[key]
    if _stopped:
        pytest.fail(f"not started: {_stopped[0]}")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    for k in UNSET:
        env.pop(k, None)
    env.update(env_extra or {})
    proc = None
    for attempt in range(2):
        cmd = make_cmd(attempt)
        try:
            proc = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd,
                                  cwd=REPO, env=env, capture_output=True,
                                  text=True, timeout=limit + 60)
        except subprocess.TimeoutExpired:
            _stopped.append(f"{key} outlived its time limit")
            raise
        faulted = proc.returncode in FAULT_CODES or \
            any(m in proc.stderr for m in FAULT_MARKS)
        # torchrun's rendezvous can fail to bind its port before any worker
        # exists; only then, and never after a fault or a time limit, is a
        # second launch allowed (on another port)
        if proc.returncode == 0 or faulted or \
                "COPY_START" in proc.stdout or "torch.distributed.run" \
                not in cmd:
            break
    sys.stdout.write(f"--- {key}: rc={proc.returncode}\n")
    sys.stdout.write(proc.stdout[-4000:])
    sys.stderr.write("\n".join(
        ln for ln in proc.stderr.splitlines()
        if " score " not in ln and " DEBUG " not in ln)[-4000:] + "\n")
    # a worker that ended badly without every rank reaching its COPY_DONE
    # line aborted, crashed or was killed, whatever exit code the launcher
    # turned that into: nothing further is started
    if faulted or (proc.returncode != 0 and
                   len(DONE.findall(proc.stdout)) != nproc):
        _stopped.append(f"{key} ended with exit {proc.returncode}")
    _cache[key] = proc
    return proc


def _done_lines(proc, mode, n, nproc):
    assert "COPY_BAD" not in proc.stdout
    assert proc.returncode == 0
    done = [m.groups() for m in DONE.finditer(proc.stdout)]
    assert len(done) == nproc
    assert all(d[0] == mode and int(d[1]) == n and int(d[5]) == 0
               for d in done), done
    assert all(int(d[2]) > 100 for d in done), done
    return done


@pytest.mark.parametrize("n", [2, 3, 8])
def test_staged_linear_inprocess(n):
    proc = _launch(f"inproc{n}",
                   lambda attempt: [sys.executable, WORKER, "inproc", str(n)],
                   INPROC_LIMIT[n], 1)
    (done,) = _done_lines(proc, "inproc", n, 1)
    n_req, refused = int(done[3]), int(done[4])
    # alltoall and alltoallv in place: refused by coll_init on every rank
    assert refused == 2 * n
    # every request was served by staged_linear, as the trace shows
    algs = [m.group(2) for m in TRACE.finditer(proc.stderr)]
    assert set(algs) == {"cdna4/staged_linear"}, set(algs)
    assert len(algs) == n_req
    assert "timed out" not in proc.stderr


def _xrun(key):
    nproc, blocks = XRUNS[key]
    env = dict(XENV)
    if blocks:
        env["UCC_TL_CDNA4_GATED_BLOCKS"] = blocks

    def cmd(attempt):
        port = 29000 + (os.getpid() * 7 + 131 * list(XRUNS).index(key) +
                        977 * attempt) % 2000
        return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                f"--nproc-per-node={nproc}", "--master-addr=127.0.0.1",
                f"--master-port={port}", WORKER, "xproc"]

    return nproc, _launch(key, cmd, XPROC_LIMIT[key], nproc, env)


@pytest.mark.parametrize("key", list(XRUNS))
def test_gated_pipeline_cross_process(key):
    nproc, proc = _xrun(key)
    done = _done_lines(proc, "xproc", nproc, nproc)
    n_req = sum(int(d[3]) for d in done)
    # every request was served by the gated pipeline, as the trace shows
    seen = [m.groups() for m in TRACE.finditer(proc.stderr)]
    assert {a for _, a in seen} == {"cdna4/gated_pipeline"}, \
        {a for _, a in seen}
    assert len(seen) == n_req
    assert {c for c, _ in seen} == {"allgather", "allgatherv", "alltoall",
                                    "alltoallv", "allreduce", "bcast"}
    # the persistent allgather and alltoall (the two with a zero-copy form)
    # of both types, on every rank: the aligned pass named the zero-copy
    # gather at set-up, the misaligned one was declined by consensus, and
    # nothing else was either
    for coll in ("allgather", "alltoall"):
        assert proc.stderr.count(f"cdna4 gated {coll}: zero-copy gather "
                                 "from the peers' user src path") == \
            2 * nproc
    assert proc.stderr.count("zero-copy gather from") == 4 * nproc
    assert proc.stderr.count("zero-copy disabled by team consensus") == \
        4 * nproc
    assert "timed out" not in proc.stderr
