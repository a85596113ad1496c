"""tl/cdna4 device active-set bcast (p2p send/recv over the peer
mappings): the pull kernel in-process through ec_p2p_pull, the score map,
and torchrun launches of tests/p2p_worker.py with 4 and 2 ranks on cuda:0.

Each worker launch happens once, under a subprocess timeout, with no
retry; after a failed launch the later launches of this module are
skipped. UCC_COLL_TRACE=1 makes every collective init log the algorithm
it chose, which is how the tests know that the p2p requests ran on
active_set_p2p and not on staged_linear.
"""

import os
import re
import subprocess
import sys

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(REPO, "tests", "p2p_worker.py")

_launch_failed = []


def _launch(nproc, mode, env_extra=None, timeout=300):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if _launch_failed:
        pytest.skip(f"earlier launch failed: {_launch_failed[0]}")
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["UCC_COLL_TRACE"] = "1"
    env["UCC_LOG_LEVEL"] = "info"
    env.update(env_extra or {})
    try:
        proc = subprocess.run(
            [sys.executable, "-m", "torch.distributed.run", "--standalone",
             "--nnodes=1", f"--nproc-per-node={nproc}", WORKER, mode],
            cwd=REPO, env=env, capture_output=True, text=True,
            timeout=timeout)
    except subprocess.TimeoutExpired:
        _launch_failed.append(f"{mode}: timeout")
        raise
    sys.stdout.write(proc.stdout[-3000:])
    # the trace is long: show the end and every line that is not a trace
    other = [ln for ln in proc.stderr.splitlines() if " score " not in ln]
    sys.stderr.write("\n".join(other[-80:]) + "\n")
    if proc.returncode != 0:
        _launch_failed.append(f"{mode}: exit {proc.returncode}")
    return proc


def _sum(proc, tag, key):
    # unanchored: the ranks share one pipe and their lines can run together
    vals = re.findall(rf"{tag} rank=\d+ [^\n]*?\b{key}=(\d+)", proc.stdout)
    return len(vals), sum(int(v) for v in vals)


def _trace(proc, alg):
    """trace lines of device bcasts that chose `alg`"""
    return [ln for ln in proc.stderr.splitlines()
            if "coll bcast mem cuda" in ln and f"cdna4/{alg} " in ln]


@pytest.fixture(scope="module")
def four_rank():
    return _launch(4, "four")


@pytest.fixture(scope="module")
def two_rank():
    return _launch(2, "two")


@pytest.fixture(scope="module")
def two_rank_off():
    return _launch(2, "two_off", env_extra={"UCC_TL_CDNA4_P2P": "0"})


# ------------------------------------------------------------ pull kernel
SRC_OFFS = (0, 1, 4, 8, 15)
DST_OFFS = (0, 3, 4, 16)
GUARD = 64
SENTINEL = 0xC3


@pytest.mark.parametrize("blocks", [1, 3])
def test_pull_kernel_alignments(blocks):
    """k_p2p_pull against the source slice for independent source and
    destination alignment, with untouched 64-byte guard bands around dst.
    The last length is one full 4-deep batch of the forced grid, one
    single-pack remainder round and a byte tail."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, REPO)
    from ucc_amd import core
    c = core()
    sizes = (0, 1, 15, 16, 17, 4095, 4096, 65_537,
             4 * blocks * 256 * 16 + 16 * 256 + 5)
    g = torch.Generator().manual_seed(1234 + blocks)
    big = max(sizes) + 16
    src_h = torch.randint(0, 256, (big,), generator=g, dtype=torch.uint8)
    src_d = src_h.cuda()
    dst_d = torch.empty(GUARD + 16 + big + GUARD, dtype=torch.uint8,
                        device="cuda")
    assert src_d.data_ptr() % 16 == 0 and dst_d.data_ptr() % 16 == 0
    for n in sizes:
        for so in SRC_OFFS:
            for do in DST_OFFS:
                dst_d.fill_(SENTINEL)
                torch.cuda.synchronize()
                lo = GUARD + do
                used = c.ec_p2p_pull(dst_d.data_ptr() + lo,
                                     src_d.data_ptr() + so, n, blocks)
                assert used == blocks
                got = dst_d.cpu()
                what = (n, so, do)
                assert torch.equal(got[lo:lo + n], src_h[so:so + n]), what
                assert bool((got[:lo] == SENTINEL).all()), what
                assert bool((got[lo + n:] == SENTINEL).all()), what


def test_pull_kernel_auto_grid():
    """blocks=0: the size-derived grid grows from 1 block and is capped."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, REPO)
    from ucc_amd import core
    c = core()
    n = 4 << 20
    src = torch.arange(n, dtype=torch.int32, device="cuda")
    dst = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    used = [c.ec_p2p_pull(dst.data_ptr(), src.data_ptr(), nb)
            for nb in (0, 8, 65536, 65537, 4 * n)]
    assert used[0] == 1 and used[1] == 1 and used[2] == 1 and used[3] == 2
    assert used[3] < used[4] <= 1024
    assert torch.equal(dst.cpu(), src.cpu())


# -------------------------------------------------------------- score map
def test_score_map_lists_active_set_p2p():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, REPO)
    torch.cuda.set_device(0)
    from ucc_amd.testing import LocalJob
    job = LocalJob(2)
    assert "active_set_p2p" in job.c.score_map_str(job.teams[0])


def test_inprocess_pair_with_idle_rank():
    """3 ranks of one process: 0 -> 2 while rank 1 posts nothing, then a
    team-wide bcast still works (same-process ranks resolve the source by
    raw pointer; the pull kernel never waits, so one hardware queue is
    enough)."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    sys.path.insert(0, REPO)
    torch.cuda.set_device(0)
    from ucc_amd import dtypes
    from ucc_amd.testing import LocalJob
    job = LocalJob(3)
    c = job.c
    n = 100_001
    src = torch.randint(0, 256, (n,), dtype=torch.uint8).cuda()
    dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reqs = [c.coll_init(job.teams[r], "bcast", src=b.data_ptr(), dst=0,
                        count=n, dt=dtypes.UINT8, root=0,
                        mem_type=dtypes.MEM_CUDA, active_set=(0, 2, 2),
                        tag=5, timeout=30)
            for r, b in ((0, src), (2, dst))]
    job.run(reqs)
    assert all(r.test() == c.OK for r in reqs)
    torch.cuda.synchronize()
    assert torch.equal(dst.cpu(), src.cpu())
    bufs = [src] + [torch.zeros(n, dtype=torch.uint8, device="cuda")
                    for _ in range(2)]
    reqs = job.coll("bcast", [dict(src=bufs[r].data_ptr(), dst=0, count=n,
                                   dt=dtypes.UINT8, root=0,
                                   mem_type=dtypes.MEM_CUDA, timeout=30)
                              for r in range(3)])
    job.run(reqs)
    torch.cuda.synchronize()
    assert all(torch.equal(b.cpu(), src.cpu()) for b in bufs)


# ------------------------------------------------------------- four ranks
def test_four_rank_cases(four_rank):
    """Every case of the 4-rank worker passed on every rank."""
    assert four_rank.returncode == 0
    assert four_rank.stdout.count("P2P4_OK") == 4
    assert "timed out" not in four_rank.stderr


def test_four_rank_trace(four_rank):
    """Each p2p request logged active_set_p2p; staged_linear served the
    team-wide bcasts of the interleaving case and nothing else."""
    assert four_rank.returncode == 0
    ranks, n_p2p = _sum(four_rank, "P2P4_OK", "n_p2p")
    _, n_bcast = _sum(four_rank, "P2P4_OK", "n_bcast")
    assert ranks == 4 and n_p2p > 0 and n_bcast > 0
    assert len(_trace(four_rank, "active_set_p2p")) == n_p2p
    assert len(_trace(four_rank, "staged_linear")) == n_bcast


# -------------------------------------------------------------- two ranks
def test_pipeline_stage_device(two_rank):
    """PipelineStage on CUDA bf16 tensors moves device to device."""
    assert two_rank.returncode == 0
    assert two_rank.stdout.count("P2P2_OK") == 2
    _, n_p2p = _sum(two_rank, "P2P2_OK", "n_p2p")
    assert n_p2p == 16
    assert len(_trace(two_rank, "active_set_p2p")) == n_p2p
    assert "timed out" not in two_rank.stderr


def test_pipeline_stage_knob_off(two_rank_off):
    """UCC_TL_CDNA4_P2P=0: the same case passes through the host fallback,
    a direct device active-set bcast is refused at init, nothing times
    out."""
    assert two_rank_off.returncode == 0
    assert two_rank_off.stdout.count("P2P2_OK") == 2
    assert not _trace(two_rank_off, "active_set_p2p")
    assert "timed out" not in two_rank_off.stderr
