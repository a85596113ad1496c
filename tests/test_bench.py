"""bench.py driver contract: seeded inputs, --dump-outputs sampling and
the plain-run result line."""

import json
import os
import signal
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


@pytest.mark.parametrize("world", [2, 4, 8])
def test_dump_indices_fixed_and_bounded(world):
    import bench

    share = bench.DUMP_TOTAL_ELEMS // world
    # outputs that fit the rank's share are written whole
    assert bench.dump_indices(share, 7, world) is None
    for n in (share + 1, 128 * 1024 * 1024):
        a = bench.dump_indices(n, 7, world)
        b = bench.dump_indices(n, 7, world)
        assert torch.equal(a, b)
        assert a.numel() == share
        assert int(a.min()) == 0 and int(a.max()) == n - 1
        # both buffer ends are always part of the sample
        e = bench.DUMP_EDGE_ELEMS
        assert torch.equal(a[:e], torch.arange(e))
        assert torch.equal(a[-e:], torch.arange(n - e, n))
        # all ranks' float32 samples together stay inside 64 MB
        assert world * 4 * a.numel() <= 64 * 1000 * 1000
    assert not torch.equal(bench.dump_indices(share + 1, 7, world),
                           bench.dump_indices(share + 1, 8, world))


def test_dump_indices_many_ranks_clamp_edges():
    import bench

    world = 4096  # share smaller than the two edge blocks
    share = bench.DUMP_TOTAL_ELEMS // world
    assert share < 2 * bench.DUMP_EDGE_ELEMS
    a = bench.dump_indices(1 << 20, 7, world)
    assert a.numel() == share
    assert int(a.min()) == 0 and int(a.max()) == (1 << 20) - 1


@pytest.mark.gpu
def test_bench_plain_run_dumps_last_step(tmp_path):
    """A plain N=1 run (2 procs on one GPU) at 16 MiB: the result line
    carries ms_per_step and no side measurements, and the dumped dst
    sample of both ranks is the bf16 sum of the two seeded inputs."""
    import bench

    mbytes, seed = 16, 99
    p = subprocess.Popen(
        [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", "--mbytes", str(mbytes),
         "--seed", str(seed), "--dump-outputs", str(tmp_path)],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
        cwd=REPO, start_new_session=True)
    try:
        stdout, stderr = p.communicate(timeout=120)
    except subprocess.TimeoutExpired:
        # the ranks are grandchildren: take the whole group down
        os.killpg(p.pid, signal.SIGKILL)
        p.communicate()
        raise
    assert p.returncode == 0, (stdout[-500:], stderr[-500:])
    out = json.loads(stdout.strip().splitlines()[-1])
    assert out["metric"] == "allreduce_busbw_GBps" and out["steps"] == 3
    assert out["ms_per_step"] > 0 and out["value"] > 0
    assert "lat8b_us" not in out["config"]
    assert "local_copy_selfTL" not in out["config"]

    count = mbytes * 1024 * 1024 // 2
    idx = bench.dump_indices(count, seed, 2)
    assert idx is not None  # the sampled path is the one under test
    srcs = [torch.randn(count, dtype=torch.float32,
                        generator=torch.Generator().manual_seed(seed + r))
            .to(torch.bfloat16).float() for r in range(2)]
    # two ranks: one fp32 add, one round-to-nearest-even to bf16
    ref = (srcs[0] + srcs[1]).to(torch.bfloat16).float()[idx].numpy()
    for r in range(2):
        got = np.load(tmp_path / f"allreduce_dst_rank{r}.npy")
        assert got.dtype == np.float32 and got.shape == ref.shape
        assert np.array_equal(got, ref)
