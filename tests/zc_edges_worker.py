"""Worker for tests/test_zc_edges_gpu.py: the protocol edges of the
one-kernel zero-copy allreduce (k_zc_allreduce) under re-posting, run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=2 \
      --master-addr 127.0.0.1 tests/zc_edges_worker.py

Both ranks share cuda:0; the test sets UCC_TL_CDNA4_FUSED_MAX low and
UCC_TL_CDNA4_GATED_BLOCKS=8 (the environment of tests/test_zc_fused_gpu.py).
Each persistent request is re-posted many times. Before every post src is
overwritten with k/2, k in [-8, 8], seeded by the post number, so the sum
of the ranks is exact in fp32 and in the element type and does not depend
on any rounding; after every post dst is compared BITWISE with that sum. A
stale src read (a missing acquire at entry) or a completion published
before the peers' writes to my dst have landed (a missing acquire at exit)
shows as a value of an earlier post.
"""

import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ucc_amd import dtypes  # noqa: E402
from zc_fused_worker import DT, Job, wait  # noqa: E402

AR_POSTS = 64
RS_POSTS = 16


def exact_inputs(world, count, tdt, seed):
    g = torch.Generator().manual_seed(seed)
    k = torch.randint(-8, 9, (world, count), generator=g)
    return (k.float() / 2).to(tdt)


def exact_sum(full):
    acc = full[0].float()
    for r in range(1, full.shape[0]):
        acc = acc + full[r].float()
    return acc.to(full.dtype)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8),
                       b.contiguous().view(torch.uint8))


def allreduce(job, name, seed, count, inplace=False):
    c, tdt = job.c, torch.bfloat16
    src = torch.zeros(count, dtype=tdt, device="cuda")
    if inplace:
        dst, flags = src, c.FLAG_PERSISTENT | c.FLAG_IN_PLACE
    else:
        dst = torch.zeros(count, dtype=tdt, device="cuda")
        flags = c.FLAG_PERSISTENT
    req = c.coll_init(job.team, "allreduce", src=src.data_ptr(),
                      dst=dst.data_ptr(), count=count, dt=DT[tdt],
                      op=dtypes.OP_SUM, mem_type=dtypes.MEM_CUDA, flags=flags)
    for it in range(AR_POSTS):
        full = exact_inputs(job.world, count, tdt, seed + it)
        src.copy_(full[job.rank])
        torch.cuda.synchronize()
        wait(req, job.ctx)
        torch.cuda.synchronize()
        got = dst.cpu()
        assert same_bits(got, exact_sum(full)), (
            f"{name}: post {it} of {AR_POSTS}, rank {job.rank}: "
            f"{int((got != exact_sum(full)).sum())} of {count} elements "
            f"differ from the exact sum")
    job.done.append(name)


def reduce_scatter(job, name, seed, per):
    """The rs_zc* shape of tests/zc_fused_worker.py: zc_write = 0, the
    exit without phase 2."""
    c, world, rank = job.c, job.world, job.rank
    src = torch.zeros(per * world, device="cuda")
    dst = torch.zeros(per, device="cuda")
    req = c.coll_init(job.team, "reduce_scatter", src=src.data_ptr(),
                      dst=dst.data_ptr(), count=per, dt=dtypes.FLOAT32,
                      mem_type=dtypes.MEM_CUDA, flags=c.FLAG_PERSISTENT)
    for it in range(RS_POSTS):
        full = exact_inputs(world, per * world, torch.float32, seed + it)
        src.copy_(full[rank])
        torch.cuda.synchronize()
        wait(req, job.ctx)
        torch.cuda.synchronize()
        exp = exact_sum(full)[rank * per:(rank + 1) * per]
        assert same_bits(dst.cpu(), exp), (
            f"{name}: post {it} of {RS_POSTS}, rank {rank}")
    job.done.append(name)


def main():
    job = Job(outdir=None)
    assert job.world == 2
    # per == 0: only the last rank owns a slice, the other must still
    # signal and complete
    allreduce(job, "tiny", 10_000, 100)
    # each of the 8 blocks re-reads 2 KiB per rank per post: the
    # L1-resident regime, where a missing acquire is near-certain to show
    allreduce(job, "l1", 20_000, 16_384)
    # one steady-state batch, the per-pack remainder and the scalar tail
    allreduce(job, "batch", 30_000, 2 * (65_536 + 8 * 300 + 5))
    allreduce(job, "l1_inplace", 40_000, 16_384, inplace=True)
    reduce_scatter(job, "rs", 50_000, 70_001)
    job.finish("ZCE_OK")


if __name__ == "__main__":
    main()
