"""Worker for tests/test_gated_rooted_gpu.py: full-team device bcast and
reduce on the device-gated pipeline (UCC_TL_CDNA4_GATED_ROOTED=1), run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=N \
      --master-addr 127.0.0.1 tests/gated_rooted_worker.py OUTDIR MODE

All ranks share cuda:0. The test sets UCC_TL_CDNA4_GATED_BLOCKS=8 and
UCC_TL_CDNA4_CHUNK_SIZE=65536 (and UCC_TL_CDNA4_FUSED_MAX=64, so the
allreduce every reduce is compared with is a gated one too). One-shot
requests of these sizes are staged, 64 KiB per fragment; persistent ones
are zero-copy, one fragment. With 8 blocks of 256 threads one grid stride
is 32 KiB and one 4-deep batch of the bcast slice phase is 128 KiB
(65,536 bf16) per slice.

MODE
  all   2 ranks: every case below for root 0 and root 1, then the
        interleave; raw destination bytes go to OUTDIR/<case>_rank<r>.npy
        so that the test can compare the ZC_FUSED=1 and =0 runs bit for bit
  three 3 ranks, roots 1 and 2: the six-fragment staged sizes and the
        persistent re-post loops (uneven slices; reduce depth U = 2)
  trig  2 ranks: persistent bcast and bf16 SUM reduce through
        ee_create / triggered_post, three iterations each
  off   2 ranks, knob unset: one bcast and one reduce (staged_linear)

Inputs are seeded per case. bcast results are compared bitwise with the
root's data. reduce results are checked against the fp32 torch reference
of tests/zc_fused_worker.py with its tolerances, and bitwise against the
dst of a gated allreduce of the same inputs in the matching mode (staged
one-shot or persistent zero-copy). Sentinel bands around every bcast
buffer and the dst passed by the non-root ranks of a reduce must keep
their fill.
"""

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zc_fused_worker import DT, Job, wait  # noqa: E402

from ucc_amd import dtypes  # noqa: E402

CHUNK = 65536
BAND = 64          # sentinel bytes on each side of a bcast buffer
FILL = 0xA5        # sentinel byte
BATCH_BF16 = 65536  # bf16 elements of one 4-deep batch per slice, B = 8


def nposts():
    return 2 * int(os.environ.get("UCC_TL_CDNA4_MAX_CONCURRENT", "4")) + 1


def raw(t):
    return t.detach().cpu().contiguous().view(torch.uint8).numpy()


class Banded:
    """`nbytes` bytes at `mis` bytes past a 16-byte boundary inside a larger
    sentinel-filled allocation, viewed as `tdt`."""

    def __init__(self, nbytes, tdt=torch.uint8, mis=0):
        self.big = torch.full((BAND + mis + nbytes + BAND,), FILL,
                              dtype=torch.uint8, device="cuda")
        assert self.big.data_ptr() % 16 == 0
        self.lo = BAND + mis
        self.hi = self.lo + nbytes
        self.buf = self.big[self.lo:self.hi].view(tdt)
        assert self.buf.data_ptr() % 16 == mis % 16

    def bands_intact(self):
        b = self.big.cpu().numpy()
        return bool((b[:self.lo] == FILL).all() and
                    (b[self.hi:] == FILL).all())


def bcast_data(seed, tdt, count):
    g = torch.Generator().manual_seed(seed)
    if tdt == torch.uint8:
        return torch.randint(0, 256, (count,), generator=g,
                             dtype=torch.uint8)
    return torch.randn(count, generator=g).to(tdt)


def run_bcast(job, name, seed, tdt, count, root, mis=0, persistent=False,
              posts=1, save=True):
    """One bcast request, `posts` posts with new data each time."""
    c = job.c
    es = torch.empty(0, dtype=tdt).element_size()
    bb = Banded(count * es, tdt, mis)
    req = c.coll_init(job.team, "bcast", src=bb.buf.data_ptr(),
                      dst=bb.buf.data_ptr(), count=count, dt=DT_ALL[tdt],
                      mem_type=dtypes.MEM_CUDA, root=root,
                      flags=c.FLAG_PERSISTENT if persistent else 0)
    for it in range(posts):
        data = bcast_data(seed + 1000 * it, tdt, count)
        if job.rank == root:
            bb.buf.copy_(data)
        else:
            bb.buf.view(torch.uint8).fill_(0x3C)
        torch.cuda.synchronize()
        wait(req, job.ctx)
        torch.cuda.synchronize()
        assert np.array_equal(raw(bb.buf), raw(data)), (name, it)
        assert bb.bands_intact(), (name, it)
    if save:
        job.save(name, bb.buf)
    job.done.append(name)
    return req, bb


def run_reduce(job, name, seed, tdt, count, root, op=dtypes.OP_SUM,
               inplace=False, persistent=False, posts=1, save=True):
    """One reduce request and one allreduce request of the same inputs in
    the same mode; the root's dst must equal the allreduce dst bit for
    bit."""
    c = job.c
    is_root = job.rank == root
    full = job.inputs(seed, tdt, count)
    sentinel = 77 if tdt == torch.int32 else 7.5
    flags = c.FLAG_PERSISTENT if persistent else 0
    if inplace:
        flags |= c.FLAG_IN_PLACE
    if inplace and is_root:
        dst = full[job.rank].clone().cuda()
        src = dst
    else:
        src = full[job.rank].clone().cuda()
        dst = torch.full((count,), sentinel, dtype=tdt, device="cuda")
    req = c.coll_init(job.team, "reduce", src=src.data_ptr(),
                      dst=dst.data_ptr(), count=count, dt=DT[tdt], op=op,
                      mem_type=dtypes.MEM_CUDA, root=root, flags=flags)
    asrc = torch.zeros(count, dtype=tdt, device="cuda")
    adst = torch.zeros(count, dtype=tdt, device="cuda")
    areq = c.coll_init(job.team, "allreduce", src=asrc.data_ptr(),
                       dst=adst.data_ptr(), count=count, dt=DT[tdt], op=op,
                       mem_type=dtypes.MEM_CUDA,
                       flags=c.FLAG_PERSISTENT if persistent else 0)
    for it in range(posts):
        cur = full if it == 0 else job.inputs(seed + 1000 * it, tdt, count)
        src.copy_(cur[job.rank])
        asrc.copy_(cur[job.rank])
        torch.cuda.synchronize()
        wait(req, job.ctx)
        torch.cuda.synchronize()
        wait(areq, job.ctx)
        torch.cuda.synchronize()
        exp = job.reference(cur, op)
        job.check(adst, exp)
        if is_root:
            job.check(dst, exp)
            assert np.array_equal(raw(dst), raw(adst)), (name, it)
        else:
            assert bool((dst == sentinel).all()), (name, it)
            if not inplace:
                assert np.array_equal(raw(src), raw(cur[job.rank])), name
    if save:
        job.save(name, dst)
    job.done.append(name)
    return req, src, dst


DT_ALL = dict(DT)
DT_ALL[torch.uint8] = dtypes.UINT8

SIX_FRAGS_B = 5 * CHUNK + 4099        # bcast bytes: six fragments, byte tail
SIX_FRAGS_F32 = 5 * 16384 + 1025      # fp32 elements: six fragments
SIX_FRAGS_BF16 = 5 * 32768 + 1025     # bf16 elements: six fragments


def per_slice_count(world):
    """bf16 count that gives each slice about three batches + 300 packs +
    5 elements (the host rounds slice starts down to 256 bytes)."""
    return world * (3 * BATCH_BF16 + 8 * 300 + 5)


def run_all(job):
    c, team, ctx, rank, world = job.c, job.team, job.ctx, job.rank, job.world
    for root in range(world):
        t = f"root{root}"
        # ---- bcast, staged one-shot, uint8
        # per == 0: only the last rank owns a slice
        run_bcast(job, f"bc_100_{t}", 11, torch.uint8, 100, root)
        run_bcast(job, f"bc_chunk_{t}", 12, torch.uint8, CHUNK, root)
        # six fragments: both parities reused, byte tail
        run_bcast(job, f"bc_six_{t}", 13, torch.uint8, SIX_FRAGS_B, root)
        run_bcast(job, f"bc_six_mis_{t}", 14, torch.uint8, SIX_FRAGS_B,
                  root, mis=4)
        # ---- bcast, persistent (zero-copy), bf16
        run_bcast(job, f"bc_zc_{t}", 15, torch.bfloat16,
                  per_slice_count(world), root, persistent=True,
                  posts=nposts())
        # misaligned: the consensus falls back to staging
        run_bcast(job, f"bc_zc_mis_{t}", 16, torch.bfloat16, 100_003, root,
                  mis=4, persistent=True, posts=2)
        # ---- reduce, staged one-shot and persistent zero-copy
        for pers, m in ((False, "st"), (True, "zc")):
            run_reduce(job, f"rd_f32_{m}_{t}", 21, torch.float32,
                       SIX_FRAGS_F32, root, persistent=pers)
            run_reduce(job, f"rd_avg_{m}_{t}", 22, torch.bfloat16,
                       SIX_FRAGS_BF16, root, op=dtypes.OP_AVG,
                       persistent=pers)
            run_reduce(job, f"rd_max_{m}_{t}", 23, torch.int32, 40_000,
                       root, op=dtypes.OP_MAX, persistent=pers)
            run_reduce(job, f"rd_inpl_{m}_{t}", 24, torch.bfloat16,
                       SIX_FRAGS_BF16, root, inplace=True, persistent=pers)
        run_reduce(job, f"rd_repost_{t}", 25, torch.bfloat16, 300_003, root,
                   persistent=True, posts=nposts())

    # ---- interleave on one team: persistent zero-copy allreduce, gated
    # bcast, staged gated reduce_scatter, gated reduce, alltoall,
    # allreduce again: ledger continuity across the patterns
    count = 150_000
    req, src, dst = job.allreduce("il_ar0", 200, torch.bfloat16, count)
    run_bcast(job, "il_bcast", 201, torch.uint8, 100_003, 1)
    per = 50_001
    rfull = job.inputs(202, torch.float32, per * world)
    rsrc = rfull[rank].clone().cuda()
    rdst = torch.zeros(per, device="cuda")
    rs = c.coll_init(team, "reduce_scatter", src=rsrc.data_ptr(),
                     dst=rdst.data_ptr(), count=per, dt=dtypes.FLOAT32,
                     mem_type=dtypes.MEM_CUDA)
    wait(rs, ctx)
    torch.cuda.synchronize()
    job.check(rdst, job.reference(rfull, dtypes.OP_SUM)[rank * per:
                                                        (rank + 1) * per])
    job.save("il_rs", rdst)
    job.done.append("il_rs")
    run_reduce(job, "il_reduce", 203, torch.float32, 70_001, 0)
    afull = job.inputs(204, torch.float32, per * world)
    asrc = afull[rank].clone().cuda()
    adst = torch.zeros(per * world, device="cuda")
    a2a = c.coll_init(team, "alltoall", src=asrc.data_ptr(),
                      dst=adst.data_ptr(), count=per * world,
                      dt=dtypes.FLOAT32, mem_type=dtypes.MEM_CUDA)
    wait(a2a, ctx)
    torch.cuda.synchronize()
    exp = torch.cat([afull[s][rank * per:(rank + 1) * per]
                     for s in range(world)])
    torch.testing.assert_close(adst.cpu(), exp, rtol=0, atol=0)
    job.save("il_a2a", adst)
    job.done.append("il_a2a")
    cur = job.inputs(205, torch.bfloat16, count)
    src.copy_(cur[rank])
    torch.cuda.synchronize()
    wait(req, ctx)
    torch.cuda.synchronize()
    job.check(dst, job.reference(cur, dtypes.OP_SUM))
    job.save("il_ar1", dst)
    job.done.append("il_ar1")


def run_three(job):
    for root in (1, 2):
        t = f"root{root}"
        run_bcast(job, f"bc_six_{t}", 31, torch.uint8, SIX_FRAGS_B, root,
                  save=False)
        run_reduce(job, f"rd_f32_st_{t}", 32, torch.float32, SIX_FRAGS_F32,
                   root, save=False)
        run_bcast(job, f"bc_zc_{t}", 33, torch.bfloat16,
                  per_slice_count(job.world), root, persistent=True,
                  posts=nposts(), save=False)
        run_reduce(job, f"rd_repost_{t}", 34, torch.bfloat16, 300_003, root,
                   persistent=True, posts=nposts(), save=False)


def run_trig(job):
    """Stream-triggered posts (derive mode, always the staged pattern):
    four fragments per post, three iterations with new inputs and a
    stream synchronise between them."""
    c, rank = job.c, job.rank
    count, root = 100_003, 1
    s = torch.cuda.Stream()
    ee = c.ee_create(job.team, s.cuda_stream)
    bb = Banded(count * 2, torch.bfloat16)
    breq = c.coll_init(job.team, "bcast", src=bb.buf.data_ptr(),
                       dst=bb.buf.data_ptr(), count=count,
                       dt=dtypes.BFLOAT16, mem_type=dtypes.MEM_CUDA,
                       root=root, flags=c.FLAG_PERSISTENT)
    for it in range(3):
        data = bcast_data(40 + it, torch.bfloat16, count)
        if rank == root:
            bb.buf.copy_(data)
        else:
            bb.buf.view(torch.uint8).fill_(0x3C)
        torch.cuda.synchronize()
        dist.barrier()
        c.triggered_post(ee, breq)
        s.synchronize()
        assert np.array_equal(raw(bb.buf), raw(data)), ("trig bcast", it)
        assert bb.bands_intact()
    job.done.append("trig_bcast")

    src = torch.zeros(count, dtype=torch.bfloat16, device="cuda")
    dst = torch.full((count,), 7.5, dtype=torch.bfloat16, device="cuda")
    rreq = c.coll_init(job.team, "reduce", src=src.data_ptr(),
                       dst=dst.data_ptr(), count=count, dt=dtypes.BFLOAT16,
                       op=dtypes.OP_SUM, mem_type=dtypes.MEM_CUDA, root=root,
                       flags=c.FLAG_PERSISTENT)
    for it in range(3):
        cur = job.inputs(50 + it, torch.bfloat16, count)
        src.copy_(cur[rank])
        torch.cuda.synchronize()
        dist.barrier()
        c.triggered_post(ee, rreq)
        s.synchronize()
        if rank == root:
            job.check(dst, job.reference(cur, dtypes.OP_SUM))
        else:
            assert bool((dst == 7.5).all()), ("trig reduce", it)
    job.done.append("trig_reduce")
    dist.barrier()
    del breq, rreq
    c.ee_destroy(ee)


def run_off(job):
    run_bcast(job, "bc_six_root1", 61, torch.uint8, SIX_FRAGS_B, 1,
              save=False)
    # no allreduce twin here: every trace line of this run is rooted
    c = job.c
    count, root = SIX_FRAGS_F32, 1
    full = job.inputs(62, torch.float32, count)
    src = full[job.rank].clone().cuda()
    dst = torch.full((count,), 7.5, device="cuda")
    req = c.coll_init(job.team, "reduce", src=src.data_ptr(),
                      dst=dst.data_ptr(), count=count, dt=dtypes.FLOAT32,
                      op=dtypes.OP_SUM, mem_type=dtypes.MEM_CUDA, root=root)
    wait(req, job.ctx)
    torch.cuda.synchronize()
    if job.rank == root:
        job.check(dst, job.reference(full, dtypes.OP_SUM))
    else:
        assert bool((dst == 7.5).all())
    job.done.append("rd_f32_root1")


def main():
    job = Job(sys.argv[1])
    {"all": run_all, "three": run_three, "trig": run_trig,
     "off": run_off}[sys.argv[2]](job)
    job.finish("GRT_OK")


if __name__ == "__main__":
    main()
