"""Worker for tests/test_zc_fused_gpu.py: the zero-copy gated allreduce /
reduce_scatter cases, run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=N \
      --master-addr 127.0.0.1 tests/zc_fused_worker.py OUTDIR [repost]

All ranks share cuda:0. The test sets UCC_TL_CDNA4_FUSED_MAX low and
UCC_TL_CDNA4_GATED_BLOCKS=8, so these small persistent messages take the
gated zero-copy path on a non-default grid, and runs the worker once with
UCC_TL_CDNA4_ZC_FUSED=0 (stage/reduce/gather launches) and once with =1
(one k_zc_allreduce launch per post). Inputs are seeded per case, every
result is checked against an fp32 torch reference, and every rank writes
the raw bytes of each dst to OUTDIR/<case>_rank<r>.npy so the test can
compare the two runs bit for bit.

With B=8 blocks of 256 threads, 8 bf16 per 16-byte pack and depth U=4
(2 ranks), one full batch of the pipelined loop is 65,536 bf16 elements
per slice.
"""

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ucc_amd import core, dtypes  # noqa: E402

# tolerances of tests/xproc_worker.py per dtype
TOL = {
    torch.bfloat16: dict(rtol=2e-2, atol=2e-1),
    torch.float32: dict(rtol=1e-5, atol=1e-4),
    torch.int32: dict(rtol=0, atol=0),
}
DT = {
    torch.bfloat16: dtypes.BFLOAT16,
    torch.float32: dtypes.FLOAT32,
    torch.int32: dtypes.INT32,
}


def oob(group, world):
    def allgather(data: bytes):
        n = len(data)
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).clone()
        outs = [torch.empty(n, dtype=torch.uint8) for _ in range(world)]
        dist.all_gather(outs, t, group=group)
        return [o.numpy().tobytes() for o in outs]

    return allgather


def wait(req, ctx):
    req.post()
    it = 0
    while req.test() == core().INPROGRESS:
        ctx.progress()
        it += 1
        if it > 200_000_000:
            raise TimeoutError("collective stuck")


class Job:
    def __init__(self, outdir):
        self.outdir = outdir
        self.rank = int(os.environ["RANK"])
        self.world = int(os.environ["WORLD_SIZE"])
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=self.rank,
                                world_size=self.world)
        self.c = core()
        self.lib = self.c.Lib()
        self.ctx = self.c.Context(self.lib)
        self.team = self.c.team_create_post(
            self.ctx, py_allgather=oob(dist.group.WORLD, self.world),
            rank=self.rank, n_ranks=self.world)
        while True:
            st = self.c.team_create_test(self.team)
            if st == self.c.OK:
                break
            if st < 0:
                raise RuntimeError(f"team create failed: {st}")
        self.done = []

    def save(self, name, t):
        raw = t.detach().cpu().contiguous().view(torch.uint8).numpy()
        np.save(os.path.join(self.outdir, f"{name}_rank{self.rank}.npy"),
                raw)

    def inputs(self, seed, tdt, count):
        """[world, count] inputs, equal on every rank and in every run."""
        g = torch.Generator().manual_seed(seed)
        if tdt == torch.int32:
            return torch.randint(-1_000_000, 1_000_000,
                                 (self.world, count), generator=g,
                                 dtype=torch.int32)
        return torch.randn(self.world, count, generator=g).to(tdt)

    def reference(self, full, op):
        """fp32 torch reference, ranks 0..n-1 in order."""
        if full.dtype == torch.int32:
            assert op == dtypes.OP_MAX
            return full.max(0).values
        acc = full[0].float()
        for r in range(1, self.world):
            acc = acc + full[r].float()
        if op == dtypes.OP_AVG:
            acc = acc / self.world
        return acc

    def check(self, dst, exp):
        got = dst.cpu()
        if got.dtype != torch.int32:
            got = got.float()
        torch.testing.assert_close(got, exp, **TOL[dst.dtype])

    def allreduce(self, name, seed, tdt, count, op=dtypes.OP_SUM,
                  inplace=False, posts=1):
        """Persistent allreduce, `posts` re-posts with changing inputs."""
        c = self.c
        full = self.inputs(seed, tdt, count)
        if inplace:
            dst = full[self.rank].clone().cuda()
            src = dst
            flags = c.FLAG_PERSISTENT | c.FLAG_IN_PLACE
        else:
            src = full[self.rank].clone().cuda()
            dst = torch.zeros(count, dtype=tdt, device="cuda")
            flags = c.FLAG_PERSISTENT
        req = c.coll_init(self.team, "allreduce", src=src.data_ptr(),
                          dst=dst.data_ptr(), count=count, dt=DT[tdt],
                          op=op, mem_type=dtypes.MEM_CUDA, flags=flags)
        for it in range(posts):
            cur = full if it == 0 else self.inputs(seed + 1000 * it, tdt,
                                                   count)
            src.copy_(cur[self.rank])
            torch.cuda.synchronize()
            wait(req, self.ctx)
            torch.cuda.synchronize()
            self.check(dst, self.reference(cur, op))
        self.save(name, dst)
        self.done.append(name)
        return req, src, dst

    def finish(self, tag):
        dist.barrier()
        print(f"{tag} rank={self.rank} {'+'.join(self.done)}", flush=True)
        dist.destroy_process_group()


def run_repost(job):
    """2*MAX_CONCURRENT + 1 lockstep re-posts of ONE request: every
    rotating slot is reused at least twice, inputs change every time."""
    nslots = int(os.environ.get("UCC_TL_CDNA4_MAX_CONCURRENT", "4"))
    job.allreduce("repost", 900, torch.bfloat16, 300_003,
                  posts=2 * nslots + 1)


def run_all(job):
    c, team, ctx, rank, world = job.c, job.team, job.ctx, job.rank, job.world
    # >= 2 pipelined batches (prologue, steady state, epilogue), the
    # vector remainder loop and the scalar tail
    job.allreduce("bf16_sum_batches", 101, torch.bfloat16,
                  2 * (3 * 65536 + 8 * 300 + 5))
    # per == 0: only the last rank has a slice; the others must still
    # signal and complete
    job.allreduce("bf16_tiny", 102, torch.bfloat16, 100)
    job.allreduce("fp32_sum", 103, torch.float32, 70001)
    # alpha applied exactly once
    job.allreduce("bf16_avg", 104, torch.bfloat16, 65536 * 2 + 8,
                  op=dtypes.OP_AVG)
    job.allreduce("int32_max", 105, torch.int32, 40000, op=dtypes.OP_MAX)
    job.allreduce("bf16_inplace", 106, torch.bfloat16, 262144,
                  inplace=True)
    run_repost(job)

    # interleaving on one team: zc allreduce, staged (non-zc) gated
    # reduce_scatter, zc allreduce, alltoall, zc allreduce — ledger
    # continuity across kernel patterns on the shared counters
    count = 150_000
    req, src, dst = job.allreduce("inter_ar0", 200, torch.bfloat16, count)

    def repost(name, seed):
        cur = job.inputs(seed, torch.bfloat16, count)
        src.copy_(cur[rank])
        torch.cuda.synchronize()
        wait(req, ctx)
        torch.cuda.synchronize()
        job.check(dst, job.reference(cur, dtypes.OP_SUM))
        job.save(name, dst)
        job.done.append(name)

    per = 50_001
    rfull = job.inputs(201, torch.float32, per * world)
    rsrc = rfull[rank].clone().cuda()
    rdst = torch.zeros(per, device="cuda")
    rs = c.coll_init(team, "reduce_scatter", src=rsrc.data_ptr(),
                     dst=rdst.data_ptr(), count=per, dt=dtypes.FLOAT32,
                     mem_type=dtypes.MEM_CUDA)
    wait(rs, ctx)
    torch.cuda.synchronize()
    exp = job.reference(rfull, dtypes.OP_SUM)
    job.check(rdst, exp[rank * per:(rank + 1) * per])
    job.save("inter_rs_staged", rdst)
    job.done.append("inter_rs_staged")

    repost("inter_ar1", 202)

    afull = job.inputs(203, torch.float32, per * world)
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
    job.save("inter_a2a", adst)
    job.done.append("inter_a2a")

    repost("inter_ar2", 204)

    # zero-copy persistent reduce_scatter through the same kernel
    per = 70001
    zsrc = torch.zeros(per * world, device="cuda")
    zdst = torch.zeros(per, device="cuda")
    zrs = c.coll_init(team, "reduce_scatter", src=zsrc.data_ptr(),
                      dst=zdst.data_ptr(), count=per, dt=dtypes.FLOAT32,
                      mem_type=dtypes.MEM_CUDA, flags=c.FLAG_PERSISTENT)
    for it in range(3):
        zfull = job.inputs(300 + it, torch.float32, per * world)
        zsrc.copy_(zfull[rank])
        torch.cuda.synchronize()
        wait(zrs, ctx)
        torch.cuda.synchronize()
        exp = job.reference(zfull, dtypes.OP_SUM)
        job.check(zdst, exp[rank * per:(rank + 1) * per])
        job.save(f"rs_zc{it}", zdst)
    job.done.append("rs_zc")


def main():
    job = Job(sys.argv[1])
    if len(sys.argv) > 2 and sys.argv[2] == "repost":
        run_repost(job)
    else:
        run_all(job)
    job.finish("ZCF_OK")


if __name__ == "__main__":
    main()
