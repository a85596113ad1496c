"""Worker for tests/test_fused_colls_gpu.py: the fused one-kernel
allgather / reduce_scatter / alltoall / bcast / reduce of tl/cdna4
(UCC_TL_CDNA4_FUSED_COLLS=1), run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=N \
      --master-addr 127.0.0.1 tests/fused_colls_worker.py OUTDIR MODE

All ranks share cuda:0. The test sets UCC_TL_CDNA4_FUSED_COLLS_MAX=524288,
UCC_COLL_TRACE=1 and UCC_LOG_LEVEL=debug.

MODE
  all   2 ranks: every shape and case below, roots 0 and 1, misaligned
        pointers on rank 1, persistent re-posts over the slot wrap, the
        interleave with other algorithms and the requests at and over the
        bound
  three 3 ranks, roots 1 and 2, SUM and AVG, persistent re-posts
  trig  2 ranks: per type a persistent request through ee_create /
        triggered_post, three eager posts, then one capture in
        torch.cuda.graph replayed three times
  off   2 ranks, knob unset: one small request per type

Inputs are seeded small integers (|x| <= 2 for fp8, <= 64 otherwise), so
every f32 partial sum and every stored value is exact and the expected
bytes follow from torch integer arithmetic; every comparison is bitwise.
AVG follows the documented rule: f32 sum x f32(1/n computed in double),
one round-to-nearest-even store. Every user buffer sits in a
sentinel-banded allocation and the bands must survive.

For every request of the five types a rank writes a line
`FC_REQ <coll> <msgsize> <F|O>` to OUTDIR/req_rank<r>.txt: F if the request
is within the bound and must trace cdna4/fused, O if it must not.
`FC_POSTS <n>` there is the number of posts of F requests.
"""

import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from gated_rooted_worker import FILL, Banded, raw  # noqa: E402
from zc_fused_worker import Job, wait  # noqa: E402

from ucc_amd import dtypes  # noqa: E402

BOUND = 524288
PAD = 0x3C  # fill of a dst before the collective

# OCP e4m3 bit patterns of the integers -6..6 (bias 7, 3 mantissa bits)
_E4M3_POS = [0x00, 0x38, 0x40, 0x44, 0x48, 0x4A, 0x4C]
_E4M3_LUT = torch.tensor([0x80 | v for v in _E4M3_POS[:0:-1]] + _E4M3_POS,
                         dtype=torch.uint8)


class Ty:
    def __init__(self, name, tdt, dt, lo, hi, enc):
        self.name, self.tdt, self.dt, self.lo, self.hi = name, tdt, dt, lo, hi
        self.enc = enc  # int32 tensor -> tensor of the storage type
        self.es = torch.empty(0, dtype=tdt).element_size()


U8 = Ty("u8", torch.uint8, dtypes.UINT8, 0, 64,
        lambda x: x.to(torch.uint8))
BF16 = Ty("bf16", torch.bfloat16, dtypes.BFLOAT16, -64, 64,
          lambda x: x.to(torch.float32).to(torch.bfloat16))
F32 = Ty("f32", torch.float32, dtypes.FLOAT32, -64, 64,
         lambda x: x.to(torch.float32))
I32 = Ty("i32", torch.int32, dtypes.INT32, -64, 64,
         lambda x: x.to(torch.int32))
E4M3 = Ty("e4m3", torch.uint8, dtypes.FLOAT8_E4M3, -2, 2,
          lambda x: _E4M3_LUT[(x + 6).long()])

COLLS = ("allgather", "reduce_scatter", "alltoall", "bcast", "reduce")
ROOTED = ("bcast", "reduce")
REDUCING = ("reduce_scatter", "reduce")


def nposts():
    return 2 * int(os.environ.get("UCC_TL_CDNA4_MAX_CONCURRENT", "4")) + 1


def ints(seed, world, count, ty):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(ty.lo, ty.hi + 1, (world, count), generator=g,
                         dtype=torch.int32)


def reduced(ty, full, op, world):
    """Expected reduction of the rows of `full`, in the storage type."""
    if op == dtypes.OP_SUM:
        return ty.enc(full.sum(0, dtype=torch.int32))
    if op == dtypes.OP_MIN:
        return ty.enc(full.min(0).values)
    assert op == dtypes.OP_AVG and ty.tdt in (torch.bfloat16, torch.float32)
    s = full.sum(0, dtype=torch.int32).to(torch.float32)
    alpha = torch.tensor(1.0 / world, dtype=torch.float64).to(torch.float32)
    return (s * alpha).to(ty.tdt)


def in_bound(job, coll, block_bytes):
    """The documented bound: the scratch of a request, one cell for
    allgather, bcast and reduce and one per rank for reduce_scatter and
    alltoall, each rounded up to 16 bytes, is at most FUSED_COLLS_MAX."""
    cells = job.world if coll in ("reduce_scatter", "alltoall") else 1
    return cells * ((block_bytes + 15) // 16 * 16) <= BOUND


def same(t, exp):
    return np.array_equal(raw(t), raw(exp))


class Case:
    """One request of `coll` with `per` elements per block (the vector for
    bcast and reduce), its buffers, and how to fill and check them."""

    def __init__(self, job, coll, ty, per, root=0, op=dtypes.OP_SUM,
                 inplace=False, mis=0, persistent=False, fused=None):
        self.job, self.coll, self.ty, self.per = job, coll, ty, per
        self.root, self.op, self.inplace = root, op, inplace
        if fused is None:
            fused = in_bound(job, coll, per * ty.es)
        elif job.knob:
            assert fused == in_bound(job, coll, per * ty.es)
        self.fused = fused
        c, w, es = job.c, job.world, ty.es
        self.is_root = job.rank == root
        self.src = self.dst = None
        vec = per * w
        flags = c.FLAG_PERSISTENT if persistent else 0
        if inplace:
            flags |= c.FLAG_IN_PLACE
        if coll == "allgather":
            self.dst = Banded(vec * es, ty.tdt, mis)
            if not inplace:
                self.src = Banded(per * es, ty.tdt, mis)
            count = vec
        elif coll == "reduce_scatter":
            self.dst = Banded((vec if inplace else per) * es, ty.tdt, mis)
            if not inplace:
                self.src = Banded(vec * es, ty.tdt, mis)
            count = vec if inplace else per
        elif coll == "alltoall":
            self.src = Banded(vec * es, ty.tdt, mis)
            self.dst = Banded(vec * es, ty.tdt, mis)
            count = vec
        elif coll == "bcast":
            self.dst = Banded(per * es, ty.tdt, mis)
            count = per
        else:
            self.dst = Banded(per * es, ty.tdt, mis)
            if not (inplace and self.is_root):
                self.src = Banded(per * es, ty.tdt, mis)
            count = per
        sp = (self.src or self.dst).buf.data_ptr()
        self.req = c.coll_init(job.team, coll, src=sp,
                               dst=self.dst.buf.data_ptr(), count=count,
                               dt=ty.dt, op=op, mem_type=dtypes.MEM_CUDA,
                               root=root, flags=flags)
        job.notes.append(
            f"FC_REQ {coll} {count * es} {'F' if fused else 'O'}")

    def fill(self, seed):
        """New inputs; returns what check() compares with."""
        job, ty, per, coll = self.job, self.ty, self.per, self.coll
        w, r = job.world, job.rank
        pad = lambda b: b.buf.view(torch.uint8).fill_(PAD)  # noqa: E731
        if coll == "allgather":
            full = ints(seed, w, per, ty)
            pad(self.dst)
            mine = ty.enc(full[r])
            if self.inplace:
                self.dst.buf[r * per:(r + 1) * per].copy_(mine)
            else:
                self.src.buf.copy_(mine)
            self.exp = ty.enc(full).reshape(-1)
        elif coll == "alltoall":
            full = ints(seed, w, per * w, ty)
            pad(self.dst)
            self.src.buf.copy_(ty.enc(full[r]))
            self.exp = ty.enc(torch.cat(
                [full[s][r * per:(r + 1) * per] for s in range(w)]))
        elif coll == "reduce_scatter":
            full = ints(seed, w, per * w, ty)
            mine = ty.enc(full[r])
            red = reduced(ty, full, self.op, w)[r * per:(r + 1) * per]
            if self.inplace:
                self.dst.buf.copy_(mine)
                self.exp = mine.clone()
                self.exp[r * per:(r + 1) * per] = red
            else:
                pad(self.dst)
                self.src.buf.copy_(mine)
                self.exp = red
        elif coll == "bcast":
            full = ints(seed, w, per, ty)
            if self.is_root:
                self.dst.buf.copy_(ty.enc(full[self.root]))
            else:
                pad(self.dst)
            self.exp = ty.enc(full[self.root])
        else:
            full = ints(seed, w, per, ty)
            mine = ty.enc(full[r])
            if self.src is None:
                self.dst.buf.copy_(mine)
            else:
                self.src.buf.copy_(mine)
                # a non-root's dst keeps the allocation's sentinel fill
                self.dst.buf.view(torch.uint8).fill_(FILL)
            self.exp = reduced(ty, full, self.op, w) if self.is_root else None
        self.src_before = None if self.src is None else self.src.buf.clone()
        torch.cuda.synchronize()

    def check(self, tag):
        torch.cuda.synchronize()
        if self.exp is None:
            assert bool((self.dst.big == FILL).all()), (tag, "non-root dst")
        else:
            assert same(self.dst.buf, self.exp), (tag, "result")
        assert self.dst.bands_intact(), (tag, "dst bands")
        if self.src is not None:
            assert self.src.bands_intact(), (tag, "src bands")
            assert same(self.src.buf, self.src_before), (tag, "src changed")

    def run(self, seed, posts=1):
        tag = (f"{self.coll}/{self.ty.name}x{self.per}/root{self.root}/"
               f"op{self.op}/ip{int(self.inplace)}")
        for it in range(posts):
            self.fill(seed + 1000 * it)
            wait(self.req, self.job.ctx)
            self.check((tag, it))
        if self.fused:
            self.job.fposts += posts
        self.job.done.append(tag)


def roots(job, coll, all_roots=None):
    if coll not in ROOTED:
        return (0,)
    return all_roots if all_roots is not None else tuple(range(job.world))


def fused_allreduce(job, seed, count):
    """A small bf16 allreduce: the fused allreduce kernel on the same slot
    sequence."""
    c = job.c
    full = ints(seed, job.world, count, BF16)
    src = BF16.enc(full[job.rank]).cuda()
    dst = torch.zeros(count, dtype=torch.bfloat16, device="cuda")
    req = c.coll_init(job.team, "allreduce", src=src.data_ptr(),
                      dst=dst.data_ptr(), count=count, dt=dtypes.BFLOAT16,
                      op=dtypes.OP_SUM, mem_type=dtypes.MEM_CUDA)
    torch.cuda.synchronize()
    wait(req, job.ctx)
    torch.cuda.synchronize()
    assert same(dst, reduced(BF16, full, dtypes.OP_SUM, job.world))
    job.done.append("allreduce")


def staged_gather(job, seed, per, root):
    c = job.c
    full = ints(seed, job.world, per, F32)
    src = F32.enc(full[job.rank]).cuda()
    dst = torch.zeros(per * job.world, device="cuda")
    count = per * job.world if job.rank == root else per
    req = c.coll_init(job.team, "gather", src=src.data_ptr(),
                      dst=dst.data_ptr(), count=count, dt=dtypes.FLOAT32,
                      mem_type=dtypes.MEM_CUDA, root=root)
    torch.cuda.synchronize()
    wait(req, job.ctx)
    torch.cuda.synchronize()
    if job.rank == root:
        assert same(dst, F32.enc(full).reshape(-1))
    job.done.append("gather")


def at_bound(job, coll):
    """bf16 elements per block of a request whose scratch is exactly the
    bound."""
    cells = job.world if coll in ("reduce_scatter", "alltoall") else 1
    return BOUND // cells // 2


# per-rank block shapes: the smallest block, exactly one pack, a scalar
# tail with an odd cell length, and about 300 KB (3 blocks, tail). With one
# cell per rank the fp32 shape of reduce_scatter and alltoall is over the
# 512 KiB bound (it must then trace another algorithm and still be right),
# so those two also run the same count in bf16, which is within it.
SHAPES = ((U8, 1), (BF16, 8), (BF16, 999), (F32, 75_001))


def run_all(job):
    seed = 100
    # ---- copy collectives, all four shapes
    for coll in ("allgather", "alltoall", "bcast"):
        for ty, per in SHAPES + (((BF16, 75_001),) if coll == "alltoall"
                                 else ()):
            for root in roots(job, coll):
                seed += 1
                Case(job, coll, ty, per, root).run(seed)
    # ---- reductions, the last three sizes
    red = ((BF16, dtypes.OP_SUM), (BF16, dtypes.OP_AVG), (I32, dtypes.OP_SUM),
           (F32, dtypes.OP_MIN), (E4M3, dtypes.OP_SUM))
    for coll in REDUCING:
        for ty, op in red:
            for per in (8, 999, 75_001):
                for root in roots(job, coll):
                    seed += 1
                    Case(job, coll, ty, per, root, op=op).run(seed)
    # ---- in place
    for per in (999, 75_001):
        seed += 1
        Case(job, "allgather", BF16, per, inplace=True).run(seed)
        seed += 1
        Case(job, "reduce_scatter", BF16, per, inplace=True).run(seed)
        for root in (0, 1):
            seed += 1
            Case(job, "reduce", BF16, per, root, inplace=True).run(seed)
    # ---- rank 1's src and dst 2 bytes past a 16-byte boundary
    mis = 2 if job.rank == 1 else 0
    for coll in COLLS:
        for root in roots(job, coll):
            seed += 1
            Case(job, coll, BF16, 999, root, mis=mis).run(seed)
    seed += 1
    Case(job, "reduce_scatter", BF16, 999, op=dtypes.OP_AVG,
         mis=mis).run(seed)
    # ---- one persistent request per type over the slot wrap
    for coll in COLLS:
        seed += 1
        Case(job, coll, BF16, 999, root=1 if coll in ROOTED else 0,
             persistent=True).run(seed, posts=nposts())
    # ---- interleave with the other algorithms on the one team
    for rnd in range(2):
        seed += 10
        fused_allreduce(job, seed, 999)
        Case(job, "allgather", BF16, 999).run(seed + 1)
        Case(job, "allgather", BF16, at_bound(job, "allgather") + 1,
             fused=False).run(seed + 2)
        Case(job, "bcast", BF16, 999, root=rnd).run(seed + 3)
        staged_gather(job, seed + 4, 999, root=rnd)
        Case(job, "reduce_scatter", BF16, 999).run(seed + 5)
        Case(job, "alltoall", BF16, at_bound(job, "alltoall") + 1,
             fused=False).run(seed + 6)
        Case(job, "reduce", BF16, 999, root=1 - rnd).run(seed + 7)
    # ---- exactly at the bound, and one element over it
    for coll in COLLS:
        per = at_bound(job, coll)
        seed += 2
        Case(job, coll, BF16, per, root=1).run(seed)
        Case(job, coll, BF16, per + 1, root=1, fused=False).run(seed + 1)


def run_three(job):
    seed = 500
    for coll in COLLS:
        for root in roots(job, coll, (1, 2)):
            for ty, per in ((BF16, 999), (F32, 75_001)) + (
                    () if coll in ROOTED + ("allgather",)
                    else ((BF16, 75_001),)):
                ops = ((dtypes.OP_SUM, dtypes.OP_AVG) if coll in REDUCING
                       else (dtypes.OP_SUM,))
                for op in ops:
                    seed += 1
                    Case(job, coll, ty, per, root, op=op).run(seed)
    for coll in COLLS:
        seed += 1
        Case(job, coll, BF16, 999, root=2 if coll in ROOTED else 0,
             op=dtypes.OP_AVG if coll in REDUCING else dtypes.OP_SUM,
             persistent=True).run(seed, posts=nposts())


def run_trig(job):
    """Per type and size: three eager triggered posts, then one captured
    post replayed three times, new data every time. Six iterations of the
    device-derived counter cover both staging parities. The request is
    finalised before the next one takes the persistent slot."""
    c = job.c
    s = torch.cuda.Stream()
    ee = c.ee_create(job.team, s.cuda_stream)
    seed = 700
    for coll in COLLS:
        for ty, per in ((BF16, 999), (F32, 40_001)):
            case = Case(job, coll, ty, per, root=1, persistent=True)
            tag = f"trig {coll} {ty.name}x{per}"
            for it in range(3):
                seed += 1
                case.fill(seed)
                dist.barrier()
                c.triggered_post(ee, case.req)
                s.synchronize()
                case.check((tag, "eager", it))
            g = torch.cuda.CUDAGraph()
            dist.barrier()
            with torch.cuda.graph(g, stream=s):
                c.triggered_post(ee, case.req)
            dist.barrier()
            for it in range(3):
                seed += 1
                case.fill(seed)
                dist.barrier()
                g.replay()
                torch.cuda.synchronize()
                case.check((tag, "replay", it))
            job.fposts += 4
            job.done.append(tag)
            dist.barrier()
            del g
            del case.req
            del case
    dist.barrier()
    c.ee_destroy(ee)


def run_off(job):
    seed = 900
    for coll in COLLS:
        seed += 1
        Case(job, coll, BF16, 999, root=1, fused=False).run(seed)


def main():
    job = Job(sys.argv[1])
    job.fposts = 0
    job.notes = []
    job.knob = os.environ.get("UCC_TL_CDNA4_FUSED_COLLS", "0") == "1"
    {"all": run_all, "three": run_three, "trig": run_trig,
     "off": run_off}[sys.argv[2]](job)
    job.notes.append(f"FC_POSTS {job.fposts}")
    with open(os.path.join(job.outdir, f"req_rank{job.rank}.txt"), "w") as f:
        f.write("\n".join(job.notes) + "\n")
    job.finish("FC_OK")


if __name__ == "__main__":
    main()
