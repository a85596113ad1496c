"""Worker for tests/test_fused_vcolls_gpu.py: the fused one-kernel
allgatherv / reduce_scatterv / alltoallv of tl/cdna4
(UCC_TL_CDNA4_FUSED_COLLS=1), run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=N \
      --master-addr 127.0.0.1 tests/fused_vcolls_worker.py OUTDIR MODE

All ranks share cuda:0. The test sets UCC_TL_CDNA4_FUSED_COLLS_MAX=524288,
UCC_COLL_TRACE=1 and UCC_LOG_LEVEL=debug. With that bound an alltoallv cell
is (524288 - 16) / n rounded down to 16: 262128 bytes for 2 ranks, 174752
for 3.

MODE
  all   2 ranks: alltoallv matrices with a zero pair, 1, 7 and 999 element
        pairs and a pair of exactly one cell, in bf16, int32 and uint8;
        pointers one element past a 16-byte boundary; one pair of a cell
        plus one element (every rank falls back); persistent re-posts, fit
        and unfit; fit / unfit / fit between a fused allreduce and a fused
        alltoall; allgatherv and reduce_scatterv ragged, in place and not,
        at and over the bound; the MoE TokenExchanger round trip
  three 3 ranks: the same alltoallv cases with the oversized pair 0 -> 1,
        so that rank 2 sees fitting lengths only; allgatherv and
        reduce_scatterv without AVG
  trig  2 ranks: persistent allgatherv and reduce_scatterv through
        ee_create / triggered_post, three eager posts, then one capture in
        torch.cuda.graph replayed three times; an alltoallv triggered_post
  off   2 ranks, knob unset: one small request per type

Inputs are seeded small integers (fused_colls_worker.py's), so every
partial sum and every result is exact in the type; expectations are
computed on the host in int64 / float64 and compared bit for bit. Blocks
lie at permuted displacements with gaps; a dst is filled with a pad byte
before the collective and compared as a whole, so the gaps count, and sits
in a sentinel-banded allocation whose bands must survive.

Every rank writes to OUTDIR/req_rank<r>.txt
  FV_REQ <coll> <msgsize> <F|O>  per request of the three types: F if it
                                 must trace cdna4/fused, O if it must not
  FV_COLL <n>      posts that must log a k_fused_coll line
  FV_GRAPH <n>     posts that must log a k_fused_coll_graph line
  FV_A2AV <n>      posts that must log a k_fused_a2av line
  FV_FALLBACK <n>  of those, posts that must log the fallback line
"""

import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fused_colls_worker import (BF16, F32, I32, PAD, U8, Case, Ty,  # noqa: E402
                                fused_allreduce, ints, same)
from gated_rooted_worker import Banded  # noqa: E402
from zc_fused_worker import Job, wait  # noqa: E402

from ucc_amd import dtypes  # noqa: E402

BOUND = 524288
I64 = Ty("i64", torch.int64, dtypes.INT64, -64, 64,
         lambda x: x.to(torch.int64))
SRC_PAD = 0x11  # fill of the gaps of a source


def stride16(nbytes):
    return (nbytes + 15) // 16 * 16


def cell_bytes(world):
    return (BOUND - 16) // world // 16 * 16


def spread(counts, gap):
    """Element displacements of the blocks in reversed rank order, `gap`
    elements in front of each; and the extent."""
    dsp, off = [0] * len(counts), 0
    for r in reversed(range(len(counts))):
        off += gap
        dsp[r] = off
        off += counts[r]
    return dsp, off + gap


def block(seed, s, d, count, ty):
    """What rank s holds for rank d: `count` seeded integers (int32)."""
    return ints(seed * 64 + s * 8 + d, 1, count, ty)[0]


def note(job, coll, msgsize, fused):
    job.notes.append(f"FV_REQ {coll} {msgsize} {'F' if fused else 'O'}")


class VCase:
    """What the three types share. A subclass makes src (None in place),
    dst, req and tag; its fill() writes new inputs and sets exp, the whole
    dst as it must be afterwards, gaps included."""

    def check(self, tag):
        torch.cuda.synchronize()
        assert same(self.dst.buf, self.exp), (tag, "result")
        assert self.dst.bands_intact(), (tag, "dst bands")
        if self.src is not None:
            assert self.src.bands_intact(), (tag, "src bands")
            assert same(self.src.buf, self.src_before), (tag, "src changed")

    def padded_dst(self):
        self.dst.buf.view(torch.uint8).fill_(PAD)
        return self.dst.buf.clone()

    def run(self, seed, posts=1):
        for it in range(posts):
            self.fill(seed + 1000 * it)
            wait(self.req, self.job.ctx)
            self.check((self.tag, it))
        self.count_posts(posts)
        self.job.done.append(self.tag)


class A2av(VCase):
    """alltoallv of the element-count matrix m[s][d]."""

    def __init__(self, job, ty, m, mis=0, persistent=False):
        self.job, self.ty, self.m = job, ty, m
        w, r, es, c = job.world, job.rank, ty.es, job.c
        self.scnt = list(m[r])
        self.rcnt = [m[s][r] for s in range(w)]
        self.sdsp, sext = spread(self.scnt, 3)
        self.rdsp, rext = spread(self.rcnt, 5)
        self.src = Banded(sext * es, ty.tdt, mis)
        self.dst = Banded(rext * es, ty.tdt, mis)
        self.fits = max(max(row) for row in m) * es <= cell_bytes(w)
        self.tag = (f"alltoallv/{ty.name}/max{max(max(x) for x in m)}/"
                    f"mis{mis}/p{int(persistent)}")
        self.req = c.coll_init(
            job.team, "alltoallv", src=self.src.buf.data_ptr(),
            dst=self.dst.buf.data_ptr(), count=0, dt=ty.dt,
            mem_type=dtypes.MEM_CUDA,
            flags=c.FLAG_PERSISTENT if persistent else 0,
            src_counts=self.scnt, src_displs=self.sdsp,
            dst_counts=self.rcnt, dst_displs=self.rdsp)
        # selection never looks at the counts: fused whenever the knob is set
        note(job, "alltoallv", 0, job.knob)

    def fill(self, seed):
        job, ty = self.job, self.ty
        w, r = job.world, job.rank
        self.src.buf.view(torch.uint8).fill_(SRC_PAD)
        for d in range(w):
            o = self.sdsp[d]
            self.src.buf[o:o + self.scnt[d]].copy_(
                ty.enc(block(seed, r, d, self.scnt[d], ty)))
        self.exp = self.padded_dst()
        for s in range(w):
            o = self.rdsp[s]
            self.exp[o:o + self.rcnt[s]].copy_(
                ty.enc(block(seed, s, r, self.rcnt[s], ty)))
        self.src_before = self.src.buf.clone()
        torch.cuda.synchronize()

    def count_posts(self, posts):
        if self.job.knob:
            self.job.a2av += posts
            if not self.fits:
                self.job.fallback += posts


class Agv(VCase):
    def __init__(self, job, ty, counts, inplace=False, persistent=False,
                 fused=None):
        self.job, self.ty, self.counts, self.inplace = job, ty, counts, inplace
        r, es, c = job.rank, ty.es, job.c
        in_bound = stride16(max(counts) * es) <= BOUND
        if fused is None:
            fused = in_bound
        elif job.knob:
            assert fused == in_bound
        self.fused = fused
        self.dsp, ext = spread(counts, 3)
        self.dst = Banded(ext * es, ty.tdt)
        self.src = None if inplace else Banded(counts[r] * es, ty.tdt)
        flags = c.FLAG_PERSISTENT if persistent else 0
        if inplace:
            flags |= c.FLAG_IN_PLACE
        self.tag = f"allgatherv/{ty.name}/{counts}/ip{int(inplace)}"
        self.req = c.coll_init(
            job.team, "allgatherv",
            src=(self.src or self.dst).buf.data_ptr(),
            dst=self.dst.buf.data_ptr(), count=counts[r], dt=ty.dt,
            mem_type=dtypes.MEM_CUDA, flags=flags, dst_counts=counts,
            dst_displs=self.dsp)
        note(job, "allgatherv", sum(counts) * es, fused)

    def fill(self, seed):
        job, ty, counts = self.job, self.ty, self.counts
        r = job.rank
        self.exp = self.padded_dst()
        for s in range(job.world):
            o = self.dsp[s]
            self.exp[o:o + counts[s]].copy_(
                ty.enc(block(seed, s, 0, counts[s], ty)))
        mine = ty.enc(block(seed, r, 0, counts[r], ty))
        if self.inplace:
            o = self.dsp[r]
            self.dst.buf[o:o + counts[r]].copy_(mine)
        else:
            self.src.buf.copy_(mine)
            self.src_before = self.src.buf.clone()
        torch.cuda.synchronize()

    def count_posts(self, posts):
        if self.fused:
            self.job.fposts += posts


def vreduced(ty, full, op, world):
    """Reduction of the int32 rows of `full` on the host, int64 / float64,
    in the storage type."""
    wide = full.to(torch.int64)
    if op == dtypes.OP_SUM:
        return ty.enc(wide.sum(0))
    if op == dtypes.OP_MAX:
        return ty.enc(wide.max(0).values)
    # AVG of two ranks: x 0.5 is exact
    assert op == dtypes.OP_AVG and world == 2 and ty.tdt == torch.float32
    return (wide.sum(0).to(torch.float64) * 0.5).to(torch.float32)


class Rsv(VCase):
    def __init__(self, job, ty, counts, op=dtypes.OP_SUM, inplace=False,
                 persistent=False, fused=None):
        self.job, self.ty, self.counts = job, ty, counts
        self.op, self.inplace = op, inplace
        r, es, c = job.rank, ty.es, job.c
        in_bound = sum(stride16(x * es) for x in counts) <= BOUND
        if fused is None:
            fused = in_bound
        elif job.knob:
            assert fused == in_bound
        self.fused = fused
        self.off = [sum(counts[:k]) for k in range(len(counts))]
        total = sum(counts)
        self.dst = Banded((total if inplace else counts[r]) * es, ty.tdt)
        self.src = None if inplace else Banded(total * es, ty.tdt)
        flags = c.FLAG_PERSISTENT if persistent else 0
        if inplace:
            flags |= c.FLAG_IN_PLACE
        self.tag = f"reduce_scatterv/{ty.name}/{counts}/op{op}/ip{int(inplace)}"
        self.req = c.coll_init(
            job.team, "reduce_scatterv",
            src=(self.src or self.dst).buf.data_ptr(),
            dst=self.dst.buf.data_ptr(), count=total, dt=ty.dt, op=op,
            mem_type=dtypes.MEM_CUDA, flags=flags, dst_counts=counts,
            dst_displs=self.off)
        note(job, "reduce_scatterv", total * es, fused)

    def fill(self, seed):
        job, ty, counts = self.job, self.ty, self.counts
        w, r = job.world, job.rank
        full = ints(seed, w, sum(counts), ty)
        mine = ty.enc(full[r])
        lo, hi = self.off[r], self.off[r] + counts[r]
        red = vreduced(ty, full[:, lo:hi], self.op, w)
        if self.inplace:
            self.dst.buf.copy_(mine)
            self.exp = mine.clone()
            self.exp[lo:hi] = red
        else:
            self.padded_dst()
            self.src.buf.copy_(mine)
            self.src_before = self.src.buf.clone()
            self.exp = red
        torch.cuda.synchronize()

    def count_posts(self, posts):
        if self.fused:
            self.job.fposts += posts


def a2av_matrices(world, ty):
    """Fitting matrices: a zero pair, 1, 7 and 999 elements, and one pair
    of exactly one cell."""
    cell = cell_bytes(world) // ty.es
    if world == 2:
        return ([[0, 1], [7, 999]], [[cell, 7], [999, 0]])
    return ([[0, 1, 7], [999, cell, 5], [3, 0, 2]],)


def a2av_unfit(world, ty):
    """One pair, 0 -> 1, of a cell plus one element; with 3 ranks rank 2's
    row and column fit."""
    over = cell_bytes(world) // ty.es + 1
    if world == 2:
        return [[7, over], [999, 1]]
    return [[7, over, 1], [5, 0, 3], [2, 999, 4]]


def run_a2av(job, seed):
    w = job.world
    for ty in (BF16, I32, U8):
        for m in a2av_matrices(w, ty):
            seed += 1
            A2av(job, ty, m).run(seed)
        seed += 1
        A2av(job, ty, a2av_matrices(w, ty)[0], mis=ty.es).run(seed)
    # one pair over the cell: every rank falls back, the result is right
    for ty in (BF16, U8):
        seed += 1
        A2av(job, ty, a2av_unfit(w, ty)).run(seed)
    seed += 1
    A2av(job, BF16, a2av_unfit(w, BF16), mis=2).run(seed)
    # persistent: a vote at every post, the inner task kept across re-posts
    seed += 1
    A2av(job, BF16, a2av_matrices(w, BF16)[0], persistent=True).run(
        seed, posts=4)
    seed += 1
    A2av(job, BF16, a2av_unfit(w, BF16), persistent=True).run(seed, posts=2)
    # fit / unfit / fit between a fused allreduce and a fused alltoall: all
    # of them on the one slot sequence
    fit, unfit = a2av_matrices(w, I32)[0], a2av_unfit(w, I32)
    for rnd in range(2):
        seed += 10
        fused_allreduce(job, seed, 999)
        A2av(job, I32, fit).run(seed + 1)
        Case(job, "alltoall", BF16, 999).run(seed + 2)
        A2av(job, I32, unfit).run(seed + 3)
        fused_allreduce(job, seed + 4, 999)
        A2av(job, I32, fit).run(seed + 5)
    return seed


def run_agv_rsv(job, seed, avg):
    w = job.world
    raggeds = (([0, 999], [1, 75_001]) if w == 2
               else ([0, 1, 999], [75_001, 13, 7]))
    for ip in (False, True):
        for ty in (BF16, U8):
            for ragged in raggeds:
                seed += 1
                Agv(job, ty, ragged, inplace=ip).run(seed)
    seed += 1
    Agv(job, BF16, [999, 0, 1][:w], persistent=True).run(seed, posts=3)
    # the largest block decides: one element over the bound is not fused
    at = BOUND // 2
    seed += 1
    Agv(job, BF16, [at] + [7] * (w - 1)).run(seed)
    seed += 1
    Agv(job, BF16, [7] * (w - 1) + [at + 1], fused=False).run(seed)
    ops = [(I32, dtypes.OP_SUM), (I64, dtypes.OP_MAX), (BF16, dtypes.OP_SUM)]
    if avg:
        ops.append((F32, dtypes.OP_AVG))
    rag = [999, 0, 40_001] if w > 2 else [40_001, 0]
    for ip in (False, True):
        for ty, op in ops:
            seed += 1
            Rsv(job, ty, rag, op=op, inplace=ip).run(seed)
            seed += 1
            Rsv(job, ty, [7, 1, 999][:w], op=op, inplace=ip).run(seed)
    seed += 1
    Rsv(job, BF16, [1, 999, 0][:w], persistent=True).run(seed, posts=3)
    # the sum of the 16-byte strides decides: w blocks that fill the bound
    # to within 16 bytes per block, then 16 bytes more in each
    per = BOUND // w // 16 * 16 // 2
    seed += 1
    Rsv(job, BF16, [per] * w, fused=True).run(seed)
    seed += 1
    Rsv(job, BF16, [per + 8] * w, fused=False).run(seed)
    return seed


class _Comm:
    """What ucc_amd.parallel.moe.TokenExchanger needs of a Communicator."""

    def __init__(self, job):
        self.c, self.team, self.world, self.job = (job.c, job.team,
                                                   job.world, job)

    def _wait(self, req):
        wait(req, self.job.ctx)


def run_moe(job, seed):
    """One dispatch + combine round trip on CUDA tensors, skewed counts."""
    from ucc_amd.parallel.moe import TokenExchanger

    hidden, ty = 64, BF16
    send = [[1, 37], [20, 0]]  # send[s][d] rows
    r = job.rank
    recv = [send[s][r] for s in range(job.world)]
    rows = {(s, d): ty.enc(block(seed, s, d, send[s][d] * hidden, ty))
            .reshape(-1, hidden) for s in range(2) for d in range(2)}
    tokens = torch.cat([rows[(r, d)] for d in range(2)]).cuda()
    ex = TokenExchanger(_Comm(job))
    got, rc = ex.dispatch(tokens, send[r], recv)
    torch.cuda.synchronize()
    assert rc == recv
    assert same(got, torch.cat([rows[(s, r)] for s in range(2)])), "dispatch"
    back = ex.combine(got, recv, send[r])
    torch.cuda.synchronize()
    assert same(back, tokens), "combine"
    for _ in range(2):
        note(job, "alltoallv", 0, True)
    job.a2av += 2
    job.done.append("moe")


def run_all(job):
    seed = run_a2av(job, 100)
    seed = run_agv_rsv(job, seed, avg=True)
    run_moe(job, seed + 1)


def run_three(job):
    seed = run_a2av(job, 400)
    run_agv_rsv(job, seed, avg=False)


def run_trig(job):
    """Persistent allgatherv and reduce_scatterv: three eager triggered
    posts, then one captured post replayed three times, new data every
    time (fused_colls_worker.run_trig's scheme). An alltoallv cannot be
    captured, a graph cannot fall back: its triggered post goes to the task
    the request has with the knob unset, and that declines it; nothing
    is launched and dst stays as it was."""
    c = job.c
    s = torch.cuda.Stream()
    ee = c.ee_create(job.team, s.cuda_stream)
    seed = 700
    for make in (lambda: Agv(job, BF16, [999, 40_001], persistent=True),
                 lambda: Agv(job, U8, [7, 0], inplace=True, persistent=True),
                 lambda: Rsv(job, I32, [40_001, 999], persistent=True),
                 lambda: Rsv(job, BF16, [0, 999], inplace=True,
                             persistent=True)):
        case = make()
        for it in range(3):
            seed += 1
            case.fill(seed)
            dist.barrier()
            c.triggered_post(ee, case.req)
            s.synchronize()
            case.check((case.tag, "eager", it))
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
            case.check((case.tag, "replay", it))
        job.graph += 4
        job.done.append("trig " + case.tag)
        dist.barrier()
        del g
        del case.req
        del case
    a2a = A2av(job, BF16, a2av_matrices(2, BF16)[0], persistent=True)
    a2a.fill(seed + 1)
    a2a.exp = a2a.padded_dst()
    torch.cuda.synchronize()
    dist.barrier()
    try:
        c.triggered_post(ee, a2a.req)
        raised = False
    except RuntimeError:
        raised = True
    s.synchronize()
    assert raised, "alltoallv triggered_post must be declined"
    a2a.check((a2a.tag, "triggered"))
    job.done.append("trig alltoallv")
    dist.barrier()
    del a2a
    c.ee_destroy(ee)


def run_off(job):
    A2av(job, BF16, [[0, 1], [7, 999]]).run(900)
    Agv(job, BF16, [999, 7], fused=False).run(901)
    Rsv(job, BF16, [999, 7], fused=False).run(902)


def main():
    job = Job(sys.argv[1])
    job.fposts = job.graph = job.a2av = job.fallback = 0
    job.notes = []
    job.knob = os.environ.get("UCC_TL_CDNA4_FUSED_COLLS", "0") == "1"
    {"all": run_all, "three": run_three, "trig": run_trig,
     "off": run_off}[sys.argv[2]](job)
    job.notes += [f"FV_COLL {job.fposts}", f"FV_GRAPH {job.graph}",
                  f"FV_A2AV {job.a2av}", f"FV_FALLBACK {job.fallback}"]
    with open(os.path.join(job.outdir, f"req_rank{job.rank}.txt"), "w") as f:
        f.write("\n".join(job.notes) + "\n")
    job.finish("FV_OK")


if __name__ == "__main__":
    main()
