"""Worker for tests/test_fused_gs_gpu.py: the fused one-kernel gather /
scatter / gatherv / scatterv of tl/cdna4
(UCC_TL_CDNA4_FUSED_GATHER_SCATTER=1), run under
  python -m torch.distributed.run --nnodes=1 --nproc-per-node=N \
      --master-addr 127.0.0.1 tests/fused_gs_worker.py OUTDIR MODE

All ranks share cuda:0. The test sets UCC_TL_CDNA4_FUSED_COLLS_MAX=524288,
UCC_COLL_TRACE=1 and UCC_LOG_LEVEL=debug. With that bound a gather is fused
up to a 524288-byte block, a scatter up to n blocks of that sum (each rounded
up to 16), and B, the bound of gatherv (largest block) and scatterv (sum of
the rounded blocks), is 524288 - 144 = 524144 bytes.

MODE
  all   2 ranks, every root: gather and scatter of (u8, 1), (bf16, 8),
        (bf16, 999) and (bf16, 75 001); rank 1's buffers 2 bytes past a
        16-byte boundary; in place at the root; exactly at the bound and one
        element over; one persistent request per type over the slot wrap;
        the interleave with a fused allreduce and staged requests; gatherv
        and scatterv with a zero count, 1, 7, 999 and 75 001 elements at
        permuted displacements with gaps, in place and not; a request that
        fits exactly; a single block over B (every rank falls back)
  three 3 ranks, roots 1 and 2: the same kinds, fewer shapes; the oversized
        block lies on rank 1, so rank 2's own count is small
  trig  2 ranks: persistent gather and scatter through ee_create /
        triggered_post, three eager posts, then one capture in
        torch.cuda.graph replayed three times; a gatherv triggered_post
  off   2 ranks, knob unset: one small request per type

Inputs are seeded small integers (fused_colls_worker.py's) and every
comparison is bitwise. A dst is filled with a pad byte before the collective
and compared as a whole, so the gaps between displaced blocks count; it sits
in a sentinel-banded allocation whose bands must survive. A non-root of
gather(v) passes a dst of its own, which must keep the sentinel.

Every rank writes to OUTDIR/req_rank<r>.txt
  FG_REQ <coll> <msgsize> <F|O>  per request of the four types: F if it must
                                 trace cdna4/fused, O if it must not
  FG_COLL <n>      posts that must log a k_fused_coll line
  FG_GRAPH <n>     posts that must log a k_fused_coll_graph line
  FG_ROOTED <n>    posts that must log a k_fused_rooted_v line
  FG_FALLBACK <n>  of those, posts that must log the fallback line
"""

import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from fused_colls_worker import (BF16, PAD, U8, fused_allreduce,  # noqa: E402
                                ints, nposts, same)
from fused_vcolls_worker import SRC_PAD, block, spread, stride16  # noqa: E402
from gated_rooted_worker import FILL, Banded  # noqa: E402
from zc_fused_worker import Job, wait  # noqa: E402

from ucc_amd import dtypes  # noqa: E402

BOUND = 524288
HDR = 144
B = (BOUND - HDR) // 16 * 16


def note(job, coll, msgsize, fused):
    job.notes.append(f"FG_REQ {coll} {msgsize} {'F' if fused else 'O'}")


def in_bound(job, coll, block_bytes):
    cells = job.world if coll == "scatter" else 1
    return cells * stride16(block_bytes) <= BOUND


def at_bound(job, coll):
    """bf16 elements per block of the largest request that is fused."""
    cells = job.world if coll == "scatter" else 1
    return BOUND // cells // 16 * 16 // 2


class RootedCase:
    """What the four types share. A subclass makes src and dst (None where a
    side is not significant), req and tag; its fill() writes new inputs and
    sets exp: the whole dst as it must be afterwards, or None where dst must
    keep the sentinel."""

    def check(self, tag):
        torch.cuda.synchronize()
        if self.dst is not None:
            if self.exp is None:
                assert bool((self.dst.big == FILL).all()), (tag, "idle dst")
            else:
                assert same(self.dst.buf, self.exp), (tag, "result")
            assert self.dst.bands_intact(), (tag, "dst bands")
        if self.src is not None:
            assert self.src.bands_intact(), (tag, "src bands")
            assert same(self.src.buf, self.src_before), (tag, "src changed")

    def padded_dst(self):
        self.dst.buf.view(torch.uint8).fill_(PAD)
        return self.dst.buf.clone()

    def ptr(self, banded):
        return 0 if banded is None else banded.buf.data_ptr()

    def run(self, seed, posts=1):
        for it in range(posts):
            self.fill(seed + 1000 * it)
            wait(self.req, self.job.ctx)
            self.check((self.tag, it))
        self.count_posts(posts)
        self.job.done.append(self.tag)


class GS(RootedCase):
    """gather or scatter of `per` elements per rank."""

    def __init__(self, job, coll, ty, per, root=0, inplace=False, mis=0,
                 persistent=False, fused=None):
        self.job, self.coll, self.ty, self.per = job, coll, ty, per
        self.root, self.inplace = root, inplace
        ok = in_bound(job, coll, per * ty.es)
        if fused is None:
            fused = ok
        elif job.knob:
            assert fused == ok
        self.fused = fused
        c, w, es = job.c, job.world, ty.es
        self.is_root = job.rank == root
        whole = lambda: Banded(per * w * es, ty.tdt, mis)  # noqa: E731
        part = lambda: Banded(per * es, ty.tdt, mis)  # noqa: E731
        ip = inplace and self.is_root
        if coll == "gather":
            self.src = None if ip else part()
            # a non-root's dst is not significant: it must stay as it is
            self.dst = whole() if self.is_root else Banded(32)
        else:
            self.src = whole() if self.is_root else None
            self.dst = None if ip else part()
        flags = c.FLAG_PERSISTENT if persistent else 0
        if ip:
            flags |= c.FLAG_IN_PLACE
        self.tag = (f"{coll}/{ty.name}x{per}/root{root}/ip{int(inplace)}/"
                    f"mis{mis}/p{int(persistent)}")
        self.req = c.coll_init(
            job.team, coll, src=self.ptr(self.src), dst=self.ptr(self.dst),
            count=per * w if self.is_root else per, dt=ty.dt,
            mem_type=dtypes.MEM_CUDA, root=root, flags=flags)
        note(job, coll, per * w * es, fused)

    def fill(self, seed):
        job, ty, per = self.job, self.ty, self.per
        w, r = job.world, job.rank
        full = ints(seed, w, per, ty)
        ip = self.inplace and self.is_root
        if self.coll == "gather":
            self.exp = None
            if self.is_root:
                self.padded_dst()
                self.exp = ty.enc(full).reshape(-1).cuda()
                if ip:
                    self.dst.buf[r * per:(r + 1) * per].copy_(ty.enc(full[r]))
            if not ip:
                self.src.buf.copy_(ty.enc(full[r]))
        else:
            if self.is_root:
                self.src.buf.copy_(ty.enc(full).reshape(-1))
            if not ip:
                self.padded_dst()
                self.exp = ty.enc(full[r]).cuda()
        self.src_before = None if self.src is None else self.src.buf.clone()
        torch.cuda.synchronize()

    def count_posts(self, posts):
        if self.fused:
            self.job.fposts += posts


class GSv(RootedCase):
    """gatherv or scatterv of counts[r] elements for rank r, at permuted
    displacements with gaps in the root's buffer. Counts and displacements
    are passed at the root only."""

    def __init__(self, job, coll, ty, counts, root=0, inplace=False,
                 persistent=False):
        self.job, self.coll, self.ty, self.counts = job, coll, ty, counts
        self.root, self.inplace = root, inplace
        c, r, es = job.c, job.rank, ty.es
        assert len(counts) == job.world
        self.is_root = r == root
        if coll == "gatherv":
            self.fits = max(counts) * es <= B
        else:
            self.fits = sum(stride16(x * es) for x in counts) <= B
        self.dsp, ext = spread(counts, 3)
        ip = inplace and self.is_root
        whole = lambda: Banded(ext * es, ty.tdt)  # noqa: E731
        part = lambda: Banded(counts[r] * es, ty.tdt)  # noqa: E731
        if coll == "gatherv":
            self.src = None if ip else part()
            self.dst = whole() if self.is_root else Banded(32)
        else:
            self.src = whole() if self.is_root else None
            self.dst = None if ip else part()
        flags = c.FLAG_PERSISTENT if persistent else 0
        if ip:
            flags |= c.FLAG_IN_PLACE
        v = {}
        if self.is_root:
            side = "dst" if coll == "gatherv" else "src"
            v = {side + "_counts": counts, side + "_displs": self.dsp}
        self.tag = (f"{coll}/{ty.name}/{counts}/root{root}/ip{int(inplace)}/"
                    f"p{int(persistent)}")
        self.req = c.coll_init(
            job.team, coll, src=self.ptr(self.src), dst=self.ptr(self.dst),
            count=counts[r], dt=ty.dt, mem_type=dtypes.MEM_CUDA, root=root,
            flags=flags, **v)
        # selection never looks at the counts: fused whenever the knob is
        # set. The traced size is the root's total, a non-root's own block.
        note(job, coll, (sum(counts) if self.is_root else counts[r]) * es,
             job.knob)

    def fill(self, seed):
        job, ty, counts = self.job, self.ty, self.counts
        w, r = job.world, job.rank
        ip = self.inplace and self.is_root
        mine = ty.enc(block(seed, r, 0, counts[r], ty))
        if self.coll == "gatherv":
            self.exp = None
            if self.is_root:
                self.exp = self.padded_dst()
                for s in range(w):
                    o = self.dsp[s]
                    self.exp[o:o + counts[s]].copy_(
                        ty.enc(block(seed, s, 0, counts[s], ty)))
                if ip:
                    o = self.dsp[r]
                    self.dst.buf[o:o + counts[r]].copy_(mine)
            if not ip:
                self.src.buf.copy_(mine)
        else:
            if self.is_root:
                self.src.buf.view(torch.uint8).fill_(SRC_PAD)
                for d in range(w):
                    o = self.dsp[d]
                    self.src.buf[o:o + counts[d]].copy_(
                        ty.enc(block(seed, d, 0, counts[d], ty)))
            if not ip:
                self.padded_dst()
                self.exp = mine.cuda()
        self.src_before = None if self.src is None else self.src.buf.clone()
        torch.cuda.synchronize()

    def count_posts(self, posts):
        if self.job.knob:
            self.job.rooted += posts
            if not self.fits:
                self.job.fallback += posts


def fit_exactly(coll, w):
    """bf16 counts of a request that fills B to the byte: one block of B for
    gatherv; for scatterv one of 16 bytes and one of B - 16."""
    if coll == "gatherv":
        return [7] * (w - 1) + [B // 2]
    return [8] + [0] * (w - 2) + [(B - 16) // 2]


def one_over(coll, w):
    """One block, on rank 1, of B plus one bf16 element; the other ranks'
    blocks are small."""
    return [7, B // 2 + 1, 999][:w]


def run_gs(job, seed, all_roots, shapes):
    w = job.world
    for coll in ("gather", "scatter"):
        for ty, per in shapes:
            for root in all_roots:
                seed += 1
                GS(job, coll, ty, per, root).run(seed)
        # rank 1's buffers 2 bytes past a 16-byte boundary
        mis = 2 if job.rank == 1 else 0
        for root in all_roots:
            seed += 1
            GS(job, coll, BF16, 999, root, mis=mis).run(seed)
        # in place at the root
        for per in (999, 75_001):
            for root in all_roots:
                seed += 1
                GS(job, coll, BF16, per, root, inplace=True).run(seed)
        # exactly at the bound, and one element over it
        per = at_bound(job, coll)
        seed += 2
        GS(job, coll, BF16, per, root=1).run(seed)
        GS(job, coll, BF16, per + 1, root=1, fused=False).run(seed + 1)
        # a persistent request over the slot wrap
        seed += 1
        GS(job, coll, BF16, 999, root=w - 1, persistent=True).run(
            seed, posts=nposts())
    return seed


def run_v(job, seed, all_roots, raggeds):
    w = job.world
    for coll in ("gatherv", "scatterv"):
        for root in all_roots:
            for ip in (False, True):
                for ty in (BF16, U8):
                    for ragged in raggeds:
                        seed += 1
                        GSv(job, coll, ty, ragged, root, inplace=ip).run(seed)
        seed += 1
        GSv(job, coll, BF16, fit_exactly(coll, w), root=1).run(seed)
        # a single block over B: every rank falls back, the result is right
        for root in all_roots:
            seed += 1
            GSv(job, coll, BF16, one_over(coll, w), root).run(seed)
        # persistent: the root decides at every post, fit and unfit
        seed += 1
        GSv(job, coll, BF16, [999, 0, 1][:w], root=w - 1,
            persistent=True).run(seed, posts=nposts())
        seed += 1
        GSv(job, coll, BF16, one_over(coll, w), root=0,
            persistent=True).run(seed, posts=2)
    # scatterv: the sum decides. Every block is far below B, the sum of the
    # rounded blocks is B + 16.
    over = list(fit_exactly("scatterv", w))
    over[0] += 1
    seed += 1
    GSv(job, "scatterv", BF16, over, root=1).run(seed)
    assert not job.knob or job.fallback > 0
    return seed


def run_interleave(job, seed):
    """The four types between fused allreduces, staged requests and a failed
    vote, all on the one slot sequence of the team."""
    w = job.world
    for rnd in range(2):
        seed += 10
        root = rnd % w
        fused_allreduce(job, seed, 999)
        GS(job, "gather", BF16, 999, root).run(seed + 1)
        GS(job, "gather", BF16, at_bound(job, "gather") + 1, root,
           fused=False).run(seed + 2)
        GS(job, "scatter", BF16, 999, root).run(seed + 3)
        GSv(job, "gatherv", BF16, [999, 7, 1][:w], root).run(seed + 4)
        GSv(job, "scatterv", BF16, one_over("scatterv", w), root).run(
            seed + 5)
        fused_allreduce(job, seed + 6, 999)
        GSv(job, "scatterv", BF16, [7, 999, 0][:w], root).run(seed + 7)
        GS(job, "scatter", BF16, at_bound(job, "scatter") + 1, root,
           fused=False).run(seed + 8)
    return seed


def run_all(job):
    seed = run_gs(job, 100, (0, 1),
                  ((U8, 1), (BF16, 8), (BF16, 999), (BF16, 75_001)))
    seed = run_v(job, seed, (0, 1), ([0, 999], [1, 75_001], [7, 0]))
    run_interleave(job, seed)


def run_three(job):
    seed = run_gs(job, 400, (1, 2), ((BF16, 999), (BF16, 75_001)))
    run_v(job, seed, (1, 2), ([0, 1, 999], [75_001, 7, 0]))


def run_trig(job):
    """Persistent gather and scatter: three eager triggered posts, then one
    captured post replayed three times, new data every time
    (fused_colls_worker.run_trig's scheme). A gatherv cannot be captured, a
    graph cannot fall back: its triggered post goes to the task the request
    has with the knob unset, and that declines it; nothing is launched and
    dst stays as it was."""
    c = job.c
    s = torch.cuda.Stream()
    ee = c.ee_create(job.team, s.cuda_stream)
    seed = 700
    for make in (lambda: GS(job, "gather", BF16, 999, root=1,
                            persistent=True),
                 lambda: GS(job, "gather", U8, 40_001, root=0, inplace=True,
                            persistent=True),
                 lambda: GS(job, "scatter", BF16, 40_001, root=1,
                            persistent=True),
                 lambda: GS(job, "scatter", BF16, 7, root=0, inplace=True,
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
    gv = GSv(job, "gatherv", BF16, [999, 7], root=1, persistent=True)
    gv.fill(seed + 1)
    if gv.is_root:
        gv.exp = gv.padded_dst()
    torch.cuda.synchronize()
    dist.barrier()
    try:
        c.triggered_post(ee, gv.req)
        raised = False
    except RuntimeError:
        raised = True
    s.synchronize()
    assert raised, "gatherv triggered_post must be declined"
    gv.check((gv.tag, "triggered"))
    job.done.append("trig gatherv")
    dist.barrier()
    del gv
    c.ee_destroy(ee)


def run_off(job):
    GS(job, "gather", BF16, 999, root=1, fused=False).run(900)
    GS(job, "scatter", BF16, 999, root=1, fused=False).run(901)
    GSv(job, "gatherv", BF16, [999, 7], root=1).run(902)
    GSv(job, "scatterv", BF16, [7, 999], root=1).run(903)


def main():
    job = Job(sys.argv[1])
    job.fposts = job.graph = job.rooted = job.fallback = 0
    job.notes = []
    job.knob = os.environ.get("UCC_TL_CDNA4_FUSED_GATHER_SCATTER", "0") == "1"
    {"all": run_all, "three": run_three, "trig": run_trig,
     "off": run_off}[sys.argv[2]](job)
    job.notes += [f"FG_COLL {job.fposts}", f"FG_GRAPH {job.graph}",
                  f"FG_ROOTED {job.rooted}", f"FG_FALLBACK {job.fallback}"]
    with open(os.path.join(job.outdir, f"req_rank{job.rank}.txt"), "w") as f:
        f.write("\n".join(job.notes) + "\n")
    job.finish("FG_OK")


if __name__ == "__main__":
    main()
