"""Worker for tests/test_ring_gpu.py: tl/cdna4's multi-ring allreduce,
reduce_scatter and allgather (algorithm `ring`), always in a fresh process:

  python tests/ring_worker.py inproc N
      N ranks of one process (LocalJob) on cuda:0, once with
      UCC_TL_CDNA4_RING_NRINGS=1 and once with auto (the knob is read when
      a team is created): the three collectives, in place and out of
      place, bf16 / f32 SUM, bf16 AVG, int32 MAX, four counts, a persistent
      request posted three times, and a reduce_scatterv that must stay on
      the old path.
  python -m torch.distributed.run ... tests/ring_worker.py xproc NRINGS
      one rank per process, all on cuda:0: the three collectives in bf16,
      the 3-fragment size included; left's outbox is read over the IPC
      mapping.

The ring knobs are set here, before the library loads. The chunk is 2 KiB:
the TL enforces no minimum, and 2 KiB is the smallest chunk at which every
staged algorithm still has a non-empty per-peer cell at 8 ranks
(chunk / n rounded down to 256 bytes), so it is the smallest size the TL
can be said to accept; the ring then moves 512 elements per fragment.

Inputs are m * 2^-7 with integer |m| <= 256: any f32 sum of up to 8 of them
is exact in any order, so the expectation is float32 arithmetic on the CPU
plus one conversion (AVG: times float32(1 / n) first) and the comparison is
bit for bit. Every request carries a timeout."""

import os
import sys

MODE = sys.argv[1]
NRINGS = sys.argv[2] if MODE == "xproc" else "1"
CHUNK = 2048
os.environ["UCC_TL_CDNA4_RING"] = "1"
os.environ["UCC_TL_CDNA4_RING_NRINGS"] = NRINGS
os.environ["UCC_TL_CDNA4_CHUNK_SIZE"] = str(CHUNK)
os.environ["UCC_COLL_TRACE"] = "1"
os.environ["UCC_LOG_LEVEL"] = "info"
os.environ["UCC_TUNE"] = ("allreduce:cuda:@ring:inf,"
                          "reduce_scatter:cuda:@ring:inf,"
                          "allgather:cuda:@ring:inf")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ucc_amd import core, dtypes as D  # noqa: E402

TIMEOUT = 60
CELL = CHUNK // 4   # elements per fragment: every type here travels as 4 B


# ----------------------------------------------------------------- kinds
class Kind:
    def __init__(self, name, tdt, dt, op):
        self.name, self.tdt, self.dt, self.op = name, tdt, dt, op
        self.is_int = tdt == torch.int32
        self.dtsz = 4 if tdt in (torch.int32, torch.float32) else 2

    def inputs(self, seed, count):
        """CPU tensor of type T, equal for equal (seed, count)"""
        g = torch.Generator().manual_seed(seed)
        if self.is_int:
            return torch.randint(-2 ** 31, 2 ** 31 - 1, (count,),
                                 generator=g, dtype=torch.int64).to(
                                     torch.int32)
        m = torch.randint(-256, 257, (count,), generator=g)
        return (m.to(torch.float32) / 128.0).to(self.tdt)

    def reduce(self, xs):
        """xs: list of n CPU tensors of T -> T, the documented rule"""
        n = len(xs)
        if self.is_int:
            acc = xs[0]
            for x in xs[1:]:
                acc = torch.maximum(acc, x)
            return acc
        acc = xs[0].to(torch.float32)
        for x in xs[1:]:
            acc = acc + x.to(torch.float32)
        if self.op == D.OP_AVG:
            acc = acc * torch.tensor(np.float32(1.0 / n))
        return acc.to(self.tdt)


KINDS = [
    Kind("bf16_sum", torch.bfloat16, D.BFLOAT16, D.OP_SUM),
    Kind("f32_sum", torch.float32, D.FLOAT32, D.OP_SUM),
    Kind("bf16_avg", torch.bfloat16, D.BFLOAT16, D.OP_AVG),
    Kind("int32_max", torch.int32, D.INT32, D.OP_MAX),
]


def same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return a.shape == b.shape and torch.equal(a.view(torch.uint8),
                                              b.view(torch.uint8))


def counts_for(n):
    """per-rank counts: 1, n - 1, 999 (block bases off 16-byte alignment),
    and 3 fragments"""
    return [1, n - 1, 999, 2 * CELL + 5]


def ar_count(n, c):
    """the allreduce vector for per-rank count c; the 3-fragment one has
    blocks of 9 * 128 elements and a last block of 5 more"""
    return 9 * 128 * n + 5 if c == 2 * CELL + 5 else c * n if c > n else c


def plan_launches(coll, n, count, dtsz):
    """ring_plan.h's launch count; count as the plan takes it"""
    accsz = 4
    if coll == "allgather":          # planned in bytes
        count, dtsz, accsz = count * dtsz, 1, 1
    pack = 16 // dtsz
    cell = (CHUNK // accsz) // pack * pack
    if coll == "allreduce":
        gran = 256 // dtsz
        per = (count // n) // gran * gran
        bmax = count - (n - 1) * per
    else:
        bmax = count
    nfrags = max(1, -(-bmax // cell))
    return nfrags * (2 * n - 1 if coll == "allreduce" else n)


# ---------------------------------------------------------------- driver
class Driver:
    """n ranks behind one interface: LocalJob, or this process's rank"""

    def __init__(self, job=None, comm=None):
        self.job, self.comm = job, comm
        self.c = job.c if job else comm.c
        self.n = job.n if job else comm.world
        self.ranks = list(range(self.n)) if job else [comm.rank]
        self.n_req = 0        # ring requests initialised in this process
        self.expect_launches = 0

    def init(self, r, coll, **kw):
        team = self.job.teams[r] if self.job else self.comm.team
        return self.c.coll_init(team, coll, mem_type=D.MEM_CUDA,
                                timeout=TIMEOUT, **kw)

    def run(self, reqs):
        for q in reqs:
            q.post()
        while any(q.test() == self.c.INPROGRESS for q in reqs):
            for ctx in (self.job.ctxs if self.job else [self.comm.ctx]):
                ctx.progress()
        assert all(q.test() == self.c.OK for q in reqs), \
            [q.test() for q in reqs]
        torch.cuda.synchronize()


def one_coll(dr, kind, coll, c, inplace, seed, persistent_reps=0):
    """one collective of per-rank count c on every rank of the driver;
    returns the allreduce outputs (for the all-ranks-identical check)"""
    n = dr.n
    vec = ar_count(n, c) if coll == "allreduce" else c * n
    what = (kind.name, coll, c, "inplace" if inplace else "oop", n)
    flags = dr.c.FLAG_IN_PLACE if inplace else 0
    if persistent_reps:
        flags |= dr.c.FLAG_PERSISTENT
    bufs, reqs = {}, []
    for r in dr.ranks:
        src_n = c if coll == "allgather" else vec
        dst_n = c if coll == "reduce_scatter" else vec
        if inplace:
            big = torch.zeros(vec, dtype=kind.tdt, device="cuda")
            src = big[r * c:(r + 1) * c] if coll == "allgather" else big
            dst = big[r * c:(r + 1) * c] if coll == "reduce_scatter" \
                else big
            count = vec
        else:
            big = None
            src = torch.zeros(src_n, dtype=kind.tdt, device="cuda")
            dst = torch.zeros(dst_n, dtype=kind.tdt, device="cuda")
            count = c if coll == "reduce_scatter" else vec
        bufs[r] = (src, dst, big)
        base = big if inplace else dst
        reqs.append(dr.init(
            r, coll, src=0 if inplace else src.data_ptr(),
            dst=base.data_ptr(), count=count, dt=kind.dt, op=kind.op,
            flags=flags))
        dr.n_req += 1
    outs = None
    for rep in range(max(1, persistent_reps)):
        ins = [kind.inputs(seed * 131 + rep * 17 + s,
                           c if coll == "allgather" else vec)
               for s in range(n)]
        for r in dr.ranks:
            src, dst, big = bufs[r]
            if not inplace:
                dst.zero_()
            src.copy_(ins[r])
        torch.cuda.synchronize()
        before = dr.c.ec_ring_step_launches()
        dr.run(reqs)
        plan_count = vec if coll == "allreduce" else c
        grew = dr.c.ec_ring_step_launches() - before
        want = len(dr.ranks) * plan_launches(coll, n, plan_count, kind.dtsz)
        assert grew == want, (what, "launches", grew, want)
        dr.expect_launches += want
        if coll == "allgather":
            exp_full = torch.cat(ins)
        else:
            exp_full = kind.reduce(ins)
        outs = []
        for r in dr.ranks:
            src, dst, big = bufs[r]
            if coll == "reduce_scatter":
                exp = exp_full[r * c:(r + 1) * c]
                assert same_bits(dst, exp), (what, "rank", r, rep)
                if inplace:   # the other blocks keep the input
                    keep = torch.ones(vec, dtype=torch.bool)
                    keep[r * c:(r + 1) * c] = False
                    assert same_bits(big.cpu()[keep], ins[r][keep]), \
                        (what, "rank", r, "other blocks touched")
            else:
                out = big if inplace else dst
                assert same_bits(out, exp_full), (what, "rank", r, rep)
                outs.append(out.cpu())
            if not inplace and coll != "allgather":
                assert same_bits(src, ins[r]), (what, "src changed")
    return outs


def reduce_scatterv_old_path(dr, kind):
    """a v-variant under the same tune: not a ring collective"""
    n = dr.n
    cnts = [5 + 3 * r for r in range(n)]
    total = sum(cnts)
    ins = [kind.inputs(9000 + s, total) for s in range(n)]
    exp = kind.reduce(ins)
    reqs, dsts = [], {}
    for r in dr.ranks:
        src = ins[r].cuda()
        dst = torch.zeros(cnts[r], dtype=kind.tdt, device="cuda")
        dsts[r] = (src, dst)
        reqs.append(dr.init(r, "reduce_scatterv", src=src.data_ptr(),
                            dst=dst.data_ptr(), count=total, dt=kind.dt,
                            op=kind.op, dst_counts=cnts))
    before = dr.c.ec_ring_step_launches()
    dr.run(reqs)
    assert dr.c.ec_ring_step_launches() == before
    for r in dr.ranks:
        off = sum(cnts[:r])
        assert same_bits(dsts[r][1], exp[off:off + cnts[r]]), \
            ("reduce_scatterv", r)


def inproc(n, nrings):
    from ucc_amd.testing import LocalJob
    torch.cuda.set_device(0)
    os.environ["UCC_TL_CDNA4_RING_NRINGS"] = nrings
    job = LocalJob(n)
    dr = Driver(job=job)
    smap = job.c.score_map_str(job.teams[0])
    assert "@cdna4/ring:" in smap, smap
    seed = 1
    for kind in KINDS:
        for coll in ("allreduce", "reduce_scatter", "allgather"):
            for c in counts_for(n):
                for inplace in (False, True):
                    seed += 1
                    outs = one_coll(dr, kind, coll, c, inplace, seed)
                    if coll == "allreduce":
                        assert all(same_bits(o, outs[0]) for o in outs)
    # one persistent request, posted three times with new inputs
    for coll in ("allreduce", "reduce_scatter", "allgather"):
        seed += 1
        one_coll(dr, KINDS[0], coll, 2 * CELL + 5, False, seed,
                 persistent_reps=3)
    reduce_scatterv_old_path(dr, KINDS[0])
    print(f"RING_INPROC_OK n={n} nrings={nrings} n_req={dr.n_req} "
          f"launches={dr.expect_launches}", flush=True)


def xproc():
    import torch.distributed as dist
    from ucc_amd.parallel import Communicator
    torch.cuda.set_device(0)
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    comm = Communicator()
    dr = Driver(comm=comm)
    seed = 500
    for coll in ("allreduce", "reduce_scatter", "allgather"):
        for c in (999, 2 * CELL + 5):
            for inplace in (False, True):
                seed += 1
                one_coll(dr, KINDS[0], coll, c, inplace, seed)
                dist.barrier()
    torch.cuda.synchronize()
    dist.barrier()
    print(f"RING_XPROC_OK rank={rank} n_req={dr.n_req} "
          f"launches={dr.expect_launches}", flush=True)
    dist.destroy_process_group()


if __name__ == "__main__":
    assert core() is not None
    if MODE == "inproc":
        for nr in ("1", "0"):
            inproc(int(sys.argv[2]), nr)
    else:
        xproc()
