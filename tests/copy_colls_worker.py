"""Worker for tests/test_copy_colls_gpu.py: the collectives that only move
bytes, compared byte for byte over whole allocations with the models of
tests/copy_cases.py. Always a fresh process:

  python tests/copy_colls_worker.py inproc N
      N ranks of one process (LocalJob) on cuda:0. Same-process ranks are
      refused by the fused and gated paths, so every request here runs
      staged_linear and its k_gather_copy launches; the test counts the
      selection trace to prove it. UCC_TL_CDNA4_CHUNK_SIZE=2048 is set
      here, before the library loads (tests/ring_worker.py says why that
      is the smallest chunk the TL accepts at 8 ranks): a fragment is
      2048 bytes and a per-peer cell 1024, 512 and 256 bytes at 2, 3 and
      8 ranks. allgather(v), alltoall(v), gather(v), scatter(v) and bcast
      in UINT8, INT16 and FLOAT64.
  python -m torch.distributed.run ... tests/copy_colls_worker.py xproc
      one rank per process, all on cuda:0, the environment set by the
      test (UCC_TL_CDNA4_CHUNK_SIZE=65536 and the rest): the device-gated
      pipeline. allgather(v) and alltoall(v) in UINT8 and INT16, one-shot
      and persistent (posted three times with rewritten sources, once with
      16-byte aligned user buffers, the zero-copy form where there is one,
      and once misaligned, where zero-copy must decline), one int32 SUM
      allreduce and one bcast.

Per collective and type the blocks are 1, 17, G, G + 1 and 2 G + 37
elements, G the collective's fragment granularity in elements (a chunk for
allgather(v), gather(v) and bcast, a per-peer cell for the others); the
v-forms mix counts of 0, less than one fragment and more than two
fragments, with gapped displacements in non-monotone order. User buffers
lie 0, 1, 4 or 8 bytes into their allocation (odd only with UINT8), source
and destination independently. Rooted collectives run with root 0, N - 1
and, at 8 ranks, 4.

Every request carries a timeout. Each failing case prints one COPY_BAD line
(collective, team size, type, shape, rank, first differing offset and the
source rank whose block lies there); each process ends with one
`COPY_DONE ... cases=<k> ... bad=<b>` line. After a request that did not
complete with OK nothing further is started."""

import os
import sys
import time

MODE = sys.argv[1]
if MODE == "inproc":
    os.environ["UCC_TL_CDNA4_CHUNK_SIZE"] = "2048"
    os.environ["UCC_COLL_TRACE"] = "1"
    os.environ["UCC_LOG_LEVEL"] = "info"
    for k in ("UCC_TUNE", "UCC_TL_CDNA4_RING", "UCC_TL_CDNA4_FUSED_COLLS",
              "UCC_TL_CDNA4_GATED_ROOTED", "UCC_TL_CDNA4_STAGE_SDMA"):
        os.environ.pop(k, None)
CHUNK = int(os.environ["UCC_TL_CDNA4_CHUNK_SIZE"])

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import copy_cases as cc  # noqa: E402
from ucc_amd import core, dtypes as D  # noqa: E402

TIMEOUT = 30      # seconds, on every request
GUARD = cc.GUARD


class Ty:
    def __init__(self, name, dt, es):
        self.name, self.dt, self.es = name, dt, es


UINT8, INT16, FLOAT64 = (Ty("UINT8", D.UINT8, 1), Ty("INT16", D.INT16, 2),
                         Ty("FLOAT64", D.FLOAT64, 8))


def say(line):
    """one write per line: the ranks of a cross-process run share a pipe"""
    sys.stdout.flush()
    os.write(1, (line + "\n").encode())


def offset_pairs(ty):
    """(source, destination) byte offsets of the user buffers"""
    if ty.es == 1:
        return [(0, 0), (1, 0), (0, 1), (1, 4), (4, 8), (8, 1), (4, 4),
                (8, 8)]
    return [(0, 0), (4, 0), (0, 4), (4, 8), (8, 4), (8, 8)]


def gran(coll, n, es):
    """fragment granularity of the collective in elements"""
    cell = (CHUNK // n) & ~255
    return (cell if coll in cc.PER_PEER else CHUNK) // es


def roots_for(coll, n):
    if coll not in cc.ROOTED:
        return [0]
    return sorted({0, n - 1} | ({n // 2} if n == 8 else set()))


# ---------------------------------------------------------------- layouts
class Layout:
    """rank-independent description of one collective call, in elements"""

    def __init__(self, coll, n, es, g, block=None, rot=None):
        self.coll, self.n, self.es = coll, n, es
        self.shape = f"block={block}" if rot is None else f"vrot={rot}"
        c = block
        self.counts = self.displs = None
        self.scounts = self.sdispls = self.rcounts = self.rdispls = None
        if coll in ("allgather", "gather", "scatter"):
            self.counts = [c] * n
            self.displs = [r * c for r in range(n)]
            self.total = n * c
        elif coll in ("allgatherv", "gatherv", "scatterv"):
            self.counts = cc.v_counts(n, g, rot)
            self.displs, self.total = cc.v_displs(self.counts, es)
            self.shape += f" counts={self.counts}"
        elif coll == "alltoall":
            self.scounts = [[c] * n for _ in range(n)]
            self.sdispls = [[d * c for d in range(n)] for _ in range(n)]
            self.rcounts = self.scounts
            self.rdispls = self.sdispls
            self.stotal = self.rtotal = [n * c] * n
        elif coll == "alltoallv":
            self.scounts = cc.v_matrix(n, g, rot)
            self.rcounts = [[self.scounts[s][d] for s in range(n)]
                            for d in range(n)]
            sd = [cc.v_displs(row, es) for row in self.scounts]
            rd = [cc.v_displs(row, es) for row in self.rcounts]
            self.sdispls, self.stotal = [x[0] for x in sd], [x[1] for x in sd]
            self.rdispls, self.rtotal = [x[0] for x in rd], [x[1] for x in rd]
            self.shape += f" row0={self.scounts[0]}"
        elif coll == "bcast":
            self.counts = [c]
        else:
            raise ValueError(coll)

    def contrib_elems(self, r, root):
        k = self.coll
        if k in ("allgather", "allgatherv", "gather", "gatherv"):
            return self.counts[r]
        if k in ("scatter", "scatterv"):
            return self.total if r == root else 0
        if k in ("alltoall", "alltoallv"):
            return self.stotal[r]
        return self.counts[0] if r == root else 0

    def dst_elems(self, r, root, inplace):
        k = self.coll
        if k in ("allgather", "allgatherv"):
            return self.total
        if k in ("gather", "gatherv"):
            return self.total if r == root else 0
        if k in ("scatter", "scatterv"):
            return 0 if (inplace and r == root) else self.counts[r]
        if k in ("alltoall", "alltoallv"):
            return self.rtotal[r]
        return self.counts[0]

    def moves(self, me, root, inplace):
        return cc.coll_moves(self.coll, self.n, me, root=root,
                             counts=self.counts, displs=self.displs,
                             scounts=self.scounts, sdispls=self.sdispls,
                             rdispls=self.rdispls, inplace=inplace)

    def own_in_dst(self, r, root, inplace):
        """in place: element offset of r's contribution inside its own
        destination, else None"""
        if not inplace:
            return None
        if self.coll in ("allgather", "allgatherv"):
            return self.displs[r]
        if self.coll in ("gather", "gatherv") and r == root:
            return self.displs[r]
        return None

    def init_kwargs(self, r, root, src, dst, flags):
        k, n = self.coll, self.n
        kw = dict(src=src, dst=dst, root=root, flags=flags)
        if k in ("allgather", "alltoall"):
            kw.update(count=n * (self.counts[0] if self.counts
                                 else self.scounts[0][0]))
        elif k == "allgatherv":
            kw.update(count=self.counts[r], dst_counts=self.counts,
                      dst_displs=self.displs)
        elif k == "alltoallv":
            kw.update(count=0, src_counts=self.scounts[r],
                      src_displs=self.sdispls[r],
                      dst_counts=self.rcounts[r],
                      dst_displs=self.rdispls[r])
        elif k in ("gather", "scatter"):
            kw.update(count=self.total if r == root else self.counts[r])
        elif k == "gatherv":
            kw.update(count=self.counts[r], dst_counts=self.counts,
                      dst_displs=self.displs)
        elif k == "scatterv":
            kw.update(count=self.counts[r], src_counts=self.counts,
                      src_displs=self.displs)
        else:
            kw.update(count=self.counts[0])
        return kw


class DevBuf:
    """a user buffer of nbytes, `off` bytes past GUARD into an allocation
    whose every other byte is seeded fill from 128..255"""

    def __init__(self, seed, off, nbytes):
        self.base = GUARD + off
        self.nbytes = nbytes
        self.fill = cc.dst_fill(seed, self.base + nbytes + GUARD)
        self.host = self.fill.copy()
        self.dev = torch.from_numpy(self.host).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.ptr = self.dev.data_ptr() + self.base

    def put(self, at, data):
        """`data` at byte `at` of the user buffer, everything else fill"""
        self.host = self.fill.copy()
        self.host[self.base + at:self.base + at + len(data)] = data
        self.dev.copy_(torch.from_numpy(self.host))

    def get(self):
        return self.dev.cpu().numpy()


# ---------------------------------------------------------------- driver
class Driver:
    """n ranks behind one interface: LocalJob, or this process's rank"""

    def __init__(self, job=None, xjob=None):
        self.job, self.xjob = job, xjob
        self.c = core()
        self.n = job.n if job else xjob.world
        self.ranks = list(range(self.n)) if job else [xjob.rank]
        self.cases = self.n_req = self.bad = self.refused = 0
        self.dead = False
        self.seed = 0

    def team(self, r):
        return self.job.teams[r] if self.job else self.xjob.team

    def init(self, r, coll, **kw):
        self.n_req += 1
        return self.c.coll_init(self.team(r), coll, mem_type=D.MEM_CUDA,
                                timeout=TIMEOUT, **kw)

    def barrier(self):
        if self.xjob:
            import torch.distributed as dist
            dist.barrier()

    def run(self, reqs):
        """post and complete; the statuses"""
        c = self.c
        ctxs = self.job.ctxs if self.job else [self.xjob.ctx]
        for q in reqs:
            q.post()
        deadline = time.monotonic() + 2 * TIMEOUT
        while any(q.test() == c.INPROGRESS for q in reqs):
            for ctx in ctxs:
                ctx.progress()
            if time.monotonic() > deadline:
                return ["no completion"]
        torch.cuda.synchronize()
        return [q.test() for q in reqs]

    def fail(self, what, msg):
        self.bad += 1
        say(f"COPY_BAD {what} {msg}")

    def done(self, tag):
        say(f"COPY_DONE mode={tag} n={self.n} ranks={self.ranks} "
            f"cases={self.cases} n_req={self.n_req} "
            f"refused={self.refused} bad={self.bad}")


def run_case(dr, ty, lay, root=0, inplace=False, soff=0, doff=0, posts=1,
             persistent=False):
    """one collective call on every rank of the driver (posted `posts`
    times with new sources when persistent), every allocation compared"""
    if dr.dead:
        return
    n, es, coll, c = dr.n, ty.es, lay.coll, dr.c
    dr.cases += 1
    dr.seed += 1
    what = (f"coll={coll} n={n} type={ty.name} {lay.shape} root={root} "
            f"inplace={int(inplace)} soff={soff} doff={doff}")
    flags = (c.FLAG_IN_PLACE if inplace else 0) | \
        (c.FLAG_PERSISTENT if persistent else 0)
    src, dst, reqs = {}, {}, []
    for r in dr.ranks:
        seed = dr.seed * 64 + r
        own = lay.own_in_dst(r, root, inplace)
        ce, de = lay.contrib_elems(r, root), lay.dst_elems(r, root, inplace)
        if coll == "bcast":
            dst[r] = DevBuf(seed, doff, de * es)
            sp, dp = dst[r].ptr, 0
        else:
            has_src = own is None and (
                coll not in ("scatter", "scatterv") or r == root)
            has_dst = coll not in ("gather", "gatherv") or r == root
            if inplace and coll in ("scatter", "scatterv") and r == root:
                has_dst = False
            src[r] = DevBuf(seed + 32, soff, ce * es) if has_src else None
            dst[r] = DevBuf(seed, doff, de * es) if has_dst else None
            sp = src[r].ptr if has_src else 0
            dp = dst[r].ptr if has_dst else 0
        reqs.append(dr.init(r, coll, dt=ty.dt,
                            **lay.init_kwargs(r, root, sp, dp, flags)))
    for post in range(posts):
        contrib = [cc.src_bytes((dr.seed * 8 + post) * 16 + r,
                                lay.contrib_elems(r, root) * es)
                   for r in range(n)]
        before = {}
        for r in dr.ranks:
            own = lay.own_in_dst(r, root, inplace)
            if coll == "bcast":
                dst[r].put(0, contrib[r] if r == root else contrib[r][:0])
            else:
                if src.get(r) is not None:
                    src[r].put(0, contrib[r])
                if dst.get(r) is not None:
                    dst[r].put(own * es if own is not None else 0,
                               contrib[r] if own is not None
                               else contrib[r][:0])
            if dst.get(r) is not None:
                before[r] = dst[r].host.copy()
        torch.cuda.synchronize()
        dr.barrier()
        sts = dr.run(reqs)
        if any(s != c.OK for s in sts):
            dr.fail(what, f"post={post} status={sts}")
            dr.dead = True
            return
        for r in dr.ranks:
            if src.get(r) is not None and \
                    cc.first_diff(src[r].get(), src[r].host) is not None:
                dr.fail(what, f"post={post} rank={r} source changed")
            if dst.get(r) is None:
                continue
            mv = lay.moves(r, root, inplace)
            exp = cc.coll_expected(before[r], dst[r].base, es, mv, contrib)
            at = cc.first_diff(dst[r].get(), exp)
            if at is not None:
                rel = at - dst[r].base
                owner = [s for s, _, d, k in mv
                         if d * es <= rel < (d + k) * es]
                dr.fail(what, f"post={post} rank={r} first_diff={rel} "
                              f"(allocation byte {at}) "
                              f"src_rank={owner[0] if owner else 'guard'}")
        dr.barrier()


def refuse_inplace_alltoall(dr, ty):
    """alltoall(v) in place has no staged or gated form: coll_init must
    refuse it (nothing is posted)"""
    n = dr.n
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    for coll in ("alltoall", "alltoallv"):
        lay = Layout(coll, n, ty.es, 64, block=8, rot=0)
        for r in dr.ranks:
            kw = lay.init_kwargs(r, 0, 0, buf.data_ptr(),
                                 dr.c.FLAG_IN_PLACE)
            try:
                dr.c.coll_init(dr.team(r), coll, mem_type=D.MEM_CUDA,
                               timeout=TIMEOUT, dt=ty.dt, **kw)
            except RuntimeError as e:
                if "Not supported" in str(e):
                    dr.refused += 1
                    continue
                dr.fail(f"coll={coll} n={n} inplace=1", f"init raised {e}")
                continue
            dr.fail(f"coll={coll} n={n} inplace=1 rank={r}",
                    "accepted at init")


def sweep(dr, ty, colls, persistent_too=False):
    """the shapes, roots and pointer offsets of one type"""
    n = dr.n
    pairs = offset_pairs(ty)
    k = 0
    for coll in colls:
        g = gran(coll, n, ty.es)
        roots = roots_for(coll, n)
        if coll in cc.V_COLLS:
            lays = [Layout(coll, n, ty.es, g, rot=rot) for rot in (0, 2)]
        else:
            lays = [Layout(coll, n, ty.es, g, block=b)
                    for b in cc.block_sizes(g)]
        for lay in lays:
            for root in roots:
                so, do = pairs[k % len(pairs)]
                k += 1
                run_case(dr, ty, lay, root=root, soff=so, doff=do)
        # every offset pair, at a small ragged size
        small = lays[0] if coll in cc.V_COLLS else lays[1]
        for j, (so, do) in enumerate(pairs):
            run_case(dr, ty, small, root=roots[j % len(roots)], soff=so,
                     doff=do)
        if persistent_too:
            big = lays[0] if coll in cc.V_COLLS else lays[-1]
            mis = (1, 4) if ty.es == 1 else (4, 8)
            for so, do in ((0, 0), mis):
                run_case(dr, ty, big, soff=so, doff=do, posts=3,
                         persistent=True)


def sweep_inplace(dr, ty):
    n = dr.n
    pairs = offset_pairs(ty)
    g = gran("allgather", n, ty.es)
    k = 0
    for lay in ([Layout("allgather", n, ty.es, g, block=b)
                 for b in (17, g + 1, 2 * g + 37)] +
                [Layout("allgatherv", n, ty.es, g, rot=rot)
                 for rot in (0, 2)]):
        run_case(dr, ty, lay, inplace=True, doff=pairs[k % len(pairs)][1])
        k += 1
    for coll in ("gather", "scatter"):
        g = gran(coll, n, ty.es)
        for b in (17, 2 * g + 37):
            lay = Layout(coll, n, ty.es, g, block=b)
            for root in roots_for(coll, n):
                so, do = pairs[k % len(pairs)]
                k += 1
                run_case(dr, ty, lay, root=root, inplace=True, soff=so,
                         doff=do)


# ------------------------------------------------------------------ modes
def inproc(n):
    from ucc_amd.testing import LocalJob
    torch.cuda.set_device(0)
    dr = Driver(job=LocalJob(n))
    for ty in (UINT8, INT16, FLOAT64):
        sweep(dr, ty, cc.COLLS)
        sweep_inplace(dr, ty)
    refuse_inplace_alltoall(dr, UINT8)
    dr.done("inproc")
    return dr


def xproc_allreduce(dr):
    """int32 SUM, four fragments: exact"""
    if dr.dead:
        return
    job, c, n = dr.xjob, dr.c, dr.n
    count = 3 * (CHUNK // 4) + 1
    dr.cases += 1
    rng = np.random.default_rng(77)
    full = rng.integers(-10 ** 6, 10 ** 6, size=(n, count), dtype=np.int32)
    src = torch.from_numpy(full[job.rank].copy()).cuda()
    dst = torch.full((count,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    req = dr.init(job.rank, "allreduce", src=src.data_ptr(),
                  dst=dst.data_ptr(), count=count, dt=D.INT32, op=D.OP_SUM)
    sts = dr.run([req])
    what = f"coll=allreduce n={n} type=INT32 count={count}"
    if sts != [c.OK]:
        dr.fail(what, f"status={sts}")
        dr.dead = True
        return
    exp = full.astype(np.int64).sum(0).astype(np.int32)
    at = cc.first_diff(dst.cpu().numpy(), exp)
    if at is not None:
        dr.fail(what, f"rank={job.rank} first_diff={at} (element)")
    if cc.first_diff(src.cpu().numpy(), full[job.rank]) is not None:
        dr.fail(what, "source changed")


def xproc():
    import torch.distributed as dist
    from zc_fused_worker import Job
    say(f"COPY_START rank={os.environ.get('RANK')}")
    job = Job("")
    dr = Driver(xjob=job)
    colls = ["allgather", "allgatherv", "alltoall", "alltoallv"]
    for ty in (UINT8, INT16):
        sweep(dr, ty, colls, persistent_too=True)
    xproc_allreduce(dr)
    g = gran("bcast", dr.n, 1)
    run_case(dr, UINT8, Layout("bcast", dr.n, 1, g, block=2 * g + 37),
             root=dr.n - 1, doff=4)
    dr.done("xproc")
    if not dr.dead:
        dist.barrier()
        dist.destroy_process_group()
    return dr


if __name__ == "__main__":
    assert core() is not None
    d = inproc(int(sys.argv[2])) if MODE == "inproc" else xproc()
    sys.exit(1 if d.bad else 0)
