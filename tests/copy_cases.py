"""Cases and byte-exact host models for the kernels that only move bytes,
shared by tests/test_copy_cases.py, tests/test_gather_copy_gpu.py and
tests/copy_colls_worker.py. Host-only: importable without a GPU.

Buffer discipline. Source bytes are seeded draws from 0..127, destination
allocations are pre-filled with seeded draws from 128..255: a byte that was
not written, or was written where it should not be, can never match by
chance, and neither stream is periodic, so a swapped stride or index cannot
reproduce the right bytes. Every destination region whose place is ours to
choose has at least GUARD bytes before it, after it and between it and its
neighbours, and every comparison is over the whole allocation.

The models say "these byte ranges of these sources land at these offsets
and nothing else changes". They are written from the definition of the
operation, not from the kernels. The one exception is path_model(): that is
a model OF the kernel's loop structure (k_gather_copy and
d_copy_bytes_part), used only to prove on the CPU that the case set reaches
every loop; it says nothing about results.
"""

import numpy as np

GUARD = 64
THREADS = 256     # k_gather_copy block size
MAX_SRCS = 8      # ec_hip::kMaxSrcs


def src_bytes(seed, n):
    return np.random.default_rng([1, seed]).integers(0, 128, n,
                                                     dtype=np.uint8)


def dst_fill(seed, n):
    return np.random.default_rng([2, seed]).integers(128, 256, n,
                                                     dtype=np.uint8)


def first_diff(got, exp):
    """offset of the first differing byte, or None"""
    if got.shape != exp.shape:
        return min(got.size, exp.size)
    bad = np.flatnonzero(got != exp)
    return int(bad[0]) if bad.size else None


# ------------------------------------------------------------ gather copy
class GatherCase:
    """One gather_copy launch: dst_base + offs[i] <- srcs[i], lens[i] bytes.

    aligns[i] = (dst address % 16, src address % 16) of source i, given
    16-byte aligned allocations. order = the order in which the regions lie
    in the destination (default: source order), extra[i] = bytes of gap in
    front of region i beyond GUARD. All sources live in one source arena,
    src_offs[i] bytes in; dst_base is the start of the destination
    allocation."""

    def __init__(self, name, lens, aligns=None, order=None, extra=None):
        n = len(lens)
        self.name, self.n, self.lens = name, n, list(lens)
        self.aligns = list(aligns) if aligns else [(0, 0)] * n
        order = list(order) if order else list(range(n))
        extra = list(extra) if extra else [0] * n
        assert sorted(order) == list(range(n)) and 1 <= n <= MAX_SRCS
        self.offs = [0] * n
        cur = 0
        for k in order:
            cur += GUARD + extra[k]
            cur += (self.aligns[k][0] - cur) % 16
            self.offs[k] = cur
            cur += self.lens[k]
        self.dst_size = cur + GUARD
        self.src_offs = []
        cur = 0
        for i in range(n):
            cur += (-cur) % 16 + 16 + self.aligns[i][1]
            self.src_offs.append(cur)
            cur += self.lens[i]
        self.src_size = cur + 16

    def seed(self):
        return sum((i + 1) * (ln + 7) for i, ln in enumerate(self.lens)) \
            + 1000 * self.n + len(self.name)

    def arena(self):
        return src_bytes(self.seed(), self.src_size)

    def dst_initial(self):
        return dst_fill(self.seed(), self.dst_size)

    def moves(self):
        """[(src bytes, dst offset, len)]"""
        a = self.arena()
        return [(a[so:so + ln], off, ln)
                for so, off, ln in zip(self.src_offs, self.offs, self.lens)]

    def expected(self):
        return gather_expected(self.dst_initial(), self.moves())


def gather_expected(dst, moves):
    out = dst.copy()
    for src, off, ln in moves:
        assert len(src) == ln
        out[off:off + ln] = src
    return out


ALIGN_PAIRS = [(0, 0), (0, 1), (1, 0), (3, 3), (4, 4), (4, 8), (8, 8),
               (15, 15)]
ALIGN_LENS = [0, 1, 17, 4099]
SINGLE_LENS = [0, 1, 15, 16, 17, 4095, 4096, 4097, 65536 + 53]


def gather_cases():
    z7 = [0] * 7
    cs = [
        # batched loop uniform over the lanes, then the single-pack loop,
        # then a 9-byte tail
        GatherCase("batched_uniform", [296521] + z7),
        # lanes leave the batched loop at different iterations
        GatherCase("batched_divergent", [259653] + z7),
        # fewer blocks than sources; one block strides the long source
        GatherCase("looped_long", [20000, 16, 1, 0, 17, 15, 31, 33]),
        # the same with the batched loop divergent inside that one block
        GatherCase("looped_divergent", [14407, 16, 1, 0, 17, 15, 31, 33]),
        GatherCase("looped_tiny", [200, 199, 16, 15, 1, 0, 48, 33]),
        GatherCase("mixed", [70001, 777, 0, 9],
                   aligns=[(0, 0), (3, 5), (0, 0), (0, 0)]),
        # destination offsets descending, unequal gaps
        GatherCase("descending_looped", [1000, 37, 4096, 333],
                   aligns=[(0, 0), (0, 0), (0, 0), (7, 2)],
                   order=[3, 2, 1, 0], extra=[5, 130, 0, 77]),
        GatherCase("descending_partitioned", [30000, 37, 4096, 333],
                   aligns=[(0, 0), (0, 0), (0, 0), (7, 2)],
                   order=[3, 2, 1, 0], extra=[5, 130, 0, 77]),
    ]
    for ln in SINGLE_LENS:
        cs.append(GatherCase(f"single_{ln}", [ln]))
    for d, s in ALIGN_PAIRS:
        for ln in ALIGN_LENS:
            cs.append(GatherCase(f"align_d{d}_s{s}_len{ln}_n1", [ln],
                                 aligns=[(d, s)]))
            cs.append(GatherCase(f"align_d{d}_s{s}_len{ln}_n3",
                                 [ln, 2 * ln + 5, ln],
                                 aligns=[(d, s)] * 3))
    assert len({c.name for c in cs}) == len(cs)
    return cs


def path_model(n, lens, aligns, grid):
    """Which loops of k_gather_copy / d_copy_bytes_part each source runs
    through when the launch has `grid` blocks of THREADS threads. One dict
    per source:
      branch         "looped" (grid < n: whole blocks take sources in
                     turn), "part16" (a group of blocks, the pack-or-byte
                     routine) or "partbyte" (a group of blocks, the
                     kernel's own byte loop)
      packed         whether the 16-byte pack loops serve it
      batched_first  4-deep batched-loop iterations of the first lane
      batched_last   ... and of the last lane of the source's lanes
      single         single-pack iterations, summed over the lanes
      tail           bytes after the last pack (0 when not packed)
      byte_site      where its byte loop is, if not packed: "routine" or
                     "kernel"
    """
    assert len(lens) == n == len(aligns)
    grp = max(grid // n, 1)
    out = []
    for ln, (d, s) in zip(lens, aligns):
        both = d | s
        if grid < n:
            branch, vgrid = "looped", 1
            packed = both % 16 == 0
            site = None if packed else "routine"
        elif both % 4 == 0:
            branch, vgrid = "part16", grp
            packed = both % 16 == 0
            site = None if packed else "routine"
        else:
            branch, vgrid, packed, site = "partbyte", grp, False, "kernel"
        r = dict(branch=branch, packed=packed, batched_first=0,
                 batched_last=0, single=0, tail=0, byte_site=site)
        if packed:
            stride = vgrid * THREADS
            nv = ln // 16
            tid = np.arange(stride, dtype=np.int64)
            room = nv - 3 * stride - tid          # > 0: enters the loop
            nb = np.where(room > 0, (room - 1) // (4 * stride) + 1, 0)
            i = tid + 4 * stride * nb
            single = np.where(i < nv, (nv - i + stride - 1) // stride, 0)
            assert int((4 * nb + single).sum()) == nv
            r.update(batched_first=int(nb[0]), batched_last=int(nb[-1]),
                     single=int(single.sum()), tail=ln % 16)
        out.append(r)
    return out


PATH_CLASSES = ["batched_uniform", "batched_divergent", "single_alone",
                "tail_after_packs", "tail_alone", "short", "zero_between",
                "looped", "bytewise", "byte_loop_routine",
                "byte_loop_kernel", "looped_batched_divergent"]


def path_classes(case, grid):
    """the PATH_CLASSES that one case reaches with this grid"""
    got = set()
    pm = path_model(case.n, case.lens, case.aligns, grid)
    for r, ln in zip(pm, case.lens):
        if r["packed"]:
            if r["batched_last"] > 0 and \
                    r["batched_first"] == r["batched_last"]:
                got.add("batched_uniform")
            if r["batched_first"] != r["batched_last"]:
                got.add("batched_divergent")
                if r["branch"] == "looped":
                    got.add("looped_batched_divergent")
            if r["batched_first"] == 0 and r["single"] > 0:
                got.add("single_alone")
            if r["tail"] and ln >= 16:
                got.add("tail_after_packs")
            if r["tail"] and ln < 16:
                got.add("tail_alone")
        if 0 < ln < 16:
            got.add("short")
        if r["branch"] == "looped" and ln > 0:
            got.add("looped")
        if not r["packed"] and ln > 0:
            got.add("bytewise")
            got.add("byte_loop_" + r["byte_site"])
    for i in range(1, case.n - 1):
        if case.lens[i] == 0 and any(case.lens[:i]) and \
                any(case.lens[i + 1:]):
            got.add("zero_between")
    return got


# ------------------------------------------------------------ collectives
COLLS = ["allgather", "allgatherv", "alltoall", "alltoallv", "gather",
         "gatherv", "scatter", "scatterv", "bcast"]
ROOTED = {"gather", "gatherv", "scatter", "scatterv", "bcast"}
V_COLLS = {"allgatherv", "alltoallv", "gatherv", "scatterv"}
PER_PEER = {"alltoall", "alltoallv", "scatter", "scatterv"}


def block_sizes(g):
    """block sizes in elements for a fragment granularity of g elements:
    1, 17, one fragment, one more, three fragments with a ragged last"""
    return [1, 17, g, g + 1, 2 * g + 37]


def v_counts(n, g, rot):
    """per-rank counts that mix 0, less than one fragment and more than two
    fragments"""
    pat = [2 * g + 37, 0, 17, g + 1, g, 1, 2 * g + 37, 17]
    return [pat[(r + rot) % len(pat)] for r in range(n)]


def v_matrix(n, g, rot):
    """alltoallv: counts[s][d], rank s sends counts[s][d] elements to d"""
    pat = [2 * g + 37, 0, 17, g + 1, g, 1, 5, 2 * g + 1]
    return [[pat[(3 * s + 5 * d + rot) % len(pat)] for d in range(n)]
            for s in range(n)]


def v_displs(counts, es):
    """displacements in elements: the blocks lie in the order odd ranks
    descending, then even ranks ascending (neither ascending nor
    descending from 3 ranks on), with unequal gaps of at least GUARD bytes
    in front of, between and behind them. Returns (displs, total
    elements)."""
    n = len(counts)
    order = list(range(1, n, 2))[::-1] + list(range(0, n, 2))
    gap = -(-GUARD // es)
    displs = [0] * n
    cur = 0
    for j, k in enumerate(order):
        cur += gap + (j * 3) % 7
        displs[k] = cur
        cur += counts[k]
    return displs, cur + gap


def coll_moves(coll, n, me, root=0, counts=None, displs=None,
               scounts=None, sdispls=None, rdispls=None, inplace=False):
    """What rank `me` receives, by the definition of the collective:
    [(source rank, offset in that rank's contribution, offset in my
    destination, count)], all in elements.

    A rank's contribution is its source buffer. In place, it is where the
    collective says the source lies inside the destination, and the move
    of a rank's own block onto itself is left out.
      allgather(v), gather(v)  counts[r], displs[r]: where r's block goes
      scatter(v)               counts[r], displs[r]: where r's block lies
                               in the root's source
      alltoall(v)              scounts[s][d], sdispls[s][d] in s's source,
                               rdispls[d][s] in d's destination
      bcast                    counts[0] elements
    """
    mv = []
    if coll in ("allgather", "allgatherv"):
        for s in range(n):
            if not (inplace and s == me):
                mv.append((s, 0, displs[s], counts[s]))
    elif coll in ("gather", "gatherv"):
        if me == root:
            for s in range(n):
                if not (inplace and s == me):
                    mv.append((s, 0, displs[s], counts[s]))
    elif coll in ("scatter", "scatterv"):
        if not (inplace and me == root):
            mv.append((root, displs[me], 0, counts[me]))
    elif coll in ("alltoall", "alltoallv"):
        assert not inplace
        for s in range(n):
            mv.append((s, sdispls[s][me], rdispls[me][s], scounts[s][me]))
    elif coll == "bcast":
        if me != root:
            mv.append((root, 0, 0, counts[0]))
    else:
        raise ValueError(coll)
    return mv


def coll_expected(dst_alloc, base, es, moves, contrib):
    """dst_alloc: my destination allocation as it was before the
    collective, the user buffer `base` bytes in; contrib[r]: rank r's
    contribution in bytes"""
    out = dst_alloc.copy()
    for s, soff, doff, cnt in moves:
        src = contrib[s][soff * es:(soff + cnt) * es]
        assert len(src) == cnt * es
        out[base + doff * es:base + (doff + cnt) * es] = src
    return out
