/* Plan of tl/cdna4's fused one-kernel small-message collectives
 * (FusedCollTask in tl_cdna4.cc, k_fused_coll in ec_fused_colls.hip): allgather,
 * reduce_scatter, alltoall, bcast and reduce. Host only, no HIP: a pure
 * function of (collective, n, rank, root, block bytes, element size,
 * in-place) that says what one rank's kernel stages, and what it reads after
 * the handshake. tests/native/test_fused_plan.cc runs it for all ranks on
 * host memory.
 *
 * Protocol (the fused allreduce's): every rank copies its stage cells from
 * its user source into its own scratch, all ranks shake hands, then every
 * rank runs its copy segments (peer scratch -> dst) or its reduce segment
 * (all n peers' scratch, ranks 0..n-1 in order -> dst). Every rank takes
 * part in the handshake, also one that stages or reads nothing.
 *
 * block_bytes is the per-rank block for allgather, reduce_scatter and
 * alltoall, and the whole vector for bcast and reduce.
 *
 * Scratch layout. Cell c lies at c * stride, stride = block_bytes rounded up
 * to 16: every scratch offset is a multiple of 16 whatever the count, so only
 * a user pointer can force the element-wise path.
 *   allgather       cell 0 = my block
 *   reduce_scatter  cell d = my contribution to rank d's block
 *   alltoall        cell d = my block for rank d
 *   bcast           cell 0 = the vector, at the root only
 *   reduce          cell 0 = my vector
 * scratch_bytes = cells * stride is the same on every rank (a non-root of
 * bcast reads that much of the root's scratch), so a bound on it is a
 * rank-invariant decision.
 *
 * Offsets. src_off counts from the stage base: the user src, or the user dst
 * when src_is_dst (in place; StagedTask::post()'s rules):
 *   allgather in place       source = dst + me * block
 *   reduce_scatter in place  source = the whole dst, result at dst + me * block
 *   reduce in place, root    source = dst
 *   bcast                    always in place (one buffer)
 *   alltoall in place        declined
 * dst_off counts from the user dst.
 *
 * The ragged forms (allgatherv, reduce_scatterv, alltoallv) have an
 * initialiser of their own, fused_plan_init_v, described at its definition;
 * tests/native/test_fused_plan_v.cc runs it for all ranks. */
#ifndef UCC_AMD_FUSED_PLAN_H_
#define UCC_AMD_FUSED_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace ucc {

constexpr int kFusedMaxRanks = 8;

enum FusedColl { FUSED_ALLGATHER = 0, FUSED_REDUCE_SCATTER = 1,
                 FUSED_ALLTOALL = 2, FUSED_BCAST = 3, FUSED_REDUCE = 4,
                 /* v-forms: fused_plan_init_v below */
                 FUSED_ALLGATHERV = 5, FUSED_REDUCE_SCATTERV = 6,
                 FUSED_ALLTOALLV = 7 };

struct FusedCell {
    uint64_t src_off = 0, scratch_off = 0, len = 0; /* bytes */
};

struct FusedSeg {
    int      peer = 0;
    uint64_t scratch_off = 0, dst_off = 0, len = 0; /* bytes */
};

struct FusedPlan {
    FusedColl coll = FUSED_ALLGATHER;
    int       n = 0, rank = 0, root = 0;
    bool      src_is_dst = false; /* stage base is the user dst           */
    int       n_cells = 0;
    FusedCell cell[kFusedMaxRanks];
    int       n_segs = 0;
    FusedSeg  seg[kFusedMaxRanks];
    /* reduce segment: red_count elements at red_scratch_off of all n peers'
     * scratch into dst + red_dst_off; red_count == 0: none */
    uint64_t  red_scratch_off = 0, red_dst_off = 0, red_count = 0;
    uint64_t  scratch_bytes = 0;
    uint64_t  stage_bytes = 0; /* sum of the cells                        */
    uint64_t  read_bytes = 0;  /* bytes read over peer pointers           */
    /* alltoallv only */
    uint64_t  cell_bytes = 0;  /* the fixed cell size                     */
    bool      fits_local = true; /* my vote: all my send lengths <= cell  */
};

static inline uint64_t fused_plan_stride(uint64_t block_bytes)
{
    return (block_bytes + 15) & ~(uint64_t)15;
}

/* the plan's scratch_bytes alone: what the accept / decline decision needs,
 * from quantities that are equal on every rank */
static inline uint64_t fused_plan_scratch_bytes(FusedColl coll, int n,
                                                uint64_t block_bytes)
{
    const uint64_t cells =
        coll == FUSED_REDUCE_SCATTER || coll == FUSED_ALLTOALL ? (uint64_t)n
                                                               : 1;
    return cells * fused_plan_stride(block_bytes);
}

/* false: not expressible (rank count, root, sizes, in-place alltoall) */
static inline bool fused_plan_init(FusedPlan *p, FusedColl coll, int n,
                                   int rank, int root, uint64_t block_bytes,
                                   size_t elem_size, bool inplace)
{
    if (n < 2 || n > kFusedMaxRanks || rank < 0 || rank >= n || root < 0 ||
        root >= n || elem_size == 0 || block_bytes == 0 ||
        block_bytes % elem_size != 0 ||
        block_bytes > (UINT64_MAX >> 8) / (uint64_t)n ||
        (coll == FUSED_ALLTOALL && inplace)) {
        return false;
    }
    *p      = FusedPlan{};
    p->coll = coll;
    p->n    = n;
    p->rank = rank;
    p->root = root;
    const uint64_t b      = block_bytes;
    const uint64_t stride = fused_plan_stride(b);
    const uint64_t me     = (uint64_t)rank;
    p->scratch_bytes      = fused_plan_scratch_bytes(coll, n, b);
    switch (coll) {
    case FUSED_ALLGATHER:
        p->src_is_dst      = inplace;
        p->n_cells         = 1;
        p->cell[0].src_off = inplace ? me * b : 0;
        p->cell[0].len     = b;
        for (int r = 0; r < n; r++) {
            FusedSeg &s = p->seg[p->n_segs++];
            s.peer      = r;
            s.dst_off   = (uint64_t)r * b;
            s.len       = b;
        }
        break;
    case FUSED_REDUCE_SCATTER:
        p->src_is_dst = inplace;
        p->n_cells    = n;
        for (int d = 0; d < n; d++) {
            p->cell[d].src_off     = (uint64_t)d * b;
            p->cell[d].scratch_off = (uint64_t)d * stride;
            p->cell[d].len         = b;
        }
        p->red_scratch_off = me * stride;
        p->red_dst_off     = inplace ? me * b : 0;
        p->red_count       = b / elem_size;
        break;
    case FUSED_ALLTOALL:
        p->n_cells = n;
        for (int d = 0; d < n; d++) {
            p->cell[d].src_off     = (uint64_t)d * b;
            p->cell[d].scratch_off = (uint64_t)d * stride;
            p->cell[d].len         = b;
        }
        for (int r = 0; r < n; r++) {
            FusedSeg &s   = p->seg[p->n_segs++];
            s.peer        = r;
            s.scratch_off = me * stride;
            s.dst_off     = (uint64_t)r * b;
            s.len         = b;
        }
        break;
    case FUSED_BCAST:
        p->src_is_dst = true;
        if (rank == root) {
            p->n_cells     = 1;
            p->cell[0].len = b;
        } else {
            p->n_segs      = 1;
            p->seg[0].peer = root;
            p->seg[0].len  = b;
        }
        break;
    case FUSED_REDUCE:
        p->src_is_dst  = inplace && rank == root;
        p->n_cells     = 1;
        p->cell[0].len = b;
        if (rank == root) {
            p->red_count = b / elem_size;
        }
        break;
    default: return false;
    }
    for (int c = 0; c < p->n_cells; c++) {
        p->stage_bytes += p->cell[c].len;
    }
    for (int s = 0; s < p->n_segs; s++) {
        p->read_bytes += p->seg[s].len;
    }
    p->read_bytes += p->red_count * elem_size * (uint64_t)n;
    return true;
}

/* ------------------------------------------------------------- v-forms
 * allgatherv, reduce_scatterv and alltoallv: byte counts and byte
 * displacements per rank instead of one block size.
 *
 *   allgatherv      counts / displs = dst.info_v of every rank (the same
 *                   array everywhere). Cell 0 = my block; segment r =
 *                   counts[r] bytes of peer r's cell 0 -> dst + displs[r].
 *                   In place: source = dst + displs[me].
 *                   scratch_bytes = stride(max counts).
 *   reduce_scatterv counts = dst.info_v.counts of every rank. Cell d = my
 *                   contribution to rank d at the running sum of
 *                   stride(counts[k]), k < d; the source is read packed in
 *                   rank order and displacements are ignored (StagedTask's
 *                   rule). Reduce segment = counts[me] / elem elements at my
 *                   cell. In place: source = the whole packed dst, result at
 *                   the packed offset of me. scratch_bytes = the sum of the
 *                   strides. A rank whose count is 0 stages its cells and
 *                   shakes hands, but has no reduce segment.
 *   alltoallv       counts / displs = my send row, rcounts / rdispls = my
 *                   recv column: NOT equal on every rank. A 16-byte header
 *                   (the rank's vote) at scratch offset 0, then n cells of
 *                   the fixed size `cell` (fused_plan_a2av_cell: knobs and n
 *                   only, equal on every rank). Cell d at 16 + d * cell = my
 *                   block for rank d; segment r = rcounts[r] bytes of peer
 *                   r's cell me -> dst + rdispls[r]. fits_local = every one
 *                   of my send lengths <= cell; a rank that does not fit
 *                   stages nothing. Whether the segments run is decided in
 *                   the kernel from all n votes (k_fused_a2av): a rank never
 *                   knows from its own row and column that all pairs fit.
 * Zero-length blocks make no cell and no segment. */

/* largest alltoallv pair: what is left of `bound` after the header, split n
 * ways, rounded down to 16. 0: no room. */
static inline uint64_t fused_plan_a2av_cell(uint64_t bound, int n)
{
    if (n < 1 || bound < 16) {
        return 0;
    }
    return ((bound - 16) / (uint64_t)n) & ~(uint64_t)15;
}

/* scratch_bytes of a v-plan from quantities equal on every rank: the counts
 * array of allgatherv / reduce_scatterv, `cell` alone for alltoallv (counts
 * is not read). UINT64_MAX: not expressible. */
static inline uint64_t fused_plan_scratch_bytes_v(FusedColl coll, int n,
                                                  const uint64_t *counts,
                                                  uint64_t cell)
{
    if (n < 2 || n > kFusedMaxRanks) {
        return UINT64_MAX;
    }
    uint64_t total = 0;
    switch (coll) {
    case FUSED_ALLTOALLV: return 16 + (uint64_t)n * cell;
    case FUSED_ALLGATHERV:
        for (int r = 0; r < n; r++) {
            if (counts[r] > (UINT64_MAX >> 8)) {
                return UINT64_MAX;
            }
            const uint64_t s = fused_plan_stride(counts[r]);
            total            = s > total ? s : total;
        }
        return total;
    case FUSED_REDUCE_SCATTERV:
        for (int r = 0; r < n; r++) {
            if (counts[r] > (UINT64_MAX >> 8)) {
                return UINT64_MAX;
            }
            total += fused_plan_stride(counts[r]);
        }
        return total;
    default: return UINT64_MAX;
    }
}

/* false: not expressible (rank count, a count that is no multiple of the
 * element size, all counts zero, in-place alltoallv, cell < 16). rcounts,
 * rdispls and cell matter for alltoallv only; elem_size for reduce_scatterv
 * only (alltoallv lengths are bytes of each side's own datatype). */
static inline bool fused_plan_init_v(FusedPlan *p, FusedColl coll, int n,
                                     int rank, const uint64_t *counts,
                                     const uint64_t *displs,
                                     const uint64_t *rcounts,
                                     const uint64_t *rdispls, uint64_t cell,
                                     size_t elem_size, bool inplace)
{
    if (n < 2 || n > kFusedMaxRanks || rank < 0 || rank >= n ||
        elem_size == 0 || !counts) {
        return false;
    }
    *p      = FusedPlan{};
    p->coll = coll;
    p->n    = n;
    p->rank = rank;
    const uint64_t sb = fused_plan_scratch_bytes_v(coll, n, counts, cell);
    if (sb == UINT64_MAX) {
        return false;
    }
    p->scratch_bytes = sb;
    uint64_t any     = 0;
    switch (coll) {
    case FUSED_ALLGATHERV:
        if (!displs) {
            return false;
        }
        p->src_is_dst = inplace;
        if (counts[rank]) {
            p->n_cells         = 1;
            p->cell[0].src_off = inplace ? displs[rank] : 0;
            p->cell[0].len     = counts[rank];
        }
        for (int r = 0; r < n; r++) {
            any |= counts[r];
            if (!counts[r]) {
                continue;
            }
            FusedSeg &s = p->seg[p->n_segs++];
            s.peer      = r;
            s.dst_off   = displs[r];
            s.len       = counts[r];
        }
        break;
    case FUSED_REDUCE_SCATTERV: {
        p->src_is_dst   = inplace;
        uint64_t packed = 0, sc = 0;
        for (int d = 0; d < n; d++) {
            if (counts[d] % elem_size != 0) {
                return false;
            }
            any |= counts[d];
            if (d == rank) {
                p->red_scratch_off = sc;
                p->red_dst_off     = inplace ? packed : 0;
                p->red_count       = counts[d] / elem_size;
            }
            if (counts[d]) {
                FusedCell &c  = p->cell[p->n_cells++];
                c.src_off     = packed;
                c.scratch_off = sc;
                c.len         = counts[d];
            }
            packed += counts[d];
            sc += fused_plan_stride(counts[d]);
        }
        break;
    }
    case FUSED_ALLTOALLV:
        if (inplace || cell < 16 || cell % 16 != 0 || !displs || !rcounts ||
            !rdispls) {
            return false;
        }
        p->cell_bytes = cell;
        p->fits_local = true;
        for (int d = 0; d < n; d++) {
            if (counts[d] > cell) {
                p->fits_local = false;
            }
        }
        for (int d = 0; p->fits_local && d < n; d++) {
            if (!counts[d]) {
                continue;
            }
            FusedCell &c  = p->cell[p->n_cells++];
            c.src_off     = displs[d];
            c.scratch_off = 16 + (uint64_t)d * cell;
            c.len         = counts[d];
        }
        for (int r = 0; r < n; r++) {
            /* a length over the cell is never read: the verdict of such a
             * request is "does not fit" on every rank */
            if (!rcounts[r] || rcounts[r] > cell) {
                continue;
            }
            FusedSeg &s   = p->seg[p->n_segs++];
            s.peer        = r;
            s.scratch_off = 16 + (uint64_t)rank * cell;
            s.dst_off     = rdispls[r];
            s.len         = rcounts[r];
        }
        any = 1; /* the counts never decide */
        break;
    default: return false;
    }
    if (!any) {
        return false;
    }
    for (int c = 0; c < p->n_cells; c++) {
        p->stage_bytes += p->cell[c].len;
    }
    for (int s = 0; s < p->n_segs; s++) {
        p->read_bytes += p->seg[s].len;
    }
    p->read_bytes += p->red_count * elem_size * (uint64_t)n;
    return true;
}

/* the alltoallv verdict, as k_fused_a2av takes it after the handshake: the
 * segments run only if every rank voted fits_local */
static inline bool fused_plan_a2av_verdict(const bool *votes, int n)
{
    for (int r = 0; r < n; r++) {
        if (!votes[r]) {
            return false;
        }
    }
    return true;
}

} // namespace ucc

#endif
