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
 * tests/native/test_fused_plan_v.cc runs it for all ranks.
 *
 * The rooted copy collectives (UCC_TL_CDNA4_FUSED_GATHER_SCATTER). gather and
 * scatter are two more plans of fused_plan_init:
 *   gather          cell 0 = my block, on every rank; the root has n
 *                   segments, peer r's cell 0 -> dst + r * block; a non-root
 *                   has none
 *   scatter         cell d = the root's block for rank d, at the root only;
 *                   rank r has one segment, the root's cell r -> dst + 0
 * In place is significant at the root only (StagedTask::post()'s rules) and
 * is ignored elsewhere: a gather root stages nothing and has no segment for
 * itself, its block already lies at dst + root * block; a scatter root makes
 * no cell and no segment for itself, its block stays in src.
 * gatherv and scatterv, whose counts only the root knows, have
 * fused_plan_init_rooted_v at the end of this file;
 * tests/native/test_fused_plan_rooted.cc runs all four for all ranks. */
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
                 FUSED_ALLTOALLV = 7,
                 /* rooted copies: fused_plan_init (gather, scatter) and
                  * fused_plan_init_rooted_v (gatherv, scatterv) */
                 FUSED_GATHER = 8, FUSED_SCATTER = 9, FUSED_GATHERV = 10,
                 FUSED_SCATTERV = 11 };

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
    /* gatherv / scatterv only (fused_plan_init_rooted_v) */
    uint64_t  bound = 0;       /* B: no scratch access at or past 144 + B  */
    uint64_t  my_len = 0;      /* bytes of my own block                    */
    /* the root's table, (scratch_off, len) per rank */
    uint64_t  tab_off[kFusedMaxRanks] = {}, tab_len[kFusedMaxRanks] = {};
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
    const uint64_t cells = coll == FUSED_REDUCE_SCATTER ||
                                   coll == FUSED_ALLTOALL ||
                                   coll == FUSED_SCATTER
                               ? (uint64_t)n
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
    case FUSED_GATHER: {
        const bool ip = inplace && rank == root;
        if (!ip) {
            p->n_cells     = 1;
            p->cell[0].len = b;
        }
        for (int r = 0; rank == root && r < n; r++) {
            if (ip && r == root) {
                continue;
            }
            FusedSeg &s = p->seg[p->n_segs++];
            s.peer      = r;
            s.dst_off   = (uint64_t)r * b;
            s.len       = b;
        }
        break;
    }
    case FUSED_SCATTER: {
        const bool ip = inplace && rank == root;
        for (int d = 0; rank == root && d < n; d++) {
            if (ip && d == root) {
                continue;
            }
            FusedCell &c  = p->cell[p->n_cells++];
            c.src_off     = (uint64_t)d * b;
            c.scratch_off = (uint64_t)d * stride;
            c.len         = b;
        }
        if (!ip) {
            p->n_segs             = 1;
            p->seg[0].peer        = root;
            p->seg[0].scratch_off = me * stride;
            p->seg[0].len         = b;
        }
        break;
    }
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

/* ------------------------------------------------- gatherv and scatterv
 * The counts are significant at the root only, so no rank but the root can
 * tell whether a request fits, and a non-root of scatterv does not know
 * where its block lies in the root's scratch. The root says both in a header
 * at offset 0 of ITS scratch (only the root's header is ever read):
 *   word 0            the root's verdict, 2 * seq + fits (k_fused_rooted_v)
 *   16 + 16 * r       rank r's entry, two u64: (scratch_off, len)
 * kFusedRootedHdr = 16 + 16 * kFusedMaxRanks bytes; the cells follow.
 *
 * B = fused_plan_rooted_v_bound(bound): what is left of `bound` (the knob,
 * capped by the staging chunk: equal on every rank) after the header, rounded
 * down to 16. scratch_bytes = header + B on every rank, and no access of any
 * rank, whatever the other ranks' counts, touches a byte at or past it.
 *
 *   gatherv   every rank with a non-zero block of at most B bytes stages it
 *             into the one cell at the header's end; a longer block is not
 *             staged. Root: segment r = counts[r] bytes of peer r's cell ->
 *             dst + displs[r]; zero counts are skipped, and the root's own
 *             when in place (the block already lies at dst + displs[root]).
 *             The root fits iff every counts[r] <= B: the bound is on the
 *             largest block, as for allgatherv.
 *   scatterv  root: cell d at header + the running sum of stride(counts[k]),
 *             k < d, from src + displs[d]; zero counts, and the root's own
 *             when in place (the block stays in src), make no cell. The
 *             table holds these offsets and lengths. The root fits iff the
 *             sum of all strides <= B: the bound is on the sum, as for
 *             reduce_scatterv. A root that does not fit stages nothing. A
 *             non-root has one segment of my_len bytes from the root's
 *             scratch to dst + 0 whose scratch offset is NOT in the plan
 *             (scratch_off stays 0): the kernel reads it, and the length the
 *             root meant, from the root's table. A root not in place reads
 *             its own cell, min(counts[root], my_len) bytes.
 * counts / displs: bytes, read at the root only (may be null elsewhere).
 * my_len: bytes of my own block, a non-root's src (gatherv) resp. every
 * not-in-place rank's dst (scatterv); a gatherv root's own length is
 * counts[root]. fits_local: at the root the verdict; at a gatherv non-root
 * whether it staged (my_len <= B). */
constexpr uint64_t kFusedRootedHdr = 16 + 16 * (uint64_t)kFusedMaxRanks;

/* B from the rank-invariant bound; 0: no room */
static inline uint64_t fused_plan_rooted_v_bound(uint64_t bound)
{
    return bound < kFusedRootedHdr + 16
               ? 0
               : (bound - kFusedRootedHdr) & ~(uint64_t)15;
}

/* false: not expressible (rank count, rank, root, a count that is no
 * multiple of the element size, all counts zero at the root, B < 16) */
static inline bool fused_plan_init_rooted_v(FusedPlan *p, FusedColl coll,
                                            int n, int rank, int root,
                                            const uint64_t *counts,
                                            const uint64_t *displs,
                                            uint64_t my_len, uint64_t B,
                                            size_t elem_size, bool inplace)
{
    if (n < 2 || n > kFusedMaxRanks || rank < 0 || rank >= n || root < 0 ||
        root >= n || elem_size == 0 || B < 16 || B % 16 != 0 ||
        B > (UINT64_MAX >> 8) ||
        (coll != FUSED_GATHERV && coll != FUSED_SCATTERV) ||
        (rank == root && (!counts || !displs))) {
        return false;
    }
    *p               = FusedPlan{};
    p->coll          = coll;
    p->n             = n;
    p->rank          = rank;
    p->root          = root;
    p->bound         = B;
    p->scratch_bytes = kFusedRootedHdr + B;
    const bool is_root = rank == root;
    const bool ip      = inplace && is_root;
    if (is_root) {
        uint64_t any = 0, sum = 0;
        bool     each_fits = true;
        for (int r = 0; r < n; r++) {
            if (counts[r] % elem_size != 0) {
                return false;
            }
            any |= counts[r];
            each_fits = each_fits && counts[r] <= B;
            /* saturate: the strides of 8 counts near 2^64 must not wrap */
            sum = counts[r] > B || sum > B ? B + 16
                                           : sum + fused_plan_stride(counts[r]);
        }
        if (!any) {
            return false;
        }
        p->fits_local = coll == FUSED_GATHERV ? each_fits : sum <= B;
    } else if (my_len % elem_size != 0) {
        return false;
    }
    if (coll == FUSED_GATHERV) {
        p->my_len = is_root ? counts[root] : my_len;
        if (!is_root) {
            p->fits_local = p->my_len <= B;
        }
        if (p->fits_local && !ip && p->my_len && p->my_len <= B) {
            p->n_cells             = 1;
            p->cell[0].scratch_off = kFusedRootedHdr;
            p->cell[0].len         = p->my_len;
        }
        for (int r = 0; is_root && r < n; r++) {
            p->tab_off[r] = kFusedRootedHdr;
            p->tab_len[r] = ip && r == root ? 0 : counts[r];
            if (!p->fits_local || !counts[r] || (ip && r == root)) {
                continue;
            }
            FusedSeg &s   = p->seg[p->n_segs++];
            s.peer        = r;
            s.scratch_off = kFusedRootedHdr;
            s.dst_off     = displs[r];
            s.len         = counts[r];
        }
    } else {
        p->my_len = ip ? 0 : my_len;
        uint64_t sc = kFusedRootedHdr;
        for (int d = 0; is_root && p->fits_local && d < n; d++) {
            p->tab_off[d] = sc;
            if (counts[d] && !(ip && d == root)) {
                FusedCell &c  = p->cell[p->n_cells++];
                c.src_off     = displs[d];
                c.scratch_off = sc;
                c.len         = counts[d];
                p->tab_len[d] = counts[d];
            }
            sc += fused_plan_stride(counts[d]);
        }
        const uint64_t own =
            !is_root ? p->my_len
                     : (counts[root] < p->my_len ? counts[root] : p->my_len);
        if (own && (!is_root || p->fits_local)) {
            p->n_segs             = 1;
            p->seg[0].peer        = root;
            p->seg[0].scratch_off = is_root ? p->tab_off[root] : 0;
            p->seg[0].len         = own;
        }
    }
    for (int c = 0; c < p->n_cells; c++) {
        p->stage_bytes += p->cell[c].len;
    }
    for (int s = 0; s < p->n_segs; s++) {
        p->read_bytes += p->seg[s].len;
    }
    return true;
}

/* what k_fused_rooted_v decides and does after the handshake, from the
 * root's plan alone: "fits" is the root's fits_local, and a scatterv
 * non-root whose dst holds my_len bytes copies *len bytes from *off of the
 * root's scratch. An entry that leaves the header + B area copies nothing. */
static inline bool fused_plan_rooted_v_verdict(const FusedPlan &root_plan,
                                               int rank, uint64_t my_len,
                                               uint64_t *off, uint64_t *len)
{
    *off = *len = 0;
    if (!root_plan.fits_local) {
        return false;
    }
    if (root_plan.coll == FUSED_SCATTERV && rank != root_plan.root &&
        rank >= 0 && rank < root_plan.n) {
        const uint64_t o = root_plan.tab_off[rank], l = root_plan.tab_len[rank];
        const uint64_t end = kFusedRootedHdr + root_plan.bound;
        if (o >= kFusedRootedHdr && o % 16 == 0 && o <= end && l <= end - o) {
            *off = o;
            *len = l < my_len ? l : my_len;
        }
    }
    return true;
}

} // namespace ucc

#endif
