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
 * dst_off counts from the user dst. */
#ifndef UCC_AMD_FUSED_PLAN_H_
#define UCC_AMD_FUSED_PLAN_H_

#include <cstddef>
#include <cstdint>

namespace ucc {

constexpr int kFusedMaxRanks = 8;

enum FusedColl { FUSED_ALLGATHER = 0, FUSED_REDUCE_SCATTER = 1,
                 FUSED_ALLTOALL = 2, FUSED_BCAST = 3, FUSED_REDUCE = 4 };

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

} // namespace ucc

#endif
