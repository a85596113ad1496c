/* Grid size and cache policy of tl/cdna4's gated collectives: one pure
 * function of what the task knows at set-up, host-only and free of every
 * other header of the library, so tests/native/test_zc_policy.cc can
 * tabulate it without a GPU. tl_cdna4.cc calls it and carries no copy of
 * the rule.
 *
 * Both results are per-task constants. `blocks` enters the launch ledger
 * (phase 1 counts blocks), so every input it depends on has to agree on
 * all ranks: the collective, the rank count, the message size, the
 * GATED_BLOCKS knob and the depth (UCC_EC_REDUCE_DEPTH). `stream` only
 * picks which instantiation of the same kernel a rank launches; it does
 * not enter the ledger and may differ between ranks. */
#ifndef UCC_AMD_TL_CDNA4_ZC_POLICY_H
#define UCC_AMD_TL_CDNA4_ZC_POLICY_H

#include <cstdint>

namespace ucc {
namespace tl_cdna4 {

enum ZcColl {
    ZC_COLL_ALLREDUCE,      /* k_zc_allreduce, zc_write = 1              */
    ZC_COLL_REDUCE_SCATTER, /* k_zc_allreduce, zc_write = 0              */
    ZC_COLL_REDUCE,         /* rooted: k_zc_allreduce into the root's dst */
    ZC_COLL_BCAST,          /* rooted: k_zc_bcast (a copy, no NT form)   */
    ZC_COLL_OTHER           /* allgather, alltoall, ...                  */
};

/* UCC_TL_CDNA4_ZC_STREAM */
enum ZcStreamKnob { ZC_STREAM_AUTO = -1, ZC_STREAM_OFF = 0, ZC_STREAM_ON = 1 };

constexpr int      kZcBlocksDefault = 64;  /* = ec_hip::kGatedBlocks */
constexpr int      kZcBlocksLarge   = 128; /* single fragment >= 160 MiB */
constexpr int      kZcBlocksBigAr   = 192; /* 2-rank depth-4 allreduce   */
constexpr uint64_t kZcMiB           = 1024 * 1024;
constexpr uint64_t kZcBigArMin      = 128 * kZcMiB;
constexpr uint64_t kZcLargeMin      = 160 * kZcMiB;

struct ZcPolicy {
    int  blocks; /* gated kernel grid                                    */
    bool stream; /* GatedArgs.zc_stream: non-temporal data phase         */
};

/* ct          the collective
 * one_kernel  the task runs the one-kernel zero-copy path (zero-copy ready,
 *             one fragment, host-posted, ZC_FUSED on)
 * n           team size
 * depth       ec_hip::zc_depth(n): the batching depth the launcher picks
 * total       message bytes
 * single_frag the task runs as one fragment
 * blocks_ov   UCC_TL_CDNA4_GATED_BLOCKS, 0 = unset
 * knob        UCC_TL_CDNA4_ZC_STREAM
 *
 * Grid, measured on the 2-process rig: 64 blocks; 128 from 160 MiB up
 * for a single fragment (profiles/rocprof_kernels_r02.md); 192 from
 * 128 MiB up for the one-kernel allreduce of 2 ranks at depth 4
 * (profiles/zc_data_phase.md). The streamed case keeps 192: 256 blocks
 * did not beat 192 in every run at 128 or at 256 MiB
 * (profiles/zc_edges_stream.md, "Grid"). The override wins over all of
 * them.
 *
 * Cache policy: streaming from the same 128 MiB in the same case, the
 * only one measured (at 256 MiB every streamed run beat every plain
 * one, 5 % in the median; the 128 MiB bound is the earlier note's).
 * There the four buffers (two src, two dst) no longer fit the 256 MiB
 * Infinity Cache; at 32 and 64 MiB they do, and streaming them was
 * measured 20-30 % slower. Reduce_scatter, rooted
 * reduce, three or more ranks and the three-kernel path are unmeasured
 * and stay plain. ZC_STREAM_ON streams wherever k_zc_allreduce has a
 * streamed instantiation (depth 4), at any size; ZC_STREAM_OFF never. */
inline ZcPolicy zc_policy(ZcColl ct, bool one_kernel, int n, int depth,
                          uint64_t total, bool single_frag, int blocks_ov,
                          int knob)
{
    const bool big_ar = one_kernel && ct == ZC_COLL_ALLREDUCE && n == 2 &&
                        depth == 4 && total >= kZcBigArMin;
    const bool has_nt = one_kernel && depth == 4 && n >= 2 &&
                        (ct == ZC_COLL_ALLREDUCE ||
                         ct == ZC_COLL_REDUCE_SCATTER ||
                         ct == ZC_COLL_REDUCE);
    ZcPolicy p;
    p.blocks = blocks_ov > 0                           ? blocks_ov
               : big_ar                                ? kZcBlocksBigAr
               : single_frag && total >= kZcLargeMin   ? kZcBlocksLarge
                                                       : kZcBlocksDefault;
    p.stream = knob == ZC_STREAM_OFF  ? false
               : knob == ZC_STREAM_ON ? has_nt
                                      : big_ar;
    return p;
}

} // namespace tl_cdna4
} // namespace ucc

#endif
