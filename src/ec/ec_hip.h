/* Device execution component: gfx950 HIP kernels for n-source reduction,
 * gather-copy, and the fused single-kernel allreduce over xGMI peer
 * pointers. Parity targets: reference components/ec/rocm kernels
 * (ec_rocm_reduce.cu dtype x op family, executor copy_multi) and the NVLS
 * allreduce kernel role (tl/cuda/kernels/allreduce_kernel.cu) — re-designed
 * for CDNA4: 64-wide wavefronts, 16B vector lanes, system-scope atomic
 * arrival flags on fine-grained memory instead of multimem. */
#ifndef UCC_AMD_EC_HIP_H_
#define UCC_AMD_EC_HIP_H_

#include <cstddef>
#include <cstdint>
#include "../api/ucc.h"

struct ihipStream_t;
typedef struct ihipStream_t *hipStream_t;

namespace ucc {
namespace ec_hip {

constexpr int kMaxSrcs  = 8;
constexpr int kMaxRanks = 8;

/* dst[i] = alpha * op(srcs[0][i] .. srcs[n-1][i]); dt/op per ucc enums. */
struct ReduceArgs {
    void        *dst;
    const void  *srcs[kMaxSrcs];
    int          n_srcs;
    uint64_t     count;
    ucc_datatype_t     dt;
    ucc_reduction_op_t op;
    double      alpha;
};
ucc_status_t reduce(const ReduceArgs &a, hipStream_t stream);
/* launches of reduce() so far that took the element-wise kernel
 * (k_reduce_scalar) because dst or a source is not 16-byte aligned; the
 * tests of that kernel read it to prove that it ran */
uint64_t reduce_scalar_launches();

/* Gather-copy: dst_base+off[i] <- srcs[i], len[i] bytes, i in [0,n). */
struct GatherArgs {
    void       *dst_base;
    const void *srcs[kMaxSrcs];
    uint64_t    offs[kMaxSrcs];
    uint64_t    lens[kMaxSrcs];
    int         n;
};
/* blocks_used, if given, receives the grid that was launched */
ucc_status_t gather_copy(const GatherArgs &a, hipStream_t stream,
                         int *blocks_used = nullptr);
/* The grid gather_copy() launches for these arguments (256 threads per
 * block): sized from the total bytes, which the kernel then deals evenly
 * over the sources. Reads n and lens only; pure host code, no device
 * needed. The copy tests take the grid from here to work out which loops
 * of the kernel a case reaches. */
int gather_copy_blocks(const GatherArgs &a);

/* Fused small-message allreduce: one kernel per rank that stages src into
 * its scratch, signals arrival on every peer's flag array (system-scope),
 * waits for all arrivals, then reduces all peers' scratch into dst.
 * flags layout: u64[slot * kMaxRanks + src_rank], monotonically increasing
 * seq values (never reset). */
struct FusedArgs {
    const void *src;
    void       *dst;
    uint64_t    count;
    void       *my_scratch;
    const void *peer_scratch[kMaxRanks];
    uint64_t   *local_flags;
    uint64_t   *peer_flags[kMaxRanks];
    int         rank, nranks, slot;
    uint64_t    seq;
    uint64_t    stage_target; /* cumulative block arrivals for this slot
                                 including this launch (host-tracked)   */
    ucc_datatype_t     dt;
    ucc_reduction_op_t op;
    double      alpha;
    uint64_t   *error_word; /* local fine-grained word set on spin timeout */
    int         nblocks;    /* workgroups; each handles a count slice     */
    uint64_t    spin_limit; /* 0 = default kSpinLimit                     */
    /* host-pinned completion flag: the LAST block (cumulative arrival
     * counter at flags[kFusedDoneBase + slot] reaching done_target)
     * release-stores done_seq here — the host polls plain memory
     * instead of hipEventRecord+Query (µs-class latency saving on the
     * small-message path). */
    uint64_t   *done_host;
    uint64_t    done_seq;
    uint64_t    done_target;
};
ucc_status_t fused_allreduce(const FusedArgs &a, hipStream_t stream);

/* Graph-capturable fused allreduce: identical to fused_allreduce but the
 * per-iteration sequence number is derived ON DEVICE from per-block launch
 * counters (flags u64[kGraphCntBase + slot*kMaxGraphBlocks + block]), so
 * the SAME launch can be captured once into a hipGraph and replayed: every
 * replay is a new collective iteration. Requires a slot dedicated to one
 * persistent request (all ranks replay in lockstep). */
constexpr int kMaxGraphBlocks = 64;
constexpr int kStageCntBase   = 8 * kMaxRanks;      /* u64 idx of stage cnts */
constexpr int kGraphCntBase   = 128;                /* u64 idx of blk cnts   */
constexpr int kFlagsBytes     = 131072;             /* flags alloc size
                                    (>= 8*(kGatedMirrorBase + 3*8*2*8)) */

struct GraphFusedArgs {
    const void *src;
    void       *dst;
    uint64_t    count;
    void       *my_scratch;
    const void *peer_scratch[kMaxRanks];
    uint64_t   *local_flags;
    uint64_t   *peer_flags[kMaxRanks];
    int         rank, nranks, slot;
    ucc_datatype_t     dt;
    ucc_reduction_op_t op;
    double      alpha;
    uint64_t   *error_word;
    int         nblocks;       /* <= kMaxGraphBlocks */
    uint64_t    parity_stride; /* bytes between parity-0 and parity-1
                                  staging areas: iteration i stages into
                                  base + (i&1)*parity_stride so a peer's
                                  replay i+1 never overwrites data still
                                  being read for replay i */
};
ucc_status_t fused_allreduce_graph(const GraphFusedArgs &a,
                                   hipStream_t stream);

/* Fused small-message allgather / reduce_scatter / alltoall / bcast /
 * reduce: the fused allreduce's protocol on the same flag words and
 * counters (so both compose on one slot sequence), with what is staged and
 * what is read given by a plan (src/tl/cdna4/fused_plan.h):
 *   1. copy n_cells cells src + c_src_off[k] -> my_scratch + c_sc_off[k]
 *   2. handshake with every rank (every rank, also one with no cell and
 *      no segment)
 *   3. copy n_segs segments peer_scratch[g_peer[k]] + g_sc_off[k] ->
 *      dst + g_dst_off[k]; and, when r_count != 0, reduce r_count elements
 *      at r_sc_off of all nranks scratch areas, ranks 0..n-1 in order, into
 *      dst + r_dst_off (dtype x op as in reduce(); op 12 is SUM with
 *      alpha).
 * Every scratch offset is a multiple of 16. src and dst may have any
 * alignment: an access whose user side is not 16-byte aligned goes byte by
 * byte resp. element by element, and no access falls outside a cell or a
 * segment. dt and op matter only when r_count != 0.
 *
 * fused_coll(): host-sequenced, the FusedArgs fields seq / stage_target /
 * spin_limit / done_*. fused_coll_graph(): iteration number from the
 * per-block launch counters and parity staging as in GraphFusedArgs; the
 * host-sequencing fields are ignored. */
struct FusedCollArgs {
    const void *src;
    void       *dst;
    void       *my_scratch;
    const void *peer_scratch[kMaxRanks];
    uint64_t   *local_flags;
    uint64_t   *peer_flags[kMaxRanks];
    int         rank, nranks, slot;
    int         n_cells, n_segs;
    uint64_t    c_src_off[kMaxRanks], c_sc_off[kMaxRanks], c_len[kMaxRanks];
    int         g_peer[kMaxRanks];
    uint64_t    g_sc_off[kMaxRanks], g_dst_off[kMaxRanks], g_len[kMaxRanks];
    uint64_t    r_sc_off, r_dst_off, r_count;
    ucc_datatype_t     dt;
    ucc_reduction_op_t op;
    double      alpha;
    uint64_t   *error_word;
    int         nblocks;      /* graph: <= kMaxGraphBlocks                 */
    /* host-sequenced only */
    uint64_t    seq, stage_target, spin_limit;
    uint64_t   *done_host;
    uint64_t    done_seq, done_target;
    /* graph only */
    uint64_t    parity_stride;
};
ucc_status_t fused_coll(const FusedCollArgs &a, hipStream_t stream);
ucc_status_t fused_coll_graph(const FusedCollArgs &a, hipStream_t stream);

/* Fused small-message alltoallv (k_fused_a2av, host-sequenced only). No rank
 * can tell from its own send row and recv column whether every pair fits a
 * scratch cell, so the ranks vote inside the kernel:
 *   1. thread 0 of block 0 stores my vote, 2 * seq + fits_local, into the
 *      16-byte header at my_scratch + 0; a rank that fits stages its cells
 *      (c.n_cells, as fused_coll), a rank that does not stages nothing
 *   2. the handshake of fused_coll, whatever the vote
 *   3. every block reads the nranks headers: the verdict is "fits" iff every
 *      vote is 2 * seq + 1
 *   4. "fits": copy the c.n_segs segments; otherwise dst is not touched
 *   5. the last block stores 2 * done_seq + verdict to *verdict_host
 *      (host-pinned), then release-stores the completion word.
 * c is a plan of fused_plan_init_v(FUSED_ALLTOALLV): cells and segments lie
 * behind the header; r_count must be 0. error_word keeps its meaning
 * (handshake timeout); the verdict never touches it. */
struct FusedA2avArgs {
    FusedCollArgs c;
    int           fits_local;
    uint64_t     *verdict_host;
};
ucc_status_t fused_a2av(const FusedA2avArgs &a, hipStream_t stream);

/* Fused small-message gather and scatter run fused_coll() /
 * fused_coll_graph() with their plans (fused_plan.h). gatherv and scatterv
 * (k_fused_rooted_v, host-sequenced only): the counts are known at the root
 * only, so the root publishes its verdict, and for scatterv where each
 * rank's block lies, in a header at offset 0 of its scratch: word 0 the
 * verdict, then nranks entries (scratch_off, len), two u64 at 16 + 16 * r
 * (kRootedHdrBytes bytes in all; the cells lie behind it).
 *   1. at the root, thread 0 of block 0 stores the table (tab_off, tab_len),
 *      then the verdict 2 * seq + fits_local; every rank whose fits_local is
 *      set stages its c.n_cells cells
 *   2. the handshake of fused_coll, whatever was voted
 *   3. every block reads word 0 of the root's header: "fits" iff it is
 *      2 * seq + 1; a non-root of scatterv then reads its entry
 *   4. "fits": the root of gatherv, and the root of a not-in-place scatterv,
 *      copy their c.n_segs segments; a non-root of scatterv copies
 *      min(entry len, my_len) bytes from the root's scratch + entry off to
 *      dst, or nothing if the entry does not lie 16-byte aligned inside
 *      [kRootedHdrBytes, kRootedHdrBytes + bound]. Otherwise dst is not
 *      touched.
 *   5. completion as fused_a2av: 2 * done_seq + verdict to *verdict_host,
 *      then the release store of the completion word.
 * No rank reads or writes a scratch byte at or past kRootedHdrBytes + bound
 * or a dst byte past its own plan, whatever the other ranks' counts: the
 * launcher refuses cells and segments that leave the area. c is a plan of
 * fused_plan_init_rooted_v; c.r_count must be 0. */
constexpr uint64_t kRootedHdrBytes = 16 + 16 * (uint64_t)kMaxRanks;
struct FusedRootedVArgs {
    FusedCollArgs c;
    int           root;
    int           is_scatter;
    int           fits_local;
    uint64_t      my_len; /* scatterv non-root: bytes my dst holds        */
    uint64_t      bound;  /* B of fused_plan.h                            */
    uint64_t      tab_off[kMaxRanks], tab_len[kMaxRanks]; /* root only    */
    uint64_t     *verdict_host;
};
ucc_status_t fused_rooted_v(const FusedRootedVArgs &a, hipStream_t stream);

bool dt_supported(ucc_datatype_t dt);
bool op_supported(ucc_datatype_t dt, ucc_reduction_op_t op);

/* ------------------------------------------------------------------------
 * Device-gated staged pipeline (large-message allreduce fast path).
 *
 * Replaces the host-polled shm gating of the staged-linear algorithm with
 * kernel-prologue spins on per-(slot,parity,phase) cumulative block
 * counters in each rank's fine-grained flags buffer: the host enqueues
 * stage/reduce/gather kernels for EVERY fragment up front (two streams)
 * and waits for one trailing event — no host round trips inside the
 * collective. Targets are host-computed cumulative launch counts
 * (collectives post in the same order on every rank), x kGatedBlocks
 * block-increments per launch.
 *
 * Counter layout in the flags buffer (u64 index):
 *   kGatedCntBase + (phase * kGatedSlots + slot) * 2 + parity
 *   phase: 0=stage 1=reduce 2=gather; slot < kGatedSlots; parity = frag&1.
 */
constexpr int kGatedBlocks    = 64;  /* default grid (UCC_TL_CDNA4_GATED_BLOCKS) */
constexpr int kGatedMaxBlocks = 512; /* flag-layout bound for the knob   */
constexpr int kGatedSlots     = 8;
constexpr int kGatedCntBase   = 704;  /* after graph counters (128..639) */
/* per-(slot,parity,block) launch counters for the graph-replayable gated
 * mode: u64 idx kGatedGraphBase + ((slot*2)+parity)*kGatedMaxBlocks + block
 * -> 1024..9215 */
constexpr int kGatedGraphBase = 1024;
/* push-model mirrors: rank r's phase counter value, WRITTEN BY RANK r
 * over xGMI into every peer's flag buffer when its last block arrives,
 * so waiters poll LOCAL memory only (B x n remote pollers would steal
 * link bandwidth - the fused kernel already works this way).
 * u64 idx kGatedMirrorBase + ((phase*kGatedSlots+slot)*2+parity)*kMaxRanks
 *         + src_rank -> 9216..9599 */
constexpr int kGatedMirrorBase = 9216;
/* fused-kernel completion arrival counters: u64 idx
 * kFusedDoneBase + slot -> 9600..9607 */
constexpr int kFusedDoneBase = 9600;

/* default device spin bound (iterations of the bounded wait loops);
 * host-side team setup scales it by the xGMI hop count of the farthest
 * peer before passing it down via GatedArgs/FusedArgs.spin_limit */
constexpr uint64_t kDefaultSpinLimit = 200u * 1000u * 1000u;

struct GatedArgs {
    /* data */
    const void *src;      /* stage: user src frag; others unused        */
    void       *dst;      /* gather: user dst frag; others unused       */
    void       *my_in;    /* my in[slot][parity] staging area           */
    void       *my_out;   /* my out[slot][parity] reduced-slice area    */
    const void *peer_in[kMaxRanks];  /* peers' in areas (xGMI)          */
    const void *peer_out[kMaxRanks]; /* peers' out areas (xGMI)         */
    uint64_t   *local_flags;
    uint64_t   *peer_flags[kMaxRanks];
    uint64_t   *error_word;
    uint64_t    len;     /* fragment bytes                              */
    uint64_t    sl_b, sl_e; /* my reduce slice [begin,end) bytes        */
    /* per-rank slice table for gather (byte offsets into out areas)    */
    uint64_t    slice_b[kMaxRanks], slice_e[kMaxRanks];
    int         rank, nranks, slot, parity;
    ucc_datatype_t     dt;
    ucc_reduction_op_t op;
    double      alpha;
    /* cumulative block-count targets (host-tracked). Counters are shared
     * by every gated collective type on a (slot,parity), so area-reuse
     * waits cover BOTH possible consumer phases:
     *   stage  waits reduce_cnt >= t_sw_reduce AND
     *                gather_cnt >= t_sw_gather   (in-area reuse)
     *   reduce waits stage_cnt  >= t_stage AND
     *                gather_cnt >= t_prev_gather (out-area reuse)
     *   gather waits phase gw_phase >= t_gather_wait
     *                (1=reduce for allreduce, 0=stage for ag/alltoall) */
    uint64_t    t_sw_reduce, t_sw_gather, t_prev_gather, t_stage,
                t_gather_wait;
    /* post-launch cumulative counter values for THIS launch's signal
     * phase (stage=0/reduce=1/gather=2): the block whose increment
     * reaches the value is the last arriver and pushes the mirrors.
     * Counters accumulate BLOCK counts, so collectives with different
     * grid sizes compose on the same (slot,parity). Derive mode
     * computes these on device as u*B instead. */
    uint64_t    t_sig_stage, t_sig_reduce, t_sig_gather;
    int         gw_phase;
    /* Graph-replayable mode (persistent colls on a dedicated slot): when
     * derive != 0, targets are computed ON DEVICE from per-block launch
     * counters at kGatedGraphBase (one counter per (slot,parity,block),
     * incremented by EVERY gated kernel of the pattern): this block's
     * count v gives the iteration u = (v-1)/pp + 1 and the host targets
     * above are ignored — so one capture replays forever. pp = kernels
     * per (slot,parity) iteration (3 for allreduce, 2 for rs/ag/a2a);
     * has_reduce/has_gather describe the pattern so waits on phases that
     * never launch resolve to zero. */
    int         derive, pp, has_reduce, has_gather;
    /* write-based distribution (zero-copy allreduce): reduce writes its
     * slice DIRECTLY into every rank's user dst (peer_out[r] =
     * mapped dst + frag_off + my_slice_off) instead of the local out
     * area; the gather launch degenerates to a pure wait+signal. */
    int         zc_write;
    int         nblocks;    /* gated grid size (team-lifetime constant,
                               same on every rank; <= kGatedMaxBlocks;
                               0 = kGatedBlocks default) */
    int         pull_wait;  /* 1 = poll peers' counters remotely instead
                               of local mirrors (debug fallback) */
    int         zc_stream;  /* zc_allreduce / zc_data, read by the
                               launcher only: 1 = the streamed (non-
                               temporal) data phase where one is
                               instantiated, see zc_has_stream() */
    /* host-pinned completion (set ONLY on the final kernel of a
     * host-posted collective): the last arriving block release-stores
     * done_seq after its signal push — host polls plain memory instead
     * of a trailing hipEvent. */
    uint64_t   *done_host;
    uint64_t    done_seq;
    uint64_t    spin_limit; /* 0 = default kSpinLimit */
    /* per-dest cell staging (alltoall): my_in[c_dst_off[k]] <-
     * src[c_src_off[k]], c_len[k] bytes; 0 = contiguous stage of len   */
    int         n_cells;
    uint64_t    c_src_off[kMaxRanks], c_dst_off[kMaxRanks],
                c_len[kMaxRanks];
};

ucc_status_t staged_stage(const GatedArgs &a, hipStream_t s);
ucc_status_t staged_reduce(const GatedArgs &a, hipStream_t s);
ucc_status_t staged_gather(const GatedArgs &a, hipStream_t s);
/* Fused zero-copy allreduce / reduce_scatter: ONE launch of a.nblocks
 * blocks in place of staged_stage (1 block) + staged_reduce +
 * staged_gather (1 block) resp. gated_wait_only. Host-target mode only
 * (derive == 0). Takes the reduce launch's GatedArgs (peer_in = peers'
 * user src, zc_write = 1 with peer_out = every rank's dst slice for
 * allreduce; zc_write = 0 with my_out = my user dst for reduce_scatter)
 * plus done_host/done_seq. Counter effects: phase 0 +1, phase 1
 * +nblocks, and for allreduce phase 2 +1 — those of the launches it
 * replaces. */
ucc_status_t zc_allreduce(const GatedArgs &a, hipStream_t s);
/* The data phase of zc_allreduce alone (k_zc_data): same device code and
 * the same depth selection, but no flag is read or written, so it needs
 * no peer and no team. Reads peer_in[0..nranks) + sl_b, writes
 * peer_out[0..nranks) (zc_write = 1) or my_out (zc_write = 0); uses
 * sl_b, sl_e, nranks, dt, op, alpha and nblocks and nothing else of `a`.
 * threads: 64, 128 or 256 per block, 0 = what zc_allreduce would use.
 * Measurement probe and kernel unit-test hook. Unlike zc_allreduce, which
 * quietly runs plain, zc_data with zc_stream set and no streamed
 * instantiation for this rank count returns UCC_ERR_NOT_SUPPORTED. */
ucc_status_t zc_data(const GatedArgs &a, hipStream_t s, int threads = 0);
/* Whether zc_allreduce honours GatedArgs.zc_stream for this rank count:
 * the streamed data phase (non-temporal batch loads of the peers' src and
 * batch stores to the dsts) is instantiated at depth 4 only, i.e. 2 ranks
 * at the default depth, the one case measured
 * (profiles/zc_edges_stream.md). */
bool zc_has_stream(int nranks);
/* The batching depth U (4, 2 or 1) that zc_allreduce and zc_data run at
 * for this rank count, UCC_EC_REDUCE_DEPTH included. The host needs it
 * to size the grid: how many blocks of k_zc_allreduce a CU holds depends
 * on U (every U = 4 instantiation compiles to at least 2 waves/SIMD,
 * some U = 2 ones to 1). */
int zc_depth(int nranks);
/* Gated bcast, the copy-only slice phase (docs/GATED_PIPELINE.md "Rooted
 * collectives"). All three move bytes [sl_b, sl_e) of ONE source,
 * peer_in[0] + sl_b, in 16-byte packs: to my_out (zc_write = 0) or to
 * every non-null peer_out[s], s < nranks (zc_write = 1; a null entry, the
 * root's own, is skipped). peer_in[0] + sl_b and every destination must be
 * 16-byte aligned; dt, op and alpha are ignored.
 *  staged_bscatter: the launch staged_reduce is in the allreduce pattern
 *    (waits stage and out-area reuse, signals phase 1 with the full grid;
 *    host-target and derive mode).
 *  zc_bcast: ONE launch per zero-copy post, the protocol and counter
 *    effects of zc_allreduce with zc_write = 1 (phase 0 +1, phase 1
 *    +nblocks, phase 2 +1) plus done_host/done_seq. Host-target mode and
 *    zc_write = 1 only.
 *  bcast_data: the data phase alone (k_bcast_data), no flag read or
 *    written; uses peer_in[0], my_out / peer_out, sl_b, sl_e, nranks,
 *    zc_write and nblocks and nothing else of `a`. threads: 64, 128 or
 *    256 per block, 0 = 256. Measurement probe and unit-test hook. */
ucc_status_t staged_bscatter(const GatedArgs &a, hipStream_t s);
ucc_status_t zc_bcast(const GatedArgs &a, hipStream_t s);
ucc_status_t bcast_data(const GatedArgs &a, hipStream_t s, int threads = 0);
/* copy-engine gating (SDMA data path): pure wait on gw_phase/t_gather_wait
 * (1 block), and signal-phase-2-then-wait-team (full gated grid). */
ucc_status_t gated_wait_only(const GatedArgs &a, hipStream_t s);
ucc_status_t gated_done(const GatedArgs &a, hipStream_t s);

/* ------------------------------------------------------------------------
 * p2p pull (device active-set bcast): dst <- src, len bytes, src usually a
 * peer mapping. src and dst alignment are independent. The kernel never
 * waits on anything; the host gates the launch.
 *
 * Completion follows FusedArgs.done_host: every block adds 1 to the
 * device-scope counter *arrive_cnt, which is never reset; the block whose
 * add reaches done_target (host-tracked: the sum of nblocks over every
 * launch on this counter so far, this one included) release-stores
 * done_seq to the host-pinned word done_host. Launches that share a
 * counter must be ordered on one stream. The counter is an allocation of
 * the caller's own, apart from the flags buffer laid out above.
 * len == 0 is legal: the kernel then only publishes completion. */
constexpr int      kP2pMaxBlocks  = 1024; /* bound for the blocks knob   */
/* auto grid: one block per kP2pBlockBytes (four 4-deep batches of 256
 * lanes x 16 B), capped. Both values come from the measured block-count
 * sweep in profiles/p2p_active_set.md: 16 blocks were fastest at 1 MiB,
 * 64 at 64 MiB. */
constexpr uint64_t kP2pBlockBytes    = 65536;
constexpr int      kP2pAutoMaxBlocks = 64;
struct P2pPullArgs {
    void       *dst;
    const void *src;
    uint64_t    len;
    uint64_t   *arrive_cnt;
    uint64_t    done_target;
    uint64_t   *done_host;
    uint64_t    done_seq;
    int         nblocks; /* 1..kP2pMaxBlocks */
};
int          p2p_auto_blocks(uint64_t len);
ucc_status_t p2p_pull(const P2pPullArgs &a, hipStream_t stream);

/* ------------------------------------------------------------------------
 * Ring step (host-gated multi-ring reduce_scatter / allgather / allreduce,
 * src/tl/cdna4/ring_plan.h): ONE launch serves every ring of one step, its
 * workgroups dealt over the pieces by size. The kernel never waits, reads
 * no flag and does no atomic; the host gates the launch and completion is
 * the stream event.
 *
 * Per element of a piece, T the datatype and A its accumulator type
 * (Cvt<T>::A: f32 for the 8/16-bit floats, else T):
 *   acc = op(in, local) when both are given, else the one that is given;
 *         `in` is read as A when in_acc, else as T and widened; `local` is
 *         always T.
 *   dst gets T: alpha * acc converted once (docs/USER_GUIDE.md, "Reduction
 *         numerics").
 *   out gets the raw accumulator (no alpha, no rounding) when out_acc, else
 *         exactly the bits dst gets.
 * The travelling partial stays in A so that the ring rounds once, at the
 * final store, like every other reduction here — not once per hop.
 *
 * With local == nullptr in every piece and in_acc = out_acc = 0 the step is
 * a byte copy (one load, up to two stores per pack); dt only gives the
 * element size and op is ignored.
 *
 * Any count is legal, 0 included; null `out` / `dst` are skipped. A piece
 * whose non-null pointers are all 16-byte aligned moves 16-byte packs of T,
 * any other goes element by element. No access falls outside
 * [ptr, ptr + count) of any buffer. dtype x op as in reduce(); op 12 is SUM
 * with alpha. */
constexpr int kMaxRings = 4;
struct RingPiece {
    const void *in;
    const void *local;
    void       *out;
    void       *dst;
    uint64_t    count;
};
struct RingStepArgs {
    RingPiece          piece[kMaxRings];
    int                n_rings;
    ucc_datatype_t     dt;
    ucc_reduction_op_t op;
    double             alpha;
    int                in_acc, out_acc;
    int                nblocks; /* grid size; 0 = size-derived */
};
ucc_status_t ring_step(const RingStepArgs &a, hipStream_t s);
/* ring_step() calls accepted so far (a step whose pieces are all empty
 * launches nothing and still counts); the ring tests read it to prove that
 * the ring ran and how many steps it took */
uint64_t ring_step_launches();

} // namespace ec_hip
} // namespace ucc

#endif
