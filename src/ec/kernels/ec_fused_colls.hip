/* gfx950 execution-component kernels: the fused small-message allgather,
 * reduce_scatter, alltoall, bcast and reduce, host-sequenced (k_fused_coll)
 * and graph-capturable (k_fused_coll_graph). One body, two kernels; the
 * sequencing, handshake and completion steps are the fused allreduce's
 * (ec_device.h, "fused one-kernel protocol"). allgatherv and
 * reduce_scatterv, gather and scatter run the same kernels with another
 * plan; alltoallv has the host-sequenced k_fused_a2av, gatherv and scatterv
 * the host-sequenced k_fused_rooted_v, at the end of this file. */
#include "ec_device.h"

namespace ucc {
namespace ec_hip {

/* Stage my cells into my scratch, signal every peer, wait for all arrivals,
 * then copy my segments out of the peers' scratch (RED = false) or reduce
 * all peers' scratch into dst (RED = true). Every rank runs the handshake,
 * whatever it stages or reads: the parity argument of graph mode (below)
 * needs every rank in every handshake.
 *
 * Alignment: every scratch address is 16-byte aligned (chunk-aligned area,
 * parity stride and plan offsets are multiples of 16), so only the user side
 * decides. d_copy_bytes moves 16-byte packs, 4 loads in flight, when both
 * sides are aligned and bytes otherwise; the reduction stores packs when dst
 * is aligned and elements otherwise.
 *
 * `a` is the kernel's by-value argument and stays const (see the note at
 * GatedTargets in ec_gated.hip). */
template <typename T, int OP, int VEC, bool DEV_SEQ, bool RED>
__device__ __forceinline__ void fused_coll_body(const FusedCollArgs &a)
{
    const FusedIter it = fused_iter<DEV_SEQ>(a);
    /* 1. stage my cells (all blocks, grid-stride; the parity area of this
     * iteration) */
    uint8_t *mysc = (uint8_t *)a.my_scratch + it.par;
    for (int k = 0; k < a.n_cells; k++) {
        d_copy_bytes(mysc + a.c_sc_off[k],
                     (const uint8_t *)a.src + a.c_src_off[k], a.c_len[k]);
    }
    /* 2.-3. publish, signal every peer, wait for all ranks */
    if (!fused_handshake(a, it)) {
        return;
    }
    /* 4. read the peers' scratch (this iteration's parity). Why parity is
     * sufficient: a peer can start staging replay i+1 while I still read
     * its replay-i data, but it writes the other parity area. It cannot
     * reach replay i+2 until the i+1 handshake completed, which needs MY
     * i+1 launch — stream-ordered after my reads of i finished. */
    if constexpr (RED) {
        if (a.r_count) {
            uint8_t       *dst = (uint8_t *)a.dst + a.r_dst_off;
            const uint64_t off = it.par + a.r_sc_off;
            if (((uintptr_t)dst & 15) == 0) {
                reduce_range<T, OP, VEC>(dst, a.peer_scratch, off, a.nranks,
                                         a.r_count, a.alpha);
            } else {
                const uint64_t tid =
                    (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
                const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
                for (uint64_t t = tid; t < a.r_count; t += str) {
                    ((T *)dst)[t] = reduce_elem<T, OP>(a.peer_scratch, off,
                                                      a.nranks, t, a.alpha);
                }
            }
        }
    } else {
        for (int k = 0; k < a.n_segs; k++) {
            d_copy_bytes((uint8_t *)a.dst + a.g_dst_off[k],
                         (const uint8_t *)a.peer_scratch[a.g_peer[k]] +
                             it.par + a.g_sc_off[k],
                         a.g_len[k]);
        }
    }
    /* 5. host-visible completion */
    if constexpr (!DEV_SEQ) {
        fused_publish_done(a);
    }
}

template <typename T, int OP, int VEC, bool RED>
__global__ void k_fused_coll(FusedCollArgs a)
{
    fused_coll_body<T, OP, VEC, false, RED>(a);
}

template <typename T, int OP, int VEC, bool RED>
__global__ void k_fused_coll_graph(FusedCollArgs a)
{
    fused_coll_body<T, OP, VEC, true, RED>(a);
}

/* ----------------------------------------------------------- launchers */
template <typename T, int OP> struct LaunchFusedRed {
    static ucc_status_t run(const FusedCollArgs &a, hipStream_t s)
    {
        hipLaunchKernelGGL((k_fused_coll<T, OP, VecOf<T>::value, true>),
                           dim3(a.nblocks), dim3(256), 0, s, a);
        return launch_status();
    }
};
template <typename T, int OP> struct LaunchFusedRedGraph {
    static ucc_status_t run(const FusedCollArgs &a, hipStream_t s)
    {
        hipLaunchKernelGGL(
            (k_fused_coll_graph<T, OP, VecOf<T>::value, true>),
            dim3(a.nblocks), dim3(256), 0, s, a);
        return launch_status();
    }
};

static bool fused_coll_args_ok(const FusedCollArgs &a, int max_blocks)
{
    return a.nranks >= 1 && a.nranks <= kMaxRanks && a.rank >= 0 &&
           a.rank < a.nranks && a.n_cells >= 0 && a.n_cells <= kMaxRanks &&
           a.n_segs >= 0 && a.n_segs <= kMaxRanks && a.nblocks >= 1 &&
           a.nblocks <= max_blocks;
}

/* a rank with no reduce segment (every rank of the copy collectives, a
 * non-root of reduce) runs the copy kernel: no dtype, no op */
ucc_status_t fused_coll(const FusedCollArgs &a_in, hipStream_t s)
{
    if (!fused_coll_args_ok(a_in, 1024)) {
        return UCC_ERR_INVALID_PARAM;
    }
    if (a_in.r_count == 0) {
        hipLaunchKernelGGL((k_fused_coll<uint8_t, 0, 16, false>),
                           dim3(a_in.nblocks), dim3(256), 0, s, a_in);
        return launch_status();
    }
    FusedCollArgs a = a_in;
    a.dt            = fold_complex(a.dt, a.op, &a.r_count);
    return dispatch<LaunchFusedRed>(a.dt, a.op, a, s);
}

ucc_status_t fused_coll_graph(const FusedCollArgs &a_in, hipStream_t s)
{
    if (!fused_coll_args_ok(a_in, kMaxGraphBlocks)) {
        return UCC_ERR_INVALID_PARAM;
    }
    if (a_in.r_count == 0) {
        hipLaunchKernelGGL((k_fused_coll_graph<uint8_t, 0, 16, false>),
                           dim3(a_in.nblocks), dim3(256), 0, s, a_in);
        return launch_status();
    }
    FusedCollArgs a = a_in;
    a.dt            = fold_complex(a.dt, a.op, &a.r_count);
    return dispatch<LaunchFusedRedGraph>(a.dt, a.op, a, s);
}

/* ------------------------------------------------------------ alltoallv */
/* The fused alltoallv: the protocol above with a vote (FusedA2avArgs in
 * ec_hip.h). The only waits are the bounded ones of fused_handshake.
 *
 * Why every block of every rank reaches the same verdict: a rank stores its
 * vote before the fence and the arrival add of its block 0, block 0 signals
 * the peers only after that, and a block reads the n headers only after it
 * saw all n signals of this seq. A vote carries the seq, so a header left
 * by an earlier use of the slot never reads as "fits". */
__global__ void k_fused_a2av(FusedA2avArgs a)
{
    const FusedCollArgs &c  = a.c;
    const FusedIter      it = fused_iter<false>(c);
    uint8_t             *mysc = (uint8_t *)c.my_scratch;
    /* 1. my vote, then my cells (none if I do not fit) */
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        sys_store((uint64_t *)mysc, 2 * it.seq + (a.fits_local ? 1 : 0));
    }
    if (a.fits_local) {
        for (int k = 0; k < c.n_cells; k++) {
            d_copy_bytes(mysc + c.c_sc_off[k],
                         (const uint8_t *)c.src + c.c_src_off[k], c.c_len[k]);
        }
    }
    /* 2. every rank takes part, whatever it voted */
    if (!fused_handshake(c, it)) {
        return;
    }
    /* 3. the verdict: n votes through LDS */
    __shared__ int s_unfit;
    if (threadIdx.x == 0) {
        s_unfit = 0;
    }
    __syncthreads();
    if ((int)threadIdx.x < c.nranks &&
        sys_load((const uint64_t *)c.peer_scratch[threadIdx.x]) !=
            2 * it.seq + 1) {
        atomicOr(&s_unfit, 1);
    }
    __syncthreads();
    const bool fits = s_unfit == 0;
    /* 4. my segments, or nothing */
    if (fits) {
        for (int k = 0; k < c.n_segs; k++) {
            d_copy_bytes((uint8_t *)c.dst + c.g_dst_off[k],
                         (const uint8_t *)c.peer_scratch[c.g_peer[k]] +
                             c.g_sc_off[k],
                         c.g_len[k]);
        }
    }
    /* 5. fused_publish_done with the verdict stored before the release */
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t v = __hip_atomic_fetch_add(
                         c.local_flags + kFusedDoneBase + c.slot, 1,
                         __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) +
                     1;
        if (v == c.done_target) {
            sys_store(a.verdict_host, 2 * c.done_seq + (fits ? 1 : 0));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(c.done_host, c.done_seq, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

ucc_status_t fused_a2av(const FusedA2avArgs &a, hipStream_t s)
{
    if (!fused_coll_args_ok(a.c, 1024) || a.c.r_count != 0 ||
        !a.verdict_host || !a.c.done_host) {
        return UCC_ERR_INVALID_PARAM;
    }
    hipLaunchKernelGGL(k_fused_a2av, dim3(a.c.nblocks), dim3(256), 0, s, a);
    return launch_status();
}

/* -------------------------------------------------- gatherv and scatterv */
/* The fused gatherv / scatterv: the protocol above with the root's verdict
 * and, for scatterv, the root's table of where each rank's block lies
 * (FusedRootedVArgs in ec_hip.h). The only waits are the bounded ones of
 * fused_handshake.
 *
 * Why every block of every rank reads this post's table and verdict: thread
 * 0 of the root's block 0 stores the entries and then the verdict before
 * that block's fence and arrival add, block 0 signals the peers only after
 * all of the root's blocks arrived, and a block reads the root's header only
 * after it saw all n signals of this seq. The verdict carries the seq, so a
 * header left by an earlier use of the slot never reads as "fits"; the
 * entries carry none, but they are only read behind a verdict of this seq,
 * and the same thread stored them before it.
 *
 * What a non-root of scatterv reads comes from another rank, so it is
 * checked here and not by the launcher: an entry that is not a 16-byte
 * aligned range inside [kRootedHdrBytes, kRootedHdrBytes + bound] copies
 * nothing, and never more than my_len bytes reach dst.
 *
 * `a` is the kernel's by-value argument and stays const (see the note at
 * GatedTargets in ec_gated.hip). */
__global__ void k_fused_rooted_v(FusedRootedVArgs a)
{
    const FusedCollArgs &c    = a.c;
    const FusedIter      it   = fused_iter<false>(c);
    uint8_t             *mysc = (uint8_t *)c.my_scratch;
    const bool           root = c.rank == a.root;
    /* 1. the root's table, then its verdict; then my cells */
    if (root && blockIdx.x == 0 && threadIdx.x == 0) {
        uint64_t *hdr = (uint64_t *)mysc;
        for (int r = 0; r < c.nranks; r++) {
            sys_store(hdr + 2 + 2 * r, a.tab_off[r]);
            sys_store(hdr + 3 + 2 * r, a.tab_len[r]);
        }
        sys_store(hdr, 2 * it.seq + (a.fits_local ? 1 : 0));
    }
    if (a.fits_local) {
        for (int k = 0; k < c.n_cells; k++) {
            d_copy_bytes(mysc + c.c_sc_off[k],
                         (const uint8_t *)c.src + c.c_src_off[k], c.c_len[k]);
        }
    }
    /* 2. every rank takes part, whatever the root decided */
    if (!fused_handshake(c, it)) {
        return;
    }
    /* 3. the root's verdict and, for a non-root of scatterv, my entry */
    __shared__ uint64_t s_verdict, s_off, s_len;
    if (threadIdx.x == 0) {
        const uint64_t *hdr = (const uint64_t *)c.peer_scratch[a.root];
        s_verdict           = sys_load(hdr);
        s_off = s_len = 0;
        if (a.is_scatter && !root && s_verdict == 2 * it.seq + 1) {
            const uint64_t off = sys_load(hdr + 2 + 2 * c.rank);
            const uint64_t len = sys_load(hdr + 3 + 2 * c.rank);
            const uint64_t end = kRootedHdrBytes + a.bound;
            if (off >= kRootedHdrBytes && (off & 15) == 0 && off <= end &&
                len <= end - off) {
                s_off = off;
                s_len = len < a.my_len ? len : a.my_len;
            }
        }
    }
    __syncthreads();
    const bool fits = s_verdict == 2 * it.seq + 1;
    /* 4. my copies, or nothing */
    if (fits) {
        if (a.is_scatter && !root) {
            d_copy_bytes((uint8_t *)c.dst,
                         (const uint8_t *)c.peer_scratch[a.root] + s_off,
                         s_len);
        } else {
            for (int k = 0; k < c.n_segs; k++) {
                d_copy_bytes((uint8_t *)c.dst + c.g_dst_off[k],
                             (const uint8_t *)c.peer_scratch[c.g_peer[k]] +
                                 c.g_sc_off[k],
                             c.g_len[k]);
            }
        }
    }
    /* 5. as k_fused_a2av: the verdict, then the release of the done word */
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t v = __hip_atomic_fetch_add(
                         c.local_flags + kFusedDoneBase + c.slot, 1,
                         __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) +
                     1;
        if (v == c.done_target) {
            sys_store(a.verdict_host, 2 * c.done_seq + (fits ? 1 : 0));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(c.done_host, c.done_seq, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

/* validates like fused_a2av(), and that no cell and no segment leaves the
 * header + bound area of a scratch: the kernel trusts them */
ucc_status_t fused_rooted_v(const FusedRootedVArgs &a, hipStream_t s)
{
    const uint64_t end = kRootedHdrBytes + a.bound;
    if (!fused_coll_args_ok(a.c, 1024) || a.c.r_count != 0 ||
        !a.verdict_host || !a.c.done_host || a.root < 0 ||
        a.root >= a.c.nranks || a.bound < 16 || (a.bound & 15) != 0 ||
        a.bound > (UINT64_MAX >> 8)) {
        return UCC_ERR_INVALID_PARAM;
    }
    for (int k = 0; k < a.c.n_cells; k++) {
        if (a.c.c_sc_off[k] < kRootedHdrBytes || (a.c.c_sc_off[k] & 15) != 0 ||
            a.c.c_sc_off[k] > end || a.c.c_len[k] > end - a.c.c_sc_off[k]) {
            return UCC_ERR_INVALID_PARAM;
        }
    }
    /* a non-root of scatterv takes its one segment from the root's table */
    const bool table_seg = a.is_scatter && a.c.rank != a.root;
    if (table_seg ? a.c.n_segs > 1
                  : a.c.n_segs > 0 && a.c.rank != a.root) {
        return UCC_ERR_INVALID_PARAM;
    }
    for (int k = 0; !table_seg && k < a.c.n_segs; k++) {
        if (a.c.g_peer[k] < 0 || a.c.g_peer[k] >= a.c.nranks ||
            a.c.g_sc_off[k] < kRootedHdrBytes || (a.c.g_sc_off[k] & 15) != 0 ||
            a.c.g_sc_off[k] > end || a.c.g_len[k] > end - a.c.g_sc_off[k]) {
            return UCC_ERR_INVALID_PARAM;
        }
    }
    hipLaunchKernelGGL(k_fused_rooted_v, dim3(a.c.nblocks), dim3(256), 0, s,
                       a);
    return launch_status();
}

} // namespace ec_hip
} // namespace ucc
