/* gfx950 execution-component kernels: the fused small-message allgather,
 * reduce_scatter, alltoall, bcast and reduce, host-sequenced (k_fused_coll)
 * and graph-capturable (k_fused_coll_graph). One body, two kernels; the
 * sequencing, handshake and completion steps are the fused allreduce's
 * (ec_device.h, "fused one-kernel protocol"). */
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

} // namespace ec_hip
} // namespace ucc
