/* gfx950 execution-component kernels: the fused small-message allreduce,
 * host-sequenced (k_fused_allreduce) and graph-capturable
 * (k_fused_allreduce_graph). One body, two kernels. */
#include "ec_device.h"

namespace ucc {
namespace ec_hip {

/* Stage src into my scratch, signal every peer, wait for all arrivals,
 * reduce all peers' scratch into dst.
 *
 * DEV_SEQ = false (FusedArgs): the host tracks the sequence number, the
 * cumulative stage target and the spin limit, and may ask for the
 * host-visible completion word.
 * DEV_SEQ = true (GraphFusedArgs): the iteration number is this block's
 * launch count, so one captured launch replays as a new collective each
 * time; staging alternates between two parity areas; the spin cap is the
 * default.
 *
 * `a` is the kernel's by-value argument and stays const (see the note at
 * GatedTargets in ec_gated.hip). */
template <typename T, int OP, int VEC, bool DEV_SEQ, typename Args>
__device__ __forceinline__ void fused_body(const Args &a)
{
    using P = Pack<T, OP, VEC>;
    const FusedIter it = fused_iter<DEV_SEQ>(a);
    const uint64_t  par = it.par;
    /* 1. stage src -> my scratch (all blocks, grid-stride, 16B packs; the
     * parity area of this iteration) */
    {
        const uint64_t tid =
            (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
        const uint64_t nv  = a.count / VEC;
        P *mysc = (P *)((uint8_t *)a.my_scratch + par);
        for (uint64_t i = tid; i < nv; i += str) {
            mysc[i] = ((const P *)a.src)[i];
        }
        for (uint64_t i = nv * VEC + tid; i < a.count; i += str) {
            ((T *)mysc)[i] = ((const T *)a.src)[i];
        }
    }
    /* 2.-3. publish, signal every peer, wait for all ranks */
    if (!fused_handshake(a, it)) {
        return;
    }
    /* 4. reduce all peers' scratch (this iteration's parity) into dst.
     * Why parity is sufficient: a peer can start staging replay i+1 while
     * I still read its replay-i data (staging precedes the handshake),
     * but it writes the other parity area. It cannot reach replay i+2
     * (same parity as i) until the i+1 handshake completed, which needs
     * MY i+1 launch — stream-ordered after my reduce of i finished. */
    reduce_range<T, OP, VEC>(a.dst, a.peer_scratch, par, a.nranks, a.count,
                             a.alpha);
    /* 5. host-visible completion */
    if constexpr (!DEV_SEQ) {
        fused_publish_done(a);
    }
}

template <typename T, int OP, int VEC>
__global__ void k_fused_allreduce(FusedArgs a)
{
    fused_body<T, OP, VEC, false>(a);
}

template <typename T, int OP, int VEC>
__global__ void k_fused_allreduce_graph(GraphFusedArgs a)
{
    fused_body<T, OP, VEC, true>(a);
}

/* ----------------------------------------------------------- launchers */
template <typename T, int OP> struct LaunchFused {
    static ucc_status_t run(const FusedArgs &a, hipStream_t s)
    {
        hipLaunchKernelGGL((k_fused_allreduce<T, OP, VecOf<T>::value>),
                           dim3(a.nblocks), dim3(256), 0, s, a);
        return launch_status();
    }
    static ucc_status_t run(const GraphFusedArgs &a, hipStream_t s)
    {
        hipLaunchKernelGGL(
            (k_fused_allreduce_graph<T, OP, VecOf<T>::value>),
            dim3(a.nblocks), dim3(256), 0, s, a);
        return launch_status();
    }
};

ucc_status_t fused_allreduce(const FusedArgs &a_in, hipStream_t s)
{
    FusedArgs a = a_in;
    a.dt        = fold_complex(a.dt, a.op, &a.count);
    return dispatch<LaunchFused>(a.dt, a.op, a, s);
}

ucc_status_t fused_allreduce_graph(const GraphFusedArgs &a_in, hipStream_t s)
{
    GraphFusedArgs a = a_in;
    a.dt             = fold_complex(a.dt, a.op, &a.count);
    return dispatch<LaunchFused>(a.dt, a.op, a, s);
}

} // namespace ec_hip
} // namespace ucc
