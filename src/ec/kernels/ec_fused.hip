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
    uint64_t seq, par, stage_target, cap;
    if constexpr (DEV_SEQ) {
        /* 0. device-side iteration number: this block's launch count.
         * Every block of every launch/replay increments its own counter
         * exactly once, so all blocks of one launch observe the same
         * value. */
        uint64_t *my_cnt = a.local_flags + kGraphCntBase +
                           (uint64_t)a.slot * kMaxGraphBlocks + blockIdx.x;
        __shared__ uint64_t s_seq;
        if (threadIdx.x == 0) {
            s_seq = __hip_atomic_fetch_add(my_cnt, 1, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT) +
                    1;
        }
        __syncthreads();
        seq          = s_seq;
        par          = (seq & 1) * a.parity_stride;
        stage_target = seq * (uint64_t)a.nblocks;
        cap          = kSpinLimit;
    } else {
        seq          = a.seq;
        par          = 0;
        stage_target = a.stage_target;
        cap          = spin_cap(a.spin_limit);
    }
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
    __threadfence_system();
    __syncthreads();
    /* 2. grid arrival: each block bumps the staging counter; block 0
     * waits for all blocks, then signals every peer (incl. self) with seq.
     * The staging counter (u64 index kStageCntBase + slot) is monotone and
     * grows by nblocks per use -> target seq*nblocks. */
    uint64_t *stage_cnt = a.local_flags + kStageCntBase + a.slot;
    __shared__ int s_err;
    if (threadIdx.x == 0) {
        s_err = 0;
        __hip_atomic_fetch_add(stage_cnt, 1, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        if (threadIdx.x == 0 &&
            !spin_until(stage_cnt, stage_target, cap, a.error_word)) {
            s_err = 1;
        }
        __syncthreads();
        if (!s_err && (int)threadIdx.x < a.nranks) {
            sys_store(a.peer_flags[threadIdx.x] +
                          (uint64_t)a.slot * kMaxRanks + a.rank,
                      seq);
        }
    }
    /* 3. all blocks wait for all ranks' arrivals (timeout: all threads
     * leave together — never return while siblings sit at a barrier) */
    if (!s_err && (int)threadIdx.x < a.nranks &&
        !spin_until(a.local_flags + (uint64_t)a.slot * kMaxRanks +
                        threadIdx.x,
                    seq, cap, a.error_word)) {
        s_err = 1;
    }
    __syncthreads();
    if (s_err) {
        return;
    }
    __threadfence_system(); /* acquire: drop stale lines before peer reads */
    /* 4. reduce all peers' scratch (this iteration's parity) into dst.
     * Why parity is sufficient: a peer can start staging replay i+1 while
     * I still read its replay-i data (staging precedes the handshake),
     * but it writes the other parity area. It cannot reach replay i+2
     * (same parity as i) until the i+1 handshake completed, which needs
     * MY i+1 launch — stream-ordered after my reduce of i finished. */
    reduce_range<T, OP, VEC>(a.dst, a.peer_scratch, par, a.nranks, a.count,
                             a.alpha);
    /* 5. host-visible completion: the last arriving block publishes
     * done_seq to the pinned word — the host polls plain memory
     * instead of event record+query (see FusedArgs.done_host). dst
     * stores are fenced before the arrival add; the release store
     * makes them visible to the host with the flag. */
    if constexpr (!DEV_SEQ) {
        if (a.done_host) {
            __threadfence_system();
            __syncthreads();
            if (threadIdx.x == 0) {
                uint64_t v = __hip_atomic_fetch_add(
                                 a.local_flags + kFusedDoneBase + a.slot, 1,
                                 __ATOMIC_ACQ_REL,
                                 __HIP_MEMORY_SCOPE_AGENT) +
                             1;
                if (v == a.done_target) {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(a.done_host, a.done_seq,
                                       __ATOMIC_RELEASE,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
        }
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
