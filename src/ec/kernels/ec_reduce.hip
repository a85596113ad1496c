/* gfx950 execution-component kernels: n-source reduction and gather-copy,
 * and the dtype/op support queries (answered from the dispatch table). */
#include "ec_device.h"

#include <atomic>

namespace ucc {
namespace ec_hip {

/* ------------------------------------------------------------- reduce  */
template <typename T, int OP, int VEC>
__global__ void k_reduce(ReduceArgs a)
{
    reduce_range<T, OP, VEC>(a.dst, a.srcs, 0, a.n_srcs, a.count, a.alpha);
}

template <typename T, int OP>
__global__ void k_reduce_scalar(ReduceArgs a)
{
    uint64_t       i   = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
    for (; i < a.count; i += str) {
        ((T *)a.dst)[i] =
            reduce_elem<T, OP>(a.srcs, 0, a.n_srcs, i, a.alpha);
    }
}

/* -------------------------------------------------------- gather copy  */
__global__ void k_gather_copy(GatherArgs a)
{
    /* blocks partitioned across sources: peers' xGMI links stream
     * concurrently (sequential per-peer copies would serialize on one
     * link at a time) */
    const int grp = (int)gridDim.x / a.n > 0 ? (int)gridDim.x / a.n : 1;
    int       s   = (int)blockIdx.x / grp;
    int       bid = (int)blockIdx.x % grp;
    if ((int)gridDim.x < a.n) { /* fewer blocks than sources: loop */
        for (s = (int)blockIdx.x; s < a.n; s += gridDim.x) {
            uint8_t       *dst = (uint8_t *)a.dst_base + a.offs[s];
            const uint8_t *src = (const uint8_t *)a.srcs[s];
            d_copy_bytes_part(dst, src, a.lens[s], 0, 1);
        }
        return;
    }
    if (s >= a.n) {
        return;
    }
    uint8_t       *dst = (uint8_t *)a.dst_base + a.offs[s];
    const uint8_t *src = (const uint8_t *)a.srcs[s];
    if ((((uintptr_t)dst | (uintptr_t)src) & 3) == 0 ||
        (((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
        d_copy_bytes_part(dst, src, a.lens[s], (uint64_t)bid,
                          (uint64_t)grp);
    } else {
        const uint64_t tid = (uint64_t)bid * blockDim.x + threadIdx.x;
        const uint64_t str = (uint64_t)grp * blockDim.x;
        for (uint64_t i = tid; i < a.lens[s]; i += str) {
            dst[i] = src[i];
        }
    }
}

/* ----------------------------------------------------------- launchers */
static bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

static std::atomic<uint64_t> g_scalar_launches{0};

uint64_t reduce_scalar_launches() { return g_scalar_launches.load(); }

template <typename T, int OP> struct LaunchReduce {
    static ucc_status_t run(const ReduceArgs &a, hipStream_t s)
    {
        constexpr int VEC = VecOf<T>::value;
        bool          vec = aligned16(a.dst);
        for (int i = 0; i < a.n_srcs; i++) {
            vec = vec && aligned16(a.srcs[i]);
        }
        int  threads = 256;
        long work    = (long)(a.count / (vec ? VEC : 1));
        int  blocks =
            (int)std::min<long>((work + threads - 1) / threads, 2048);
        if (blocks < 1) {
            blocks = 1;
        }
        if (vec) {
            hipLaunchKernelGGL((k_reduce<T, OP, VEC>), dim3(blocks),
                               dim3(threads), 0, s, a);
        } else {
            g_scalar_launches.fetch_add(1, std::memory_order_relaxed);
            hipLaunchKernelGGL((k_reduce_scalar<T, OP>), dim3(blocks),
                               dim3(threads), 0, s, a);
        }
        return launch_status();
    }
};

ucc_status_t reduce(const ReduceArgs &a_in, hipStream_t s)
{
    ReduceArgs a = a_in;
    a.dt         = fold_complex(a.dt, a.op, &a.count);
    return dispatch<LaunchReduce>(a.dt, a.op, a, s);
}

constexpr int kGatherThreads = 256;

int gather_copy_blocks(const GatherArgs &a)
{
    uint64_t total = 0;
    for (int i = 0; i < a.n; i++) {
        total += a.lens[i];
    }
    int blocks = (int)std::min<uint64_t>(
        (total / 16 + kGatherThreads - 1) / kGatherThreads, 2048);
    if (blocks < 1) {
        blocks = 1;
    }
    return blocks;
}

ucc_status_t gather_copy(const GatherArgs &a, hipStream_t s,
                         int *blocks_used)
{
    const int blocks = gather_copy_blocks(a);
    hipLaunchKernelGGL(k_gather_copy, dim3(blocks), dim3(kGatherThreads), 0,
                       s, a);
    if (blocks_used) {
        *blocks_used = blocks;
    }
    return launch_status();
}

/* a cell of the dispatch table exists iff a launcher is reachable there */
template <typename T, int OP> struct Probe {
    static ucc_status_t run(const int &, hipStream_t) { return UCC_OK; }
};

bool dt_supported(ucc_datatype_t dt)
{
    return dispatch<Probe>(dt, UCC_OP_SUM, 0, nullptr) == UCC_OK;
}

bool op_supported(ucc_datatype_t dt, ucc_reduction_op_t op)
{
    return dispatch<Probe>(fold_complex(dt, op, nullptr), op, 0, nullptr) ==
           UCC_OK;
}

} // namespace ec_hip
} // namespace ucc
