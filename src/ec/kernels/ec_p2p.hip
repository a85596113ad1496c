/* gfx950 execution-component kernel: the pull of the device active-set
 * bcast (p2p send/recv). One rank copies `len` bytes from a peer-mapped
 * source into its own dst; the last block to finish publishes completion
 * to a host-pinned word.
 *
 * The kernel never waits: no spin, no flag poll, no dependence on another
 * process's kernel. The host gates the launch on the mailbox
 * (tl/cdna4/p2p_mbox.h), so the source is complete before the launch and
 * a dead peer cannot hang the device. */
#include "ec_device.h"

namespace ucc {
namespace ec_hip {

/* 16 source bytes at pack i. ALIGNED: src is 16-byte aligned, one dwordx4
 * load. Otherwise src is only 4-byte aligned: four dword loads assembled
 * into the pack (the compiler merges them into one dword-aligned dwordx4
 * load, which global loads on gfx950 allow). */
template <bool ALIGNED>
__device__ __forceinline__ uint4 p2p_ld16(const uint8_t *src, uint64_t i)
{
    if constexpr (ALIGNED) {
        return ((const uint4 *)src)[i];
    } else {
        const uint32_t *w = (const uint32_t *)src + 4 * i;
        return make_uint4(w[0], w[1], w[2], w[3]);
    }
}

/* nv 16-byte packs, dst 16-byte aligned, grid-stride; 4-deep load
 * batching: all four loads issue before the first dependent store */
template <bool ALIGNED>
__device__ __forceinline__ void p2p_copy_packs(uint8_t *dst,
                                               const uint8_t *src,
                                               uint64_t nv, uint64_t tid,
                                               uint64_t str)
{
    uint64_t i = tid;
    for (; i + 3 * str < nv; i += 4 * str) {
        uint4 v0 = p2p_ld16<ALIGNED>(src, i);
        uint4 v1 = p2p_ld16<ALIGNED>(src, i + str);
        uint4 v2 = p2p_ld16<ALIGNED>(src, i + 2 * str);
        uint4 v3 = p2p_ld16<ALIGNED>(src, i + 3 * str);
        ((uint4 *)dst)[i]           = v0;
        ((uint4 *)dst)[i + str]     = v1;
        ((uint4 *)dst)[i + 2 * str] = v2;
        ((uint4 *)dst)[i + 3 * str] = v3;
    }
    for (; i < nv; i += str) {
        ((uint4 *)dst)[i] = p2p_ld16<ALIGNED>(src, i);
    }
}

/* Source and destination alignment are independent (slices of tensors):
 *  (a) src == dst (mod 16): byte head up to 16-byte alignment of dst,
 *      dwordx4 loads and stores, byte tail;
 *  (b) src == dst (mod 4) only: the same, with dword loads assembled into
 *      the 16-byte stores;
 *  (c) anything else: byte loop.
 * Every access stays inside [src, src+len) and [dst, dst+len). */
__global__ void __launch_bounds__(256) k_p2p_pull(P2pPullArgs a)
{
    uint8_t       *dst = (uint8_t *)a.dst;
    const uint8_t *src = (const uint8_t *)a.src;
    const uint64_t len = a.len;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
    const unsigned delta =
        (unsigned)(((uintptr_t)src - (uintptr_t)dst) & 15);
    if (delta & 3) {
        for (uint64_t t = tid; t < len; t += str) {
            dst[t] = src[t];
        }
    } else {
        uint64_t head = (16 - ((uintptr_t)dst & 15)) & 15;
        head          = head < len ? head : len;
        for (uint64_t t = tid; t < head; t += str) {
            dst[t] = src[t];
        }
        uint8_t       *d   = dst + head;
        const uint8_t *s   = src + head;
        const uint64_t rem = len - head;
        const uint64_t nv  = rem / 16;
        if (delta == 0) {
            p2p_copy_packs<true>(d, s, nv, tid, str);
        } else {
            p2p_copy_packs<false>(d, s, nv, tid, str);
        }
        for (uint64_t t = nv * 16 + tid; t < rem; t += str) {
            d[t] = s[t];
        }
    }
    /* completion (the done_host pattern of FusedArgs): dst stores are
     * fenced before the arrival add; the block whose add reaches the
     * host-tracked cumulative target is the last one and release-stores
     * the sequence number to the pinned word the host polls. */
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t v = __hip_atomic_fetch_add(a.arrive_cnt, 1,
                                            __ATOMIC_ACQ_REL,
                                            __HIP_MEMORY_SCOPE_AGENT) +
                     1;
        if (v == a.done_target) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_store(a.done_host, a.done_seq, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

int p2p_auto_blocks(uint64_t len)
{
    uint64_t b = (len + kP2pBlockBytes - 1) / kP2pBlockBytes;
    return (int)(b < 1 ? 1 : b > (uint64_t)kP2pAutoMaxBlocks
                                 ? (uint64_t)kP2pAutoMaxBlocks
                                 : b);
}

ucc_status_t p2p_pull(const P2pPullArgs &a, hipStream_t s)
{
    if (!a.arrive_cnt || !a.done_host || a.nblocks < 1 ||
        a.nblocks > kP2pMaxBlocks || (a.len && (!a.dst || !a.src))) {
        return UCC_ERR_INVALID_PARAM;
    }
    hipLaunchKernelGGL(k_p2p_pull, dim3(a.nblocks), dim3(256), 0, s, a);
    return launch_status();
}

} // namespace ec_hip
} // namespace ucc
