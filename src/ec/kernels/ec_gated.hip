/* gfx950 execution-component kernels: the device-gated family — staged
 * stage / reduce / gather, the copy-engine gates, the fused zero-copy
 * allreduce (k_zc_allreduce), and the copy-only slice phase of the rooted
 * collectives (k_staged_bscatter, k_zc_bcast). */
#include "ec_device.h"

namespace ucc {
namespace ec_hip {

/* ------------------------------------------- device-gated staged colls */
__device__ __forceinline__ int gated_idx(int phase, int slot, int parity)
{
    return kGatedCntBase + (phase * kGatedSlots + slot) * 2 + parity;
}

__device__ __forceinline__ int gated_mirror_idx(int phase, int slot,
                                                int parity, int src)
{
    return kGatedMirrorBase +
           ((phase * kGatedSlots + slot) * 2 + parity) * kMaxRanks + src;
}

/* Wait targets for this launch. Host-target mode reads them straight
 * from the (const) kernarg struct; graph mode derives them from this
 * block's launch ordinal within the (slot,parity) pattern: every gated
 * kernel of the pattern increments the same per-block counter, so with
 * pp kernels per iteration, counter value v maps to iteration
 * u = (v-1)/pp + 1 on every block of the same launch (fixed grid).
 * IMPORTANT: `a` stays const — mutating the by-value kernel argument
 * would force the whole ~660-byte struct into scratch memory and put
 * scratch reloads inside the hot loops (observed in gfx950 ISA). */
struct GatedTargets {
    uint64_t sw_reduce, sw_gather, prev_gather, stage, gather_wait;
    uint64_t sig_stage, sig_reduce, sig_gather;
};

__device__ __forceinline__ GatedTargets gated_targets(const GatedArgs &a)
{
    if (!a.derive) {
        return {a.t_sw_reduce,  a.t_sw_gather,  a.t_prev_gather,
                a.t_stage,      a.t_gather_wait,
                a.t_sig_stage,  a.t_sig_reduce, a.t_sig_gather};
    }
    uint64_t *cnt = a.local_flags + kGatedGraphBase +
                    ((uint64_t)a.slot * 2 + a.parity) * kGatedMaxBlocks +
                    blockIdx.x;
    __shared__ uint64_t s_u;
    if (threadIdx.x == 0) {
        uint64_t v = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT) +
                     1;
        s_u = (v - 1) / (uint64_t)a.pp + 1;
    }
    __syncthreads();
    const uint64_t u = s_u;
    const uint64_t B = (uint64_t)(a.nblocks ? a.nblocks : kGatedBlocks);
    return {a.has_reduce ? (u - 1) * B : 0,
            a.has_gather ? (u - 1) * B : 0,
            a.has_gather ? (u - 1) * B : 0, u * B, u * B,
            u * B, u * B, u * B};
}

/* where rank j's phase counter is polled: my local mirror of it, or (debug
 * fallback) the counter itself in rank j's flags */
__device__ __forceinline__ const uint64_t *
gated_flag(const GatedArgs &a, int phase, int j)
{
    return a.pull_wait
               ? a.peer_flags[j] + gated_idx(phase, a.slot, a.parity)
               : a.local_flags +
                     gated_mirror_idx(phase, a.slot, a.parity, j);
}

/* all blocks wait until every rank reached counter[idx] >= target; on
 * spin timeout ALL threads leave together (no thread may return while
 * others sit at __syncthreads — that would hang the block forever).
 * PUSH protocol: ranks publish their phase counters into every peer's
 * mirror slots (gated_signal), so this wait polls LOCAL memory only —
 * remote xGMI reads during the wait would steal link bandwidth from the
 * concurrently-running data phases (B x n remote pollers; see
 * MI355X_MICROARCH.md "polling-cost"). */
__device__ __forceinline__ bool
gated_wait(const GatedArgs &a, int phase, uint64_t target)
{
    __shared__ int s_err;
    if (threadIdx.x == 0) {
        s_err = 0;
    }
    __syncthreads();
    if (target != 0 && threadIdx.x < 64) {
        int j = (int)threadIdx.x;
        if (j < a.nranks &&
            !spin_until(gated_flag(a, phase, j), target,
                        spin_cap(a.spin_limit), a.error_word)) {
            s_err = 1;
        }
    }
    __syncthreads();
    if (s_err) {
        return false;
    }
    __threadfence_system(); /* acquire: see peers' payload writes */
    return true;
}

/* per-block completion signal on my own counter, called by one thread;
 * the LAST arriving block (true is returned to it)
 * of this launch pushes the new cumulative value into every rank's
 * mirror slot (n system-scope stores over xGMI — the only remote flag
 * traffic in the whole pipeline). acq_rel on the counter makes every
 * earlier block's release (and thus its payload writes, xGMI ones
 * included) visible-before the mirror store. */
__device__ __forceinline__ bool gated_arrive(const GatedArgs &a, int phase,
                                             uint64_t sig_target)
{
    uint64_t v = __hip_atomic_fetch_add(
                     a.local_flags + gated_idx(phase, a.slot, a.parity), 1,
                     __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_SYSTEM) +
                 1;
    if (v != sig_target) {
        return false;
    }
    /* last arriver of this launch. Guard against the ROCm 7.2
     * dropped-vmcnt hazard (MI355X_MICROARCH.md "Compiler hazard"): the
     * release write-back must drain before the mirror stores leave */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int j = 0; j < a.nranks; j++) {
        __hip_atomic_store(
            a.peer_flags[j] +
                gated_mirror_idx(phase, a.slot, a.parity, a.rank),
            v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    return true;
}

/* the whole block signals: payload fenced, then thread 0 arrives; the
 * last arriver also publishes the host completion word if asked to */
__device__ __forceinline__ void gated_signal(const GatedArgs &a, int phase,
                                             uint64_t sig_target,
                                             bool pub_done = true)
{
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0 && gated_arrive(a, phase, sig_target) &&
        pub_done && a.done_host) {
        /* final kernel of a host-posted collective */
        __hip_atomic_store(a.done_host, a.done_seq, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void k_staged_stage(const GatedArgs a)
{
    const GatedTargets t = gated_targets(a);
    if (!gated_wait(a, 1, t.sw_reduce) ||
        !gated_wait(a, 2, t.sw_gather)) { /* in-area reuse */
        return;
    }
    if (a.n_cells > 0) { /* per-dest cells (alltoall) */
        for (int c = 0; c < a.n_cells; c++) {
            if (a.c_len[c]) {
                d_copy_bytes((uint8_t *)a.my_in + a.c_dst_off[c],
                             (const uint8_t *)a.src + a.c_src_off[c],
                             a.c_len[c]);
            }
        }
    } else if (a.len) {
        d_copy_bytes((uint8_t *)a.my_in, (const uint8_t *)a.src, a.len);
    }
    gated_signal(a, 0, t.sig_stage);
}

template <typename T, int OP, int VEC, int U>
__global__ void k_staged_reduce(const GatedArgs a)
{
    using A = typename Cvt<T>::A;
    const GatedTargets gt = gated_targets(a);
    if (!gated_wait(a, 0, gt.stage) ||
        !gated_wait(a, 2, gt.prev_gather)) {
        return;
    }
    const uint64_t cnt = (a.sl_e - a.sl_b) / sizeof(T);
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t nv  = cnt / VEC;
    const int      n   = a.nranks;
    using P            = Pack<T, OP, VEC>;
    /* fully unrolled over kMaxRanks with a uniform guard: a runtime-
     * indexed pointer array would be materialized in scratch memory and
     * re-loaded inside the hot loop (observed in the gfx950 ISA);
     * unrolling keeps the 8 peer base pointers in SGPRs and issues all
     * peer loads back-to-back for xGMI latency overlap. */
    P *out = (P *)a.my_out;
    /* U-deep batching: all U x n peer loads are issued before any
     * reduction consumes them. The per-lane bytes-in-flight must cover
     * the bandwidth-latency product (≈6.3 TB/s x ~600 ns needs ~4 MB
     * chip-wide): U is chosen at launch so U*n*16B stays ~128B/lane
     * without spilling the pack registers (U=4 at n<=2, 2 at n<=4,
     * 1 at n>=5 where the peer unroll already provides the depth). */
    uint64_t i = tid;
    if (U > 1) {
        for (; i + (U - 1) * str < nv; i += U * str) {
            P x[U][kMaxRanks];
#pragma unroll
            for (int s = 0; s < kMaxRanks; s++) {
                if (s < n) {
                    const P *src =
                        (const P *)((const uint8_t *)a.peer_in[s] +
                                    a.sl_b);
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        x[u][s] = src[i + (uint64_t)u * str];
                    }
                }
            }
            A r[U][VEC];
#pragma unroll
            for (int u = 0; u < U; u++) {
                vload<T, OP, VEC, A>(x[u][0], r[u]);
            }
#pragma unroll
            for (int s = 1; s < kMaxRanks; s++) {
                if (s < n) {
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        vaccum<T, OP, VEC, A>(r[u], x[u][s]);
                    }
                }
            }
            P o[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                vstore<T, OP, VEC, A>(o[u], r[u], a.alpha);
            }
            if (a.zc_write) {
                /* write my reduced slice into every rank's dst */
#pragma unroll
                for (int s = 0; s < kMaxRanks; s++) {
                    if (s < n) {
#pragma unroll
                        for (int u = 0; u < U; u++) {
                            ((P *)a.peer_out[s])[i + (uint64_t)u * str] =
                                o[u];
                        }
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    out[i + (uint64_t)u * str] = o[u];
                }
            }
        }
    }
    for (; i < nv; i += str) {
        A r[VEC];
        {
            P acc = ((const P *)((const uint8_t *)a.peer_in[0] +
                                 a.sl_b))[i];
            vload<T, OP, VEC, A>(acc, r);
        }
#pragma unroll
        for (int s = 1; s < kMaxRanks; s++) {
            if (s < n) {
                P x = ((const P *)((const uint8_t *)a.peer_in[s] +
                                   a.sl_b))[i];
                vaccum<T, OP, VEC, A>(r, x);
            }
        }
        P o;
        vstore<T, OP, VEC, A>(o, r, a.alpha);
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < kMaxRanks; s++) {
                if (s < n) {
                    ((P *)a.peer_out[s])[i] = o;
                }
            }
        } else {
            out[i] = o;
        }
    }
    for (uint64_t t = nv * VEC + tid; t < cnt; t += str) {
        A r = Cvt<T>::load(
            ((const T *)((const uint8_t *)a.peer_in[0] + a.sl_b))[t]);
#pragma unroll
        for (int s = 1; s < kMaxRanks; s++) {
            if (s < n) {
                r = red<A, OP>(
                    r, Cvt<T>::load(((const T *)((const uint8_t *)
                                                     a.peer_in[s] +
                                                 a.sl_b))[t]));
            }
        }
        T ov = Cvt<T>::store(apply_alpha<A>(r, a.alpha));
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < kMaxRanks; s++) {
                if (s < n) {
                    ((T *)a.peer_out[s])[t] = ov;
                }
            }
        } else {
            ((T *)out)[t] = ov;
        }
    }
    gated_signal(a, 1, gt.sig_reduce);
}

__global__ void k_staged_gather(const GatedArgs a)
{
    const GatedTargets t = gated_targets(a);
    if (!gated_wait(a, a.gw_phase, t.gather_wait)) {
        return;
    }
    /* partition the grid across sources: every peer link streams
     * concurrently instead of one-after-another (7 x 153 GB/s at once) */
    const int grp = gridDim.x / a.nranks > 0 ? gridDim.x / a.nranks : 1;
    const int src = (int)blockIdx.x / grp;
    const int bid = (int)blockIdx.x % grp;
    if ((int)gridDim.x < a.nranks) {
        /* fewer blocks than sources (a small GATED_BLOCKS): each block
         * takes whole sources in turn, as k_gather_copy does. Every block
         * still signals exactly once below. */
        for (int s = (int)blockIdx.x; s < a.nranks; s += (int)gridDim.x) {
            uint64_t b = a.slice_b[s], e = a.slice_e[s];
            if (e > b) {
                d_copy_bytes_part((uint8_t *)a.dst + b,
                                  (const uint8_t *)a.peer_out[s], e - b, 0,
                                  1);
            }
        }
    } else if (src < a.nranks) {
        uint64_t b = a.slice_b[src], e = a.slice_e[src];
        if (e > b) {
            d_copy_bytes_part((uint8_t *)a.dst + b,
                              (const uint8_t *)a.peer_out[src], e - b,
                              (uint64_t)bid, (uint64_t)grp);
        }
    }
    gated_signal(a, 2, t.sig_gather);
}

/* Copy-engine collectives (reference alltoallv_ce.c:50,218-226 role):
 * data moves by hipMemcpyAsync on SDMA engines, kernels only gate.
 * k_gated_wait_only orders the memcpys after every rank's entry signal;
 * k_gated_done publishes my-copies-complete and waits the team. */
__global__ void k_gated_wait_only(const GatedArgs a)
{
    if (!gated_wait(a, a.gw_phase, a.t_gather_wait)) {
        return;
    }
    if (a.done_host && blockIdx.x == 0 && threadIdx.x == 0) {
        /* completion point: the team's final phase is confirmed, so
         * every peer has stopped reading this rank's buffers */
        __hip_atomic_store(a.done_host, a.done_seq, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ void k_gated_done(const GatedArgs a)
{
    gated_signal(a, 2, a.t_sig_gather, /*pub_done=*/false);
    if (!gated_wait(a, 2, a.t_gather_wait)) {
        return;
    }
    if (a.done_host && blockIdx.x == 0 && threadIdx.x == 0) {
        __hip_atomic_store(a.done_host, a.done_seq, __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

/* ------------------------------- fused zero-copy allreduce (one launch) */
/* gated_signal that tells the WHOLE block whether it was the last
 * arriver of this launch (LDS broadcast), so the block can go on into a
 * gated_wait together. Publishes no done_host. */
__device__ __forceinline__ bool
gated_signal_last(const GatedArgs &a, int phase, uint64_t sig_target)
{
    __shared__ int s_last;
    /* every wave's stores have reached L2, then ONE release for the
     * block (the acq_rel add of gated_arrive: a single L2 write-back per
     * block instead of one per wave plus one — the write-backs of a
     * grid's blocks queue up on their XCD's L2) */
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        s_last = gated_arrive(a, phase, sig_target);
    }
    __syncthreads();
    return s_last != 0;
}

/* gated_wait on two phases at once with ONE acquire per block: wave 0
 * polls both mirrors (local memory), invalidates, and the barrier
 * orders every other wave's loads behind that invalidate. */
__device__ __forceinline__ bool zc_wait2(const GatedArgs &a, int ph0,
                                         uint64_t t0, int ph1,
                                         uint64_t t1)
{
    __shared__ int s_err2;
    if (threadIdx.x == 0) {
        s_err2 = 0;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int j = (int)threadIdx.x;
        if (j < a.nranks) {
            const uint64_t cap = spin_cap(a.spin_limit);
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int      ph = k ? ph1 : ph0;
                const uint64_t t  = k ? t1 : t0;
                if (t != 0 &&
                    !spin_until(gated_flag(a, ph, j), t, cap, a.error_word)) {
                    s_err2 = 1;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    return s_err2 == 0;
}

/* peer unroll bound of the fused kernel by batching depth: the launcher
 * only picks U with U * nranks <= kMaxRanks, so the uniform `s < n`
 * guard never has to cover more peers than this and the two pack
 * buffers of the pipelined loop stay at U * NR * 16 B per lane each. */
template <int U> struct ZcPeers {
    static constexpr int value = kMaxRanks / U > 0 ? kMaxRanks / U : 1;
};

/* 16-byte pack moves of the batches, by cache policy. NT: non-temporal
 * (streaming) — a message that does not fit the Infinity Cache gains
 * nothing from allocating there, and src is read and dst written exactly
 * once per post. Pack is a struct, and the non-temporal builtins take
 * scalar and vector types only, hence the bit casts. An nt store is an
 * ordinary store to the memory model: the block's release at exit covers
 * it like any other. */
typedef uint32_t zc_u32x4 __attribute__((ext_vector_type(4)));
template <bool NT, typename P>
__device__ __forceinline__ P zc_ld(const P *p)
{
    static_assert(sizeof(P) == sizeof(zc_u32x4), "16-byte packs");
    if constexpr (NT) {
        return __builtin_bit_cast(
            P, __builtin_nontemporal_load((const zc_u32x4 *)p));
    } else {
        return *p;
    }
}
template <bool NT, typename P>
__device__ __forceinline__ void zc_st(P *p, const P &v)
{
    if constexpr (NT) {
        __builtin_nontemporal_store(__builtin_bit_cast(zc_u32x4, v),
                                    (zc_u32x4 *)p);
    } else {
        *p = v;
    }
}

/* issue one batch's U x n peer loads (no consumer in between) */
template <typename P, int U, int NR, bool NT>
__device__ __forceinline__ void
zc_batch_load(P (&x)[U][NR], const GatedArgs &a, int n, uint64_t i,
              uint64_t str)
{
#pragma unroll
    for (int s = 0; s < NR; s++) {
        if (s < n) {
            const P *src =
                (const P *)((const uint8_t *)a.peer_in[s] + a.sl_b);
#pragma unroll
            for (int u = 0; u < U; u++) {
                x[u][s] = zc_ld<NT>(src + i + (uint64_t)u * str);
            }
        }
    }
}

/* convert, reduce ranks 0..n-1 in order, scale, store one loaded batch:
 * the arithmetic of k_staged_reduce's batched loop, element for element */
template <typename T, int OP, int VEC, int U, int NR, bool NT, typename P>
__device__ __forceinline__ void
zc_batch_reduce_store(const P (&x)[U][NR], const GatedArgs &a, P *out,
                      int n, uint64_t i, uint64_t str)
{
    using A = typename Cvt<T>::A;
    A r[U][VEC];
#pragma unroll
    for (int u = 0; u < U; u++) {
        vload<T, OP, VEC, A>(x[u][0], r[u]);
    }
#pragma unroll
    for (int s = 1; s < NR; s++) {
        if (s < n) {
#pragma unroll
            for (int u = 0; u < U; u++) {
                vaccum<T, OP, VEC, A>(r[u], x[u][s]);
            }
        }
    }
    P o[U];
#pragma unroll
    for (int u = 0; u < U; u++) {
        vstore<T, OP, VEC, A>(o[u], r[u], a.alpha);
    }
    if (a.zc_write) {
#pragma unroll
        for (int s = 0; s < NR; s++) {
            if (s < n) {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    zc_st<NT>((P *)a.peer_out[s] + i + (uint64_t)u * str,
                              o[u]);
                }
            }
        }
    } else {
        /* `out` is a.my_out read ahead of the zc_write branch (see
         * zc_data_phase). At NR == 2 the in-branch read is kept: there
         * the struct stays out of scratch either way, and the early read
         * costs the flagship instantiation a waves/SIMD band (188
         * instead of 159 VGPRs), as does reading it once above this
         * loop. */
#pragma unroll
        for (int u = 0; u < U; u++) {
            zc_st<NT>((NR > 2 ? out : (P *)a.my_out) + i + (uint64_t)u * str,
                      o[u]);
        }
    }
}

/* The data phase of the fused kernel — everything between its entry wait
 * and its exit signal: the pipelined batches, their epilogue, the
 * per-pack loop and the scalar tail over my slice [sl_b, sl_e) of every
 * rank's src. No flag is read or written here, so k_zc_data below can
 * time it without a peer process (docs/GATED_PIPELINE.md "Data phase
 * and its probe"). */
template <typename T, int OP, int VEC, int U, bool NT>
__device__ __forceinline__ void zc_data_phase(const GatedArgs &a)
{
    using A          = typename Cvt<T>::A;
    using P          = Pack<T, OP, VEC>;
    constexpr int NR = ZcPeers<U>::value;
    const uint64_t cnt = (a.sl_e - a.sl_b) / sizeof(T);
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t nv  = cnt / VEC;
    /* read before any zc_write branch: a load of my_out on one side and
     * of peer_out[s] on the other would be merged into one load through
     * a pointer INTO the argument struct, and that keeps the whole
     * struct in scratch memory (observed in gfx950 ISA, U = 2) */
    P *const out = (P *)a.my_out;
    /* 2 <= nranks <= NR (launcher-checked). At NR == 2 that pins n, so
     * the uniform peer guards fold away. This is what lets the pipeline
     * work: behind a branch that may or may not have issued loads the
     * compiler can only wait for vmcnt(0), which would drain the batch
     * just issued along with the one about to be consumed. */
    const int n = NR == 2 ? 2 : a.nranks;
    __builtin_assume(n >= 2 && n <= NR);
    uint64_t i = tid;
    if (U > 1) {
        /* software-pipelined batches over two pack buffers: the loads
         * of batch k+1 are in flight while batch k is converted, added
         * and stored, so the bytes-in-flight figure of k_staged_reduce
         * holds through the whole iteration instead of only between
         * its load and its first use (one wave per SIMD here: no
         * sibling wave covers that bubble). Batches touch disjoint
         * elements, so in-place (dst == src) stays correct. */
        const uint64_t bs   = (uint64_t)U * str;
        const uint64_t tail = (uint64_t)(U - 1) * str;
        if (i + tail < nv) {
            P xa[U][NR], xb[U][NR];
            /* prologue: xa <- batch i. The steady-state body below has
             * no branch around a load (see the note on n above): it
             * runs while batches i, i+bs and i+2bs all exist, and on
             * exit xa again holds batch i. */
            zc_batch_load<P, U, NR, NT>(xa, a, n, i, str);
            while (i + 2 * bs + tail < nv) {
                zc_batch_load<P, U, NR, NT>(xb, a, n, i + bs, str);
                zc_batch_reduce_store<T, OP, VEC, U, NR, NT, P>(xa, a, out, n,
                                                            i, str);
                zc_batch_load<P, U, NR, NT>(xa, a, n, i + 2 * bs, str);
                zc_batch_reduce_store<T, OP, VEC, U, NR, NT, P>(xb, a, out, n,
                                                            i + bs, str);
                i += 2 * bs;
            }
            /* epilogue: one or two full batches left */
            if (i + bs + tail < nv) {
                zc_batch_load<P, U, NR, NT>(xb, a, n, i + bs, str);
                zc_batch_reduce_store<T, OP, VEC, U, NR, NT, P>(xa, a, out, n,
                                                            i, str);
                zc_batch_reduce_store<T, OP, VEC, U, NR, NT, P>(xb, a, out, n,
                                                            i + bs, str);
                i += 2 * bs;
            } else {
                zc_batch_reduce_store<T, OP, VEC, U, NR, NT, P>(xa, a, out, n,
                                                            i, str);
                i += bs;
            }
        }
    }
    for (; i < nv; i += str) {
        A r[VEC];
        {
            P acc = ((const P *)((const uint8_t *)a.peer_in[0] +
                                 a.sl_b))[i];
            vload<T, OP, VEC, A>(acc, r);
        }
#pragma unroll
        for (int s = 1; s < NR; s++) {
            if (s < n) {
                P x = ((const P *)((const uint8_t *)a.peer_in[s] +
                                   a.sl_b))[i];
                vaccum<T, OP, VEC, A>(r, x);
            }
        }
        P o;
        vstore<T, OP, VEC, A>(o, r, a.alpha);
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < NR; s++) {
                if (s < n) {
                    ((P *)a.peer_out[s])[i] = o;
                }
            }
        } else {
            out[i] = o;
        }
    }
    for (uint64_t t = nv * VEC + tid; t < cnt; t += str) {
        A r = Cvt<T>::load(
            ((const T *)((const uint8_t *)a.peer_in[0] + a.sl_b))[t]);
#pragma unroll
        for (int s = 1; s < NR; s++) {
            if (s < n) {
                r = red<A, OP>(
                    r, Cvt<T>::load(((const T *)((const uint8_t *)
                                                     a.peer_in[s] +
                                                 a.sl_b))[t]));
            }
        }
        T ov = Cvt<T>::store(apply_alpha<A>(r, a.alpha));
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < NR; s++) {
                if (s < n) {
                    ((T *)a.peer_out[s])[t] = ov;
                }
            }
        } else {
            ((T *)out)[t] = ov;
        }
    }
}

/* One launch per zero-copy post (host-target mode only): the stage
 * signal, the reduce and the completion wait of the three-kernel pattern
 * in one grid of a.nblocks blocks. Counter effects are those of the
 * three launches (phase 0 +1, phase 1 +B, phase 2 +1), so every other
 * gated collective composes with it on the shared (slot,parity)
 * counters. zc_write = 1: allreduce, my reduced slice goes into every
 * rank's dst. zc_write = 0: reduce_scatter, my slice goes to my_out only
 * and phase 2 is neither waited on nor signalled. See
 * docs/GATED_PIPELINE.md "Fused zero-copy allreduce". */
template <typename T, int OP, int VEC, int U, bool NT>
__global__ void __launch_bounds__(256) k_zc_allreduce(const GatedArgs a)
{
    /* entry: block 0 is this rank's stage launch — area-reuse waits
     * (already satisfied in steady state), then "my stream reached this
     * post" on phase 0 (+1, so this one increment is the last arriver
     * and pushes the mirrors). Thread 0 alone, no block-wide fence: the
     * block has stored nothing that the signal would publish. What the
     * signal promises is that src is final, and src was written before
     * the post (the API's contract) by work that ended at a kernel or
     * copy boundary, which writes it back; the acq_rel add of
     * gated_arrive is itself a release. zc_wait2 ended in a barrier, so
     * the whole block is past its reuse wait. */
    if (blockIdx.x == 0) {
        if (!zc_wait2(a, 1, a.t_sw_reduce, 2, a.t_sw_gather)) {
            return;
        }
        if (threadIdx.x == 0) {
            gated_arrive(a, 0, a.t_sig_stage);
        }
    }
    if (!zc_wait2(a, 0, a.t_stage, 2, a.t_prev_gather)) {
        return;
    }
    zc_data_phase<T, OP, VEC, U, NT>(a);
    /* exit: every block counts on phase 1; the last arriver pushed the
     * mirrors and stays on as this rank's gather launch: wait for the
     * TEAM's reduces (every peer has written my dst and stopped reading
     * my src), then phase 2 (+1, mirrors) and the host completion word */
    if (!gated_signal_last(a, 1, a.t_sig_reduce)) {
        return;
    }
    /* one acquire by wave 0 and a barrier, as at entry (a 0 target is
     * not waited on); on spin timeout all threads leave together */
    if (!zc_wait2(a, 1, a.t_gather_wait, 2, 0)) {
        return;
    }
    /* One lane from here: the block has stored nothing since its phase-1
     * arrive, so there is nothing for a block-wide fence to write back.
     * Thread 0 is in the wave that acquired above, so its release add
     * (phase 2) and its release store (done_host) stay ordered behind
     * that acquire, and with it behind every peer's phase-1 release,
     * i.e. behind their writes to my dst. */
    if (threadIdx.x == 0) {
        const bool last =
            a.zc_write ? gated_arrive(a, 2, a.t_sig_gather) : true;
        if (last && a.done_host) {
            __hip_atomic_store(a.done_host, a.done_seq, __ATOMIC_RELEASE,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

/* The data phase alone, for measurement and unit tests: no flags, no
 * waits, no signals, so it runs without a peer process and hardware
 * counters can be collected on it. */
template <typename T, int OP, int VEC, int U, bool NT>
__global__ void __launch_bounds__(256) k_zc_data(const GatedArgs a)
{
    zc_data_phase<T, OP, VEC, U, NT>(a);
}

/* ------------------------------------- rooted collectives: bcast phase */
/* The data phase of the gated bcast, datatype-free: bytes [sl_b, sl_e) of
 * ONE source (peer_in[0]: the root's in-area, or its user buffer in the
 * zero-copy form) go to my_out (zc_write = 0: my out area, slice at
 * offset 0, as k_staged_reduce leaves it) or to every non-null
 * peer_out[s], s < nranks (zc_write = 1: push into the non-root ranks'
 * buffers; the root's own entry is null and skipped). Source + sl_b and
 * every destination are 16-byte aligned: areas are, sl_b is a multiple of
 * 256, and the zero-copy consensus admits aligned user buffers only.
 *
 * 16-byte packs, U loads issued before the first store as in
 * d_copy_bytes_part, each loaded pack stored to every destination, then a
 * per-pack loop and a byte tail. U is a fixed 4, NOT the depth rule of
 * the reduce kernels: that rule trades depth against the n sources a
 * reduction holds in registers, and a copy has one source whatever n is,
 * so 4 packs (64 B in flight per lane, d_copy_bytes_part's figure) cost
 * 16 VGPRs at every team size. Nobody has measured another depth. */
template <int U>
__device__ __forceinline__ void bcast_phase(const GatedArgs &a)
{
    const uint64_t len = a.sl_e - a.sl_b;
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t nv  = len / 16;
    const uint8_t *const src8 = (const uint8_t *)a.peer_in[0] + a.sl_b;
    const uint4 *const   src  = (const uint4 *)src8;
    /* read before any zc_write branch (see zc_data_phase) */
    uint8_t *const out8 = (uint8_t *)a.my_out;
    uint4 *const   out  = (uint4 *)out8;
    const int      n    = a.nranks;
    uint64_t       i    = tid;
    for (; i + (U - 1) * str < nv; i += U * str) {
        uint4 v[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            v[u] = src[i + (uint64_t)u * str];
        }
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < kMaxRanks; s++) {
                if (s < n && a.peer_out[s]) {
                    uint4 *d = (uint4 *)a.peer_out[s];
#pragma unroll
                    for (int u = 0; u < U; u++) {
                        d[i + (uint64_t)u * str] = v[u];
                    }
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; u++) {
                out[i + (uint64_t)u * str] = v[u];
            }
        }
    }
    for (; i < nv; i += str) {
        const uint4 v = src[i];
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < kMaxRanks; s++) {
                if (s < n && a.peer_out[s]) {
                    ((uint4 *)a.peer_out[s])[i] = v;
                }
            }
        } else {
            out[i] = v;
        }
    }
    for (uint64_t t = nv * 16 + tid; t < len; t += str) {
        const uint8_t v = src8[t];
        if (a.zc_write) {
#pragma unroll
            for (int s = 0; s < kMaxRanks; s++) {
                if (s < n && a.peer_out[s]) {
                    ((uint8_t *)a.peer_out[s])[t] = v;
                }
            }
        } else {
            out8[t] = v;
        }
    }
}

constexpr int kBcastDepth = 4;

/* The slot k_staged_reduce has in the allreduce pattern, copy-only: wait
 * for the team's stage of this fragment and for the out-area reuse, move
 * my slice of the root's data, signal phase 1 with the full grid. */
__global__ void k_staged_bscatter(const GatedArgs a)
{
    const GatedTargets gt = gated_targets(a);
    if (!gated_wait(a, 0, gt.stage) ||
        !gated_wait(a, 2, gt.prev_gather)) {
        return;
    }
    bcast_phase<kBcastDepth>(a);
    gated_signal(a, 1, gt.sig_reduce);
}

/* One launch per zero-copy bcast post (host-target mode only): entry and
 * exit protocol of k_zc_allreduce with zc_write = 1, counter effects
 * phase 0 +1, phase 1 +B, phase 2 +1. The entry wait on the team's phase
 * 0 says that every rank has posted, so the non-root buffers may be
 * written and the root's holds the message; the exit wait on the team's
 * phase 1 says that every slice has landed in my buffer (non-root) and
 * that nobody reads it any more (root). */
__global__ void __launch_bounds__(256) k_zc_bcast(const GatedArgs a)
{
    if (blockIdx.x == 0) {
        if (!zc_wait2(a, 1, a.t_sw_reduce, 2, a.t_sw_gather)) {
            return;
        }
        gated_signal(a, 0, a.t_sig_stage, /*pub_done=*/false);
    }
    if (!zc_wait2(a, 0, a.t_stage, 2, a.t_prev_gather)) {
        return;
    }
    bcast_phase<kBcastDepth>(a);
    if (!gated_signal_last(a, 1, a.t_sig_reduce)) {
        return;
    }
    if (!gated_wait(a, 1, a.t_gather_wait)) {
        return;
    }
    gated_signal(a, 2, a.t_sig_gather, /*pub_done=*/true);
}

/* bcast_phase alone, for measurement and unit tests: no flags, no waits,
 * no signals (the k_zc_data of the bcast). */
__global__ void __launch_bounds__(256) k_bcast_data(const GatedArgs a)
{
    bcast_phase<kBcastDepth>(a);
}

/* ----------------------------------------------------------- launchers */
static inline int gated_grid(const GatedArgs &a)
{
    int b = a.nblocks ? a.nblocks : kGatedBlocks;
    return b > kGatedMaxBlocks ? kGatedMaxBlocks : b;
}

ucc_status_t staged_stage(const GatedArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_staged_stage, dim3(gated_grid(a)), dim3(256), 0,
                       s, a);
    return launch_status();
}

ucc_status_t staged_gather(const GatedArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_staged_gather, dim3(gated_grid(a)), dim3(256), 0,
                       s, a);
    return launch_status();
}

ucc_status_t gated_wait_only(const GatedArgs &a, hipStream_t s)
{
    /* pure wait: one block is enough (it adds no signal counts) */
    hipLaunchKernelGGL(k_gated_wait_only, dim3(1), dim3(256), 0, s, a);
    return launch_status();
}

ucc_status_t gated_done(const GatedArgs &a, hipStream_t s)
{
    /* must launch the full gated grid: signal arithmetic is counts*B */
    hipLaunchKernelGGL(k_gated_done, dim3(gated_grid(a)), dim3(256),
                       0, s, a);
    return launch_status();
}

/* tuning knobs of the two reduce kernels, read once. UCC_EC_REDUCE_DEPTH
 * overrides the batching depth (0 = auto), UCC_EC_REDUCE_THREADS the
 * threads per block (each launcher keeps the values it supports, else
 * 256). The protocol counts BLOCKS, so the grid is fixed by the ledger;
 * threads-per-block is a free tuning axis (the wait/signal logic only
 * needs >= 64 threads). */
struct ReduceKnobs {
    int depth, threads;
};
static const ReduceKnobs &reduce_knobs()
{
    static const ReduceKnobs k = [] {
        const char *d = getenv("UCC_EC_REDUCE_DEPTH");
        const char *t = getenv("UCC_EC_REDUCE_THREADS");
        return ReduceKnobs{d ? atoi(d) : 0, t ? atoi(t) : 0};
    }();
    return k;
}

/* batching depth by rank count (bytes-in-flight per lane vs pack register
 * budget — see k_staged_reduce), or the override */
static int reduce_depth(int nranks)
{
    const int ov = reduce_knobs().depth;
    return ov ? ov : (nranks <= 2 ? 4 : nranks <= 4 ? 2 : 1);
}

/* launch(integral_constant<int, U>) for the instantiated depth U <= MAXU
 * that `depth` names; any other depth runs as 1 */
template <int MAXU, typename F>
static ucc_status_t launch_by_depth(int depth, F &&launch)
{
    if constexpr (MAXU >= 8) {
        if (depth == 8) {
            launch(std::integral_constant<int, 8>{});
            return launch_status();
        }
    }
    if (depth == 4) {
        launch(std::integral_constant<int, 4>{});
    } else if (depth == 2) {
        launch(std::integral_constant<int, 2>{});
    } else {
        launch(std::integral_constant<int, 1>{});
    }
    return launch_status();
}

template <typename T, int OP> struct LaunchStagedReduce {
    static ucc_status_t run(const GatedArgs &a, hipStream_t s)
    {
        const int thr     = reduce_knobs().threads;
        const int threads = (thr == 128 || thr == 512 || thr == 1024) ? thr
                                                                      : 256;
        return launch_by_depth<8>(reduce_depth(a.nranks), [&](auto u) {
            hipLaunchKernelGGL(
                (k_staged_reduce<T, OP, VecOf<T>::value, decltype(u)::value>),
                dim3(gated_grid(a)), dim3(threads), 0, s, a);
        });
    }
};

ucc_status_t staged_reduce(const GatedArgs &a, hipStream_t s)
{
    return dispatch<LaunchStagedReduce>(fold_complex(a.dt, a.op, nullptr),
                                        a.op, a, s);
}

/* Batching depth of the zero-copy data phase. It unrolls kMaxRanks / U
 * peers, so the depth is halved until U * nranks fits; depth 8 runs as 4
 * (the second pack buffer already doubles the bytes in flight). */
int zc_depth(int nranks)
{
    int depth = std::min(reduce_depth(nranks), 4);
    while (depth > 1 && depth * nranks > kMaxRanks) {
        depth /= 2;
    }
    return depth;
}

/* threads per block of the zero-copy kernels, compiled for at most 256 */
static int zc_threads()
{
    return reduce_knobs().threads == 128 ? 128 : 256;
}

/* The streamed (NT) data phase exists at depth 4 only: 2 ranks at the
 * default depth, the one case measured (profiles/zc_edges_stream.md). */
bool zc_has_stream(int nranks)
{
    return nranks >= 2 && nranks <= kMaxRanks && zc_depth(nranks) == 4;
}

template <typename T, int OP> struct LaunchZcAllreduce {
    static ucc_status_t run(const GatedArgs &a, hipStream_t s)
    {
        if (a.zc_stream && zc_has_stream(a.nranks)) {
            hipLaunchKernelGGL(
                (k_zc_allreduce<T, OP, VecOf<T>::value, 4, true>),
                dim3(gated_grid(a)), dim3(zc_threads()), 0, s, a);
            return launch_status();
        }
        return launch_by_depth<4>(zc_depth(a.nranks), [&](auto u) {
            hipLaunchKernelGGL((k_zc_allreduce<T, OP, VecOf<T>::value,
                                               decltype(u)::value, false>),
                               dim3(gated_grid(a)), dim3(zc_threads()), 0,
                               s, a);
        });
    }
};

struct ZcDataLaunch {
    const GatedArgs &a;
    int              threads;
};
template <typename T, int OP> struct LaunchZcData {
    static ucc_status_t run(const ZcDataLaunch &l, hipStream_t s)
    {
        if (l.a.zc_stream) { /* zc_data checked zc_has_stream */
            hipLaunchKernelGGL((k_zc_data<T, OP, VecOf<T>::value, 4, true>),
                               dim3(gated_grid(l.a)), dim3(l.threads), 0, s,
                               l.a);
            return launch_status();
        }
        return launch_by_depth<4>(zc_depth(l.a.nranks), [&](auto u) {
            hipLaunchKernelGGL((k_zc_data<T, OP, VecOf<T>::value,
                                          decltype(u)::value, false>),
                               dim3(gated_grid(l.a)), dim3(l.threads), 0, s,
                               l.a);
        });
    }
};

ucc_status_t zc_allreduce(const GatedArgs &a, hipStream_t s)
{
    if (a.derive || a.nranks < 2 || a.nranks > kMaxRanks) {
        return UCC_ERR_NOT_SUPPORTED; /* host-target mode only */
    }
    return dispatch<LaunchZcAllreduce>(fold_complex(a.dt, a.op, nullptr),
                                       a.op, a, s);
}

ucc_status_t zc_data(const GatedArgs &a, hipStream_t s, int threads)
{
    if (a.nranks < 2 || a.nranks > kMaxRanks || a.sl_e < a.sl_b ||
        (threads != 0 && threads != 64 && threads != 128 &&
         threads != 256)) {
        return UCC_ERR_INVALID_PARAM;
    }
    if (a.zc_stream && !zc_has_stream(a.nranks)) {
        return UCC_ERR_NOT_SUPPORTED; /* no streamed instantiation */
    }
    const ZcDataLaunch l{a, threads ? threads : zc_threads()};
    return dispatch<LaunchZcData>(fold_complex(a.dt, a.op, nullptr), a.op,
                                  l, s);
}

ucc_status_t staged_bscatter(const GatedArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_staged_bscatter, dim3(gated_grid(a)), dim3(256), 0,
                       s, a);
    return launch_status();
}

ucc_status_t zc_bcast(const GatedArgs &a, hipStream_t s)
{
    if (a.derive || !a.zc_write || a.nranks < 2 || a.nranks > kMaxRanks ||
        a.sl_e < a.sl_b) {
        return UCC_ERR_NOT_SUPPORTED; /* host-target push form only */
    }
    hipLaunchKernelGGL(k_zc_bcast, dim3(gated_grid(a)), dim3(256), 0, s, a);
    return launch_status();
}

ucc_status_t bcast_data(const GatedArgs &a, hipStream_t s, int threads)
{
    if (a.nranks < 1 || a.nranks > kMaxRanks || a.sl_e < a.sl_b ||
        !a.peer_in[0] || (!a.zc_write && !a.my_out) ||
        (threads != 0 && threads != 64 && threads != 128 &&
         threads != 256)) {
        return UCC_ERR_INVALID_PARAM;
    }
    hipLaunchKernelGGL(k_bcast_data, dim3(gated_grid(a)),
                       dim3(threads ? threads : 256), 0, s, a);
    return launch_status();
}

} // namespace ec_hip
} // namespace ucc
