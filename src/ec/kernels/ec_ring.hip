/* gfx950 execution-component kernel of the host-gated multi-ring
 * collectives: one ring step (ec_hip.h, RingStepArgs). Element-wise and
 * memory-bound: 256-thread workgroups dealt over the pieces by size,
 * grid-stride loops over 16-byte packs of T, the loads of `in` and `local`
 * issued together before the arithmetic. No waits, no flags, no atomics. */
#include "ec_device.h"

#include <atomic>

namespace ucc {
namespace ec_hip {

/* RingStepArgs plus what the launcher worked out: piece k owns workgroups
 * [blk0[k], blk0[k + 1]); bit k of vec_mask: every non-null pointer of the
 * piece is 16-byte aligned; copy_w[k]: access width of the byte copy */
struct RingKArgs {
    RingStepArgs a;
    int          blk0[kMaxRings + 1];
    uint32_t     vec_mask;
    int          copy_w[kMaxRings];
    int          dtsz;
};

__device__ __forceinline__ int ring_my_piece(const RingKArgs &ka)
{
    int k = 0;
    while (k + 1 < ka.a.n_rings && (int)blockIdx.x >= ka.blk0[k + 1]) {
        k++;
    }
    return k;
}

template <typename T, int OP>
__device__ __forceinline__ void ring_elem(const RingPiece &pc, bool in_acc,
                                          bool out_acc, uint64_t t,
                                          double alpha)
{
    using A = typename Cvt<T>::A;
    A r;
    if (pc.in) {
        r = in_acc ? ((const A *)pc.in)[t]
                   : Cvt<T>::load(((const T *)pc.in)[t]);
        if (pc.local) {
            r = red<A, OP>(r, Cvt<T>::load(((const T *)pc.local)[t]));
        }
    } else {
        r = Cvt<T>::load(((const T *)pc.local)[t]);
    }
    if (pc.out && out_acc) {
        ((A *)pc.out)[t] = r;
    }
    if (pc.dst || (pc.out && !out_acc)) {
        const T o = Cvt<T>::store(apply_alpha<A>(r, alpha));
        if (pc.dst) {
            ((T *)pc.dst)[t] = o;
        }
        if (pc.out && !out_acc) {
            ((T *)pc.out)[t] = o;
        }
    }
}

template <typename T, int OP>
__global__ void k_ring_step(RingKArgs ka)
{
    constexpr int VEC = VecOf<T>::value;
    using A           = typename Cvt<T>::A;
    using P           = Pack<T, OP, VEC>;
    struct __align__(16) PA {
        A v[VEC];
    };
    const int       k  = ring_my_piece(ka);
    const RingPiece pc = ka.a.piece[k];
    const uint64_t  vg = (uint64_t)(ka.blk0[k + 1] - ka.blk0[k]);
    const uint64_t  vb = (uint64_t)((int)blockIdx.x - ka.blk0[k]);
    const uint64_t  tid = vb * blockDim.x + threadIdx.x;
    const uint64_t  str = vg * blockDim.x;
    const bool      in_acc  = ka.a.in_acc != 0;
    const bool      out_acc = ka.a.out_acc != 0;
    const double    alpha   = ka.a.alpha;
    uint64_t        done    = 0; /* elements the pack loop covers */
    if ((ka.vec_mask >> k) & 1u) {
        const uint64_t nv = pc.count / VEC;
        done              = nv * VEC;
        for (uint64_t i = tid; i < nv; i += str) {
            A  r[VEC];
            P  ip, lp;
            PA ia;
            /* both loads in flight before the first use */
            if (pc.in) {
                if (in_acc) {
                    ia = ((const PA *)pc.in)[i];
                } else {
                    ip = ((const P *)pc.in)[i];
                }
            }
            if (pc.local) {
                lp = ((const P *)pc.local)[i];
            }
            if (pc.in) {
                if (in_acc) {
#pragma unroll
                    for (int e = 0; e < VEC; e++) {
                        r[e] = ia.v[e];
                    }
                } else {
                    vload<T, OP, VEC, A>(ip, r);
                }
                if (pc.local) {
                    vaccum<T, OP, VEC, A>(r, lp);
                }
            } else {
                vload<T, OP, VEC, A>(lp, r);
            }
            if (pc.out && out_acc) {
                PA oa;
#pragma unroll
                for (int e = 0; e < VEC; e++) {
                    oa.v[e] = r[e];
                }
                ((PA *)pc.out)[i] = oa;
            }
            if (pc.dst || (pc.out && !out_acc)) {
                P o;
                vstore<T, OP, VEC, A>(o, r, alpha);
                if (pc.dst) {
                    ((P *)pc.dst)[i] = o;
                }
                if (pc.out && !out_acc) {
                    ((P *)pc.out)[i] = o;
                }
            }
        }
    }
    for (uint64_t t = done + tid; t < pc.count; t += str) {
        ring_elem<T, OP>(pc, in_acc, out_acc, t, alpha);
    }
}

/* ----------------------------------------------------------- byte copy  */
template <typename W>
__device__ __forceinline__ void ring_copy_w(const RingPiece &pc,
                                            uint64_t nbytes, uint64_t tid,
                                            uint64_t str)
{
    const uint64_t n = nbytes / sizeof(W);
    for (uint64_t i = tid; i < n; i += str) {
        const W v = ((const W *)pc.in)[i];
        if (pc.dst) {
            ((W *)pc.dst)[i] = v;
        }
        if (pc.out) {
            ((W *)pc.out)[i] = v;
        }
    }
}

__global__ void k_ring_copy(RingKArgs ka)
{
    const int       k  = ring_my_piece(ka);
    const RingPiece pc = ka.a.piece[k];
    const uint64_t  vg = (uint64_t)(ka.blk0[k + 1] - ka.blk0[k]);
    const uint64_t  vb = (uint64_t)((int)blockIdx.x - ka.blk0[k]);
    const uint64_t  tid = vb * blockDim.x + threadIdx.x;
    const uint64_t  str = vg * blockDim.x;
    const uint64_t  nbytes = pc.count * (uint64_t)ka.dtsz;
    switch (ka.copy_w[k]) {
    case 16: {
        const uint64_t nv = nbytes / 16;
        uint64_t       i  = tid;
        /* 4-deep load batching, as d_copy_bytes_part */
        for (; i + 3 * str < nv; i += 4 * str) {
            const uint4 v0 = ((const uint4 *)pc.in)[i];
            const uint4 v1 = ((const uint4 *)pc.in)[i + str];
            const uint4 v2 = ((const uint4 *)pc.in)[i + 2 * str];
            const uint4 v3 = ((const uint4 *)pc.in)[i + 3 * str];
            if (pc.dst) {
                ((uint4 *)pc.dst)[i]           = v0;
                ((uint4 *)pc.dst)[i + str]     = v1;
                ((uint4 *)pc.dst)[i + 2 * str] = v2;
                ((uint4 *)pc.dst)[i + 3 * str] = v3;
            }
            if (pc.out) {
                ((uint4 *)pc.out)[i]           = v0;
                ((uint4 *)pc.out)[i + str]     = v1;
                ((uint4 *)pc.out)[i + 2 * str] = v2;
                ((uint4 *)pc.out)[i + 3 * str] = v3;
            }
        }
        for (; i < nv; i += str) {
            const uint4 v = ((const uint4 *)pc.in)[i];
            if (pc.dst) {
                ((uint4 *)pc.dst)[i] = v;
            }
            if (pc.out) {
                ((uint4 *)pc.out)[i] = v;
            }
        }
        for (uint64_t t = nv * 16 + tid; t < nbytes; t += str) {
            const uint8_t v = ((const uint8_t *)pc.in)[t];
            if (pc.dst) {
                ((uint8_t *)pc.dst)[t] = v;
            }
            if (pc.out) {
                ((uint8_t *)pc.out)[t] = v;
            }
        }
        break;
    }
    case 8: ring_copy_w<uint64_t>(pc, nbytes, tid, str); break;
    case 4: ring_copy_w<uint32_t>(pc, nbytes, tid, str); break;
    case 2: ring_copy_w<uint16_t>(pc, nbytes, tid, str); break;
    default: ring_copy_w<uint8_t>(pc, nbytes, tid, str); break;
    }
}

/* ----------------------------------------------------------- launchers */
static std::atomic<uint64_t> g_ring_launches{0};

uint64_t ring_step_launches() { return g_ring_launches.load(); }

static inline uintptr_t ring_ptr_bits(const RingPiece &pc)
{
    return (uintptr_t)pc.in | (uintptr_t)pc.local | (uintptr_t)pc.out |
           (uintptr_t)pc.dst;
}

/* deal the grid over the pieces: one workgroup per 256 units of a piece,
 * scaled down to `cap` in total, at least one for a piece with work */
static int ring_deal_blocks(RingKArgs &ka, const uint64_t (&units)[kMaxRings],
                            int cap)
{
    uint64_t want[kMaxRings] = {}, total = 0;
    for (int k = 0; k < ka.a.n_rings; k++) {
        want[k] = (units[k] + 255) / 256;
        total += want[k];
    }
    int at = 0;
    for (int k = 0; k < ka.a.n_rings; k++) {
        ka.blk0[k] = at;
        uint64_t b = want[k];
        if (total > (uint64_t)cap && b > 0) {
            b = b * (uint64_t)cap / total;
            b = b < 1 ? 1 : b;
        }
        at += (int)b;
    }
    for (int k = ka.a.n_rings; k <= kMaxRings; k++) {
        ka.blk0[k] = at;
    }
    return at;
}

template <typename T, int OP> struct LaunchRing {
    static ucc_status_t run(const RingKArgs &ka_in, hipStream_t s)
    {
        using A           = typename Cvt<T>::A;
        constexpr int VEC = VecOf<T>::value;
        RingKArgs     ka  = ka_in;
        uint64_t      units[kMaxRings] = {};
        ka.vec_mask                    = 0;
        for (int k = 0; k < ka.a.n_rings; k++) {
            const RingPiece &pc = ka.a.piece[k];
            if (pc.count == 0) {
                continue;
            }
            /* every pointer aligned to the type stored behind it */
            const uintptr_t in_al =
                (ka.a.in_acc ? sizeof(A) : sizeof(T)) - 1;
            const uintptr_t out_al =
                (ka.a.out_acc ? sizeof(A) : sizeof(T)) - 1;
            if (((uintptr_t)pc.in & in_al) || ((uintptr_t)pc.out & out_al) ||
                (((uintptr_t)pc.local | (uintptr_t)pc.dst) &
                 (sizeof(T) - 1))) {
                return UCC_ERR_INVALID_PARAM;
            }
            const bool vec = (ring_ptr_bits(pc) & 15) == 0;
            ka.vec_mask |= vec ? 1u << k : 0u;
            units[k] = vec ? (pc.count + VEC - 1) / VEC : pc.count;
        }
        const int cap    = ka.a.nblocks > 0 ? ka.a.nblocks : 2048;
        const int blocks = ring_deal_blocks(ka, units, cap);
        g_ring_launches.fetch_add(1, std::memory_order_relaxed);
        if (blocks == 0) {
            return UCC_OK;
        }
        hipLaunchKernelGGL((k_ring_step<T, OP>), dim3(blocks), dim3(256), 0,
                           s, ka);
        return launch_status();
    }
};

ucc_status_t ring_step(const RingStepArgs &a, hipStream_t s)
{
    if (a.n_rings < 1 || a.n_rings > kMaxRings || a.nblocks < 0) {
        return UCC_ERR_INVALID_PARAM;
    }
    RingKArgs ka{};
    ka.a      = a;
    bool copy = !a.in_acc && !a.out_acc;
    for (int k = 0; k < a.n_rings; k++) {
        const RingPiece &pc = a.piece[k];
        if (pc.count > 0 && !pc.in && !pc.local) {
            return UCC_ERR_INVALID_PARAM;
        }
        copy = copy && (pc.count == 0 || (pc.in && !pc.local));
    }
    if (!copy) {
        /* complex SUM / AVG: float on 2x the elements */
        ka.a.dt = fold_complex(a.dt, a.op, nullptr);
        if (ka.a.dt != a.dt) {
            for (int k = 0; k < a.n_rings; k++) {
                ka.a.piece[k].count *= 2;
            }
        }
        return dispatch<LaunchRing>(ka.a.dt, ka.a.op, ka, s);
    }
    /* byte copy: dt gives the element size only */
    ka.dtsz = (int)ucc_dt_size(a.dt);
    if (ka.dtsz <= 0) {
        return UCC_ERR_NOT_SUPPORTED;
    }
    uint64_t units[kMaxRings] = {};
    for (int k = 0; k < a.n_rings; k++) {
        const RingPiece &pc = a.piece[k];
        if (pc.count == 0) {
            continue;
        }
        const uint64_t  nbytes = pc.count * (uint64_t)ka.dtsz;
        const uintptr_t bits   = ring_ptr_bits(pc);
        int             w      = 16;
        if (bits & 15) {
            /* the widest access that divides every address and the length */
            w = 8;
            while (w > 1 && ((bits | (uintptr_t)nbytes) & (uintptr_t)(w - 1))) {
                w >>= 1;
            }
        }
        ka.copy_w[k] = w;
        units[k]     = (nbytes + (uint64_t)w - 1) / (uint64_t)w;
    }
    const int cap    = a.nblocks > 0 ? a.nblocks : 2048;
    const int blocks = ring_deal_blocks(ka, units, cap);
    g_ring_launches.fetch_add(1, std::memory_order_relaxed);
    if (blocks == 0) {
        return UCC_OK;
    }
    hipLaunchKernelGGL(k_ring_copy, dim3(blocks), dim3(256), 0, s, ka);
    return launch_status();
}

} // namespace ec_hip
} // namespace ucc
