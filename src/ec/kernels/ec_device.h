/* Device code shared by the gfx950 execution-component kernels
 * (ec_reduce.hip, ec_fused.hip, ec_gated.hip): conversions, the reduce
 * core, byte copies, system-scope flag access with THE bounded spin, and
 * THE dtype x op dispatch table.
 *
 * Design (MI355X-first; G-numbers are the CDNA HIP programming guide's):
 *  - 256-thread workgroups (4 waves of 64), grid-stride loops capped so the
 *    scheduler keeps the chip busy without oversubscription (G11).
 *  - 16 B per lane vector packs (G13): bf16/fp16 loaded as ushort8-class
 *    packs, converted to f32, accumulated in f32; fp64 in f64; ints in T.
 *  - cross-GPU arrival flags are u64 system-scope atomics on fine-grained
 *    memory; payload ordering = __threadfence_system on the producer
 *    before the flag store, one system acquire on the consumer after the
 *    poll matches (the G16 protocol lifted to system scope for xGMI
 *    peers). Every spin is bounded and reports via error_word.
 */
#ifndef UCC_AMD_EC_DEVICE_H_
#define UCC_AMD_EC_DEVICE_H_

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "../ec_hip.h"

namespace ucc {
namespace ec_hip {

/* ------------------------------------------------------------ convert  */
__device__ __forceinline__ float d_bf16_to_f(uint16_t v)
{
    union {
        uint32_t u;
        float    f;
    } c;
    c.u = (uint32_t)v << 16;
    return c.f;
}
__device__ __forceinline__ uint16_t d_f_to_bf16(float f)
{
    union {
        uint32_t u;
        float    f;
    } c;
    c.f = f;
    uint32_t r = 0x7fff + ((c.u >> 16) & 1);
    return (uint16_t)((c.u + r) >> 16);
}

/* fp8 (OCP): gfx950 has native OCP fp8<->f32 converts (VOP1/VOP3
 * v_cvt_f32_fp8 / v_cvt_pk_fp8_f32) — use them on device; the bit-math
 * path below stays as the portable reference (and matches the host
 * codec bit-for-bit on finite values). */
#if defined(__gfx950__)
#define UCC_NATIVE_FP8 1
#endif

#ifdef UCC_NATIVE_FP8
/* The reduction rule (docs/USER_GUIDE.md, "Reduction numerics") saturates
 * FINITE overflow to +-max. The pk converts are not relied on for that
 * (ROCm's own fp8 header clamps in front of them too): clamp in f32
 * first; NaN and +-inf (exponent field all ones) pass through untouched. */
__device__ __forceinline__ float d_satfinite(float f, float big)
{
    return (__float_as_uint(f) & 0x7f800000u) == 0x7f800000u
               ? f
               : __builtin_amdgcn_fmed3f(f, big, -big);
}
constexpr float kE4m3Max = 448.0f;
constexpr float kE5m2Max = 57344.0f;
/* paired converts: one VOP handles 2 elements (v_cvt_pk_f32_fp8 /
 * v_cvt_pk_fp8_f32) — halves the VALU cost of the fp8 reduce, which is
 * 2x the elements per byte of bf16 */
__device__ __forceinline__ void d_e4m3x2_to_f(uint8_t lo, uint8_t hi,
                                              float &a, float &b)
{
    int packed = (int)lo | ((int)hi << 8);
    auto v2    = __builtin_amdgcn_cvt_pk_f32_fp8(packed, false);
    a          = v2[0];
    b          = v2[1];
}
__device__ __forceinline__ void d_f_to_e4m3x2(float a, float b,
                                              uint8_t &lo, uint8_t &hi)
{
    a = d_satfinite(a, kE4m3Max);
    b = d_satfinite(b, kE4m3Max);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    lo    = (uint8_t)w;
    hi    = (uint8_t)(w >> 8);
}
__device__ __forceinline__ void d_e5m2x2_to_f(uint8_t lo, uint8_t hi,
                                              float &a, float &b)
{
    int packed = (int)lo | ((int)hi << 8);
    auto v2    = __builtin_amdgcn_cvt_pk_f32_bf8(packed, false);
    a          = v2[0];
    b          = v2[1];
}
__device__ __forceinline__ void d_f_to_e5m2x2(float a, float b,
                                              uint8_t &lo, uint8_t &hi)
{
    a = d_satfinite(a, kE5m2Max);
    b = d_satfinite(b, kE5m2Max);
    int w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    lo    = (uint8_t)w;
    hi    = (uint8_t)(w >> 8);
}
/* dword-wide converts: the pk builtins take a word-select operand, so
 * one dword (4 fp8) costs exactly 2 VOPs each way with NO byte
 * repacking VALU (the paired path above still assembles a 16-bit
 * packed operand from two byte registers per pair). */
__device__ __forceinline__ void d_e4m3x4_to_f(uint32_t w, float &a,
                                              float &b, float &c,
                                              float &d)
{
    auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    a       = lo[0];
    b       = lo[1];
    c       = hi[0];
    d       = hi[1];
}
__device__ __forceinline__ uint32_t d_f_to_e4m3x4(float a, float b,
                                                  float c, float d)
{
    a = d_satfinite(a, kE4m3Max);
    b = d_satfinite(b, kE4m3Max);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    c = d_satfinite(c, kE4m3Max);
    d = d_satfinite(d, kE4m3Max);
    w     = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}
__device__ __forceinline__ void d_e5m2x4_to_f(uint32_t w, float &a,
                                              float &b, float &c,
                                              float &d)
{
    auto lo = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, false);
    auto hi = __builtin_amdgcn_cvt_pk_f32_bf8((int)w, true);
    a       = lo[0];
    b       = lo[1];
    c       = hi[0];
    d       = hi[1];
}
__device__ __forceinline__ uint32_t d_f_to_e5m2x4(float a, float b,
                                                  float c, float d)
{
    a = d_satfinite(a, kE5m2Max);
    b = d_satfinite(b, kE5m2Max);
    int w = __builtin_amdgcn_cvt_pk_bf8_f32(a, b, 0, false);
    c = d_satfinite(c, kE5m2Max);
    d = d_satfinite(d, kE5m2Max);
    w     = __builtin_amdgcn_cvt_pk_bf8_f32(c, d, w, true);
    return (uint32_t)w;
}
__device__ __forceinline__ float d_e4m3_to_f(uint8_t v)
{
    return __builtin_amdgcn_cvt_f32_fp8((int)v, 0);
}
__device__ __forceinline__ uint8_t d_f_to_e4m3(float f)
{
    f = d_satfinite(f, kE4m3Max);
    return (uint8_t)__builtin_amdgcn_cvt_pk_fp8_f32(f, f, 0, false);
}
__device__ __forceinline__ float d_e5m2_to_f(uint8_t v)
{
    return __builtin_amdgcn_cvt_f32_bf8((int)v, 0);
}
__device__ __forceinline__ uint8_t d_f_to_e5m2(float f)
{
    f = d_satfinite(f, kE5m2Max);
    return (uint8_t)__builtin_amdgcn_cvt_pk_bf8_f32(f, f, 0, false);
}
#else
__device__ __forceinline__ float d_e4m3_to_f(uint8_t v)
{
    uint32_t sign = v >> 7, exp = (v >> 3) & 0xf, man = v & 7;
    float    val;
    if (exp == 0xf && man == 7) {
        return __builtin_nanf("");
    }
    if (exp == 0) {
        val = (float)man * (1.0f / 512.0f);
    } else {
        val = (1.0f + (float)man * 0.125f) * exp2f((float)exp - 7.0f);
    }
    return sign ? -val : val;
}
__device__ __forceinline__ uint8_t d_f_to_e4m3(float f)
{
    if (isnan(f)) {
        return 0x7f;
    }
    uint8_t sign = signbit(f) ? 0x80 : 0;
    float   a    = fabsf(f);
    if (a >= 448.0f) {
        return sign | 0x7e;
    }
    if (a == 0.0f) {
        return sign;
    }
    int   e;
    float m   = frexpf(a, &e);
    int   exp = e - 1 + 7;
    if (exp <= 0) {
        int mi = (int)rintf(a * 512.0f);
        if (mi >= 8) {
            return sign | 0x08;
        }
        return sign | (uint8_t)mi;
    }
    int mi = (int)rintf((m * 2.0f - 1.0f) * 8.0f);
    if (mi >= 8) {
        mi = 0;
        exp++;
    }
    if (exp > 0xf || (exp == 0xf && mi == 7)) {
        return sign | 0x7e;
    }
    return sign | (uint8_t)(exp << 3) | (uint8_t)mi;
}
__device__ __forceinline__ float d_e5m2_to_f(uint8_t v)
{
    uint32_t sign = v >> 7, exp = (v >> 2) & 0x1f, man = v & 3;
    if (exp == 0x1f) {
        return man ? __builtin_nanf("")
                   : (sign ? -__builtin_inff() : __builtin_inff());
    }
    float val;
    if (exp == 0) {
        val = (float)man * 0.25f * exp2f(-14.0f);
    } else {
        val = (1.0f + (float)man * 0.25f) * exp2f((float)exp - 15.0f);
    }
    return sign ? -val : val;
}
__device__ __forceinline__ uint8_t d_f_to_e5m2(float f)
{
    if (isnan(f)) {
        return 0x7f;
    }
    uint8_t sign = signbit(f) ? 0x80 : 0;
    float   a    = fabsf(f);
    if (isinf(f)) {
        return sign | 0x7c;
    }
    if (a == 0.0f) {
        return sign;
    }
    int   e;
    float m   = frexpf(a, &e);
    int   exp = e - 1 + 15;
    if (exp <= 0) {
        int mi = (int)rintf(a * exp2f(14.0f) * 4.0f);
        if (mi >= 4) {
            return sign | 0x04;
        }
        return sign | (uint8_t)mi;
    }
    int mi = (int)rintf((m * 2.0f - 1.0f) * 4.0f);
    if (mi >= 4) {
        mi = 0;
        exp++;
    }
    if (exp >= 0x1f) { /* finite overflow saturates to max finite */
        return sign | 0x7b;
    }
    return sign | (uint8_t)(exp << 2) | (uint8_t)mi;
}
#endif /* UCC_NATIVE_FP8 */

/* type traits: storage type T <-> accumulator A */
template <typename T> struct Cvt {
    using A = T;
    static __device__ __forceinline__ A load(T v) { return v; }
    static __device__ __forceinline__ T store(A v) { return (T)v; }
};
struct bf16_t {
    uint16_t v;
};
template <> struct Cvt<bf16_t> {
    using A = float;
    static __device__ __forceinline__ float load(bf16_t x)
    {
        return d_bf16_to_f(x.v);
    }
    static __device__ __forceinline__ bf16_t store(float f)
    {
        return {d_f_to_bf16(f)};
    }
};
struct fp16_t {
    _Float16 v;
};
template <> struct Cvt<fp16_t> {
    using A = float;
    static __device__ __forceinline__ float load(fp16_t x)
    {
        return (float)x.v;
    }
    static __device__ __forceinline__ fp16_t store(float f)
    {
        return {(_Float16)f};
    }
};
struct e4m3_t {
    uint8_t v;
};
template <> struct Cvt<e4m3_t> {
    using A = float;
    static __device__ __forceinline__ float load(e4m3_t x)
    {
        return d_e4m3_to_f(x.v);
    }
    static __device__ __forceinline__ e4m3_t store(float f)
    {
        return {d_f_to_e4m3(f)};
    }
};
struct e5m2_t {
    uint8_t v;
};
template <> struct Cvt<e5m2_t> {
    using A = float;
    static __device__ __forceinline__ float load(e5m2_t x)
    {
        return d_e5m2_to_f(x.v);
    }
    static __device__ __forceinline__ e5m2_t store(float f)
    {
        return {d_f_to_e5m2(f)};
    }
};

/* op ids match ucc_reduction_op_t */
template <typename A, int OP>
__device__ __forceinline__ A red(A a, A b)
{
    if constexpr (OP == 0 || OP == 12) { /* SUM / AVG */
        return a + b;
    } else if constexpr (OP == 1) {
        return a * b;
    } else if constexpr (OP == 2) {
        return a > b ? a : b;
    } else if constexpr (OP == 3) {
        return a < b ? a : b;
    } else if constexpr (OP == 4) {
        return (A)((a != (A)0) && (b != (A)0));
    } else if constexpr (OP == 5) {
        return (A)((a != (A)0) || (b != (A)0));
    } else if constexpr (OP == 6) {
        return (A)((a != (A)0) != (b != (A)0));
    } else if constexpr (OP == 7) {
        if constexpr (!std::is_floating_point<A>::value) {
            return a & b;
        }
    } else if constexpr (OP == 8) {
        if constexpr (!std::is_floating_point<A>::value) {
            return a | b;
        }
    } else if constexpr (OP == 9) {
        if constexpr (!std::is_floating_point<A>::value) {
            return a ^ b;
        }
    }
    return a;
}

template <typename A>
__device__ __forceinline__ A apply_alpha(A v, double alpha)
{
    if constexpr (std::is_floating_point<A>::value) {
        /* The product is rounded to A HERE; the store converts it once
         * more. The empty asm pins that: without it instruction selection
         * folds this multiply into the fp16 convert
         * (v_fma_mixlo_f16 v, alpha, 0), which rounds once from the exact
         * product and turns -0 into +0 (-0 * alpha + 0). It is selection,
         * not contraction: `#pragma clang fp contract(off)` leaves it. */
        A p = v * (A)alpha;
        asm("" : "+v"(p));
        return p;
    } else {
        (void)alpha;
        return v;
    }
}

/* ------------------------------------------------------------- reduce  */
/* VEC chosen so VEC*sizeof(T) == 16 bytes (one dwordx4 per lane). */
template <typename T> struct VecOf {
    static constexpr int value = 16 / (int)sizeof(T);
};

template <typename T, int OP, int VEC>
struct __align__(16) Pack {
    T v[VEC];
};

#ifdef UCC_NATIVE_FP8
template <typename T>
inline constexpr bool is_fp8_v = std::is_same<T, e4m3_t>::value ||
                                 std::is_same<T, e5m2_t>::value;

template <typename T>
__device__ __forceinline__ void cvt2_load(T lo, T hi, float &a, float &b)
{
    if constexpr (std::is_same<T, e4m3_t>::value) {
        d_e4m3x2_to_f(lo.v, hi.v, a, b);
    } else {
        d_e5m2x2_to_f(lo.v, hi.v, a, b);
    }
}
template <typename T>
__device__ __forceinline__ void cvt2_store(float a, float b, T &lo, T &hi)
{
    if constexpr (std::is_same<T, e4m3_t>::value) {
        d_f_to_e4m3x2(a, b, lo.v, hi.v);
    } else {
        d_f_to_e5m2x2(a, b, lo.v, hi.v);
    }
}
template <typename T>
__device__ __forceinline__ void cvt4_load(uint32_t w, float &a, float &b,
                                          float &c, float &d)
{
    if constexpr (std::is_same<T, e4m3_t>::value) {
        d_e4m3x4_to_f(w, a, b, c, d);
    } else {
        d_e5m2x4_to_f(w, a, b, c, d);
    }
}
template <typename T>
__device__ __forceinline__ uint32_t cvt4_store(float a, float b, float c,
                                               float d)
{
    if constexpr (std::is_same<T, e4m3_t>::value) {
        return d_f_to_e4m3x4(a, b, c, d);
    }
    return d_f_to_e5m2x4(a, b, c, d);
}
#else
template <typename T> inline constexpr bool is_fp8_v = false;
template <typename T>
__device__ __forceinline__ void cvt2_load(T, T, float &, float &) {}
template <typename T>
__device__ __forceinline__ void cvt2_store(float, float, T &, T &) {}
template <typename T>
__device__ __forceinline__ void cvt4_load(uint32_t, float &, float &,
                                          float &, float &)
{
}
template <typename T>
__device__ __forceinline__ uint32_t cvt4_store(float, float, float,
                                               float)
{
    return 0;
}
#endif

/* vector-wide load/accumulate/store with dword-wide fp8 fast paths
 * (4 elements per word-selected pk convert pair, zero repack VALU) */
template <int N> struct __align__(16) PackW {
    uint32_t w[N];
};

template <typename T, int OP, int VEC, typename A, typename P>
__device__ __forceinline__ void vload(const P &x, A (&r)[VEC])
{
    if constexpr (is_fp8_v<T> && std::is_same<A, float>::value &&
                  VEC % 4 == 0) {
        auto pw = __builtin_bit_cast(PackW<VEC / 4>, x);
#pragma unroll
        for (int j = 0; j < VEC / 4; j++) {
            cvt4_load<T>(pw.w[j], r[4 * j], r[4 * j + 1], r[4 * j + 2],
                         r[4 * j + 3]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            r[k] = Cvt<T>::load(x.v[k]);
        }
    }
}
template <typename T, int OP, int VEC, typename A, typename P>
__device__ __forceinline__ void vaccum(A (&r)[VEC], const P &x)
{
    if constexpr (is_fp8_v<T> && std::is_same<A, float>::value &&
                  VEC % 4 == 0) {
        auto pw = __builtin_bit_cast(PackW<VEC / 4>, x);
#pragma unroll
        for (int j = 0; j < VEC / 4; j++) {
            float a, b, c, d;
            cvt4_load<T>(pw.w[j], a, b, c, d);
            r[4 * j]     = red<A, OP>(r[4 * j], a);
            r[4 * j + 1] = red<A, OP>(r[4 * j + 1], b);
            r[4 * j + 2] = red<A, OP>(r[4 * j + 2], c);
            r[4 * j + 3] = red<A, OP>(r[4 * j + 3], d);
        }
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            r[k] = red<A, OP>(r[k], Cvt<T>::load(x.v[k]));
        }
    }
}
template <typename T, int OP, int VEC, typename A, typename P>
__device__ __forceinline__ void vstore(P &o, const A (&r)[VEC],
                                       double alpha)
{
    if constexpr (is_fp8_v<T> && std::is_same<A, float>::value &&
                  VEC % 4 == 0) {
        PackW<VEC / 4> pw;
#pragma unroll
        for (int j = 0; j < VEC / 4; j++) {
            pw.w[j] = cvt4_store<T>(apply_alpha<A>(r[4 * j], alpha),
                                    apply_alpha<A>(r[4 * j + 1], alpha),
                                    apply_alpha<A>(r[4 * j + 2], alpha),
                                    apply_alpha<A>(r[4 * j + 3], alpha));
        }
        o = __builtin_bit_cast(P, pw);
    } else {
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            o.v[k] = Cvt<T>::store(apply_alpha<A>(r[k], alpha));
        }
    }
}

/* -------------------------------------------------------- reduce core  */
/* One 16 B pack / one element at index i of n sources: load from
 * srcs[s] + off (bytes), reduce sources 0..n-1 in that order, apply
 * alpha. srcs is a pointer array of the kernel argument, indexed at run
 * time in the kernarg segment. */
template <typename T, int OP, int VEC, int N>
__device__ __forceinline__ Pack<T, OP, VEC>
reduce_pack(const void *const (&srcs)[N], uint64_t off, int n, uint64_t i,
            double alpha)
{
    using A = typename Cvt<T>::A;
    using P = Pack<T, OP, VEC>;
    P acc   = ((const P *)((const uint8_t *)srcs[0] + off))[i];
    A r[VEC];
    vload<T, OP, VEC, A>(acc, r);
    for (int s = 1; s < n; s++) {
        P x = ((const P *)((const uint8_t *)srcs[s] + off))[i];
        vaccum<T, OP, VEC, A>(r, x);
    }
    P o;
    vstore<T, OP, VEC, A>(o, r, alpha);
    return o;
}

template <typename T, int OP, int N>
__device__ __forceinline__ T
reduce_elem(const void *const (&srcs)[N], uint64_t off, int n, uint64_t t,
            double alpha)
{
    using A = typename Cvt<T>::A;
    A r = Cvt<T>::load(((const T *)((const uint8_t *)srcs[0] + off))[t]);
    for (int s = 1; s < n; s++) {
        r = red<A, OP>(
            r,
            Cvt<T>::load(((const T *)((const uint8_t *)srcs[s] + off))[t]));
    }
    return Cvt<T>::store(apply_alpha<A>(r, alpha));
}

/* the grid-stride "packs, then scalar tail" reduction of count elements
 * from n sources into dst (k_reduce, the fused small-message kernels) */
template <typename T, int OP, int VEC, int N>
__device__ __forceinline__ void
reduce_range(void *dst, const void *const (&srcs)[N], uint64_t off, int n,
             uint64_t count, double alpha)
{
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t str = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t nv  = count / VEC;
    using P            = Pack<T, OP, VEC>;
    for (uint64_t i = tid; i < nv; i += str) {
        ((P *)dst)[i] = reduce_pack<T, OP, VEC>(srcs, off, n, i, alpha);
    }
    for (uint64_t t = nv * VEC + tid; t < count; t += str) {
        ((T *)dst)[t] = reduce_elem<T, OP>(srcs, off, n, t, alpha);
    }
}

/* -------------------------------------------------------- gather copy  */
__device__ __forceinline__ void d_copy_bytes_part(uint8_t *dst,
                                                  const uint8_t *src,
                                                  uint64_t len,
                                                  uint64_t vblock,
                                                  uint64_t vgrid)
{
    const uint64_t tid = vblock * blockDim.x + threadIdx.x;
    const uint64_t str = vgrid * blockDim.x;
    if ((((uintptr_t)dst | (uintptr_t)src) & 15) == 0) {
        uint64_t nv = len / 16;
        uint64_t i  = tid;
        /* 4-deep load batching: all four 16B loads issue before the
         * first dependent store (64B outstanding per lane — G7). */
        for (; i + 3 * str < nv; i += 4 * str) {
            uint4 v0 = ((const uint4 *)src)[i];
            uint4 v1 = ((const uint4 *)src)[i + str];
            uint4 v2 = ((const uint4 *)src)[i + 2 * str];
            uint4 v3 = ((const uint4 *)src)[i + 3 * str];
            ((uint4 *)dst)[i]           = v0;
            ((uint4 *)dst)[i + str]     = v1;
            ((uint4 *)dst)[i + 2 * str] = v2;
            ((uint4 *)dst)[i + 3 * str] = v3;
        }
        for (; i < nv; i += str) {
            ((uint4 *)dst)[i] = ((const uint4 *)src)[i];
        }
        for (uint64_t t = nv * 16 + tid; t < len; t += str) {
            dst[t] = src[t];
        }
    } else {
        for (uint64_t i = tid; i < len; i += str) {
            dst[i] = src[i];
        }
    }
}

__device__ __forceinline__ void d_copy_bytes(uint8_t *dst,
                                             const uint8_t *src,
                                             uint64_t len)
{
    d_copy_bytes_part(dst, src, len, blockIdx.x, gridDim.x);
}

/* ------------------------------------------- system-scope flags, spins  */
__device__ __forceinline__ uint64_t
sys_load(const uint64_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void sys_store(uint64_t *p, uint64_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

constexpr uint64_t kSpinLimit = kDefaultSpinLimit;
__device__ __forceinline__ uint64_t spin_cap(uint64_t v)
{
    return v ? v : kSpinLimit;
}

/* THE bounded wait: poll *f until it reaches target; after cap polls set
 * *error_word and give up (false). The caller records the failure in its
 * own LDS flag and leaves through its own barriers: all threads of a block
 * leave together, none returns past a sibling's __syncthreads. */
__device__ __forceinline__ bool spin_until(const uint64_t *f,
                                           uint64_t target, uint64_t cap,
                                           uint64_t *error_word)
{
    uint64_t spins = 0;
    while (sys_load(f) < target) {
        if (++spins > cap) {
            sys_store(error_word, 1);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
    return true;
}

/* ------------------------------------------ fused one-kernel protocol  */
/* The sequencing, handshake and completion steps shared by the fused
 * small-message kernels (ec_fused.hip: allreduce; ec_fused_colls.hip: the
 * other collectives). All of them run on the same flag words and counters
 * of a slot, so they compose on one slot sequence.
 *
 * DEV_SEQ = false (FusedArgs-style fields): the host tracks the sequence
 * number, the cumulative stage target and the spin limit, and may ask for
 * the host-visible completion word.
 * DEV_SEQ = true (GraphFusedArgs-style fields): the iteration number is
 * this block's launch count, so one captured launch replays as a new
 * collective each time; staging alternates between two parity areas; the
 * spin cap is the default. */
struct FusedIter {
    uint64_t seq, par, stage_target, cap;
};

template <bool DEV_SEQ, typename Args>
__device__ __forceinline__ FusedIter fused_iter(const Args &a)
{
    FusedIter it;
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
        it.seq          = s_seq;
        it.par          = (it.seq & 1) * a.parity_stride;
        it.stage_target = it.seq * (uint64_t)a.nblocks;
        it.cap          = kSpinLimit;
    } else {
        it.seq          = a.seq;
        it.par          = 0;
        it.stage_target = a.stage_target;
        it.cap          = spin_cap(a.spin_limit);
    }
    return it;
}

/* Called by every thread once its staging stores are issued. Publishes the
 * staged data, signals every peer and waits for all ranks. false: a spin
 * timed out (error_word is set); all threads of the block get the same
 * answer and must leave. */
template <typename Args>
__device__ __forceinline__ bool fused_handshake(const Args &a,
                                                const FusedIter &it)
{
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
            !spin_until(stage_cnt, it.stage_target, it.cap, a.error_word)) {
            s_err = 1;
        }
        __syncthreads();
        if (!s_err && (int)threadIdx.x < a.nranks) {
            sys_store(a.peer_flags[threadIdx.x] +
                          (uint64_t)a.slot * kMaxRanks + a.rank,
                      it.seq);
        }
    }
    /* 3. all blocks wait for all ranks' arrivals (timeout: all threads
     * leave together — never return while siblings sit at a barrier) */
    if (!s_err && (int)threadIdx.x < a.nranks &&
        !spin_until(a.local_flags + (uint64_t)a.slot * kMaxRanks +
                        threadIdx.x,
                    it.seq, it.cap, a.error_word)) {
        s_err = 1;
    }
    __syncthreads();
    if (s_err) {
        return false;
    }
    __threadfence_system(); /* acquire: drop stale lines before peer reads */
    return true;
}

/* 5. host-visible completion: the last arriving block publishes
 * done_seq to the pinned word — the host polls plain memory
 * instead of event record+query (see FusedArgs.done_host). dst
 * stores are fenced before the arrival add; the release store
 * makes them visible to the host with the flag. */
template <typename Args>
__device__ __forceinline__ void fused_publish_done(const Args &a)
{
    if (a.done_host) {
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) {
            uint64_t v = __hip_atomic_fetch_add(
                             a.local_flags + kFusedDoneBase + a.slot, 1,
                             __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) +
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

/* ------------------------------------------------------------ dispatch  */
/* THE dtype x op table. L<T, OP>::run(a, s) is a launcher; OP ids match
 * ucc_reduction_op_t. Float types take SUM PROD MAX MIN AVG, integer
 * types SUM PROD MAX MIN and the logical / bitwise ops. */
template <template <typename, int> class L, typename T, typename Args>
static inline ucc_status_t dispatch_op(ucc_reduction_op_t op, const Args &a,
                                       hipStream_t s)
{
    switch (op) {
    case UCC_OP_SUM: return L<T, 0>::run(a, s);
    case UCC_OP_PROD: return L<T, 1>::run(a, s);
    case UCC_OP_MAX: return L<T, 2>::run(a, s);
    case UCC_OP_MIN: return L<T, 3>::run(a, s);
    default: break;
    }
    if constexpr (std::is_floating_point<typename Cvt<T>::A>::value) {
        if (op == UCC_OP_AVG) {
            return L<T, 12>::run(a, s);
        }
    } else {
        switch (op) {
        case UCC_OP_LAND: return L<T, 4>::run(a, s);
        case UCC_OP_LOR: return L<T, 5>::run(a, s);
        case UCC_OP_LXOR: return L<T, 6>::run(a, s);
        case UCC_OP_BAND: return L<T, 7>::run(a, s);
        case UCC_OP_BOR: return L<T, 8>::run(a, s);
        case UCC_OP_BXOR: return L<T, 9>::run(a, s);
        default: break;
        }
    }
    return UCC_ERR_NOT_SUPPORTED;
}

template <template <typename, int> class L, typename Args>
static inline ucc_status_t dispatch(ucc_datatype_t dt, ucc_reduction_op_t op,
                                    const Args &a, hipStream_t s)
{
    switch (dt) {
    case UCC_DT_BFLOAT16: return dispatch_op<L, bf16_t>(op, a, s);
    case UCC_DT_FLOAT16: return dispatch_op<L, fp16_t>(op, a, s);
    case UCC_DT_FLOAT32: return dispatch_op<L, float>(op, a, s);
    case UCC_DT_FLOAT64: return dispatch_op<L, double>(op, a, s);
    case UCC_DT_FLOAT8_E4M3: return dispatch_op<L, e4m3_t>(op, a, s);
    case UCC_DT_FLOAT8_E5M2: return dispatch_op<L, e5m2_t>(op, a, s);
    case UCC_DT_INT8: return dispatch_op<L, int8_t>(op, a, s);
    case UCC_DT_UINT8: return dispatch_op<L, uint8_t>(op, a, s);
    case UCC_DT_INT16: return dispatch_op<L, int16_t>(op, a, s);
    case UCC_DT_UINT16: return dispatch_op<L, uint16_t>(op, a, s);
    case UCC_DT_INT32: return dispatch_op<L, int32_t>(op, a, s);
    case UCC_DT_UINT32: return dispatch_op<L, uint32_t>(op, a, s);
    case UCC_DT_INT64: return dispatch_op<L, int64_t>(op, a, s);
    case UCC_DT_UINT64: return dispatch_op<L, uint64_t>(op, a, s);
    default: return UCC_ERR_NOT_SUPPORTED;
    }
}

static inline bool is_complex(ucc_datatype_t dt)
{
    return dt == UCC_DT_FLOAT32_COMPLEX || dt == UCC_DT_FLOAT64_COMPLEX;
}

/* complex SUM/AVG == elementwise float SUM/AVG on 2x the elements: the
 * float type to dispatch on. Args that count elements pass their count to
 * be doubled; byte-based GatedArgs pass nullptr. */
static inline ucc_datatype_t fold_complex(ucc_datatype_t dt,
                                          ucc_reduction_op_t op,
                                          uint64_t *count)
{
    if (!is_complex(dt) || (op != UCC_OP_SUM && op != UCC_OP_AVG)) {
        return dt;
    }
    if (count) {
        *count *= 2;
    }
    return dt == UCC_DT_FLOAT32_COMPLEX ? UCC_DT_FLOAT32 : UCC_DT_FLOAT64;
}

/* ------------------------------------------------------ launch helpers  */
static inline ucc_status_t launch_status()
{
    return hipGetLastError() == hipSuccess ? UCC_OK : UCC_ERR_NO_RESOURCE;
}

} // namespace ec_hip
} // namespace ucc

#endif
