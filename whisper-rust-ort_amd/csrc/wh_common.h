// wh_common.h — shared device helpers for the gfx950 kernels (wave64, MFMA 16x16 tiles).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <type_traits>

#include "../../include/whisper_hip.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) float f32x8;
typedef __attribute__((ext_vector_type(4))) double f64x4;

#define WH_WAVE 64
#define WH_HEAD_DIM 64

// ---------------------------------------------------------------------------------------------
// One "fragment" = 8 consecutive k-elements per lane.  Lane l of a wave holds, for the row/column
// index (l & 15), the k-range 8*(l>>4) .. 8*(l>>4)+7 of a 32-deep k-slab.
//   mma16(acc, a, b):  D[i][j] += sum_k A[i][k] * B[k][j]
//     a = A[i = l&15][k-range],  b = B[k-range][j = l&15]
//     D layout (all dtypes): column j = l & 15, rows i = 4*(l>>4) + r for r = 0..3 (acc[r]).
// bf16: one v_mfma_f32_16x16x32_bf16.  f32: eight v_mfma_f32_16x16x4_f32 (exact f32 fma chain);
// the per-instruction k assignment {8g+e : g=0..3} is a permutation of the slab, identical for
// both operands, so the contraction is the same sum.
// ---------------------------------------------------------------------------------------------
template <typename T> struct FragT;
template <> struct FragT<bf16> { typedef bf16x8 type; };
template <> struct FragT<float> { typedef f32x8 type; };

template <typename T>
__device__ __forceinline__ typename FragT<T>::type load_frag(const T* p) {
    return *reinterpret_cast<const typename FragT<T>::type*>(p);
}

__device__ __forceinline__ void mma16(f32x4& acc, const bf16x8& a, const bf16x8& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
__device__ __forceinline__ void mma16(f32x4& acc, const f32x8& a, const f32x8& b) {
#pragma unroll
    for (int e = 0; e < 8; e++) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[e], b[e], acc, 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// WH_PREC_F16X3: f32 storage, contractions on the fp16 matrix cores.  An operand value x is carried as two fp16 limbs,
// hi = f16(x), lo = f16(x - hi) (x - hi is exact in f32; 11 + 11 significant bits), and a product is three MFMAs:
//   sum_k a_k b_k  ~=  sum a.lo b.hi + sum a.hi b.lo + sum a.hi b.hi      (the lo.lo term, 2^-22 relative, is dropped)
// accumulated in f32 — measured against exact f32 on whisper-base: max |d logit| 6e-5, the distance between two f32
// implementations being 3e-5 (tools/x3_numerics.py; with bf16 limbs the same scheme measures 4e-4).
// `xf32` is the element-type tag of such an operand in memory (the bytes of a float); its fragment holds the limbs, so a
// fragment is split once when it is loaded and reused by every MFMA it feeds.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
struct xf32 { float v; };
struct xfrag { f16x8 hi, lo; };
template <> struct FragT<xf32> { typedef xfrag type; };
__device__ __forceinline__ xfrag x3_split(const f32x8& x) {
    xfrag r;
    r.hi = __builtin_convertvector(x, f16x8);                    // 4 x v_cvt_pk_f16_f32 (RNE)
    r.lo = __builtin_convertvector(x - __builtin_convertvector(r.hi, f32x8), f16x8);
    return r;
}
template <>
__device__ __forceinline__ xfrag load_frag<xf32>(const xf32* p) {
    return x3_split(*reinterpret_cast<const f32x8*>(p));
}
__device__ __forceinline__ void mma16(f32x4& acc, const xfrag& a, const xfrag& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.lo, b.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.lo, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.hi, b.hi, acc, 0, 0, 0);
}

// `h2`: the same operand already split, in memory.  32 consecutive k of a row take 128 bytes, [32 x fp16 hi | 32 x fp16 lo] — as many
// bytes as the f32 values, so every pitch and offset of an h2 array is the f32 one (an h2* advances 4 bytes per element) and
// the limbs of element k of a 128-byte-aligned 32-block sit at block + 2 (k % 32) and block + 64 + 2 (k % 32).  A fragment (8
// consecutive k) is two 16-byte loads and no arithmetic; producers write the limbs (store4 / store8 / store1 below).  The
// accessors take the ELEMENT address and find the block from its low seven bits, so kernels index h2 arrays exactly like
// float arrays; every h2 array (global or LDS) therefore starts 128-byte aligned and keeps row pitches that are multiples of 32.
struct h2 { unsigned v; };
template <> struct FragT<h2> { typedef xfrag type; };
__device__ __forceinline__ const char* h2_limb(const void* elem) {   // address of the element's hi limb (its lo limb: + 64)
    const uintptr_t a = (uintptr_t)elem;
    return reinterpret_cast<const char*>((a & ~(uintptr_t)127) + ((a & 127) >> 1));
}
template <>
__device__ __forceinline__ xfrag load_frag<h2>(const h2* p) {   // p = element address of the fragment's first k (a multiple of 8)
    const char* b = h2_limb(p);
    xfrag r;
    r.hi = *reinterpret_cast<const f16x8*>(b);
    r.lo = *reinterpret_cast<const f16x8*>(b + 64);
    return r;
}
typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
__device__ __forceinline__ f32x4 load4_f32(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4_f32(const xf32* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 load4_f32(const bf16* p) {
    const bf16x4 v = *reinterpret_cast<const bf16x4*>(p);
    return f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
}
__device__ __forceinline__ f32x4 load4_f32(const h2* p) {   // 4 consecutive elements as f32 (hi + lo: exact)
    const char* b = h2_limb(p);
    const f16x4 hi = *reinterpret_cast<const f16x4*>(b), lo = *reinterpret_cast<const f16x4*>(b + 64);
    return f32x4{(float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1], (float)hi[2] + (float)lo[2], (float)hi[3] + (float)lo[3]};
}

template <typename T> __device__ __forceinline__ T cvt_out(float v);
template <> __device__ __forceinline__ xf32 cvt_out<xf32>(float v) { return xf32{v}; }
template <> __device__ __forceinline__ float cvt_out<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16 cvt_out<bf16>(float v) { return (bf16)v; }  // v_cvt_pk_bf16_f32: RNE, NaN-safe

template <typename T> __device__ __forceinline__ float cvt_in(T v) { return (float)v; }
template <> __device__ __forceinline__ float cvt_in<xf32>(xf32 v) { return v.v; }

// store 4 consecutive outputs
__device__ __forceinline__ void store4(float* p, float a, float b, float c, float d) {
    *reinterpret_cast<f32x4*>(p) = f32x4{a, b, c, d};
}
__device__ __forceinline__ void store4(xf32* p, float a, float b, float c, float d) {
    *reinterpret_cast<f32x4*>(p) = f32x4{a, b, c, d};
}
__device__ __forceinline__ void store4(h2* p, float a, float b, float c, float d) {   // the limbs of 4 consecutive elements: two 8-byte stores
    char* q = const_cast<char*>(h2_limb(p));
    const f32x4 v = {a, b, c, d};
    const f16x4 hi = __builtin_convertvector(v, f16x4);
    const f16x4 lo = __builtin_convertvector(v - __builtin_convertvector(hi, f32x4), f16x4);
    *reinterpret_cast<f16x4*>(q) = hi;
    *reinterpret_cast<f16x4*>(q + 64) = lo;
}
__device__ __forceinline__ void store8(float* p, const f32x8& v) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p + 4) = f32x4{v[4], v[5], v[6], v[7]};
}
// fragment of k-group fg (8 consecutive k) of the 32-deep slab that starts at `slab` — for LDS tiles whose rows are not 128-byte
// aligned (padded pitches), where an h2 block cannot be found from the element address: the slab start is given instead
template <typename T>
__device__ __forceinline__ typename FragT<T>::type slab_frag(const T* slab, int fg) { return load_frag<T>(slab + 8 * fg); }
template <>
__device__ __forceinline__ xfrag slab_frag<h2>(const h2* slab, int fg) {
    const char* b = reinterpret_cast<const char*>(slab) + 16 * fg;
    xfrag r;
    r.hi = *reinterpret_cast<const f16x8*>(b);
    r.lo = *reinterpret_cast<const f16x8*>(b + 64);
    return r;
}
__device__ __forceinline__ void store8(h2* p, const f32x8& v) {   // 8 consecutive elements: two 16-byte stores
    char* q = const_cast<char*>(h2_limb(p));
    const xfrag f = x3_split(v);
    *reinterpret_cast<f16x8*>(q) = f.hi;
    *reinterpret_cast<f16x8*>(q + 64) = f.lo;
}
__device__ __forceinline__ void store1(h2* p, float v) {
    char* q = const_cast<char*>(h2_limb(p));
    const _Float16 hi = (_Float16)v;
    *reinterpret_cast<_Float16*>(q) = hi;
    *reinterpret_cast<_Float16*>(q + 64) = (_Float16)(v - (float)hi);
}
__device__ __forceinline__ void store1(float* p, float v) { *p = v; }
__device__ __forceinline__ void store1(bf16* p, float v) { *p = (bf16)v; }
__device__ __forceinline__ void store4(bf16* p, float a, float b, float c, float d) {
    *reinterpret_cast<bf16x4*>(p) = bf16x4{(bf16)a, (bf16)b, (bf16)c, (bf16)d};
}

// exact (erf) GELU — activation_function "gelu" ([3P] configuration_whisper.py:140)
// erf by Abramowitz & Stegun 7.1.26 (|error| <= 1.5e-7): branch-free, one v_exp + one v_rcp, about half the
// VALU work of libm erff.  The 1e-3 logit budget of the f32 mode is four orders of magnitude above it.
__device__ __forceinline__ float erf_as(float x) {
#pragma clang fp contract(off)   // (only the fmaf calls below fuse: the same bits in every kernel that inlines this)
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float p = fmaf(1.061405429f, t, -1.453152027f);
    p = fmaf(p, t, 1.421413741f);
    p = fmaf(p, t, -0.284496736f);
    p = fmaf(p, t, 0.254829592f);
    const float e = 1.0f - p * t * __expf(-ax * ax);
    return copysignf(e, x);
}
__device__ __forceinline__ float gelu_erf(float x) {
#pragma clang fp contract(off)
    return 0.5f * x * (1.0f + erf_as(x * 0.70710678118654752440f));
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Sum over aligned groups of 8 or 16 consecutive lanes with DPP only (no LDS crossbar, no waits):
// quad_perm[1,0,3,2], quad_perm[2,3,0,1], then row_half_mirror (lane i <-> 7-i pairs the two quads,
// which already hold equal sums), then row_mirror for 16 lanes.  Every lane ends with the group sum.
template <int LANES>
__device__ __forceinline__ float dpp_group_sum(float v) {
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
    v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
    if (LANES >= 8) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
    if (LANES >= 16) v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
    return v;
}

// Full-wave (64-lane) sum / max: DPP inside each 16-lane row, then the four row results through SGPRs
// (v_readlane) — no LDS crossbar (ds_bpermute) round trips.
__device__ __forceinline__ float dpp_wave_sum(float v) {
    v = dpp_group_sum<16>(v);
    return (__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)) +
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16))) +
           (__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)) +
            __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48)));
}
__device__ __forceinline__ float dpp_max16(float v) {
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true)));
    v = fmaxf(v, __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true)));
    return v;
}
__device__ __forceinline__ float dpp_wave_max(float v) {
    v = dpp_max16(v);
    return fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0)),
                       __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16))),
                 fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32)),
                       __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48))));
}

// All-reduce over the four 16-lane rows of a wave (lanes l, l^16, l^32, l^48) without the LDS crossbar:
// v_permlane16_swap (x, x) -> {[r0 r0 r2 r2], [r1 r1 r3 r3]}, v_permlane32_swap (x, x) -> {[r0 r1 r0 r1], [r2 r3 r2 r3]}
// (gfx950; semantics checked in tools/permlane_check.hip).  `__shfl_xor(v, 16)` lowers to ds_bpermute + a wait.
typedef __attribute__((ext_vector_type(2))) unsigned wh_u32x2;
__device__ __forceinline__ float xrow_max(float v) {
    wh_u32x2 t = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = fmaxf(__uint_as_float(t.x), __uint_as_float(t.y));
    t = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return fmaxf(__uint_as_float(t.x), __uint_as_float(t.y));
}
__device__ __forceinline__ float xrow_sum(float v) {
    wh_u32x2 t = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    v = __uint_as_float(t.x) + __uint_as_float(t.y);
    t = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(t.x) + __uint_as_float(t.y);
}
// (value, index) argmax the same way: every lane ends with the largest value of its four rows and that value's index, the lowest
// index on ties (the LM heads' reduction over the four lane groups that share a row of the MFMA result)
__device__ __forceinline__ void xrow_argmax(float& bv, int& bi) {
    wh_u32x2 tv = __builtin_amdgcn_permlane16_swap(__float_as_uint(bv), __float_as_uint(bv), false, false);
    wh_u32x2 ti = __builtin_amdgcn_permlane16_swap((unsigned)bi, (unsigned)bi, false, false);
    float v0 = __uint_as_float(tv.x), v1 = __uint_as_float(tv.y);
    int i0 = (int)ti.x, i1 = (int)ti.y;
    bool take1 = v1 > v0 || (v1 == v0 && i1 < i0);
    bv = take1 ? v1 : v0;
    bi = take1 ? i1 : i0;
    tv = __builtin_amdgcn_permlane32_swap(__float_as_uint(bv), __float_as_uint(bv), false, false);
    ti = __builtin_amdgcn_permlane32_swap((unsigned)bi, (unsigned)bi, false, false);
    v0 = __uint_as_float(tv.x); v1 = __uint_as_float(tv.y);
    i0 = (int)ti.x; i1 = (int)ti.y;
    take1 = v1 > v0 || (v1 == v0 && i1 < i0);
    bv = take1 ? v1 : v0;
    bi = take1 ? i1 : i0;
}

typedef __attribute__((ext_vector_type(4))) unsigned wh_u32x4;
// NOTE: hipcc (ROCm 7.2) miscompiles __builtin_bit_cast(bf16x2, <element of a uint vector>) — every
// element resolves to element 0.  Going through memcpy produces the intended register moves.
__device__ __forceinline__ bf16x2 as_bf16x2(unsigned u) { bf16x2 r; __builtin_memcpy(&r, &u, 4); return r; }
template <typename V> __device__ __forceinline__ wh_u32x4 as_u32x4(const V& v) { wh_u32x4 r; __builtin_memcpy(&r, &v, 16); return r; }
// dot product of 8 packed bf16 pairs (two 16-byte chunks) accumulated into t: 4 x v_dot2c_f32_bf16
__device__ __forceinline__ float dot8_bf16(wh_u32x4 a, wh_u32x4 b, float t) {
    t = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(a.x), as_bf16x2(b.x), t, false);
    t = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(a.y), as_bf16x2(b.y), t, false);
    t = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(a.z), as_bf16x2(b.z), t, false);
    t = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(a.w), as_bf16x2(b.w), t, false);
    return t;
}
// o0, o1 += p0 * va.{lo,hi} + p1 * vb.{lo,hi} for one packed dword of two keys
__device__ __forceinline__ void pv2_bf16(unsigned va, unsigned vb, bf16x2 pp, float& o0, float& o1) {
    const unsigned lo = __builtin_amdgcn_perm(vb, va, 0x05040100u);  // (va.lo, vb.lo)
    const unsigned hi = __builtin_amdgcn_perm(vb, va, 0x07060302u);  // (va.hi, vb.hi)
    o0 = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(lo), pp, o0, false);
    o1 = __builtin_amdgcn_fdot2_f32_bf16(as_bf16x2(hi), pp, o1, false);
}

// order-preserving float <-> uint map for atomicMax on floats of either sign
__device__ __forceinline__ unsigned f2ord(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __host__ __forceinline__ float ord2f(unsigned u) {
    unsigned v = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
#ifdef __HIP_DEVICE_COMPILE__
    return __uint_as_float(v);
#else
    float f;
    __builtin_memcpy(&f, &v, 4);
    return f;
#endif
}

// Sum of the LayerNorm partials {sum x, sum x^2} of row `row` over tiles q, q + step, q + 2 step, ... < n_tiles,
// eight 8-byte loads in flight at a time (clamped re-reads are masked): a run-time loop with one load per
// iteration costs one memory round trip per tile.
__device__ __forceinline__ void ln_partial_sum(const float* __restrict__ part, int n_tiles, int x_mpad, int row, int q, int step,
                                               float& s1, float& s2) {
    typedef __attribute__((ext_vector_type(2))) float f32x2;
    s1 = 0.0f;
    s2 = 0.0f;
    for (int t0 = q; t0 < n_tiles; t0 += 8 * step) {
        f32x2 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int tl = min(t0 + u * step, n_tiles - 1);
            v[u] = *reinterpret_cast<const f32x2*>(part + ((long)tl * x_mpad + row) * 2);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const bool ok = t0 + u * step < n_tiles;
            s1 += ok ? v[u].x : 0.0f;
            s2 += ok ? v[u].y : 0.0f;
        }
    }
}

// Epilogue arithmetic of kernels that must agree BIT FOR BIT whichever of them computes a row (k_dec_gemm / k_dec_gemm_wide,
// k_lm_head / k_lm_head_tile: the choice follows the batch, a clip's result must not): explicit, un-contracted operations, so
// the value does not depend on how the compiler happens to fuse multiplies and adds in each kernel (moving a load in
// k_dec_gemm_wide once changed an fma choice and with it a token of the fp8 path).
__device__ __forceinline__ float wh_ln_fold(float acc, float mean, float rstd, float s, float c) {   // rstd (acc - mean s) + c
#pragma clang fp contract(off)
    const float p = mean * s;
    const float t = acc - p;
    const float u = rstd * t;
    return u + c;
}
// {mean, rstd} of a row from its {sum x, sum x^2}: biased variance, eps 1e-5 (torch LayerNorm)
__device__ __forceinline__ void wh_ln_mean_rstd(float s1, float s2, float inv_or_k, bool is_inv, float& mean, float& rstd) {
#pragma clang fp contract(off)
    mean = is_inv ? s1 * inv_or_k : s1 / inv_or_k;
    const float ex2 = is_inv ? s2 * inv_or_k : s2 / inv_or_k;
    const float var = ex2 - mean * mean;
    rstd = rsqrtf(fmaxf(var, 0.0f) + 1e-5f);
}

// {mean, rstd} of a row from the partials that ln_partial_sum reads, in the ONE term order that every kernel whose results must agree bit for
// bit uses (k_dec_gemm / k_dec_gemm_wide; k_lm_head / k_lang_head / the LM-head tile kernels): thread (row r, quarter q) sums every 4th tile
// with ln_partial_sum and leaves its pair in LDS, lnq [4][rows][2]; behind a barrier the quarters of a row are added as (q0 + q1) + (q2 + q3)
// and wh_ln_mean_rstd finishes over the row's k columns.  (k_dec_tile adds two halves — a different sum, whose results are that kernel's own.)
// The shape is deliberate: the row count is a template parameter, each sum is one expression and k arrives as an int, because with a
// run-time row count, a sum built in two statements or the conversion of k at the call site the callers' instruction streams changed.
template <int rows>
__device__ __forceinline__ void ln_part_store(float* lnq, int r, int q, float s1, float s2) {
    lnq[(q * rows + r) * 2] = s1;
    lnq[(q * rows + r) * 2 + 1] = s2;
}
template <int rows>
__device__ __forceinline__ void ln_row_stats(const float* lnq, int r, int k, float& mean, float& rstd) {
    const float s1 = (lnq[r * 2] + lnq[(rows + r) * 2]) + (lnq[(2 * rows + r) * 2] + lnq[(3 * rows + r) * 2]);
    const float s2 = (lnq[r * 2 + 1] + lnq[(rows + r) * 2 + 1]) + (lnq[(2 * rows + r) * 2 + 1] + lnq[(3 * rows + r) * 2 + 1]);
    wh_ln_mean_rstd(s1, s2, (float)k, false, mean, rstd);
}
__device__ __forceinline__ float wh_scale(float acc, float ws) {   // acc * ws (fp8 weights: the channel scale; exact for ws = 1)
#pragma clang fp contract(off)
    return acc * ws;
}
__device__ __forceinline__ float wh_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float wh_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// ---- Whisper's timestamp rules in the LM head's epilogue (the RULES variants) --------------------------------------------
// Row m of a position may emit text in [text_lo, tb) and timestamps in [ts_lo, ts_hi].  At the first generated position (gen == 0) the ranges
// are rule 4's; later ones come from the row state k_argmax_finish<T, true> wrote ({text_lo, ts_lo, ts_hi, last timestamp} per row).
__device__ __forceinline__ void ts_ranges(const int* state, int m, int gen, int tb, int max_init, int N, int& text_lo, int& ts_lo, int& ts_hi) {
    if (gen == 0) {
        text_lo = tb;
        ts_lo = tb;
        ts_hi = (max_init >= 0 && max_init < N - 1 - tb) ? tb + max_init : N - 1;   // (no tb + max_init overflow)
    } else {
        text_lo = state[4 * m];
        ts_lo = state[4 * m + 1];
        ts_hi = state[4 * m + 2];
    }
}
// The ranges of the NEXT position from the history it will see (rules 2 and 3): `next` = the token fed next (seq[-1]), pen_ts = seq[-2] is a
// timestamp or does not exist, prev_last_t = the last timestamp before `next` (-1: none).  Shared by k_argmax_finish<T, true> and k_beam_select.
__device__ __forceinline__ void ts_next_state(int next, bool pen_ts, int prev_last_t, int tb, int eot, int vocab, int& text_lo, int& ts_lo, int& ts_hi,
                                              int& last_t) {
    const bool last_ts = next >= tb;
    last_t = last_ts ? next : prev_last_t;
    text_lo = 0;
    ts_lo = tb;
    if (last_ts && pen_ts) ts_lo = vocab;          // after a pair: no timestamp
    else if (last_ts) text_lo = eot;               // after a single one: no text id below EOT
    if (last_t >= 0 && ts_lo < vocab) ts_lo = max(ts_lo, (last_ts && !pen_ts) ? last_t : last_t + 1);
    ts_hi = vocab - 1;
}
// exp(x) for x <= 0 as one v_exp_f32 (2^(x log2 e)): relative error ~1e-6 over the range that matters to a log-sum-exp
__device__ __forceinline__ float ts_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.44269504088896341f); }
// online (max, sum of exp(v - max), index of the max) over the allowed timestamp logits, columns ascending: strict >, so the lowest index keeps
// a tie; NaN is neither the max nor part of the sum
__device__ __forceinline__ void ts_acc(float v, int n, float& tm, float& ts, int& ti) {
    if (v > tm) { ts = ts * ts_exp(tm - v) + 1.0f; tm = v; ti = n; }
    else if (v > -INFINITY) ts += ts_exp(v - tm);
}
__device__ __forceinline__ void ts_merge(float& tm, float& ts, int& ti, float m1, float s1, int i1) {
    const float mx = fmaxf(tm, m1);
    const float s = mx == -INFINITY ? 0.0f : ts * ts_exp(tm - mx) + s1 * ts_exp(m1 - mx);
    if (m1 > tm || (m1 == tm && i1 < ti)) ti = i1;
    tm = mx;
    ts = s;
}
// one logit of the rules epilogue: the text argmax below tb inside [text_lo, tb); a timestamp goes to the row's timestamp logits, -inf where
// suppressed or outside [ts_lo, ts_hi] (k_argmax_finish<T, true> reduces them: one predicated store here instead of an online sum of exp,
// which spilled k_lm_head_tile's accumulators)
__device__ __forceinline__ void ts_take(float v, int n, bool sup, int tb, int text_lo, int ts_lo, int ts_hi, float& bv, int& bi, float* ts_row) {
    if (n < tb) {
        if (!sup && n >= text_lo && v > bv) { bv = v; bi = n; }
    } else {
        ts_row[n - tb] = (!sup && n >= ts_lo && n <= ts_hi) ? v : -INFINITY;
    }
}

// ---- token log-probabilities in the LM head's epilogue (the LP variants) --------------------------------------------------
// The recorded token is the argmax of the allowed ids, so its log-probability is -log(sum of exp(v - max)) over them: the kernels carry a
// (max, sum) pair wherever they carry a (max, index) pair.  NaN and -inf logits add nothing, as they never win the argmax.
// online form, one logit: (m, s) is the running pair; m itself is moved by the caller's argmax (same condition: v > m)
__device__ __forceinline__ void lp_acc(float v, float m, float& s) {
    if (v > m) s = s * ts_exp(m - v) + 1.0f;
    else if (v > -INFINITY) s += ts_exp(v - m);
}
// a sum relative to the maximum m moved to the maximum mx >= m
__device__ __forceinline__ float lp_rescale(float s, float m, float mx) { return m == -INFINITY ? 0.0f : s * ts_exp(m - mx); }
// (m, s) += (m1, s1); m is left to the caller's argmax merge
__device__ __forceinline__ float lp_merge(float m, float s, float m1, float s1) {
    const float mx = fmaxf(m, m1);
    return lp_rescale(s, m, mx) + lp_rescale(s1, m1, mx);
}
// second pass over one row of a tile kernel's accumulators (still live after the argmax): the sum of exp(v - bv) over this lane's columns
// that are not suppressed and lie in [lo, hi), bv = the row's maximum over exactly those columns.  Branch-free: one v_exp_f32 and a select per
// logit.  The column tests do not depend on the row; left to themselves they are hoisted out of the caller's unrolled row loop as sixteen
// live lane masks (scalar-register spills), so the lane's first column and mask words pass through an empty asm per row and are tested again.
// PROBE: the logit of column probe_id, if it is one of this lane's, goes to *probe.
template <int TN, bool PROBE>
__device__ __forceinline__ float lp_tile_row(const f32x4 (&acc)[TN], bool ln, float mean, float rstd, const float (&sv)[TN][4], const float (&cv)[TN][4],
                                             const unsigned (&mbits)[TN], int n_first, int lo, int hi, float bv, int probe_id, float* probe) {
    float s = 0.0f, pv = 0.0f;
    asm volatile("" : "+v"(n_first));
#pragma unroll
    for (int j = 0; j < TN; j++) {
        unsigned mb = mbits[j];
        asm volatile("" : "+v"(mb));
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int nn = n_first + j * 16 + e;
            const float v = ln ? wh_ln_fold(acc[j][e], mean, rstd, sv[j][e], cv[j][e]) : acc[j][e];
            if constexpr (PROBE) pv = (nn == probe_id) ? v : pv;
            const bool ok = !((mb >> e) & 1u) && nn >= lo && nn < hi && v > -INFINITY;   // (NaN: not greater)
            s += ok ? ts_exp(v - bv) : 0.0f;
        }
    }
    if constexpr (PROBE) {
        const int rel = probe_id - n_first;
        if (rel >= 0 && rel < TN * 16 && (rel & 15) < 4) *probe = pv;
    }
    return s;
}

#define WH_HIP_CHECK(expr)                                                                     \
    do {                                                                                        \
        hipError_t _e = (expr);                                                                 \
        if (_e != hipSuccess) return wh_fail_hip(_e, #expr, __FILE__, __LINE__);                \
    } while (0)

int wh_fail_hip(hipError_t e, const char* what, const char* file, int line);
// Dynamic-LDS opt-in above the 64 KB default, once per (current device, kernel, size): hipFuncSetAttribute applies to the
// device that is current when it is called, so a process that opens several devices needs it on each.  A failure is
// recorded through wh_set_error (the launch that follows then fails and surfaces at the call's hipGetLastError).
bool wh_ensure_dyn_lds(const void* kernel, size_t bytes);
// raise a kernel's dynamic-LDS limit once per (device, kernel, size)
template <typename K>
void set_max_smem(K kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return;
    wh_ensure_dyn_lds((const void*)kernel, bytes);
}
void wh_set_error(const char* fmt, ...);

// Runtime choices -> template arguments, for the launchers of kernels with variant flags.
// wh_with_flags(f, b0, b1, ...) calls the generic lambda f with one std::bool_constant per flag, in order:
//   wh_with_flags([&](auto R, auto L) { launch(k<decltype(R)::value, decltype(L)::value>); }, rules, lp);
// Every combination is instantiated; one more flag is one more argument.
template <typename F>
void wh_with_flags(F&& f) { f(); }
template <typename F, typename... Bs>
void wh_with_flags(F&& f, bool b, Bs... rest) {
    if (b) wh_with_flags([&](auto... cs) { f(std::true_type{}, cs...); }, rest...);
    else wh_with_flags([&](auto... cs) { f(std::false_type{}, cs...); }, rest...);
}
// the element type of a precision mode's operands where it is {WH_PREC_F32: float, WH_PREC_F16X3: h2, else bf16}: f(wh_type_tag<T>{})
template <typename T> struct wh_type_tag { typedef T type; };
template <typename F>
void wh_with_dtype(int prec, F&& f) {
    if (prec == WH_PREC_F32) f(wh_type_tag<float>{});
    else if (prec == WH_PREC_F16X3) f(wh_type_tag<h2>{});
    else f(wh_type_tag<bf16>{});
}
// the smallest power of two in [LO, HI] that is >= n as an std::integral_constant (anything above HI counts as HI)
template <int LO, int HI, typename F>
void wh_with_pow2(int n, F&& f) {
    if constexpr (LO < HI) {
        if (n > LO) return wh_with_pow2<2 * LO, HI>(n, f);
    }
    f(std::integral_constant<int, LO>{});
}
// 1 .. 4 as an std::integral_constant (the LM heads' row groups per workgroup; anything above 4 counts as 4)
template <typename F>
void wh_with_1to4(int n, F&& f) {
    switch (n) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}
