// wh_dec_gemm.hip — per-token decoder kernels for gfx950: the body of the with-past loop of
// greedy_decode_with_past (reference src/main.rs:793-826) for a BATCH of independent clips.
// This file holds the decode GEMMs; the header describes the whole step (the other files: its last paragraph).
//
// The reference runs decoder_with_past_model.onnx once per token per clip through ORT's IoBinding
// and re-binds 4*Ld past tensors every step (src/main.rs:798-812).  Here the KV past is an
// on-device cache with an append position, the token loop never leaves the device (masked argmax,
// EOT bookkeeping and the next input token are computed by kernels), and up to 64 clips advance
// together so each weight byte streamed from HBM serves all of them.
//
// Launch structure per decoder layer (8 kernels):
//   [LN1 + QKV]  [self-attn]  [out-proj + residual]  [LN2 + cross-Q]  [cross-attn + merge]
//   [cross out-proj + residual]  [LN3 + fc1 + GELU]  [fc2 + residual]
// plus per position [final LN + LM head + masked argmax partials] [argmax finish].  LayerNorm and
// the token/position embedding run in the prologue of the GEMM that consumes them (activations
// staged in LDS as MFMA operands, weight fragments already in flight), the key-range merge of the
// cross-attention runs in the last workgroup of each clip, and the position counter is advanced by
// the last workgroup of the last kernel of a step.
//
// Every kernel reads the current position from device memory (*pos), never from a kernel argument,
// so one captured hipGraph of a step can be replayed for every step.
//
// [3P] decoder definition: modeling_whisper.py WhisperDecoderLayer.forward (:466-500), learned
// positions offset by the past length (:208-212), final LN (:790), tied LM head, no bias (:965,970).
//
// The kernels of a step live in three files: the decode GEMMs here (k_dec_gemm, k_dec_gemm_wide), the end of a position in
// wh_lm_head.hip (embedding, LM head, finish and language kernels) and the attention in wh_dec_attn.hip.
#include <stdlib.h>

#include "wh_common.h"
#include "wh_dec_epilogue.h"
#include "wh_kernels.h"

#include <algorithm>

// tuning knobs (tools/microbench.cpp flips them; product code leaves the defaults)
int wh_dbg_mt = 0;
int wh_dbg_nw = 0;   // 4 / 8: force the K split of the decode GEMM (0 = heuristic)
int wh_dbg_wide = -1;  // column tiles per workgroup at > 256 rows: -1 heuristic, 0 off (k_dec_gemm only), 2 / 4 forced

namespace {

// (advance_if_last, the position ticket, and slab_idx, the k-slab-major activation layout: wh_dec_epilogue.h)

// ---- decode GEMM: C[m][n] = act(sum_k X[m][k] W[n][k] + bias[n]) (+ R[m][n]),  M <= 64 per row group
// Weight-streaming: every weight element is read once per launch straight into MFMA fragments (up
// to 8 per wave in flight before the first MFMA); activations are read as MFMA column operands from
// the slab layout.  The waves of a workgroup split K (4 or 8 ways) and reduce through LDS; wave w
// then finishes row-tile w (bias, erf-GELU, f32 residual; output row-major or slab).
// Merge of split attention partials (one row, 4 consecutive columns per item), in two phases so that the
// caller can put every load of several items in flight before any arithmetic.  SP = compile-time bound on
// the number of key ranges (everything unrolled, selects instead of branches: a branch would end the basic
// block and serialise the memory round trips).
template <int SP>
struct PartRaw {
    float mv[SP], lv[SP];
    f32x4 p[SP];
};
template <int SP>
__device__ __forceinline__ void partials_load(const SkinnyArgs& a, int m, int k, PartRaw<SP>& r) {
    const int h = k / WH_HEAD_DIM, hs = a.x_heads * 2;
    const float* mb = a.xml + (long)m * a.x_splits * hs + h;
    const float* pb = a.xpart + (long)m * a.x_splits * a.K + k;
#pragma unroll
    for (int s2 = 0; s2 < SP; s2++) {
        const int sc = s2 < a.x_splits ? s2 : 0;  // clamped re-read, weight forced to 0 in partials_merge
        r.mv[s2] = mb[sc * hs];
        r.lv[s2] = mb[sc * hs + a.x_heads];
        r.p[s2] = *reinterpret_cast<const f32x4*>(pb + (long)sc * a.K);
    }
}
template <int SP>
__device__ __forceinline__ f32x4 partials_merge(const SkinnyArgs& a, PartRaw<SP>& r, bool live) {
    float M = -INFINITY;
#pragma unroll
    for (int s2 = 0; s2 < SP; s2++) {
        r.mv[s2] = (s2 < a.x_splits) ? r.mv[s2] : -INFINITY;
        M = fmaxf(M, r.mv[s2]);
    }
    M = (M == -INFINITY) ? 0.0f : M;  // every range empty: exp(-inf - 0) = 0 below, never inf - inf
    f32x4 acc = {0, 0, 0, 0};
    float den = 0.0f;
#pragma unroll
    for (int s2 = 0; s2 < SP; s2++) {
        const float w = __builtin_amdgcn_exp2f((r.mv[s2] - M) * 1.44269504088896341f);  // empty key range: m = -inf, weight 0
        den += w * r.lv[s2];
#pragma unroll
        for (int e = 0; e < 4; e++) acc[e] += w * r.p[s2][e];
    }
    const float inv = live ? __builtin_amdgcn_rcpf(den) : 0.0f;
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e] *= inv;
    return acc;
}

// Weight operand of one k-step.  Native dtype: 8 consecutive k per lane (one MFMA per load).  e4m3 codes: 8 per lane
// (fp8x8_t, one MFMA) or 16 per lane (fp8x16_t: one 16-byte load feeds two MFMAs — half the load instructions for
// the same bytes); codes are dequantised in registers with v_cvt_scalef32_pk_bf16_fp8 (byte j of the dword is
// element j, exact: tools/fp8_check.hip).  A k-step covers 4 * KW k-values; within it lane group fg holds
// k = fg*KW .. fg*KW+KW-1, sub-fragment j the eight starting at 8j — the activation operand follows the same map.
struct fp8x8_t { unsigned char v; };
struct fp8x16_t { unsigned char v; };
template <typename T, typename TW> struct WTraits { static constexpr int KW = 8; };
template <> struct WTraits<bf16, fp8x16_t> { static constexpr int KW = 16; };

__device__ __forceinline__ bf16x8 cvt8_e4m3_bf16(unsigned lo, unsigned hi) {
    const bf16x2 a = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, false), b = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(lo, 1.0f, true);
    const bf16x2 c = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, false), d = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(hi, 1.0f, true);
    return bf16x8{a.x, a.y, b.x, b.y, c.x, c.y, d.x, d.y};
}
template <typename T, typename TW>
__device__ __forceinline__ void load_wfrags(const TW* p, typename FragT<T>::type (&out)[WTraits<T, TW>::KW / 8]) {
    if constexpr (sizeof(TW) == sizeof(T)) {
        out[0] = load_frag<T>(reinterpret_cast<const T*>(p));
    } else if constexpr (WTraits<T, TW>::KW == 8) {
        typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
        const u32x2 u = *reinterpret_cast<const u32x2*>(p);
        out[0] = cvt8_e4m3_bf16(u.x, u.y);
    } else {
        const wh_u32x4 u = *reinterpret_cast<const wh_u32x4*>(p);
        out[0] = cvt8_e4m3_bf16(u.x, u.y);
        out[1] = cvt8_e4m3_bf16(u.z, u.w);
    }
}

template <typename T, typename TO, int MT, int NW, int XP, typename TW = T>  // XP > 0: X from XP-bounded attention partials
__global__ __launch_bounds__(NW * 64) void k_dec_gemm(SkinnyArgs a) {
    extern __shared__ __attribute__((aligned(128))) char smem_raw[];   // 128: h2 tiles find their 32-blocks from the address
    dec_gemm_group<T, TO, TW>(a);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fl = lane & 15, fg = lane >> 4;
    const int n0 = blockIdx.x * 16;
    const int m0 = blockIdx.y * MT * 16;  // first row of this workgroup's row group
    int nrow = n0 + fl;
    if (nrow > a.N - 1) nrow = a.N - 1;
    constexpr int KW = WTraits<T, TW>::KW, SUB = KW / 8, KSTEP = 4 * KW;  // k-values per lane / MFMAs / k-values per step
    const int kspan = a.K / NW, kb = wave * kspan, iters = kspan / KSTEP;
    const TW* wp = (const TW*)a.W + (long)nrow * a.K + kb + fg * KW;
    // activation operand of (step i, sub-fragment j): slab (kb + i*KSTEP + fg*KW) / 32, offset (fg*KW) % 32 + 8j
    const long xstep = (long)a.x_mpad * 32 * (KSTEP / 32);
    const T* xp = XP > 0 ? nullptr : (const T*)a.X + ((long)((kb + fg * KW) >> 5) * a.x_mpad + m0 + fl) * 32 + ((fg * KW) & 31);
    // k-steps in flight per wave: 8 for 16-byte fragments; 32-byte ones (f32, fp16 limbs) keep the register budget of MT = 1
    // (8 x (1 + MT) fragments would spill from MT = 2 on: 1,074 spilled registers at MT = 4 before this rule)
    constexpr int FRB = (int)sizeof(typename FragT<T>::type);
    constexpr int DEPTH = FRB <= 16 ? 8 / SUB : (MT == 1 ? 8 : MT == 2 ? 4 : 2);
    typename FragT<T>::type wq[DEPTH][SUB], xq[DEPTH][SUB][MT];
#pragma unroll
    for (int i = 0; i < DEPTH; i++)
        if (i < iters) {
            load_wfrags<T, TW>(wp + i * KSTEP, wq[i]);
            if constexpr (XP == 0) {
#pragma unroll
                for (int j = 0; j < SUB; j++)
#pragma unroll
                    for (int t = 0; t < MT; t++) xq[i][j][t] = load_frag<T>(xp + i * xstep + t * 512 + 8 * j);
            }
        }
    // epilogue operands (wave w finishes row-tile w): fetched now, used last
    f32x4 pre_bias = {0, 0, 0, 0}, pre_r = {0, 0, 0, 0}, pre_ws = {1, 1, 1, 1}, pre_g = {1, 1, 1, 1};
    float pre_sh = 0.0f;   // the row's running offset (producers: SkinnyArgs::row_shift)
    const int en = n0 + 4 * fg, em = m0 + wave * 16 + fl;
    const bool ep_ok = wave < MT && en < a.N && em < a.M;
    if (ep_ok) {
        if (a.bias) pre_bias = *reinterpret_cast<const f32x4*>(a.bias + en);
        if (a.wscale) pre_ws = *reinterpret_cast<const f32x4*>(a.wscale + en);
        if (a.xgamma) pre_g = *reinterpret_cast<const f32x4*>(a.xgamma + en);
        if (a.R) pre_r = *reinterpret_cast<const f32x4*>(a.R + (long)em * a.ldr + en);
        if (a.row_shift) pre_sh = a.row_shift[em];
    }
    // LayerNorm folded in: reduce the producer's per-tile partial sums of this row group to mean / rstd
    // (while the weight and activation fragments above are in flight)
    typedef DecGemmLds<NW, MT, MT> Lds;
    float* lnred = Lds::lnq(smem_raw);
    float ln_mean = 0.0f, ln_rstd = 1.0f, ln_sv[4] = {0, 0, 0, 0};
    if (a.ln_part) {
        constexpr int ROWS = MT * 16;
        if (tid < 4 * ROWS) {
            const int r = tid % ROWS, q = tid / ROWS;
            float s1, s2;
            ln_partial_sum(a.ln_part, a.ln_tiles, a.x_mpad, m0 + r, q, 4, s1, s2);
            ln_part_store<ROWS>(lnred, r, q, s1, s2);
        }
        __syncthreads();
        if (ep_ok) {
            ln_row_stats<ROWS>(lnred, wave * 16 + fl, a.K, ln_mean, ln_rstd);
            const f32x4 sv = *reinterpret_cast<const f32x4*>(a.ln_s + en);
            ln_sv[0] = sv[0]; ln_sv[1] = sv[1]; ln_sv[2] = sv[2]; ln_sv[3] = sv[3];
        }
    }
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0, 0, 0, 0};
    if constexpr (XP > 0) {
        // X = merge of the key ranges' partials, built once per workgroup in LDS (slab layout [K/32][16][32]) with
        // row-contiguous 16-byte loads; the weight fragments above are in flight meanwhile (iters <= DEPTH here)
        static_assert(MT == 1, "merged-X variant runs 16-row groups");
        T* Xs = reinterpret_cast<T*>(smem_raw + Lds::BYTES);
        constexpr int NT = NW * 64, IF = XP <= 4 ? 4 : (XP <= 8 ? 2 : 1);    // items in flight per thread
        // 4-column chunks per row; only live rows are merged (a dead row of X feeds only its own, never stored,
        // output column of the MFMA tile)
        const int cpr = a.K >> 2, items = min(16, a.M - m0) * cpr;
        for (int it0 = tid; it0 < items; it0 += NT * IF) {
            PartRaw<XP> raw[IF];
            int row[IF], ch[IF];
            bool live[IF];
#pragma unroll
            for (int u = 0; u < IF; u++) {
                const int item = min(it0 + u * NT, items - 1);
                row[u] = item / cpr;
                ch[u] = item - row[u] * cpr;
                live[u] = it0 + u * NT < items;
                partials_load<XP>(a, m0 + row[u], ch[u] * 4, raw[u]);
            }
            __builtin_amdgcn_sched_barrier(0);  // all loads above, all arithmetic below
#pragma unroll
            for (int u = 0; u < IF; u++) {
                const f32x4 v = partials_merge<XP>(a, raw[u], live[u]);
                const int k = ch[u] * 4;
                if (live[u]) store4(Xs + ((long)(k >> 5) * 16 + row[u]) * 32 + (k & 31), v[0], v[1], v[2], v[3]);
            }
        }
        __syncthreads();
        const T* xl = Xs + ((long)((kb + fg * KW) >> 5) * 16 + fl) * 32 + ((fg * KW) & 31);
        constexpr int lstep = 512 * (KSTEP / 32);
#pragma unroll
        for (int i = 0; i < DEPTH; i++)
            if (i < iters) {
#pragma unroll
                for (int j = 0; j < SUB; j++) mma16(acc[0], wq[i][j], load_frag<T>(xl + i * lstep + 8 * j));
            }
        for (int i = DEPTH; i < iters; i++) {  // deep K tail
            typename FragT<T>::type wt[SUB];
            load_wfrags<T, TW>(wp + i * KSTEP, wt);
#pragma unroll
            for (int j = 0; j < SUB; j++) mma16(acc[0], wt[j], load_frag<T>(xl + i * lstep + 8 * j));
        }
    } else
    for (int c0 = 0; c0 < iters; c0 += DEPTH) {
        if (c0 > 0) {
#pragma unroll
            for (int i = 0; i < DEPTH; i++)
                if (c0 + i < iters) {
                    load_wfrags<T, TW>(wp + (c0 + i) * KSTEP, wq[i]);
#pragma unroll
                    for (int j = 0; j < SUB; j++)
#pragma unroll
                        for (int t = 0; t < MT; t++) xq[i][j][t] = load_frag<T>(xp + (c0 + i) * xstep + t * 512 + 8 * j);
                }
        }
#pragma unroll
        for (int i = 0; i < DEPTH; i++)
            if (c0 + i < iters) {
#pragma unroll
                for (int j = 0; j < SUB; j++)
#pragma unroll
                    for (int t = 0; t < MT; t++) mma16(acc[t], wq[i][j], xq[i][j][t]);  // D rows = n (4*fg + r), col = m (fl)
            }
    }
    f32x4* red = Lds::red(smem_raw);
#pragma unroll
    for (int t = 0; t < MT; t++) red[(wave * MT + t) * 64 + lane] = acc[t];
    __syncthreads();
    if (ep_ok) {
        f32x4 s = red[(0 * MT + wave) * 64 + lane];
#pragma unroll
        for (int w = 1; w < NW; w++) {
            f32x4 o = red[(w * MT + wave) * 64 + lane];
            s[0] += o[0]; s[1] += o[1]; s[2] += o[2]; s[3] += o[3];
        }
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; e++) {
            s[e] = wh_scale(s[e], pre_ws[e]);  // fp8 weights: the channel scale (1 otherwise)
            v[e] = a.ln_part ? wh_ln_fold(s[e], ln_mean, ln_rstd, ln_sv[e], pre_bias[e]) : wh_add(s[e], pre_bias[e]);
            if (a.act == 1) v[e] = gelu_erf(v[e]);
            v[e] += pre_r[e];
        }
        // a slab output is another GEMM's operand: the compute type T (== TO wherever both are 2-byte); row-major outputs are TO
        if (a.c_mpad) store4((T*)a.C + slab_idx(em, en, a.c_mpad), v[0], v[1], v[2], v[3]);
        else store4((TO*)a.C + (long)em * a.ldc + en, v[0], v[1], v[2], v[3]);
        if (a.xslab_out) store4((T*)a.xslab_out + slab_idx(em, en, a.x_mpad), wh_sub(v[0], pre_sh) * pre_g[0], wh_sub(v[1], pre_sh) * pre_g[1],
                                wh_sub(v[2], pre_sh) * pre_g[2], wh_sub(v[3], pre_sh) * pre_g[3]);
        // the one consumer of a LayerNorm keeps the rows' running offsets up to date (first column tile only)
        if (a.shift_io && blockIdx.x == 0 && blockIdx.z == 0 && fg == 0) a.shift_io[em] += ln_mean;
    }
    if (a.stats_out && wave < MT) {
        // this column tile's {sum x, sum x^2} per row: 4 values per lane, then the 4 lane groups of the row
        float s1 = 0.0f, s2 = 0.0f;
        if (ep_ok) {
            f32x4 s = red[(0 * MT + wave) * 64 + lane];
#pragma unroll
            for (int w = 1; w < NW; w++) {
                f32x4 o = red[(w * MT + wave) * 64 + lane];
                s[0] += o[0]; s[1] += o[1]; s[2] += o[2]; s[3] += o[3];
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float v = wh_sub(wh_add(wh_add(wh_scale(s[e], pre_ws[e]), pre_bias[e]), pre_r[e]), pre_sh);  // producers have no activation
                s1 += v;
                s2 = __builtin_fmaf(v, v, s2);   // explicit: the same bits in k_dec_gemm and k_dec_gemm_wide
            }
        }
        s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
        s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
        if (fg == 0 && em < a.M) {
            a.stats_out[((long)blockIdx.x * a.x_mpad + em) * 2] = s1;
            a.stats_out[((long)blockIdx.x * a.x_mpad + em) * 2 + 1] = s2;
        }
    }
    advance_if_last(a.ticket, a.pos_w, gridDim.x * gridDim.y);
}

// Batches of hundreds of rows: a workgroup owns NT 16-column tiles x MT 16-row tiles, so every activation fragment a wave
// loads feeds NT MFMAs and every weight fragment MT (k_dec_gemm at NT = 1 pulls the activations through L2 once per 16
// output columns: 123 MB for the 1536 x 512 QKV projection at 1024 rows, 49 MB here).  Same K split over the waves, same
// k order inside a wave and the same order of the cross-wave sum as k_dec_gemm: an output element is bit-identical
// whichever of the two computes it, so the choice may follow the batch.  Wave w finishes tiles w, w + NW, ...
// (tile id = nt * MT + mt).  No merged-X (attention partials) variant: large batches run one key range per clip.
template <typename T, typename TO, int MT, int NT, int NW, typename TW = T>
__global__ __launch_bounds__(NW * 64, 2) void k_dec_gemm_wide(SkinnyArgs a) {
    extern __shared__ __attribute__((aligned(128))) char smem_raw[];   // 128: h2 tiles find their 32-blocks from the address
    dec_gemm_group<T, TO, TW>(a);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fl = lane & 15, fg = lane >> 4;
    const int n0 = blockIdx.x * 16 * NT;
    const int m0 = blockIdx.y * MT * 16;
    constexpr int KW = WTraits<T, TW>::KW, SUB = KW / 8, KSTEP = 4 * KW;
    constexpr int TILES = MT * NT, TPW = (TILES + NW - 1) / NW;
    const int kspan = a.K / NW, kb = wave * kspan, iters = kspan / KSTEP;
    const TW* wp[NT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++) wp[nt] = (const TW*)a.W + (long)min(n0 + nt * 16 + fl, a.N - 1) * a.K + kb + fg * KW;
    const long xstep = (long)a.x_mpad * 32 * (KSTEP / 32);
    const T* xp = (const T*)a.X + ((long)((kb + fg * KW) >> 5) * a.x_mpad + m0 + fl) * 32 + ((fg * KW) & 31);
    // four 32-deep k-slabs in flight per wave: (NT + MT) KiB each; two with 32-byte fragments (the register file holds NT + MT of them per slab)
    constexpr int DEPTH = sizeof(typename FragT<T>::type) <= 16 ? 4 / SUB : 2;
    typename FragT<T>::type wq[DEPTH][NT][SUB], xq[DEPTH][SUB][MT];
#pragma unroll
    for (int i = 0; i < DEPTH; i++)
        if (i < iters) {
#pragma unroll
            for (int nt = 0; nt < NT; nt++) load_wfrags<T, TW>(wp[nt] + i * KSTEP, wq[i][nt]);
#pragma unroll
            for (int j = 0; j < SUB; j++)
#pragma unroll
                for (int t = 0; t < MT; t++) xq[i][j][t] = load_frag<T>(xp + i * xstep + t * 512 + 8 * j);
        }
    // the tiles this wave finishes; their residual rows are fetched now, the per-column operands after the main loop
    int en[TPW], em[TPW];
    bool ep_ok[TPW];
    f32x4 pre_r[TPW];
    float pre_sh[TPW];   // the rows' running offsets (producers: SkinnyArgs::row_shift)
#pragma unroll
    for (int j = 0; j < TPW; j++) {
        const int t = wave + j * NW;
        en[j] = n0 + (t / MT) * 16 + 4 * fg;
        em[j] = m0 + (t % MT) * 16 + fl;
        ep_ok[j] = t < TILES && en[j] < a.N && em[j] < a.M;
        pre_r[j] = f32x4{0, 0, 0, 0};
        pre_sh[j] = 0.0f;
        if (ep_ok[j] && a.R) pre_r[j] = *reinterpret_cast<const f32x4*>(a.R + (long)em[j] * a.ldr + en[j]);
        if (ep_ok[j] && a.row_shift) pre_sh[j] = a.row_shift[em[j]];
    }
    typedef DecGemmLds<NW, MT, TILES> Lds;
    float* lnred = Lds::lnq(smem_raw);
    if (a.ln_part) {
        constexpr int ROWS = MT * 16;
        static_assert(4 * ROWS <= NW * 64, "one thread per (quarter, row)");
        if (tid < 4 * ROWS) {
            const int r = tid % ROWS, q = tid / ROWS;
            float s1, s2;
            ln_partial_sum(a.ln_part, a.ln_tiles, a.x_mpad, m0 + r, q, 4, s1, s2);
            ln_part_store<ROWS>(lnred, r, q, s1, s2);
        }
    }
    // per-column operands of the tiles this wave finishes: requested AFTER the main loop.  Requesting them before it where the
    // register file has room (two column tiles per workgroup) was measured slower in round 3 — the trace of the whole step reads
    // 9.68 instead of 8.74 us for the QKV / cross-Q launches, 7.17 instead of 6.97 us for the out-projections
    // (profiles/r03_kernel_stats_base_bf16_b1024.txt history) — they only lengthen the queue in front of the first fragments.
    f32x4 pre_bias[TPW], pre_ws[TPW], pre_g[TPW], pre_sv[TPW];
    auto load_cols = [&]() {
#pragma unroll
        for (int j = 0; j < TPW; j++) {
            pre_bias[j] = f32x4{0, 0, 0, 0}; pre_ws[j] = f32x4{1, 1, 1, 1}; pre_g[j] = f32x4{1, 1, 1, 1}; pre_sv[j] = f32x4{0, 0, 0, 0};
            if (ep_ok[j]) {
                if (a.bias) pre_bias[j] = *reinterpret_cast<const f32x4*>(a.bias + en[j]);
                if (a.wscale) pre_ws[j] = *reinterpret_cast<const f32x4*>(a.wscale + en[j]);
                if (a.xgamma) pre_g[j] = *reinterpret_cast<const f32x4*>(a.xgamma + en[j]);
                if (a.ln_part) pre_sv[j] = *reinterpret_cast<const f32x4*>(a.ln_s + en[j]);
            }
        }
    };
    f32x4 acc[NT][MT];
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int t = 0; t < MT; t++) acc[nt][t] = f32x4{0, 0, 0, 0};
    // rolling prefetch: a slot is refilled with the k-slab DEPTH ahead as soon as its MFMAs are issued, so the next round's
    // loads fly under this round's arithmetic instead of starting after it
    for (int c0 = 0; c0 < iters; c0 += DEPTH) {
#pragma unroll
        for (int i = 0; i < DEPTH; i++) {
            if (c0 + i < iters) {
#pragma unroll
                for (int j = 0; j < SUB; j++)
#pragma unroll
                    for (int nt = 0; nt < NT; nt++)
#pragma unroll
                        for (int t = 0; t < MT; t++) mma16(acc[nt][t], wq[i][nt][j], xq[i][j][t]);
            }
            if (c0 + DEPTH + i < iters) {
#pragma unroll
                for (int nt = 0; nt < NT; nt++) load_wfrags<T, TW>(wp[nt] + (c0 + DEPTH + i) * KSTEP, wq[i][nt]);
#pragma unroll
                for (int j = 0; j < SUB; j++)
#pragma unroll
                    for (int t = 0; t < MT; t++) xq[i][j][t] = load_frag<T>(xp + (c0 + DEPTH + i) * xstep + t * 512 + 8 * j);
            }
        }
    }
    load_cols();
    f32x4* red = Lds::red(smem_raw);
#pragma unroll
    for (int nt = 0; nt < NT; nt++)
#pragma unroll
        for (int t = 0; t < MT; t++) red[(wave * TILES + nt * MT + t) * 64 + lane] = acc[nt][t];
    __syncthreads();
#pragma unroll
    for (int j = 0; j < TPW; j++) {
        const int t = wave + j * NW;
        if (t >= TILES) break;  // wave-uniform
        f32x4 s = {0, 0, 0, 0};
        float v[4] = {0, 0, 0, 0};
        if (ep_ok[j]) {
            s = red[(0 * TILES + t) * 64 + lane];
#pragma unroll
            for (int w = 1; w < NW; w++) {
                f32x4 o = red[(w * TILES + t) * 64 + lane];
                s[0] += o[0]; s[1] += o[1]; s[2] += o[2]; s[3] += o[3];
            }
            float ln_mean = 0.0f, ln_rstd = 1.0f;
            if (a.ln_part) {
                ln_row_stats<MT * 16>(lnred, (t % MT) * 16 + fl, a.K, ln_mean, ln_rstd);
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const float sc = wh_scale(s[e], pre_ws[j][e]);  // fp8 weights: the channel scale (1 otherwise)
                v[e] = a.ln_part ? wh_ln_fold(sc, ln_mean, ln_rstd, pre_sv[j][e], pre_bias[j][e]) : wh_add(sc, pre_bias[j][e]);
                if (a.act == 1) v[e] = gelu_erf(v[e]);
                v[e] += pre_r[j][e];
            }
            if (a.c_mpad) store4((T*)a.C + slab_idx(em[j], en[j], a.c_mpad), v[0], v[1], v[2], v[3]);
            else store4((TO*)a.C + (long)em[j] * a.ldc + en[j], v[0], v[1], v[2], v[3]);
            if (a.xslab_out) store4((T*)a.xslab_out + slab_idx(em[j], en[j], a.x_mpad), wh_sub(v[0], pre_sh[j]) * pre_g[j][0], wh_sub(v[1], pre_sh[j]) * pre_g[j][1],
                                    wh_sub(v[2], pre_sh[j]) * pre_g[j][2], wh_sub(v[3], pre_sh[j]) * pre_g[j][3]);
            if (a.shift_io && blockIdx.x == 0 && blockIdx.z == 0 && t / MT == 0 && fg == 0) a.shift_io[em[j]] += ln_mean;   // (first column tile only)
        }
        if (a.stats_out) {
            // this column tile's {sum x, sum x^2} per row (producers have no activation: v = s*ws + bias + r, as in k_dec_gemm)
            float s1 = 0.0f, s2 = 0.0f;
            if (ep_ok[j]) {
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const float u = wh_sub(wh_add(wh_add(wh_scale(s[e], pre_ws[j][e]), pre_bias[j][e]), pre_r[j][e]), pre_sh[j]);
                    s1 += u;
                    s2 = __builtin_fmaf(u, u, s2);
                }
            }
            s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
            s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
            if (fg == 0 && em[j] < a.M) {
                const long tile = (long)blockIdx.x * NT + t / MT;
                a.stats_out[(tile * a.x_mpad + em[j]) * 2] = s1;
                a.stats_out[(tile * a.x_mpad + em[j]) * 2 + 1] = s2;
            }
        }
    }
    advance_if_last(a.ticket, a.pos_w, gridDim.x * gridDim.y);
}

template <typename T, typename TO, int NW, typename TW>
void launch_dec_gemm_mt(hipStream_t s, const SkinnyArgs& a) {
    const int n_tiles = (a.N + 15) / 16;
    const int Ms = a.m_sel ? a.m_sel : a.M;   // the rows the variant is chosen for: the whole batch's, also when the launch runs a row range of it
    auto launch = [&](auto kernel, dim3 grid, size_t smem) {
        set_max_smem(kernel, smem);
        hipLaunchKernelGGL(kernel, grid, dim3(NW * 64), smem, s, a);
    };
    // rows per workgroup: 64, or 32 when K is deep (every workgroup pulls its rows of X through L2; halving
    // them costs a second read of the 16-column weight tile but doubles the workgroups sharing the load)
    // measured (tools/microbench.cpp, M = 64): N = 512 → 16 rows best (2.6 vs 3.7 us), N = 1536 / 2048 → 32 rows
    // (2.95 vs 3.5 us), K = 2048 → 16 rows (4.6 vs 7.5 us): aim for >= 128 workgroups
    int mt_cap = (NW == 8 || n_tiles <= 48) ? 1 : 2;
    // wide models (K >= 1024: weights stream from HBM, profiles/r02_dec_gemm_wide_m32.txt): 32-row groups only for the 8-way
    // split of a wide N (QKV: 6.9 vs 7.6 us); everything else 16 rows (fc1 9.9 vs 10.5 us, N = 1280 4.6 vs 5.3 us)
    if (a.K >= 1024) mt_cap = (NW == 8 && n_tiles > 96) ? 2 : 1;
    if (wh_dbg_mt > 0) mt_cap = wh_dbg_mt;  // microbench override
    // batches beyond 64 rows (measured at 256 clips): 64-row groups for the 4-way K split — the row groups already give
    // hundreds of workgroups, and each weight fragment then feeds four MFMAs instead of one or two (-0.7 % step time)
    if (wh_dbg_mt <= 0 && Ms > 64 && NW == 4) mt_cap = n_tiles <= 32 ? 2 : 4;   // (narrow N at 256 rows: 4.1 vs 4.8 us)
    if (wh_dbg_mt <= 0 && Ms > 64 && NW == 8 && !a.xpart) mt_cap = 2;  // fc2: 32-row groups (-0.5 %; 64 is slower again)
    // hundreds of rows (one key range per clip, so no merged X): NT column tiles per workgroup while >= 256 workgroups remain
    // (k_dec_gemm_wide; bit-identical results, so following the batch is allowed)
    if constexpr (!__is_same(T, float) && !__is_same(T, xf32))   // (f32 rows keep k_dec_gemm: the exact-f32 mode and the small-context form of the split-fp16 mode)
    if (Ms > 64 && !a.xpart && wh_dbg_mt <= 0 && a.K % (NW * 4 * WTraits<T, TW>::KW) == 0) {
        constexpr int WMT = 4;
        int wide = wh_dbg_wide;
        if (const char* e = getenv("WH_DEC_WIDE")) wide = atoi(e);   // A/B switch for the parity test (0: k_dec_gemm only)
        const int rg = (Ms + 16 * WMT - 1) / (16 * WMT);   // (of the whole batch: decides nt; the grid below covers this launch's rows)
        // measured (tools/dec_gemm_sweep.cpp, profiles/r02_dec_gemm_sweep.txt): four column tiles while >= 512 workgroups
        // remain (fc1 at 1024 rows: 11.7 vs 13.2 us), else two while >= 128 remain (1280 x 1280 at 256 rows: 8.5 vs 11.3 us;
        // 512 x 512 at 256 rows would leave 64: 5.7 vs 4.1 us), else k_dec_gemm.  Eight waves x 16 tiles of partial sums
        // would take 128 KB of LDS: two tiles at most there.
        int nt = 1;
        if (NW == 4 && n_tiles % 4 == 0 && (n_tiles / 4) * rg * a.zn >= 512) nt = 4;
        else if (n_tiles % 2 == 0 && (n_tiles / 2) * rg * a.zn >= 128) nt = 2;
        if (wide == 2 || (wide == 4 && NW == 4)) nt = wide;
        if (wide != 0 && nt > 1 && n_tiles % nt == 0) {
            wh_with_pow2<2, 4>(nt, [&](auto NT) {
                launch(k_dec_gemm_wide<T, TO, WMT, decltype(NT)::value, NW, TW>, dim3(n_tiles / nt, (a.M + 16 * WMT - 1) / (16 * WMT), a.zn), DecGemmLds<NW, WMT, WMT * decltype(NT)::value>::BYTES);
            });
            return;
        }
    }
    const int mt = std::min(mt_cap, (Ms + 15) / 16);
    if (a.xpart) {  // X merged from attention partials: 16-row groups only (the merge is per-lane work)
        wh_with_pow2<4, 32>(a.x_splits, [&](auto XP) {   // + merged X tile
            launch(k_dec_gemm<T, TO, 1, NW, decltype(XP)::value, TW>, dim3(n_tiles, (a.M + 15) / 16), DecGemmLds<NW, 1, 1>::BYTES + (size_t)16 * a.K * sizeof(T));
        });
        return;
    }
    wh_with_1to4(mt, [&](auto MT) {   // grid and LDS follow the run-time mt as they always did (the carve is linear in the row tiles)
        launch(k_dec_gemm<T, TO, decltype(MT)::value, NW, 0, TW>, dim3(n_tiles, (a.M + 16 * mt - 1) / (16 * mt), a.zn), mt * DecGemmLds<NW, 1, 1>::BYTES);
    });
}

// K split over the waves of a workgroup: 8 ways when K is deep, when X is merged from attention partials, or when the
// launch would otherwise put fewer than ~128 workgroups on the chip (small batch x narrow N: more waves per
// workgroup keep more weight bytes in flight per CU); else 4.  Needs K % 256 == 0.
static inline bool dec_gemm_8way(const SkinnyArgs& a) {
    // (K >= 1024, N <= 4096: eight waves per workgroup keep twice the weight bytes in flight per CU — 4.6 vs 5.8 us for
    // N = K = 1280 at 32 rows, 5.7 vs 6.5 us for the QKV projection; the widest N has enough workgroups without it.
    // The choice never depends on the batch: a batch must not change the summation order of a row)
    return (a.K >= 2048 || a.xpart || (a.K >= 1024 && a.N <= 4096)) && a.K % 256 == 0;
}

template <typename T, typename TO, typename TW>
void launch_dec_gemm_split(hipStream_t s, const SkinnyArgs& a) {
    // K is split over the waves of a workgroup: 8 ways when it is deep, else 4 (K % 128 == 0 always
    // holds: d_model and ffn are multiples of 128, checked at model load)
    // (X from attention partials: 8 ways too — fewer fragments to merge per lane)
    const bool eight = wh_dbg_nw ? (wh_dbg_nw == 8 && a.K % 256 == 0) : dec_gemm_8way(a);
    if (eight) launch_dec_gemm_mt<T, TO, 8, TW>(s, a);
    else launch_dec_gemm_mt<T, TO, 4, TW>(s, a);
}

}  // namespace

void wh_launch_dec_gemm(hipStream_t s, int prec, bool out_f32, const SkinnyArgs& a) {
    if (prec == WH_PREC_F32) launch_dec_gemm_split<float, float, float>(s, a);
    else if (prec == WH_PREC_F16X3) launch_dec_gemm_split<h2, float, h2>(s, a);   // operands as fp16 limbs (weights, slabs), f32 row-major results
    else if (prec == WH_PREC_FP8 && a.wscale) {  // e4m3 weight codes, bf16 activations
        // 16 codes per lane per load when every wave's K share is a multiple of 64, else 8
        const int nw = dec_gemm_8way(a) ? 8 : 4;
        const bool wide = (a.K / nw) % 64 == 0;
        if (wide) { if (out_f32) launch_dec_gemm_split<bf16, float, fp8x16_t>(s, a); else launch_dec_gemm_split<bf16, bf16, fp8x16_t>(s, a); }
        else { if (out_f32) launch_dec_gemm_split<bf16, float, fp8x8_t>(s, a); else launch_dec_gemm_split<bf16, bf16, fp8x8_t>(s, a); }
    } else if (out_f32) launch_dec_gemm_split<bf16, float, bf16>(s, a);
    else launch_dec_gemm_split<bf16, bf16, bf16>(s, a);
}
