// wh_score.hip — the two kernels of wh_score_tokens: causal self-attention over all positions of a hypothesis at once, and
// the finish that turns each position's raw logits into the log-probability of the given token and the masked argmax.
//
// The scoring pass runs every (hypothesis, position) as one row of the decode workspace: hypothesis g occupies the T adjacent rows
// g * T .. g * T + T - 1, row g * T + t being model position t.  Every other kernel of a decoder layer is row-wise (or, the cross-attention,
// shares a clip's states between rows); self-attention is the one that ties the rows of a hypothesis together.
#include "wh_common.h"
#include "wh_dec_epilogue.h"
#include "wh_kernels.h"

namespace {

// ---- causal self-attention over a hypothesis's T rows, straight from the QKV buffer ([3P] :417-425, 468-475) ----------------------------
// qkv [R][3d] (q pre-scaled | k | v) in the compute dtype, R = G * T.  Row (g, t) attends to the k / v of rows (g, 0 .. t): there is no cache.
// One workgroup = (head h, block of QB = 64 query rows of hypothesis g), four waves, 16 query rows per wave in four groups of 4.  The keys are
// walked in chunks of KC = 64 (chunk c covers keys 64 c .. 64 c + 63; the block of queries 64 qb .. needs chunks 0 .. qb): a chunk's K and V
// rows are staged in LDS as f32 with 16-byte global loads, and every row keeps an online softmax (m, l, o) in registers, so one code path serves
// any T and both dtypes.  Per chunk and group of 4 rows: lane j scores key j for the 4 rows (K row j from LDS at a 65-float pitch, conflict
// free; the 4 rows' q as one broadcast 16-byte LDS read), the wave reduces max and sum, the probabilities go to the wave's own LDS strip, and
// lane e accumulates column e of P.V for the 4 rows.  Softmax and accumulation in f32.
// Invariants, for any T >= 1, any G and any grid that covers them:
//   * only rows g * T + kj with kj < T (and < R) are loaded: nothing of another hypothesis, nothing beyond R; unstaged LDS rows are zero;
//   * key kj enters row t's result only if kj <= t: its score is -inf otherwise, its probability exactly 0 (so, with finite V, its term is 0);
//     every chunk a block walks starts at a key <= the block's first row, so every row's running maximum is finite from its first chunk on;
//   * a query row t >= T computes on row T - 1's data and stores nothing; row (g, t < T) stores its own 64 columns of head h only.
constexpr int SC_QB = 64, SC_KC = 64, SC_KP = WH_HEAD_DIM + 1;
template <typename T, typename TO>
__global__ __launch_bounds__(256) void k_score_self_attn(const T* __restrict__ qkv, TO* __restrict__ out, int d, int Tn, long R, int mpad) {
    constexpr int HD = WH_HEAD_DIM, EPC = 16 / (int)sizeof(T), CPR = HD / EPC;   // elements per 16-byte load, loads per 64-element row
    typedef __attribute__((ext_vector_type(EPC))) T vrow_t;
    __shared__ __attribute__((aligned(16))) float qs[SC_QB / 4][HD][4];   // [group of 4 rows][e][row in group]
    __shared__ __attribute__((aligned(16))) float Ks[SC_KC * SC_KP];
    __shared__ __attribute__((aligned(16))) float Vs[SC_KC * HD];
    __shared__ __attribute__((aligned(16))) float ps[4][SC_KC][4];        // per wave: [key][row in group]
    const int h = blockIdx.x, qb = blockIdx.y, g = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = qb * SC_QB;
    const long row0 = (long)g * Tn;   // the hypothesis's first row
    // the block's queries (rows past T: row T - 1 again)
    for (int i = tid; i < SC_QB * CPR; i += 256) {
        const int r = i / CPR, ch = i % CPR, t = min(q0 + r, Tn - 1);
        const vrow_t v = *reinterpret_cast<const vrow_t*>(qkv + (row0 + t) * 3 * d + h * HD + ch * EPC);
#pragma unroll
        for (int e = 0; e < EPC; e++) qs[r >> 2][ch * EPC + e][r & 3] = cvt_in<T>(v[e]);
    }
    float m[16], l[16], o[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { m[i] = -INFINITY; l[i] = 0.0f; o[i] = 0.0f; }
    for (int c = 0; c <= qb; c++) {
        const int k0 = c * SC_KC;
        __syncthreads();   // (the previous chunk's readers are done; first pass: qs is complete)
        for (int i = tid; i < SC_KC * CPR; i += 256) {
            const int j = i / CPR, ch = i % CPR, kj = k0 + j;
            vrow_t kv = {}, vv = {};
            if (kj < Tn && row0 + kj < R) {
                const T* src = qkv + (row0 + kj) * 3 * d + d + h * HD + ch * EPC;
                kv = *reinterpret_cast<const vrow_t*>(src);
                vv = *reinterpret_cast<const vrow_t*>(src + d);
            }
#pragma unroll
            for (int e = 0; e < EPC; e++) {
                Ks[j * SC_KP + ch * EPC + e] = cvt_in<T>(kv[e]);
                Vs[j * HD + ch * EPC + e] = cvt_in<T>(vv[e]);
            }
        }
        __syncthreads();
#pragma unroll
        for (int gi = 0; gi < 4; gi++) {
            const int grp = wave * 4 + gi, t0 = q0 + grp * 4;   // rows t0 .. t0 + 3
            if (k0 > min(t0 + 3, Tn - 1)) continue;             // (wave-uniform) the whole chunk lies behind these rows
            f32x4 s = {0, 0, 0, 0};
#pragma unroll 16
            for (int e = 0; e < HD; e++) {
                const f32x4 qv = *reinterpret_cast<const f32x4*>(&qs[grp][e][0]);
                s += qv * Ks[lane * SC_KP + e];
            }
            f32x4 p;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int t = min(t0 + r, Tn - 1);
                const float sr = (k0 + lane <= t) ? s[r] : -INFINITY;
                const float mn = fmaxf(m[gi * 4 + r], dpp_wave_max(sr));   // finite: key k0 <= t
                const float a = __expf(m[gi * 4 + r] - mn);
                p[r] = __expf(sr - mn);
                l[gi * 4 + r] = l[gi * 4 + r] * a + dpp_wave_sum(p[r]);
                o[gi * 4 + r] *= a;
                m[gi * 4 + r] = mn;
            }
            *reinterpret_cast<f32x4*>(&ps[wave][lane][0]) = p;   // (a wave's strip: written and read by that wave only, in program order)
            f32x4 acc = {0, 0, 0, 0};
#pragma unroll 16
            for (int j = 0; j < SC_KC; j++) {
                const f32x4 pv = *reinterpret_cast<const f32x4*>(&ps[wave][j][0]);
                acc += pv * Vs[j * HD + lane];
            }
#pragma unroll
            for (int r = 0; r < 4; r++) o[gi * 4 + r] += acc[r];
        }
    }
#pragma unroll
    for (int gi = 0; gi < 4; gi++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int t = q0 + (wave * 4 + gi) * 4 + r;
            if (t < Tn && row0 + t < R) store1(out + slab_idx((int)(row0 + t), h * HD + lane, mpad), o[gi * 4 + r] / l[gi * 4 + r]);
        }
}

// ---- the finish: one workgroup per virtual row over the [rows][vocab] f32 scratch the LM head filled -------------------------------------
// Row (g, t) is entry i = t - (P - 1) of hypothesis g.  Prompt rows (i < 0) and padded rows (i >= len[g]) do nothing.  Otherwise, over the
// allowed ids (not suppressed by the entry's mask — mask_first for i == 0, mask_base after — and a logit that is neither NaN nor -inf):
//   argmax (ties: the lowest id; nothing allowed: 0) and logprob = v[target] - (m + logf(sum expf(v - m))), -inf for a target that is not allowed,
// written compactly at [g][i] of [G][Lmax].  The row pitch is `vocab` floats, so a row starts at any 4-byte offset: the elements before the
// first 16-byte boundary and after the last whole group are read one by one, the rest with 16-byte loads.  Reads stay in [row V, row V + V).
__device__ __forceinline__ bool sc_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
template <typename F>
__device__ __forceinline__ void sc_scan(const float* __restrict__ row, int V, int tid, F&& f) {
    const int head = min(V, (int)((4 - (((uintptr_t)row >> 2) & 3)) & 3)), ng = (V - head) >> 2, tail0 = head + ng * 4;
    if (tid < head) f(row[tid], tid);
    for (int gq = tid; gq < ng; gq += 256) {
        const int i = head + gq * 4;
        const f32x4 x = *reinterpret_cast<const f32x4*>(row + i);
        f(x[0], i); f(x[1], i + 1); f(x[2], i + 2); f(x[3], i + 3);
    }
    if (tail0 + tid < V && tid < 4) f(row[tail0 + tid], tail0 + tid);
}
__global__ __launch_bounds__(256) void k_score_finish(const float* __restrict__ logits, int V, const unsigned* __restrict__ mask_first,
                                                      const unsigned* __restrict__ mask_base, int Tn, int P, int Lmax, const int* __restrict__ len,
                                                      const int* __restrict__ target, float* __restrict__ lp_out, int* __restrict__ am_out) {
    extern __shared__ unsigned sc_mask[];   // the entry's suppress mask, V / 32 + 1 words
    __shared__ float sbv[4], sbs[4];
    __shared__ int sbi[4];
    const int row = blockIdx.x, tid = threadIdx.x, g = row / Tn, i = row % Tn - (P - 1);
    if (i < 0 || i >= len[g]) return;   // (workgroup-uniform)
    const unsigned* mask = i == 0 ? mask_first : mask_base;
    for (int w = tid; w < V / 32 + 1; w += 256) sc_mask[w] = mask[w];
    __syncthreads();
    const float* v = logits + (long)row * V;
    const int tgt = target[(long)g * Lmax + i];
#define SC_OK(x, n) (!((sc_mask[(n) >> 5] >> ((n) & 31)) & 1u) && (x) > -INFINITY)   // (NaN: not greater)
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    sc_scan(v, V, tid, [&](float x, int n) {
        const bool take = SC_OK(x, n) && sc_before(x, n, bv, bi);
        bv = take ? x : bv;
        bi = take ? n : bi;
    });
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (sc_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if ((tid & 63) == 0) { sbv[tid >> 6] = bv; sbi[tid >> 6] = bi; }
    __syncthreads();
    bv = sbv[0]; bi = sbi[0];
#pragma unroll
    for (int q = 1; q < 4; q++)
        if (sc_before(sbv[q], sbi[q], bv, bi)) { bv = sbv[q]; bi = sbi[q]; }
    const float m = bv;   // the largest allowed logit (-inf: nothing is allowed)
    float sum = 0.0f;
    if (m > -INFINITY) sc_scan(v, V, tid, [&](float x, int n) { sum += SC_OK(x, n) ? expf(x - m) : 0.0f; });
    sum = wave_sum(sum);
    if ((tid & 63) == 0) sbs[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        sum = (sbs[0] + sbs[1]) + (sbs[2] + sbs[3]);
        const float vt = v[tgt];
        const bool ok = bi != 0x7fffffff && SC_OK(vt, tgt);
        lp_out[(long)g * Lmax + i] = ok ? wh_sub(vt, m) - logf(sum) : -INFINITY;
        am_out[(long)g * Lmax + i] = bi == 0x7fffffff ? 0 : bi;
    }
#undef SC_OK
}

}  // namespace

void wh_launch_score_self_attn(hipStream_t s, int prec, const void* qkv, void* out, int d, int n_heads, int T, int n_hyp, int mpad) {
    const dim3 grid(n_heads, (T + SC_QB - 1) / SC_QB, n_hyp);
    const long R = (long)n_hyp * T;
    if (prec == WH_PREC_F32) hipLaunchKernelGGL((k_score_self_attn<float, float>), grid, dim3(256), 0, s, (const float*)qkv, (float*)out, d, T, R, mpad);
    else hipLaunchKernelGGL((k_score_self_attn<bf16, bf16>), grid, dim3(256), 0, s, (const bf16*)qkv, (bf16*)out, d, T, R, mpad);
}

void wh_launch_score_finish(hipStream_t s, const float* logits, int vocab, const unsigned* mask_first, const unsigned* mask_base, int rows, int T, int P,
                            int Lmax, const int* len, const int* target, float* lp_out, int* am_out) {
    hipLaunchKernelGGL(k_score_finish, dim3(rows), dim3(256), (size_t)(vocab / 32 + 1) * 4, s, logits, vocab, mask_first, mask_base, T, P, Lmax, len, target,
                       lp_out, am_out);
}
