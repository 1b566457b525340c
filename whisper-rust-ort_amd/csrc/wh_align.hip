// wh_align.hip — word-level timestamps (wh_ctx_set_alignment): the per-position copy of the alignment heads' cross-attention
// queries inside the token loop (k_align_gather: the same for every position of a forced pass at once, wh_align_tokens), and the
// post-pass of a decode call — scores + row softmax, column normalisation + median filter + head
// average, dynamic time warping with its backtrace — for a chunk of clips per launch.
//
// Every kernel bounds a row by its own generated-token count n = clamp(n_out[b] - n_prompt, 0, cap), read on the device: rows that finished
// early kept running in the loop and their later queries are garbage.  A row with n <= 1 does nothing (its one frame is 0).
#include <algorithm>

#include "wh_common.h"
#include "wh_kernels.h"

namespace {

__device__ __forceinline__ int align_rows(const AlignArgs& a, int b) { return min(max(a.n_out[b] - a.n_prompt, 0), a.cap); }

// ---- token loop: the listed heads' queries of one layer as f32, at index pos - (n_prompt - 1) = the generated token this position emits --------
// grid (rows of the batch, listed heads of the layer); prompt positions before the emitting one write nothing.
template <typename T>
__global__ __launch_bounds__(64) void k_align_copy(const T* __restrict__ src, long row_pitch, long head_pitch, int dk, AlignLayerHeads hs, const int* __restrict__ pos_p,
                                                   int first_emit, int cap, int nb, float* __restrict__ dst) {
    const int g = *pos_p - first_emit;
    if (g < 0 || g >= cap) return;
    const int b = blockIdx.x, a = hs.slot[blockIdx.y], h = hs.head[blockIdx.y];
    const T* s = src + (long)b * row_pitch + (long)h * head_pitch;
    float* d = dst + (((long)a * nb + b) * cap + g) * dk;
    for (int k = threadIdx.x; k < dk; k += 64) d[k] = (float)s[k];
}

// ---- forced pass (wh_align_tokens): the same copy for all positions of all hypotheses of a pass at once -----------------------
// grid (rows of the pass, listed heads of the layer).  Row r = g * T + t is entry i = t - (P - 1) of hypothesis g; a row outside 0 <= i < len[g]
// (an earlier prompt position, the padding of a shorter hypothesis) or at or past `rows` returns before it reads anything.  VEC: every source
// and destination address is 16-byte aligned (the launcher checks pitches, dk and the bases): a thread moves 16 source bytes per trip.
template <typename T, bool VEC>
__global__ __launch_bounds__(64) void k_align_gather(const T* __restrict__ src, long row_pitch, long head_pitch, int dk, AlignLayerHeads hs, int rows, int Tn, int P,
                                                     int Lmax, const int* __restrict__ len, int G, float* __restrict__ dst) {
    const int r = blockIdx.x;
    if (r >= rows) return;
    const int g = r / Tn, i = r - g * Tn - (P - 1);
    if (g >= G || i < 0 || i >= min(len[g], Lmax)) return;
    const int a = hs.slot[blockIdx.y], h = hs.head[blockIdx.y];
    const T* s = src + (long)r * row_pitch + (long)h * head_pitch;
    float* d = dst + (((long)a * G + g) * Lmax + i) * dk;
    if constexpr (VEC) {
        constexpr int E = 16 / (int)sizeof(T);
        for (int k = E * threadIdx.x; k < dk; k += E * 64) {
            if constexpr (sizeof(T) == 2) {
                const bf16x8 v = *reinterpret_cast<const bf16x8*>(s + k);
                *reinterpret_cast<f32x4*>(d + k) = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
                *reinterpret_cast<f32x4*>(d + k + 4) = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
            } else {
                *reinterpret_cast<f32x4*>(d + k) = *reinterpret_cast<const f32x4*>(s + k);
            }
        }
    } else {
        for (int k = threadIdx.x; k < dk; k += 64) d[k] = (float)s[k];
    }
}

// the row softmax both score kernels end with: wave `wave` of four normalises rows wave, wave + 4, ... of its workgroup's raw scores in place
__device__ __forceinline__ void softmax_rows(float* P, int Sp, int n, int Sb, int wave, int lane) {
    for (int g = wave; g < n; g += 4) {
        float* row = P + (long)g * Sp;
        float m = -INFINITY;
        for (int s = lane; s < Sb; s += 64) m = fmaxf(m, row[s]);
        for (int o = 32; o; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        float sum = 0.0f;
        for (int s = lane; s < Sb; s += 64) sum += expf(row[s] - m);
        for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
        for (int s = lane; s < Sb; s += 64) row[s] = expf(row[s] - m) / sum;
    }
}

// ---- scores + row softmax, one workgroup per (head, clip) ------------------------------------------------------------------------------------
// P[g][s] = softmax over s < S_b of q_g . k_s.  The key rows are read once per (clip, head): a wave keeps the 16 keys of its frame tile as the
// MFMA column operand and runs over the row tiles; the queries (f32, a few KB, cache resident) are the row operand.  SPLIT: the query enters as
// bf16 hi + lo (the expanded f32 query of the encoder-state form; the K/V form's query was bf16 to begin with, lo == 0).  The raw scores go to P,
// then the workgroup normalises its own rows in place.
template <int DK, bool SPLIT>
__global__ __launch_bounds__(256) void k_align_scores_bf16(AlignArgs a) {
    const int hd = blockIdx.x, cl = blockIdx.y, b = a.clip0 + cl;
    const int n = align_rows(a, b);
    if (n <= 1) return;
    const int Sb = a.sb[b];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, fl = lane & 15, fg = lane >> 4;
    const bf16* K = (const bf16*)a.k_base[hd] + (long)(a.k_clip0 + b / a.k_div) * a.k_clip_pitch;
    const float* Q = a.q + ((long)hd * a.nb + b) * a.cap * DK;
    float* P = a.P + ((long)cl * a.n_heads + hd) * a.cap * a.Sp;
    const int n_st = (Sb + 15) >> 4, n_rt = (n + 15) >> 4;
    for (int st = wave; st < n_st; st += 4) {
        const int sk = min(st * 16 + fl, Sb - 1);
        bf16x8 kf[DK / 32];
#pragma unroll
        for (int ks = 0; ks < DK / 32; ks++) kf[ks] = *reinterpret_cast<const bf16x8*>(K + (long)sk * a.k_row_pitch + 32 * ks + 8 * fg);
        for (int rt = 0; rt < n_rt; rt++) {
            const float* qp = Q + (long)min(rt * 16 + fl, n - 1) * DK + 8 * fg;
            f32x4 acc = {0, 0, 0, 0};
#pragma unroll
            for (int ks = 0; ks < DK / 32; ks++) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(qp + 32 * ks), v = *reinterpret_cast<const f32x4*>(qp + 32 * ks + 4);
                bf16x8 qh, ql;
#pragma unroll
                for (int e = 0; e < 8; e++) {
                    const float x = e < 4 ? u[e & 3] : v[e & 3];
                    qh[e] = (bf16)x;
                    if constexpr (SPLIT) ql[e] = (bf16)(x - (float)qh[e]);
                }
                if constexpr (SPLIT) mma16(acc, ql, kf[ks]);
                mma16(acc, qh, kf[ks]);   // D column = frame fl, D rows = tokens 4 fg + r
            }
            const int sc = st * 16 + fl;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int g = rt * 16 + 4 * fg + r;
                if (g < n && sc < Sb) P[(long)g * a.Sp + sc] = acc[r];
            }
        }
    }
    __syncthreads();
    softmax_rows(P, a.Sp, n, Sb, wave, lane);
}

// The f32 mode (K rows of the f32 cross-K/V plane, 64 wide): a thread keeps one key row in registers and runs over the queries, staged through
// LDS 64 rows at a time; plain f32 fma chains in k order.
__global__ __launch_bounds__(256) void k_align_scores_f32(AlignArgs a) {
    constexpr int DK = WH_HEAD_DIM, RC = 64;
    __shared__ float qs[RC][DK];
    const int hd = blockIdx.x, cl = blockIdx.y, b = a.clip0 + cl;
    const int n = align_rows(a, b);
    if (n <= 1) return;
    const int Sb = a.sb[b], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* K = (const float*)a.k_base[hd] + (long)(a.k_clip0 + b / a.k_div) * a.k_clip_pitch;
    const float* Q = a.q + ((long)hd * a.nb + b) * a.cap * DK;
    float* P = a.P + ((long)cl * a.n_heads + hd) * a.cap * a.Sp;
    for (int s0 = 0; s0 < Sb; s0 += 256) {
        const int s = s0 + tid;
        const float* kp = K + (long)min(s, Sb - 1) * a.k_row_pitch;
        f32x4 kr[DK / 4];
#pragma unroll
        for (int k = 0; k < DK / 4; k++) kr[k] = *reinterpret_cast<const f32x4*>(kp + 4 * k);
        for (int g0 = 0; g0 < n; g0 += RC) {
            __syncthreads();
            for (int e = tid; e < RC * DK; e += 256) qs[e / DK][e % DK] = (g0 + e / DK < n) ? Q[(long)g0 * DK + e] : 0.0f;
            __syncthreads();
            const int ng = min(RC, n - g0);
            for (int gi = 0; gi < ng; gi++) {
                float acc = 0.0f;
#pragma unroll
                for (int k = 0; k < DK / 4; k++) {
                    const f32x4 q4 = *reinterpret_cast<const f32x4*>(&qs[gi][4 * k]);
                    acc = fmaf(q4[0], kr[k][0], acc); acc = fmaf(q4[1], kr[k][1], acc); acc = fmaf(q4[2], kr[k][2], acc); acc = fmaf(q4[3], kr[k][3], acc);
                }
                if (s < Sb) P[(long)(g0 + gi) * a.Sp + s] = acc;
            }
        }
    }
    __syncthreads();
    softmax_rows(P, a.Sp, n, Sb, wave, lane);
}

// ---- column statistics, normalisation, median of 7, head average: one workgroup per (frame tile, clip) ----------------------------------------
// A tile is 58 frames plus a halo of 3 on each side (64 columns; at the two ends of the clip the halo is the reflection, i.e. up to 3 mirrored
// columns are computed again).  Per head: mean and population standard deviation of every column over the n rows (two passes, f64 sums, the
// four row groups of the workgroup combined through LDS); then, 64 rows at a time, W = (P - mean) / std (0 where std == 0) into LDS, the median
// of the 7 columns around each frame, summed over the heads in list order and divided by their number.
constexpr int AF_TILE = 58, AF_EXT = 64, AF_ROWS = 64;

__device__ __forceinline__ void cswap(float& x, float& y) { const float lo = fminf(x, y), hi = fmaxf(x, y); x = lo; y = hi; }
__device__ __forceinline__ float median7(float v0, float v1, float v2, float v3, float v4, float v5, float v6) {
    float v[7] = {v0, v1, v2, v3, v4, v5, v6};
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6 - i; j++) cswap(v[j], v[j + 1]);
    return v[3];
}

__global__ __launch_bounds__(256) void k_align_filter(AlignArgs a) {
    __shared__ float s_mean[WH_MAX_ALIGN_HEADS][AF_EXT], s_std[WH_MAX_ALIGN_HEADS][AF_EXT];
    __shared__ double s_red[4][AF_EXT];
    __shared__ float s_w[AF_ROWS][AF_EXT + 1];
    const int tile = blockIdx.x, cl = blockIdx.y, b = a.clip0 + cl;
    const int n = align_rows(a, b);
    if (n <= 1) return;
    const int Sb = a.sb[b];
    if (tile * AF_TILE >= Sb) return;
    const int tid = threadIdx.x, c = tid & 63, rg = tid >> 6;
    auto reflect = [&](int col) {   // frame of extended column col: numpy's "reflect" padding of 3 (S_b >= 8)
        int s = tile * AF_TILE - 3 + col;
        if (s < 0) s = -s;
        if (s >= Sb) s = 2 * (Sb - 1) - s;
        return min(max(s, 0), Sb - 1);   // (columns past the halo of the last tile: unused)
    };
    const int sr = reflect(c);
    const float* Pc = a.P + (long)cl * a.n_heads * a.cap * a.Sp;
    for (int hd = 0; hd < a.n_heads; hd++) {
        const float* P = Pc + (long)hd * a.cap * a.Sp + sr;
        double acc = 0.0;
        for (int g = rg; g < n; g += 4) acc += (double)P[(long)g * a.Sp];
        s_red[rg][c] = acc;
        __syncthreads();
        const double mean = (s_red[0][c] + s_red[1][c] + s_red[2][c] + s_red[3][c]) / (double)n;
        __syncthreads();
        acc = 0.0;
        for (int g = rg; g < n; g += 4) { const double dlt = (double)P[(long)g * a.Sp] - mean; acc += dlt * dlt; }
        s_red[rg][c] = acc;
        __syncthreads();
        if (rg == 0) {
            s_mean[hd][c] = (float)mean;
            s_std[hd][c] = (float)sqrt((s_red[0][c] + s_red[1][c] + s_red[2][c] + s_red[3][c]) / (double)n);
        }
        __syncthreads();
    }
    float* M = a.M + (long)cl * a.cap * a.Sp;
    for (int g0 = 0; g0 < n; g0 += AF_ROWS) {
        float out[AF_ROWS * AF_EXT / 256];
#pragma unroll
        for (int k = 0; k < AF_ROWS * AF_EXT / 256; k++) out[k] = 0.0f;
        for (int hd = 0; hd < a.n_heads; hd++) {
            const float* P = Pc + (long)hd * a.cap * a.Sp;
            const float mean = s_mean[hd][c], sd = s_std[hd][c];
            __syncthreads();   // the previous head's medians have been taken
#pragma unroll
            for (int k = 0; k < AF_ROWS * AF_EXT / 256; k++) {
                const int row = rg + 4 * k, g = g0 + row;
                float w = 0.0f;
                if (g < n && sd != 0.0f) w = (P[(long)g * a.Sp + sr] - mean) / sd;
                s_w[row][c] = w;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < AF_ROWS * AF_EXT / 256; k++) {
                const int row = rg + 4 * k;
                if (c < AF_TILE)
                    out[k] += median7(s_w[row][c], s_w[row][c + 1], s_w[row][c + 2], s_w[row][c + 3], s_w[row][c + 4], s_w[row][c + 5], s_w[row][c + 6]);
            }
        }
#pragma unroll
        for (int k = 0; k < AF_ROWS * AF_EXT / 256; k++) {
            const int g = g0 + rg + 4 * k, s = tile * AF_TILE + c;
            if (c < AF_TILE && g < n && s < Sb) M[(long)g * a.Sp + s] = out[k] / (float)a.n_heads;
        }
    }
}

// ---- dynamic time warping on x = -M, one workgroup per clip: an anti-diagonal wavefront -------------------------------------------------------
// cost[i][j], 0 <= i <= n, 0 <= j <= S_b; diagonal d = i + j.  Three rolling diagonals indexed by i live in LDS (cap + 1 floats each); a cell
// reads c0 = cost[i-1][j-1] (diagonal d - 2, index i - 1), c1 = cost[i-1][j] (d - 1, i - 1), c2 = cost[i][j-1] (d - 1, i).  The steps go to
// global memory as bytes [cap + 1][S + 1]; one barrier per diagonal.  Lane 0 then walks back from (n, S_b) and leaves in frames[g] the last
// (smallest) frame the path visits in row g.
__global__ __launch_bounds__(512) void k_align_dtw(AlignArgs a) {
    extern __shared__ float diag[];
    const int cl = blockIdx.x, b = a.clip0 + cl, tid = threadIdx.x;
    const int n = align_rows(a, b);
    int* fr = a.frames + (long)b * a.frames_ld;
    if (n <= 1) return;   // (frames are zeroed before the launch)
    const int Sb = a.sb[b], W = a.S + 1, L = a.cap + 1;
    const float* M = a.M + (long)cl * a.cap * a.Sp;
    unsigned char* tr = a.trace + (long)cl * L * W;
    float *p2 = diag, *p1 = diag + L, *cur = diag + 2 * L;
    if (tid == 0) { p2[0] = 0.0f; p1[0] = INFINITY; p1[1] = INFINITY; }
    __syncthreads();
    for (int d = 2; d <= n + Sb; d++) {
        const int ilo = max(1, d - Sb), ihi = min(n, d - 1);
        for (int i = ilo + tid; i <= ihi; i += blockDim.x) {
            const int j = d - i;
            const float x = -M[(long)(i - 1) * a.Sp + (j - 1)];
            const float c0 = p2[i - 1], c1 = p1[i - 1], c2 = p1[i];
            float cmin;
            unsigned char step;
            if (c0 < c1 && c0 < c2) { cmin = c0; step = 0; }
            else if (c1 < c0 && c1 < c2) { cmin = c1; step = 1; }
            else { cmin = c2; step = 2; }
            cur[i] = x + cmin;
            tr[(long)i * W + j] = step;
        }
        if (tid == 0) {
            cur[0] = INFINITY;              // cost[0][d]
            if (d <= n) cur[d] = INFINITY;  // cost[d][0]
        }
        __syncthreads();
        float* t = p2; p2 = p1; p1 = cur; cur = t;
    }
    if (tid == 0) {
        int i = n, j = Sb;
        for (int guard = 0; (i > 0 || j > 0) && guard < n + Sb + 2; guard++) {
            if (i > 0 && j > 0) fr[i - 1] = j - 1;
            const int step = i == 0 ? 2 : j == 0 ? 1 : tr[(long)i * W + j];
            if (step == 0) { i--; j--; }
            else if (step == 1) i--;
            else j--;
        }
    }
}

}  // namespace

void wh_launch_align_copy(hipStream_t s, bool src_bf16, const void* src, long row_pitch, long head_pitch, int dk, const AlignLayerHeads& hs, const int* pos_p,
                          int first_emit, int cap, int nb, float* dst) {
    if (hs.n <= 0) return;
    if (src_bf16) hipLaunchKernelGGL(k_align_copy<bf16>, dim3(nb, hs.n), dim3(64), 0, s, (const bf16*)src, row_pitch, head_pitch, dk, hs, pos_p, first_emit, cap, nb, dst);
    else hipLaunchKernelGGL(k_align_copy<float>, dim3(nb, hs.n), dim3(64), 0, s, (const float*)src, row_pitch, head_pitch, dk, hs, pos_p, first_emit, cap, nb, dst);
}

void wh_launch_align_gather(hipStream_t s, bool src_bf16, const void* src, long row_pitch, long head_pitch, int dk, const AlignLayerHeads& hs, int rows, int T,
                            int P, int Lmax, const int* len, int G, float* dst) {
    if (hs.n <= 0 || rows <= 0) return;
    const long e = src_bf16 ? 8 : 4;   // elements in 16 source bytes
    const bool vec = row_pitch % e == 0 && head_pitch % e == 0 && dk % 8 == 0 && (uintptr_t)src % 16 == 0 && (uintptr_t)dst % 16 == 0;
    const dim3 grid(rows, hs.n);
#define GATHER(TY, V) hipLaunchKernelGGL((k_align_gather<TY, V>), grid, dim3(64), 0, s, (const TY*)src, row_pitch, head_pitch, dk, hs, rows, T, P, Lmax, len, G, dst)
    if (src_bf16) { if (vec) GATHER(bf16, true); else GATHER(bf16, false); }
    else { if (vec) GATHER(float, true); else GATHER(float, false); }
#undef GATHER
}

bool wh_align_scores_supported(int form, int dk) { return form == WH_ALIGN_ES_BF16 ? dk == 512 : dk == WH_HEAD_DIM; }

int wh_launch_align_scores(hipStream_t s, int form, const AlignArgs& a, int n_clips) {
    const dim3 grid(a.n_heads, n_clips);
    if (form == WH_ALIGN_KV_F32) hipLaunchKernelGGL(k_align_scores_f32, grid, dim3(256), 0, s, a);
    else if (form == WH_ALIGN_KV_BF16) hipLaunchKernelGGL((k_align_scores_bf16<WH_HEAD_DIM, false>), grid, dim3(256), 0, s, a);
    else if (form == WH_ALIGN_ES_BF16 && a.dk == 512) hipLaunchKernelGGL((k_align_scores_bf16<512, true>), grid, dim3(256), 0, s, a);
    else {   // (align_check refuses such a context before anything is launched: wh_align_scores_supported)
        wh_set_error("alignment scores: no kernel for form %d with %d-wide keys", form, a.dk);
        return WH_ERR_UNSUPPORTED;
    }
    return WH_OK;
}

void wh_launch_align_filter(hipStream_t s, const AlignArgs& a, int n_clips) {
    hipLaunchKernelGGL(k_align_filter, dim3((a.S + AF_TILE - 1) / AF_TILE, n_clips), dim3(256), 0, s, a);
}

void wh_launch_align_dtw(hipStream_t s, const AlignArgs& a, int n_clips) {
    const int threads = std::min(512, std::max(64, (a.cap + 63) / 64 * 64));
    hipLaunchKernelGGL(k_align_dtw, dim3(n_clips), dim3(threads), 3 * (size_t)(a.cap + 1) * sizeof(float), s, a);
}
