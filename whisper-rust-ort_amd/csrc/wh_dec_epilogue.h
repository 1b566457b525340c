// wh_dec_epilogue.h — what the decode GEMM kernels share around their epilogues: k_dec_gemm and k_dec_gemm_wide (wh_dec_gemm.hip; bit-identical
// to each other) and k_dec_tile (wh_dec_tile.hip; its own accumulation order).  The contract of all three is
//
//   C[m][n] = act( LN-fold( sum_k X[m][k] W[n][k] ) * wscale[n] + bias[n] ) (+ R[m][n])
//
// and, for the producer of the next LayerNorm's input, the raw slab copy (C - row_shift[m]) * xgamma[n] with the per-16-column {sum, sum of
// squares} of C - row_shift[m]; for the consumer of a LayerNorm the shift_io update; the grouped-launch offsets; the position ticket.
// tools/dec_gemm_check.cpp holds each of the three kernels to a double-precision host restatement of that contract, and k_dec_gemm_wide
// to k_dec_gemm bit for bit.
//
// Shared here: the position ticket, the slab index, the grouped-launch offsets and the LDS carve of the two K-split kernels; the LayerNorm
// row-statistics reduce is ln_part_store / ln_row_stats (wh_common.h).  NOT shared: the per-lane finish (scale, fold, GELU, residual, the
// two stores) and the statistics partial.  Each kernel keeps its own text of those, because every shared form that was tried — operand
// structs passed by reference, plain f32x4 values, with and without the statistics — changed the instruction stream of all 156
// instantiations of the two K-split kernels and cost 0.4 to 1.4 % per launch (2.943 -> 2.968 us at 64 x 1536 x 512, 5.621 -> 5.699 us at
// 256 x 512 x 2048), and in k_dec_tile 7 % (12.13 -> 13.05 us at 2048 x 1536 x 512).  With what is shared here the generated code of every
// instantiation is instruction for instruction what the kernels' own text gave, except the 48-row (MT = 3) forms, whose LayerNorm
// prologue is scheduled three instructions longer.  k_dec_tile also keeps its own group offsets and ticket: through dec_gemm_group and
// advance_if_last its register allocation changes.
#pragma once
#include "wh_common.h"
#include "wh_kernels.h"

// One workgroup arrives; the last one of the grid bumps *pos (every workgroup read *pos at its
// start, so nobody can observe the new value within this launch) and re-arms the ticket.
// n_blocks: the caller's workgroup count (tickets are only used with SkinnyArgs::zn == 1)
__device__ __forceinline__ void advance_if_last(int* ticket, int* pos_p, int n_blocks) {
    if (!ticket) return;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int t = atomicAdd(ticket, 1);
        if (t == n_blocks - 1) {
            *ticket = 0;
            *pos_p += 1;
        }
    }
}

// ---- decode activation layout ("k-slab major") ------------------------------------------------
// Activations that feed a decode GEMM are stored [K/32][Mpad][32]: the 32-deep k-slab of 16
// consecutive rows is one contiguous 1 KiB block, so the MFMA column-operand load of a wave (lane
// (row fl, group fg) reads 8 consecutive k of row 16t+fl) is a single fully coalesced access — the
// same shape as the weight-fragment loads — instead of 16 rows x 64 B scattered over a row-major
// [M][K] buffer.  Producers (LayerNorm, attention, fc1 epilogue) write this layout directly.
__device__ __forceinline__ long slab_idx(int m, int k, int mpad) { return ((long)(k >> 5) * mpad + m) * 32 + (k & 31); }

// Token + position embedding of row b's NEXT position by a 256-thread workgroup (k_dec_embed's work, fused into the kernel that chooses the
// token: k_argmax_finish, k_beam_select): the f32 residual row, the slab copy and the row sums, with the row's mean first (k_dec_embed's
// two passes: the slab copy and the sums are of the centred row).  sv: 12 floats of LDS nobody else uses until the call returns; every
// thread of the workgroup calls it (barriers inside).  Thread 0 still reads sv when the call returns: a caller that calls it again, or reuses
// sv, puts a __syncthreads() in between (k_beam_select's loop over a clip's rows).  The term order of the sums is fixed: a row's values do not depend on the caller.
template <typename T>
__device__ __forceinline__ void embed_next_row(const NextEmbed& ne, int b, int next, int mpos, float* sv) {
    const int tid = threadIdx.x;
    const T* er = (const T*)ne.tok_emb + (long)next * ne.d;
    const float* pr = ne.pos_emb + (long)mpos * ne.d;
    float mean = 0.0f;
    if (ne.shift) {
        float s0 = 0.0f;
        for (int c = tid * 4; c < ne.d; c += 1024) {
            const f32x4 v = load4_f32(er + c) + *reinterpret_cast<const f32x4*>(pr + c);
            s0 += (v[0] + v[1]) + (v[2] + v[3]);
        }
        s0 = dpp_wave_sum(s0);
        if ((tid & 63) == 0) sv[8 + (tid >> 6)] = s0;
        __syncthreads();
        mean = ((sv[8] + sv[9]) + (sv[10] + sv[11])) / (float)ne.d;
    }
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = tid * 4; c < ne.d; c += 1024) {
        const f32x4 p4 = *reinterpret_cast<const f32x4*>(pr + c);
        f32x4 v = load4_f32(er + c) + p4;
        *reinterpret_cast<f32x4*>(ne.x + (long)b * ne.d + c) = v;
        v -= mean;
        f32x4 g = {1, 1, 1, 1};
        if (ne.xgamma) g = *reinterpret_cast<const f32x4*>(ne.xgamma + c);
        store4((T*)ne.xslab + slab_idx(b, c, ne.mpad), v[0] * g[0], v[1] * g[1], v[2] * g[2], v[3] * g[3]);
        s1 += (v[0] + v[1]) + (v[2] + v[3]);
        s2 += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
    }
    s1 = dpp_wave_sum(s1);
    s2 = dpp_wave_sum(s2);
    if ((tid & 63) == 0) { sv[tid >> 6] = s1; sv[4 + (tid >> 6)] = s2; }
    __syncthreads();
    if (tid == 0) {
        ne.stats[2 * b] = (sv[0] + sv[1]) + (sv[2] + sv[3]);
        ne.stats[2 * b + 1] = (sv[4] + sv[5]) + (sv[6] + sv[7]);
        if (ne.shift) ne.shift[b] = mean;
    }
}

// grouped launches (SkinnyArgs::zn): group blockIdx.z works on its own X, W, bias and C (a slab: type T, else row-major TO)
template <typename T, typename TO, typename TW>
__device__ __forceinline__ void dec_gemm_group(SkinnyArgs& a) {
    const long z = blockIdx.z;
    if (z == 0) return;
    a.X = (const T*)a.X + z * a.x_zs;
    a.W = (const TW*)a.W + z * a.w_zs;
    a.C = a.c_mpad ? (void*)((T*)a.C + z * a.c_zs) : (void*)((TO*)a.C + z * a.c_zs);
    if (a.bias) a.bias += z * a.bias_zs;
}

// LDS of k_dec_gemm / k_dec_gemm_wide, read by the kernels and by their launcher: the waves' partial sums [NW][TILES][64] f32x4, then the
// LayerNorm quarter sums [4][MT * 16][2] (ln_part_store / ln_row_stats); k_dec_gemm's merged-X tile follows at BYTES.
template <int NW, int MT, int TILES>
struct DecGemmLds {
    static constexpr size_t RED = (size_t)NW * TILES * 64 * 16, BYTES = RED + (size_t)4 * MT * 16 * 2 * 4;
    static __device__ __forceinline__ f32x4* red(char* smem) { return reinterpret_cast<f32x4*>(smem); }
    static __device__ __forceinline__ float* lnq(char* smem) { return reinterpret_cast<float*>(smem) + RED / 4; }
};
