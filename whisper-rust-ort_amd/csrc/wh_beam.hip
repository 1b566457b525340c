// wh_beam.hip — beam search in the token loop (wh_ctx_set_beam_search).  A clip's K beams are the batch rows clip * K + j: the
// decoder layers and the LM head run on them as on any rows and leave the current position's raw logits in a [rows][vocab] scratch.
//   k_beam_select   one workgroup per clip: masks, rule ranges, log-softmax and the top K + 1 of every row, the walk over the K (K + 1)
//                   candidates, the new scores / parents / rule states, the pool, the trace, and the next position's embedding of the K rows.
//   k_beam_reorder  dst[j] = src[parent[j]] over the self-attention K and V caches of a clip's rows; advances the position.
// Histories are not moved on the device: every position's (parent, token, lp) of every row is kept (the trace), a pool entry names the position
// and the parent it ends, and the host walks the parents back at read-back.
#include "wh_common.h"
#include "wh_dec_epilogue.h"
#include "wh_kernels.h"

namespace {

constexpr int KMAX = WH_MAX_BEAMS, NC = WH_MAX_BEAMS + 1;

// candidate order inside a row: value descending, then id ascending
__device__ __forceinline__ bool cand_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }
__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (cand_before(ov, oi, v, i)) { v = ov; i = oi; }
    }
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One pass of a wave over ids [lo, hi) of a row, eight loads in flight per lane: f(value, id) for every id in range.
template <typename F>
__device__ __forceinline__ void scan_row(const float* __restrict__ row, int lo, int hi, int lane, F&& f) {
    for (int i0 = lo + lane; i0 < hi; i0 += 64 * 8) {
        float x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = (i0 + 64 * u < hi) ? row[i0 + 64 * u] : 0.0f;
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (i0 + 64 * u < hi) f(x[u], i0 + 64 * u);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_beam_select(BeamArgs a, NextEmbed ne) {
    __shared__ float sv[16];
    __shared__ float c_lp[KMAX][NC], s_old[KMAX], n_score[KMAX], n_lp[KMAX];
    __shared__ int c_id[KMAX][NC], c_n[KMAX], c_h[KMAX], st_old[KMAX][WH_BEAM_STATE], n_parent[KMAX], n_tok[KMAX], s_complete;
    const int clip = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = a.K, V = a.vocab, r0 = clip * K;
    const int pos = *a.pos_p, gen = pos - (a.n_prompt - 1);
    if (gen < 0) return;
    if (a.done[r0]) {   // a complete clip: nothing more of it is recorded; its rows keep running and are fed the stop token, so their values stay bounded
        const int stop = a.eot >= 0 && a.eot < V ? a.eot : 0;
        for (int j = 0; j < K; j++) {
            embed_next_row<T>(ne, r0 + j, stop, pos + 1, sv);
            __syncthreads();   // (sv is read by thread 0 at the end of a call)
        }
        return;
    }
    const bool rules = a.ts_begin >= 0;
    const int tb = rules ? a.ts_begin : V;
    const unsigned* mask = gen == 0 ? a.mask_first : a.mask_base;
    if (tid < K) {
        s_old[tid] = gen == 0 ? (tid == 0 ? 0.0f : -INFINITY) : a.scores[r0 + tid];
        for (int e = 0; e < WH_BEAM_STATE; e++) st_old[tid][e] = a.state[(long)(r0 + tid) * WH_BEAM_STATE + e];
        c_n[tid] = 0;
        c_h[tid] = 0;
    }
    __syncthreads();
    // ---- per row (a wave owns rows wave, wave + 4): the allowed set, (max, sum of exp), the top K + 1 ----
    for (int j = wave; j < K; j += 4) {
        const int r = r0 + j;
        const float* row = a.logits + (long)r * V;
        if (a.logits_out && gen < a.logits_rows) {   // parity harness: this row's raw logits of this position
            const int slot = a.logits_sel ? a.logits_sel[r] : r;
            if (slot >= 0) {
                float* dst = a.logits_out + ((long)slot * a.logits_rows + gen) * V;
                scan_row(row, 0, V, lane, [&](float x, int i) { dst[i] = x; });
            }
        }
        if (!(s_old[j] > -INFINITY)) continue;   // a dead beam: none of its candidates is ever taken
        int text_lo = 0, ts_lo = V, ts_hi = V - 1;
        if (rules) {
            if (gen == 0) ts_ranges(nullptr, 0, 0, tb, a.ts_max_init, V, text_lo, ts_lo, ts_hi);   // rule 4
            else { text_lo = st_old[j][0]; ts_lo = st_old[j][1]; ts_hi = st_old[j][2]; }
        }
        // (NaN: not greater; -inf adds nothing and is no candidate)
#define BEAM_OK(x, i) (((i) < tb ? (i) >= text_lo : ((i) >= ts_lo && (i) <= ts_hi)) && !((mask[(i) >> 5] >> ((i) & 31)) & 1u) && (x) > -INFINITY)
        // pass A: the best allowed text id and the best allowed timestamp
        float tv = -INFINITY, sv_ = -INFINITY;
        int ti = 0x7fffffff, si_ = 0x7fffffff;
        scan_row(row, 0, V, lane, [&](float x, int i) {
            if (!BEAM_OK(x, i)) return;
            if (i < tb) { if (cand_before(x, i, tv, ti)) { tv = x; ti = i; } }
            else if (cand_before(x, i, sv_, si_)) { sv_ = x; si_ = i; }
        });
        wave_best(tv, ti);
        wave_best(sv_, si_);
        if (rules && sv_ > -INFINITY) {   // rule 5: the allowed timestamps' log-sum-exp against the best allowed text logit
            float ts_sum = 0.0f;
            scan_row(row, max(ts_lo, tb), min(ts_hi + 1, V), lane, [&](float x, int i) { if (BEAM_OK(x, i)) ts_sum += expf(x - sv_); });
            ts_sum = wave_sum(ts_sum);
            if (sv_ + logf(ts_sum) > tv) { text_lo = tb; tv = -INFINITY; ti = 0x7fffffff; }
        }
        float bv = tv;
        int bi = ti;
        if (cand_before(sv_, si_, bv, bi)) { bv = sv_; bi = si_; }
        if (!(bv > -INFINITY)) continue;   // nothing allowed: no candidate
        const float m = bv;
        // pass B: the sum of exp over the allowed ids, and this lane's best NC ids of its share of the row as a sorted list in registers
        // (an id enters at the tail when it beats the tail and bubbles up; every index is static).  The row's top K + 1 are then merged out of
        // the 64 lists with one wave reduction per candidate: the lane whose head won pops it.
        float sum = 0.0f, lv[NC];
        int li[NC];
#pragma unroll
        for (int q = 0; q < NC; q++) { lv[q] = -INFINITY; li[q] = 0x7fffffff; }
        scan_row(row, 0, V, lane, [&](float x, int i) {
            if (!BEAM_OK(x, i)) return;
            sum += expf(x - m);
            if (!cand_before(x, i, lv[NC - 1], li[NC - 1])) return;
            lv[NC - 1] = x;
            li[NC - 1] = i;
#pragma unroll
            for (int q = NC - 1; q > 0; q--) {
                const bool up = cand_before(lv[q], li[q], lv[q - 1], li[q - 1]);
                const float tv2 = lv[q - 1];
                const int ti2 = li[q - 1];
                lv[q - 1] = up ? lv[q] : tv2; li[q - 1] = up ? li[q] : ti2;
                lv[q] = up ? tv2 : lv[q]; li[q] = up ? ti2 : li[q];
            }
        });
        sum = wave_sum(sum);
        const float lse = m + logf(sum);
        int n = 0;
        for (int cnum = 0; cnum <= K; cnum++) {
            float hv = lv[0];
            int hi = li[0];
            wave_best(hv, hi);
            if (!(hv > -INFINITY)) break;
            if (lane == 0) { c_lp[j][cnum] = hv; c_id[j][cnum] = hi; }   // (the raw logit for now)
            n = cnum + 1;
            if (li[0] == hi) {   // ids are unique: exactly one lane pops
#pragma unroll
                for (int q = 0; q + 1 < NC; q++) { lv[q] = lv[q + 1]; li[q] = li[q + 1]; }
                lv[NC - 1] = -INFINITY;
                li[NC - 1] = 0x7fffffff;
            }
        }
        if (lane == 0) {
            for (int q = 0; q < n; q++) c_lp[j][q] = c_lp[j][q] - lse;
            c_n[j] = n;
        }
#undef BEAM_OK
    }
    __syncthreads();
    // ---- the walk: candidates by score descending, then beam, then id ----
    if (tid == 0) {
        int nl = 0, pn = a.pool_n[clip];
        if (gen == 0) pn = 0;
        while (nl < K) {
            int bj = -1;
            float bs = -INFINITY;
            for (int j = 0; j < K; j++) {
                if (c_h[j] >= c_n[j]) continue;
                const float sc = s_old[j] + c_lp[j][c_h[j]];
                if (!(sc > -INFINITY)) { c_h[j] = c_n[j]; continue; }   // -inf or NaN: no candidate, and none after it in this row
                if (bj < 0 || sc > bs) { bj = j; bs = sc; }
            }
            if (bj < 0) break;
            const int q = c_h[bj]++;
            const int id = c_id[bj][q];
            if (id == a.eot) {
                if (pn < a.C) {
                    int* pe = a.pool + ((long)clip * WH_MAX_BEAM_CANDIDATES + pn) * 4;
                    pe[0] = gen; pe[1] = bj; pe[2] = __float_as_int(bs); pe[3] = __float_as_int(c_lp[bj][q]);
                    pn++;
                }
            } else {
                n_parent[nl] = bj; n_tok[nl] = id; n_score[nl] = bs; n_lp[nl] = c_lp[bj][q];
                nl++;
            }
        }
        for (; nl < K; nl++) { n_parent[nl] = nl; n_tok[nl] = -1; n_score[nl] = -INFINITY; n_lp[nl] = 0.0f; }
        a.pool_n[clip] = pn;
        a.n_steps[clip] = gen + 1;
        a.tr_pool[(long)gen * a.rows_ld + clip] = pn;
        s_complete = pn >= a.C;
    }
    __syncthreads();
    if (tid < K) {
        const int r = r0 + tid, p = n_parent[tid], tok = n_tok[tid];
        int* st = a.state + (long)r * WH_BEAM_STATE;
        if (tok >= 0) {
            int text_lo = 0, ts_lo = V, ts_hi = V - 1, last_t = -1;
            if (rules) {
                const bool pen_ts = gen == 0 || st_old[p][4] >= tb;   // (the parent's last token is seq[-2])
                ts_next_state(tok, pen_ts, gen == 0 ? -1 : st_old[p][3], tb, a.eot, V, text_lo, ts_lo, ts_hi, last_t);
            }
            st[0] = text_lo; st[1] = ts_lo; st[2] = ts_hi; st[3] = last_t; st[4] = tok; st[5] = gen + 1;
        }
        a.scores[r] = n_score[tid];
        a.parent[r] = p;
        const long t = (long)gen * a.rows_ld + r;
        a.tr_parent[t] = p; a.tr_token[t] = tok; a.tr_score[t] = n_score[tid]; a.tr_lp[t] = n_lp[tid];
        if (pos + 1 < a.tok_ld) a.feed[(long)r * a.tok_ld + pos + 1] = tok >= 0 ? tok : 0;
        if (s_complete) a.done[r] = 1;
    }
    // ---- the next position's embedding of the K rows (a dead beam is fed id 0: its row keeps running) ----
    for (int j = 0; j < K; j++) {
        const int tok = n_tok[j];
        embed_next_row<T>(ne, r0 + j, tok >= 0 ? tok : 0, pos + 1, sv);
        __syncthreads();   // (sv is read by thread 0 at the end of a call)
    }
}

// One thread owns one 16-byte element offset of the [tc][64] plane of a (layer, head): it loads that element from the K rows of the clip, then
// stores dst[j] = src[parent[j]].  The parents are wave-uniform, so the source is chosen by K scalar branches per destination around a store of a
// statically indexed register (a select chain over the K values was turned back into a dynamically indexed array in scratch by the compiler).
// No two threads touch the same address.
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
template <int K>
__global__ __launch_bounds__(256) void k_beam_reorder(u32x4* __restrict__ kc, u32x4* __restrict__ vc, const int* __restrict__ parent, const int* __restrict__ done,
                                                      int n_heads, long plane16, int row16, long layer16, int* pos_p, int* ticket) {
    const int clip = blockIdx.z, layer = blockIdx.y / n_heads, head = blockIdx.y % n_heads, tid = threadIdx.x;
    const int pos = *pos_p, r0 = clip * K;
    int par[K];
    bool ident = true;
#pragma unroll
    for (int j = 0; j < K; j++) {
        par[j] = min(max(parent[r0 + j], 0), K - 1);
        ident = ident && par[j] == j;
    }
    if (!ident && !done[r0]) {
        const long n16 = (long)(pos + 1) * row16;   // positions 0 .. pos: <= plane16
        const long base = layer * layer16 + ((long)r0 * n_heads + head) * plane16, rstep = (long)n_heads * plane16;
        for (long e = (long)blockIdx.x * 256 + tid; e < n16; e += (long)gridDim.x * 256) {
            u32x4 kv[K], vv[K];
#pragma unroll
            for (int j = 0; j < K; j++) { kv[j] = kc[base + j * rstep + e]; vv[j] = vc[base + j * rstep + e]; }
#pragma unroll
            for (int j = 0; j < K; j++) {
#pragma unroll
                for (int q = 0; q < K; q++)
                    if (q != j && par[j] == q) { kc[base + j * rstep + e] = kv[q]; vc[base + j * rstep + e] = vv[q]; }
            }
        }
    }
    advance_if_last(ticket, pos_p, gridDim.x * gridDim.y * gridDim.z);
}

template <int K>
void launch_reorder(hipStream_t s, dim3 grid, u32x4* kc, u32x4* vc, const int* parent, const int* done, int want, int n_heads, long plane16, int row16, long layer16,
                    int* pos_p, int* ticket) {
    if constexpr (K < WH_MAX_BEAMS) {
        if (want > K) return launch_reorder<K + 1>(s, grid, kc, vc, parent, done, want, n_heads, plane16, row16, layer16, pos_p, ticket);
    }
    hipLaunchKernelGGL(k_beam_reorder<K>, grid, dim3(256), 0, s, kc, vc, parent, done, n_heads, plane16, row16, layer16, pos_p, ticket);
}

}  // namespace

void wh_launch_beam_select(hipStream_t s, int prec, const BeamArgs& a, const NextEmbed& ne) {
    if (prec == WH_PREC_F32) hipLaunchKernelGGL(k_beam_select<float>, dim3(a.n_clips), dim3(256), 0, s, a, ne);
    else hipLaunchKernelGGL(k_beam_select<bf16>, dim3(a.n_clips), dim3(256), 0, s, a, ne);
}

void wh_launch_beam_reorder(hipStream_t s, int esz, void* kc, void* vc, const int* parent, const int* done, int K, int n_clips, int layers, int n_heads, int tc,
                            int* pos_p, int* ticket) {
    const int row16 = WH_HEAD_DIM * esz / 16;
    const long plane16 = (long)tc * row16, layer16 = (long)n_clips * K * n_heads * plane16;
    // two workgroups per (clip, layer, head): 512 threads cover 64 (bf16) or 32 (f32) positions per sweep
    launch_reorder<1>(s, dim3(2, layers * n_heads, n_clips), (u32x4*)kc, (u32x4*)vc, parent, done, K, n_heads, plane16, row16, layer16, pos_p, ticket);
}
