// wh_sample.hip — temperature sampling in the token loop (wh_ctx_set_sampling).  The LM head leaves the current position's raw
// logits in a [rows][vocab] scratch (SkinnyArgs::logits_cur, the route beam search opened); its argmax partials are not read.
//   k_sample_select  one 256-thread workgroup per batch row: the allowed set (suppress masks, timestamp rules 1-5), the row's log-sum-exp, the
//                    Gumbel-max draw at the row's temperature (plain argmax at T = 0), then k_argmax_finish's bookkeeping — record the token and
//                    its log-probability, EOT / forced handling, the next position's rule state, feed, embedding — and the position ticket.
// A workgroup per row, not a wave per row: embed_next_row is written for a 256-thread workgroup that owns the row, and four waves on one row
// keep 512 sixteen-byte loads of it in flight; at 2048 rows all 2048 workgroups are resident at once (8 per CU, 32 waves per CU).
// The draw of an id depends on (seed, row id, position, id) only — Philox4x32-10, one block per four consecutive ids — so the walk is over
// id-aligned groups of four (16-byte loads at 4-byte alignment: a row's pitch is vocab * 4 bytes, odd vocabularies included), and no result
// depends on the reduction order but the sums of exp.
#include "wh_common.h"
#include "wh_dec_epilogue.h"
#include "wh_kernels.h"

namespace {

typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

// candidate order: value descending, then id ascending
__device__ __forceinline__ bool cand_before(float v, int i, float bv, int bi) { return v > bv || (v == bv && i < bi); }

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c, key k -> four words
__device__ __forceinline__ void philox4x32_10(unsigned& c0, unsigned& c1, unsigned& c2, unsigned& c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// u = ((x >> 9) + 0.5) * 2^-23: exact in f32, strictly inside (0, 1); the Gumbel score -log(-log u) on the accurate logf
__device__ __forceinline__ float gumbel_of(unsigned x) {
    const float u = ((float)(x >> 9) + 0.5f) * 1.1920928955078125e-07f;
    return -logf(-logf(u));
}

// f(value, id, word) for every id of [lo, hi) of a row, the workgroup's threads over id-aligned groups of four, two groups in flight per
// thread; g4(first id of the group) runs once per group before its four values and returns the group's four words.  A thread's ids ascend.
struct Words4 { unsigned w0, w1, w2, w3; };
template <typename G, typename F>
__device__ __forceinline__ void scan_row4(const float* __restrict__ row, int lo, int hi, int tid, G&& g4, F&& f) {
    const int g_lo = lo >> 2, g_hi = (hi + 3) >> 2;   // groups [g_lo, g_hi)
    for (int g0 = g_lo + tid; g0 < g_hi; g0 += 512) {
        const int ia = g0 * 4, ib = (g0 + 256) * 4;
        const bool hb = g0 + 256 < g_hi;
        float a0 = 0, a1 = 0, a2 = 0, a3 = 0, b0 = 0, b1 = 0, b2 = 0, b3 = 0;
        if (ia >= lo && ia + 4 <= hi) {
            const f32x4u x = *reinterpret_cast<const f32x4u*>(row + ia);
            a0 = x[0]; a1 = x[1]; a2 = x[2]; a3 = x[3];
        } else {   // the range's ragged first / last group: element loads inside [lo, hi)
            if (ia >= lo && ia < hi) a0 = row[ia];
            if (ia + 1 >= lo && ia + 1 < hi) a1 = row[ia + 1];
            if (ia + 2 >= lo && ia + 2 < hi) a2 = row[ia + 2];
            if (ia + 3 >= lo && ia + 3 < hi) a3 = row[ia + 3];
        }
        if (hb) {
            if (ib >= lo && ib + 4 <= hi) {
                const f32x4u x = *reinterpret_cast<const f32x4u*>(row + ib);
                b0 = x[0]; b1 = x[1]; b2 = x[2]; b3 = x[3];
            } else {
                if (ib >= lo && ib < hi) b0 = row[ib];
                if (ib + 1 >= lo && ib + 1 < hi) b1 = row[ib + 1];
                if (ib + 2 >= lo && ib + 2 < hi) b2 = row[ib + 2];
                if (ib + 3 >= lo && ib + 3 < hi) b3 = row[ib + 3];
            }
        }
        {
            const Words4 w = g4(ia);
            if (ia >= lo && ia < hi) f(a0, ia, w.w0);
            if (ia + 1 >= lo && ia + 1 < hi) f(a1, ia + 1, w.w1);
            if (ia + 2 >= lo && ia + 2 < hi) f(a2, ia + 2, w.w2);
            if (ia + 3 >= lo && ia + 3 < hi) f(a3, ia + 3, w.w3);
        }
        if (hb) {
            const Words4 w = g4(ib);
            if (ib >= lo && ib < hi) f(b0, ib, w.w0);
            if (ib + 1 >= lo && ib + 1 < hi) f(b1, ib + 1, w.w1);
            if (ib + 2 >= lo && ib + 2 < hi) f(b2, ib + 2, w.w2);
            if (ib + 3 >= lo && ib + 3 < hi) f(b3, ib + 3, w.w3);
        }
    }
}

__device__ __forceinline__ void wave_best(float& v, int& i, float& w) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(v, off, 64), ow = __shfl_xor(w, off, 64);
        const int oi = __shfl_xor(i, off, 64);
        if (cand_before(ov, oi, v, i)) { v = ov; i = oi; w = ow; }
    }
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// the workgroup's best (value, id, payload) and, for sums, the four waves' totals in a fixed order; sb: 16 words of LDS
__device__ __forceinline__ void block_best(float& v, int& i, float& w, float* sb, int tid) {
    wave_best(v, i, w);
    __syncthreads();   // (sb may still be read from the previous reduce)
    if ((tid & 63) == 0) { sb[tid >> 6] = v; sb[4 + (tid >> 6)] = __int_as_float(i); sb[8 + (tid >> 6)] = w; }
    __syncthreads();
    v = sb[0]; i = __float_as_int(sb[4]); w = sb[8];
#pragma unroll
    for (int q = 1; q < 4; q++)
        if (cand_before(sb[q], __float_as_int(sb[4 + q]), v, i)) { v = sb[q]; i = __float_as_int(sb[4 + q]); w = sb[8 + q]; }
}
__device__ __forceinline__ float block_sum(float v, float* sb, int tid) {
    v = wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) sb[12 + (tid >> 6)] = v;
    __syncthreads();
    return (sb[12] + sb[13]) + (sb[14] + sb[15]);
}

template <typename T>
__global__ __launch_bounds__(256) void k_sample_select(SampleArgs a, DecodeState st, NextEmbed ne, int* pos_p, int* ticket) {
    __shared__ float sv[16];
    __shared__ float sb[16];
    __shared__ int s_next;
    const int b = blockIdx.x, tid = threadIdx.x, V = a.vocab;
    const int pos = *pos_p, gen = pos - (st.n_prompt - 1);
    int mpos = pos + 1;   // the row's next model position (per-clip prefixes: DESIGN.md §5j)
    if (ne.off) mpos = max(pos + 1 - max(ne.off[b], 0), 0);
    if (gen < 0 || st.done[b]) {
        // a done row (an inactive one from the start): nothing more of it is recorded; it keeps running on the stop token, so its values stay bounded
        const int stop = st.eot >= 0 && st.eot < V ? st.eot : 0;
        if (tid == 0 && pos + 1 < st.tok_ld) st.feed[b * st.tok_ld + pos + 1] = stop;
        embed_next_row<T>(ne, b, stop, mpos, sv);
        advance_if_last(ticket, pos_p, gridDim.x);
        return;
    }
    const float* row = a.logits + (long)b * V;
    if (a.logits_out && gen < a.logits_rows) {   // parity harness: this row's raw logits of this position
        const int slot = a.logits_sel ? a.logits_sel[b] : b;
        if (slot >= 0) {
            float* dst = a.logits_out + ((long)slot * a.logits_rows + gen) * V;
            for (int i = tid; i < V; i += 256) dst[i] = row[i];
        }
    }
    const bool rules = a.ts_begin >= 0;
    const int tb = rules ? a.ts_begin : V;
    const unsigned* mask = gen == 0 ? a.mask_first : a.mask_base;
    int text_lo = 0, ts_lo = V, ts_hi = V - 1;
    if (rules) ts_ranges(a.ts_state, b, gen, tb, a.ts_max_init, V, text_lo, ts_lo, ts_hi);
    // (NaN: not greater; -inf adds nothing and never wins)
#define SAMPLE_OK(x, i) (((i) < tb ? (i) >= text_lo : ((i) >= ts_lo && (i) <= ts_hi)) && !((mask[(i) >> 5] >> ((i) & 31)) & 1u) && (x) > -INFINITY)
    // ---- pass 1: the best allowed text id and the best allowed timestamp (rule 5, and m) ----
    float tv = -INFINITY, sv_ = -INFINITY, dummy = 0.0f;
    int ti = 0x7fffffff, si_ = 0x7fffffff;
    scan_row4(row, 0, V, tid, [](int) { return Words4{0, 0, 0, 0}; }, [&](float x, int i, unsigned) {
        // (selects, not branches: an if / else over the two running pairs was compiled into a dynamically indexed array in scratch)
        const bool ok = SAMPLE_OK(x, i), take_t = ok && i < tb && cand_before(x, i, tv, ti), take_s = ok && i >= tb && cand_before(x, i, sv_, si_);
        tv = take_t ? x : tv; ti = take_t ? i : ti;
        sv_ = take_s ? x : sv_; si_ = take_s ? i : si_;
    });
    block_best(tv, ti, dummy, sb, tid);
    if (rules) {
        block_best(sv_, si_, dummy, sb, tid);
        if (sv_ > -INFINITY) {   // rule 5: the allowed timestamps' log-sum-exp against the best allowed text logit (a walk over the timestamp range only)
            float ts_sum = 0.0f;
            scan_row4(row, max(ts_lo, tb), min(ts_hi + 1, V), tid, [](int) { return Words4{0, 0, 0, 0}; }, [&](float x, int i, unsigned) { if (SAMPLE_OK(x, i)) ts_sum += expf(x - sv_); });
            ts_sum = block_sum(ts_sum, sb, tid);
            if (sv_ + logf(ts_sum) > tv) { text_lo = tb; tv = -INFINITY; ti = 0x7fffffff; }
        }
    }
    const float m = fmaxf(tv, sv_);   // the largest allowed logit (-inf: nothing is allowed)
    // ---- pass 2: the sum of exp over the allowed ids and the running argmax of z + gum (v at T = 0), over the ids that can be allowed ----
    const float temp = a.temperature[b];
    const bool draw = temp > 0.0f;
    const float invT = draw ? 1.0f / temp : 1.0f;
    const unsigned long long seed = *a.seed, rid = a.row_ids[b];
    float sum = 0.0f, bs = -INFINITY, bv = -INFINITY;   // best score and its raw logit
    int bi = 0x7fffffff;
    if (m > -INFINITY) {
        const bool any_text = text_lo < tb, any_ts = ts_lo <= ts_hi && ts_lo < V;
        const int lo = any_text ? text_lo : max(ts_lo, tb), hi = any_ts ? min(ts_hi + 1, V) : tb;
        scan_row4(row, max(lo, 0), hi, tid,
                  [&](int i0) {
                      unsigned c0 = (unsigned)(i0 >> 2), c1 = (unsigned)gen, c2 = (unsigned)rid, c3 = (unsigned)(rid >> 32);
                      if (draw) philox4x32_10(c0, c1, c2, c3, (unsigned)seed, (unsigned)(seed >> 32));
                      return Words4{c0, c1, c2, c3};
                  },
                  [&](float x, int i, unsigned word) {
                      if (!SAMPLE_OK(x, i)) return;
                      sum += expf(x - m);
                      const float sc = draw ? wh_add(wh_scale(x, invT), gumbel_of(word)) : x;
                      if (cand_before(sc, i, bs, bi)) { bs = sc; bi = i; bv = x; }
                  });
    }
#undef SAMPLE_OK
    block_best(bs, bi, bv, sb, tid);
    sum = block_sum(sum, sb, tid);
    if (tid == 0) {
        const int tok = bi == 0x7fffffff ? 0 : bi;
        const float lp = bi == 0x7fffffff ? -INFINITY : wh_sub(bv, m) - logf(sum);
        int next = tok;
        st.out_tokens[b * st.tok_ld + st.n_prompt + gen] = tok;
        st.n_out[b] = st.n_prompt + gen + 1;
        st.logprob[b * st.tok_ld + st.n_prompt + gen] = lp;
        if (gen < st.n_forced) next = st.forced[gen];
        else if (tok == st.eot) st.done[b] = 1;
        if (pos + 1 < st.tok_ld) st.feed[b * st.tok_ld + pos + 1] = next;
        if (rules) {
            // the next position's ranges from the history it sees (seq = the fed tokens, `next` its last one): rules 2 and 3
            const bool pen_ts = gen == 0 || st.feed[b * st.tok_ld + pos] >= tb;   // (the token fed at this position is seq[-2])
            int n_text_lo, n_ts_lo, n_ts_hi, last_t;
            ts_next_state(next, pen_ts, gen == 0 ? -1 : a.ts_state[4 * b + 3], tb, st.eot, V, n_text_lo, n_ts_lo, n_ts_hi, last_t);
            a.ts_state[4 * b] = n_text_lo;
            a.ts_state[4 * b + 1] = n_ts_lo;
            a.ts_state[4 * b + 2] = n_ts_hi;
            a.ts_state[4 * b + 3] = last_t;
        }
        s_next = next;
    }
    __syncthreads();
    embed_next_row<T>(ne, b, s_next, mpos, sv);
    advance_if_last(ticket, pos_p, gridDim.x);
}

}  // namespace

void wh_launch_sample_select(hipStream_t s, int prec, const SampleArgs& a, const DecodeState& st, const NextEmbed& ne, int rows, int* pos_p, int* ticket) {
    wh_with_dtype(prec, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        hipLaunchKernelGGL(k_sample_select<T>, dim3(rows), dim3(256), 0, s, a, st, ne, pos_p, ticket);
    });
}
