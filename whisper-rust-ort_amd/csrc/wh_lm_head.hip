// wh_lm_head.hip — the end of a decoder position for gfx950: token + position embedding, the LM head with its masked argmax
// partials, the finish kernels that turn the partials into the next token, and the language head.  How a decode step is launched,
// and why every kernel reads the position from device memory: the header of wh_dec_gemm.hip.
#include "wh_common.h"
#include "wh_dec_epilogue.h"
#include "wh_kernels.h"

#include <algorithm>

// tuning knobs (tools/microbench.cpp flips them; product code leaves the defaults)
int wh_dbg_lm_blocks_per_cu = 2;
int wh_dbg_lm_mt = 4;

namespace {

// (advance_if_last, the position ticket, and slab_idx, the k-slab-major activation layout: wh_dec_epilogue.h)

// Token embedding + learned position ([3P] :737, :757-766) for the rows of this position: writes the f32
// residual stream, its raw copy in the compute dtype (slab layout) and each row's {sum x, sum x^2}
// (one "tile" of LayerNorm partials).  One wave per row.
// PFX (per-clip prefixes): row b sits at model position max(g - off[b], 0) of the global position g = *pos_p — the token
// is still feed[b][g] (the host laid the rows out right-aligned), only the position row differs.  0 <= off[b] <= g + 1 keeps the position
// row inside [0, g] ⊂ [0, n_text_ctx); an idle row (g < off[b]) embeds its filler token at position 0 and nothing reads the result.
template <typename T, bool PFX = false>
__global__ __launch_bounds__(256) void k_dec_embed(const T* __restrict__ tok_emb, const float* __restrict__ pos_emb,
                                                   const int* __restrict__ feed, int feed_ld,
                                                   const int* __restrict__ pos_p, float* __restrict__ x,
                                                   T* __restrict__ xslab, float* __restrict__ stats, int rows, int d,
                                                   int mpad, const float* __restrict__ xgamma, float* __restrict__ shift,
                                                   const int* __restrict__ off) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63, pos = *pos_p;
    const T* er = tok_emb + (long)feed[row * feed_ld + pos] * d;
    int mpos = pos;   // the row's model position
    if constexpr (PFX) mpos = max(pos - max(off[row], 0), 0);
    const float* pr = pos_emb + (long)mpos * d;
    // pass 1: the residual row and its mean; pass 2: the slab copy and the sums of the CENTRED row (SkinnyArgs::row_shift)
    // The sums are taken in embed_next_row's order (wh_dec_epilogue.h: 256 threads, thread t the columns 4 t + 1024 i, one sum per wave, the four
    // waves' sums added as (0 + 1) + (2 + 3)): lane l stands for the threads l, l + 64, l + 128, l + 192, so a token at a position gets the same
    // mean, slab copy and row sums bit for bit whether it is embedded here (prompt positions, the scoring pass) or by the kernel that chose it
    // (tools/lm_check.cpp, group finish).  Up to d = 256 the two orders coincide; above, one wave sum per row differed in the last bit.
    float s0[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int w = 0; w < 4; w++)
        for (int c = (lane + 64 * w) * 4; c < d; c += 1024) {
            const f32x4 v = load4_f32(er + c) + *reinterpret_cast<const f32x4*>(pr + c);
            *reinterpret_cast<f32x4*>(x + (long)row * d + c) = v;
            s0[w] += (v[0] + v[1]) + (v[2] + v[3]);
        }
    float mean = 0.0f;
    if (shift) mean = ((dpp_wave_sum(s0[0]) + dpp_wave_sum(s0[1])) + (dpp_wave_sum(s0[2]) + dpp_wave_sum(s0[3]))) / (float)d;
    float s1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, s2[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int w = 0; w < 4; w++)
        for (int c = (lane + 64 * w) * 4; c < d; c += 1024) {
            f32x4 v = load4_f32(er + c) + *reinterpret_cast<const f32x4*>(pr + c);
            v -= mean;
            f32x4 g = {1, 1, 1, 1};
            if (xgamma) g = *reinterpret_cast<const f32x4*>(xgamma + c);  // fp8 mode: the first LayerNorm's γ rides on the slab copy
            store4(xslab + slab_idx(row, c, mpad), v[0] * g[0], v[1] * g[1], v[2] * g[2], v[3] * g[3]);
            s1[w] += (v[0] + v[1]) + (v[2] + v[3]);
            s2[w] += (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
        }
    const float t1 = (dpp_wave_sum(s1[0]) + dpp_wave_sum(s1[1])) + (dpp_wave_sum(s1[2]) + dpp_wave_sum(s1[3]));
    const float t2 = (dpp_wave_sum(s2[0]) + dpp_wave_sum(s2[1])) + (dpp_wave_sum(s2[2]) + dpp_wave_sum(s2[3]));
    if (lane == 0) {
        stats[2 * row] = t1;
        stats[2 * row + 1] = t2;
        if (shift) shift[row] = mean;
    }
}

// ---- LM head: logits = LN(x) · E^T over the whole vocabulary ([3P] :790, :965-970) + masked argmax
// partials per 16-column tile (reference argmax_last_dim_raw, src/main.rs:709-735).  The [M][K]
// activation tile is staged in LDS once per workgroup; each wave then walks 16-row tiles of the
// embedding matrix with all of a tile's weight fragments in flight before its first MFMA.
// RULES: Whisper's timestamp rules (SkinnyArgs::ts_*): the masked argmax covers the allowed text ids only, the timestamp logits go to
// SkinnyArgs::ts_logits for k_argmax_finish<T, true>; the logits are the same expression (the rules-off instantiations are unchanged).
// LP: token log-probabilities (SkinnyArgs::part_sum): beside each (max, index) partial the sum of exp(v - max) over the ids the
// partial ranged over, kept online per lane (a tile's accumulators are gone once the next tile starts) and merged over the row's four lane
// groups; the logit of SkinnyArgs::probe_id goes to probe_out (the no-speech probe).  The LP = false instantiations are unchanged.
// REP: repetition penalty / no-repeat n-grams (SkinnyArgs::rep_*): the row's touched-id bits are OR-ed into the suppress bits, so a
// touched id enters no partial, no sum and no timestamp logit; its raw logit (the same expression) leaves by one predicated store to the row's
// side buffer for k_argmax_finish<..., REP>.  Bitmap and side-buffer indices stay inside row m's slice (m < M, nn < N).  The REP = false
// instantiations are unchanged.
template <typename T, int MT, bool RULES = false, bool LP = false, bool REP = false>
__global__ __launch_bounds__(256) void k_lm_head(SkinnyArgs a) {
    extern __shared__ __attribute__((aligned(128))) char smem_raw[];   // 128: h2 tiles find their 32-blocks from the address
    constexpr int EPC = 16 / (int)sizeof(T);
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fl = lane & 15, fg = lane >> 4;
    const int n_tiles = (a.N + 15) >> 4;
    const int m0 = blockIdx.y * MT * 16;
    // activation tile: the row group's rows of every k-slab, LDS layout [K/32][MT*16][32]
    T* Xs = reinterpret_cast<T*>(smem_raw);
    constexpr int ROWS = MT * 16;
    const int nslab = a.K >> 5, cps = ROWS * 32 / EPC;  // 16-B chunks per slab of this row group
    // sixteen 16-byte loads in flight per thread, then the LDS stores (a load -> store loop costs a round trip per
    // chunk); the first batch's stores wait until the first weight unit is in flight too (see below)
    u32x4 xr[16];
    int xo[16];
    auto stage_load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int c = min(c0 + i * 256, nslab * cps - 1), sl = c / cps, o = (c - sl * cps) * EPC;
            xo[i] = sl * ROWS * 32 + o;
            xr[i] = *reinterpret_cast<const u32x4*>((const T*)a.X + ((long)sl * a.x_mpad + m0) * 32 + o);
        }
    };
    auto stage_store = [&](int c0) {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (c0 + i * 256 < nslab * cps) *reinterpret_cast<u32x4*>(Xs + xo[i]) = xr[i];
    };
    stage_load(tid);
    // final LayerNorm folded in: mean / rstd of this row group from the producer's per-tile partial sums
    float* lnstat = reinterpret_cast<float*>(smem_raw + (size_t)nslab * ROWS * 32 * sizeof(T));  // [ROWS][2]
    if (a.ln_part) {
        // all 256 threads: thread (row r, quarter q) sums every 4th tile, the four quarters meet through LDS
        float* lnq = lnstat + 2 * ROWS;  // [4][ROWS][2]
        if (tid < 4 * ROWS) {
            const int r = tid % ROWS, q = tid / ROWS;
            float s1, s2;
            ln_partial_sum(a.ln_part, a.ln_tiles, a.x_mpad, m0 + r, q, 4, s1, s2);
            ln_part_store<ROWS>(lnq, r, q, s1, s2);
        }
        __syncthreads();
        if (tid < ROWS) {
            float mean, rstd;
            ln_row_stats<ROWS>(lnq, tid, a.K, mean, rstd);
            lnstat[2 * tid] = mean;
            lnstat[2 * tid + 1] = rstd;
        }
    }
    const int pos = *a.pos_p;
    const int gen = pos - (a.n_prompt - 1);  // index of the token this row generates
    const int lrow = a.logits_cur ? min(gen, 0) : gen;   // the row of a.logits this position's logits go to
    const unsigned* mask = (gen == 0) ? a.mask_first : a.mask_base;
    // Pipeline unit = (tile, 16-fragment chunk of K).  Two register sets: the next unit's weight
    // fragments are in flight while the current unit's MFMAs issue.
    const int iters = a.K >> 5;
    constexpr int DEPTH = sizeof(typename FragT<T>::type) <= 16 ? 16 : 8;   // two register sets of DEPTH weight fragments
    const int nchunk = (iters + DEPTH - 1) / DEPTH;
    const int stride = gridDim.x * 4, first = blockIdx.x * 4 + wave;
    const int my_tiles = first < n_tiles ? (n_tiles - first + stride - 1) / stride : 0;
    const int units = my_tiles * nchunk;
    typedef typename FragT<T>::type frag_t;
    frag_t wA[DEPTH], wB[DEPTH];
    f32x4 acc[MT];
    // masked argmax, lane-local across ALL of this wave's tiles (they are visited in increasing column order, so
    // strict > keeps the lowest index on ties): the cross-lane reduce and the partial store happen once per wave
    float bvw[MT];
    int biw[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) { bvw[t] = -INFINITY; biw[t] = 0x7fffffff; }
    float lsw[LP ? MT : 1];   // LP: sum of exp(v - bvw[t]) over the ids bvw[t] ranged over
    if constexpr (LP) {
#pragma unroll
        for (int t = 0; t < MT; t++) lsw[t] = 0.0f;
    }
    // RULES: the allowed ranges of each of this lane's rows
    int tlo[MT], slo[MT], shi[MT];
    if constexpr (RULES) {
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const int m = m0 + t * 16 + fl;
            tlo[t] = a.ts_begin; slo[t] = a.N; shi[t] = 0;
            if (m < a.M) ts_ranges(a.ts_state, m, gen, a.ts_begin, a.ts_max_init, a.N, tlo[t], slo[t], shi[t]);
        }
    }
    auto load_unit = [&](frag_t (&wq)[DEPTH], int u) {
        const int tile = first + (u / nchunk) * stride, c0 = (u % nchunk) * DEPTH;
        int nrow = tile * 16 + fl;
        if (nrow > a.N - 1) nrow = a.N - 1;
        const T* wp = (const T*)a.W + (long)nrow * a.K + fg * 8;
#pragma unroll
        for (int i = 0; i < DEPTH; i++)
            if (c0 + i < iters) wq[i] = load_frag<T>(wp + (c0 + i) * 32);
    };
    auto compute_unit = [&](const frag_t (&wq)[DEPTH], int u) {
        const int tile = first + (u / nchunk) * stride, ck = u % nchunk, c0 = ck * DEPTH;
        if (ck == 0) {
#pragma unroll
            for (int t = 0; t < MT; t++) acc[t] = f32x4{0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < DEPTH; i++) {
            if (c0 + i < iters) {
#pragma unroll
                for (int t = 0; t < MT; t++) {
                    frag_t xf = load_frag<T>(Xs + ((long)(c0 + i) * ROWS + t * 16 + fl) * 32 + fg * 8);
                    mma16(acc[t], wq[i], xf);
                }
            }
        }
        if (ck != nchunk - 1) return;
        const int n = tile * 16 + 4 * fg;
        float sv[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0};
        if (a.ln_part) {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (n + e < a.N) { sv[e] = a.ln_s[n + e]; cv[e] = a.bias[n + e]; }
        }
        unsigned mbits = 0;  // suppress bits of this lane's 4 columns (one mask word covers a 16-column tile)
        if (n < a.N) mbits = mask[n >> 5] >> (n & 31);
#pragma unroll
        for (int t = 0; t < MT; t++) {
            const int m = m0 + t * 16 + fl;
            const float mean = a.ln_part ? lnstat[2 * (t * 16 + fl)] : 0.0f, rstd = a.ln_part ? lnstat[2 * (t * 16 + fl) + 1] : 1.0f;
            unsigned rbits = 0;   // REP: touched bits of this lane's 4 columns of row m
            if constexpr (REP) {
                if (n < a.N && m < a.M) rbits = a.rep_bits[(long)m * a.rep_words + (n >> 5)] >> (n & 31);
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int nn = n + e;
                const float v = a.ln_part ? wh_ln_fold(acc[t][e], mean, rstd, sv[e], cv[e]) : acc[t][e];
                if (nn < a.N && m < a.M) {
                    if (a.logits && lrow >= 0 && lrow < a.logits_rows) {
                        const int slot = a.logits_sel ? a.logits_sel[m] : m;
                        if (slot >= 0) a.logits[((long)slot * a.logits_rows + lrow) * a.N + nn] = v;
                    }
                    if constexpr (REP) {
                        if ((rbits >> e) & 1u) a.rep_side[(long)m * a.N + nn] = v;
                    }
                    const bool sup = ((mbits | rbits) >> e) & 1u;
                    if constexpr (LP) {
                        if (nn == a.probe_id) a.probe_out[m] = v;
                        const bool text_ok = RULES ? (!sup && nn >= tlo[t] && nn < a.ts_begin) : !sup;
                        if (text_ok) lp_acc(v, bvw[t], lsw[t]);   // (before the argmax below moves bvw[t])
                    }
                    if constexpr (RULES) {
                        if (tile * 16 + 16 <= a.ts_begin) { if (!sup && nn >= tlo[t] && v > bvw[t]) { bvw[t] = v; biw[t] = nn; } }   // text-only tile
                        else ts_take(v, nn, sup, a.ts_begin, tlo[t], slo[t], shi[t], bvw[t], biw[t], a.ts_logits + (long)m * a.ts_ld);
                    } else if (!sup && v > bvw[t]) { bvw[t] = v; biw[t] = nn; }  // strict >, NaN never wins
                }
            }
        }
    };
    if (units > 0) load_unit(wA, 0);   // in flight while the activation tile is staged
    stage_store(tid);
    for (int c0 = tid + 256 * 16; c0 < nslab * cps; c0 += 256 * 16) {  // K > 512
        stage_load(c0);
        stage_store(c0);
    }
    __syncthreads();
    for (int u = 0; u < units; u += 2) {
        const bool hasB = u + 1 < units;
        if (hasB) load_unit(wB, u + 1);
        compute_unit(wA, u);
        if (hasB) {
            if (u + 2 < units) load_unit(wA, u + 2);
            compute_unit(wB, u + 1);
        }
    }
    // one partial per (wave, row): argmax over the four lane groups of a row on v_permlane*_swap, then 16 consecutive
    // rows leave as one 64-byte store — layout [part][x_mpad], part = blockIdx.x * 4 + wave (k_argmax_finish reads
    // gridDim.x * 4 parts per row)
    const int part = blockIdx.x * 4 + wave;
#pragma unroll
    for (int t = 0; t < MT; t++) {
        float bv = bvw[t];
        int bi = biw[t];
        xrow_argmax(bv, bi);
        const int m = m0 + t * 16 + fl;
        if constexpr (LP) {   // this lane's sum moved to the row's maximum, then the four lane groups' sums added
            const float ls = xrow_sum(lp_rescale(lsw[t], bvw[t], bv));
            if (fg == 0 && m < a.M) a.part_sum[(long)part * a.x_mpad + m] = ls;
        }
        if (fg == 0 && m < a.M) {
            a.part_val[(long)part * a.x_mpad + m] = bv;
            a.part_idx[(long)part * a.x_mpad + m] = bi;
        }
    }
}

// Final reduce of the per-tile argmax partials + greedy bookkeeping for one clip per workgroup:
// records the generated token, EOT stop (src/main.rs:781-783, 820-822) and the next input token.
// RULES (ts.rules): the text partials of k_lm_head*<RULES> are merged as above; the row's allowed timestamp logits (ts.ts_logits) are reduced
// to their (max, index, sum of exp); step 5 of the timestamp rules picks between the two (timestamps only when the log-sum-exp of the allowed
// timestamps exceeds the best allowed text logit), and the next position's allowed ranges are written from the token fed next.
// LP (part_sum): the (max, sum of exp) pairs of the LM head's LP variants are merged beside the (max, index) pairs; the recorded token's
// log-probability, -log(sum of exp(v - max) over the allowed ids), goes to st.logprob next to the token.  With RULES the text side and the
// timestamp side are combined by what rule 5 decided: timestamps only -> the timestamp log-sum-exp alone.
// PFX (per-clip prefixes): the next position's embedding takes position row max(pos + 1 - ne.off[b], 0) — inside
// [0, pos + 1] ⊂ [0, n_text_ctx) for any ne.off[b] >= 0; tokens, `gen`, the rules and the log-probabilities are in global positions and
// do not change (every row reaches <|startoftranscript|> at the same global position).
// REP (rp.on; repetition penalty / no-repeat n-grams): the LM head's REP variants kept the row's touched ids out of the partials
// and left their raw logits in rp.side.  The workgroup walks the row's generated history h = st.feed[b][n_prompt .. pos] (reads stay in those
// columns; at most WH_REP_MAX_HIST entries, in LDS), and for each distinct touched id reads the stored logit, drops it if it is banned,
// suppressed by the masks or below the rules' text_lo, else applies the penalty (one f32 multiplication by p or 1 / p) and merges
// (value, id[, 1]) into its reduction — before rule 5 and the log-probability are formed.  After `next` is chosen it rewrites the row's bits
// for the next position (history h ++ [next]): clears this position's bans, sets `next` when the penalty is on, sets the new bans.  Row b's
// bits are written by workgroup b only, and the LM head of position pos + 1 runs after this kernel in stream / graph order.
// entry i of the history hs[0 .. L) is banned when it closes an n-gram whose first n - 1 ids equal the history's last n - 1
__device__ __forceinline__ void rep_bans(const int* hs, unsigned char* ban, int L, int n, int exempt_from, int tid) {
    for (int i = tid; i < L; i += 256) {
        bool b = n > 0 && L >= n - 1 && i >= n - 1 && hs[i] < exempt_from;
        for (int k = 0; b && k < n - 1; k++) b = hs[i - (n - 1) + k] == hs[L - (n - 1) + k];
        ban[i] = b ? 1 : 0;
    }
}

template <typename T, bool RULES = false, bool LP = false, bool PFX = false, bool REP = false>
__global__ __launch_bounds__(256) void k_argmax_finish(const float* __restrict__ part_val,
                                                       const int* __restrict__ part_idx, int n_tiles, int mpad, int* pos_p,
                                                       int* ticket, DecodeState st, NextEmbed ne, TsFinish ts, const float* __restrict__ part_sum,
                                                       RepFinish rp) {
    __shared__ float sv[256];
    __shared__ int si[256];
    __shared__ float ssum[LP ? 256 : 1];
    __shared__ int rh[REP ? WH_REP_MAX_HIST + 1 : 1];              // REP: the row's generated history, then `next`
    __shared__ unsigned char rban[REP ? WH_REP_MAX_HIST + 1 : 1];  // REP: entry i's id is banned
    const int b = blockIdx.x, tid = threadIdx.x;
    const int pos = *pos_p;
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    float bs = 0.0f;   // LP: sum of exp(v - bv)
    for (int i0 = tid; i0 < n_tiles; i0 += 256 * 8) {   // n_tiles = number of partials per row, layout [part][mpad]
        float v[8];
        int ix[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int i = i0 + u * 256;
            v[u] = -INFINITY;
            ix[u] = 0x7fffffff;
            if (i < n_tiles) { v[u] = part_val[(long)i * mpad + b]; ix[u] = part_idx[(long)i * mpad + b]; }
        }
        if constexpr (LP) {   // eight sums folded pairwise at their common maximum, then into the running pair
            float sm[8];
#pragma unroll
            for (int u = 0; u < 8; u++) sm[u] = (i0 + u * 256 < n_tiles) ? part_sum[(long)(i0 + u * 256) * mpad + b] : 0.0f;
            float mx = v[0];
#pragma unroll
            for (int u = 1; u < 8; u++) mx = fmaxf(mx, v[u]);
            float r[8];
#pragma unroll
            for (int u = 0; u < 8; u++) r[u] = lp_rescale(sm[u], v[u], mx);
            bs = lp_merge(bv, bs, mx, ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7])));
        }
#pragma unroll
        for (int u = 0; u < 8; u++)
            if (v[u] > bv || (v[u] == bv && ix[u] < bi)) { bv = v[u]; bi = ix[u]; }
    }
    int rep_L = 0;
    if constexpr (REP) {
        const int gen = pos - (st.n_prompt - 1);
        rep_L = min(max(gen, 0), WH_REP_MAX_HIST);
        const int* hrow = st.feed + (long)b * st.tok_ld + st.n_prompt;   // columns [n_prompt, pos]
        for (int i = tid; i < rep_L; i += 256) rh[i] = hrow[i];
        __syncthreads();
        rep_bans(rh, rban, rep_L, rp.ngram, rp.exempt_from, tid);
        __syncthreads();
        const unsigned* mask = (gen == 0) ? rp.mask_first : rp.mask_base;
        int text_lo = 0;
        if constexpr (RULES) text_lo = gen > 0 ? ts.state[4 * b] : ts.ts_begin;   // (read before thread 0 writes the next position's state)
        const unsigned* brow = rp.bits + (long)b * rp.words;
        for (int i = tid; i < rep_L; i += 256) {
            const int id = rh[i];
            bool first = true, banned = false;
            for (int j = 0; j < rep_L; j++)
                if (rh[j] == id) { first = first && j >= i; banned = banned || rban[j]; }
            if (!first || id < 0 || id >= rp.vocab) continue;                   // each distinct id once
            if (!((brow[id >> 5] >> (id & 31)) & 1u)) continue;                 // not touched: the LM head's partials hold it
            if (banned || ((mask[id >> 5] >> (id & 31)) & 1u) || id < text_lo) continue;
            float v = rp.side[(long)b * rp.vocab + id];
            v = v > 0.0f ? v * rp.inv : v * rp.p;
            if (!(v > -INFINITY)) continue;                                     // NaN and -inf: never win, add nothing
            if constexpr (LP) bs = lp_merge(bv, bs, v, 1.0f);
            if (v > bv || (v == bv && id < bi)) { bv = v; bi = id; }
        }
    }
    sv[tid] = bv; si[tid] = bi;
    if constexpr (LP) ssum[tid] = bs;
    int rule_tok = 0;
    float lp = -INFINITY;   // LP: the recorded token's log-probability (nothing allowed: -inf)
    if constexpr (RULES) {
        __shared__ float stm[256], sts[256];
        __shared__ int sti[256];
        float tm = -INFINITY, tsum = 0.0f;
        int ti = 0x7fffffff;
        const float* tr = ts.ts_logits + (long)b * ts.ts_ld;
        for (int i = tid; i < ts.ts_ld; i += 256) ts_acc(tr[i], ts.ts_begin + i, tm, tsum, ti);   // (each thread's columns ascend)
        stm[tid] = tm; sts[tid] = tsum; sti[tid] = ti;
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                float ov = sv[tid + s]; int oi = si[tid + s];
                if constexpr (LP) ssum[tid] = lp_merge(sv[tid], ssum[tid], ov, ssum[tid + s]);
                if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
                float m1 = stm[tid], s1 = sts[tid];
                int i1 = sti[tid];
                ts_merge(m1, s1, i1, stm[tid + s], sts[tid + s], sti[tid + s]);
                stm[tid] = m1; sts[tid] = s1; sti[tid] = i1;
            }
            __syncthreads();
        }
        if (tid == 0) {
            const float text_v = sv[0], ts_v = stm[0];
            const float lse = ts_v == -INFINITY ? -INFINITY : ts_v + logf(sts[0]);
            int w;
            if (lse > text_v) w = sti[0];                                          // step 5: every id below tb is suppressed
            else w = (ts_v > text_v || (ts_v == text_v && sti[0] < si[0])) ? sti[0] : si[0];   // step 6 over both
            rule_tok = (w == 0x7fffffff) ? 0 : w;
            if constexpr (LP) {
                if (w != 0x7fffffff) lp = -logf(lse > text_v ? sts[0] : lp_merge(text_v, ssum[0], ts_v, sts[0]));
            }
        }
    } else {
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) {
            if (tid < s) {
                float ov = sv[tid + s]; int oi = si[tid + s];
                if constexpr (LP) ssum[tid] = lp_merge(sv[tid], ssum[tid], ov, ssum[tid + s]);
                if (ov > sv[tid] || (ov == sv[tid] && oi < si[tid])) { sv[tid] = ov; si[tid] = oi; }
            }
            __syncthreads();
        }
        if constexpr (LP) {
            if (tid == 0 && si[0] != 0x7fffffff) lp = -logf(ssum[0]);
        }
    }
    if (tid == 0) {
        const int gen = pos - (st.n_prompt - 1);
        // nothing beat -inf (all suppressed / NaN / -inf): the reference's best_i stays 0
        const int tok = RULES ? rule_tok : (si[0] == 0x7fffffff) ? 0 : si[0];
        int next = tok;
        if (!st.done[b]) {
            st.out_tokens[b * st.tok_ld + st.n_prompt + gen] = tok;
            st.n_out[b] = st.n_prompt + gen + 1;
            if constexpr (LP) st.logprob[b * st.tok_ld + st.n_prompt + gen] = lp;
            const bool forced = gen < st.n_forced;
            if (forced) next = st.forced[gen];
            else if (tok == st.eot) st.done[b] = 1;
        }
        if (pos + 1 < st.tok_ld) st.feed[b * st.tok_ld + pos + 1] = next;
        if constexpr (RULES) {
            // the next position's ranges from the history it sees (seq = the fed tokens, `next` its last one): rules 2 and 3
            const int tb = ts.ts_begin;
            const bool pen_ts = gen == 0 || st.feed[b * st.tok_ld + pos] >= tb;   // (the token fed at this position is seq[-2])
            int text_lo, ts_lo, ts_hi, last_t;
            ts_next_state(next, pen_ts, gen == 0 ? -1 : ts.state[4 * b + 3], tb, st.eot, ts.vocab, text_lo, ts_lo, ts_hi, last_t);
            ts.state[4 * b] = text_lo;
            ts.state[4 * b + 1] = ts_lo;
            ts.state[4 * b + 2] = ts_hi;
            ts.state[4 * b + 3] = last_t;
        }
        si[0] = next;
    }
    if constexpr (REP) {
        // the row's bits for the next position, whose history is h ++ [next]
        __syncthreads();
        const int next = si[0];
        unsigned* brow = rp.bits + (long)b * rp.words;
        const bool pen = rp.p != 1.0f;
        if (!pen) {   // this position's bans leave (with the penalty on they stay set: every banned id is in the history)
            for (int i = tid; i < rep_L; i += 256)
                if (rban[i] && rh[i] >= 0 && rh[i] < rp.vocab) {
                    const unsigned old = atomicAnd(&brow[rh[i] >> 5], ~(1u << (rh[i] & 31)));   // (returning form: done before the barrier below)
                    asm volatile("" ::"v"(old));
                }
        }
        __syncthreads();
        if (tid == 0) rh[rep_L] = next;
        __syncthreads();
        rep_bans(rh, rban, rep_L + 1, rp.ngram, rp.exempt_from, tid);
        __syncthreads();
        if (tid == 0 && pen && next >= 0 && next < min(rp.exempt_from, rp.vocab)) atomicOr(&brow[next >> 5], 1u << (next & 31));
        for (int i = tid; i < rep_L + 1; i += 256)
            if (rban[i] && rh[i] >= 0 && rh[i] < rp.vocab) atomicOr(&brow[rh[i] >> 5], 1u << (rh[i] & 31));
    }
    if (ne.tok_emb) {
        // token + position embedding of the next position for this clip's row (k_dec_embed's work, one launch
        // and one kernel boundary per token saved): f32 residual row, slab copy, row sums
        __syncthreads();
        const int next = si[0];
        __syncthreads();
        int mpos = pos + 1;   // the row's next model position
        if constexpr (PFX) mpos = max(pos + 1 - max(ne.off[b], 0), 0);
        embed_next_row<T>(ne, b, next, mpos, sv);
    }
    advance_if_last(ticket, pos_p, gridDim.x);
}

// The no-speech probe's finish: row b's (max, sum of exp) partials of an LP launch of the LM head over the unfiltered logits of
// a prompt position -> softmax(v)[no_speech] = exp(probe_v[b] - max - log(sum)).  One wave per row.  The probe's prompt step does not advance the
// position through its last GEMM's ticket (the LM head above still reads it): block 0 does it here, nothing in this kernel reads it.
__global__ __launch_bounds__(64) void k_nospeech_finish(const float* __restrict__ part_val, const float* __restrict__ part_sum, int n_parts, int mpad,
                                                        const float* __restrict__ probe_v, float* __restrict__ prob, int* pos_p) {
    __shared__ float sm[64], ss[64];
    const int b = blockIdx.x, tid = threadIdx.x;
    float m = -INFINITY, s = 0.0f;
    for (int i = tid; i < n_parts; i += 64) {
        const float m1 = part_val[(long)i * mpad + b], s1 = part_sum[(long)i * mpad + b];
        s = lp_merge(m, s, m1, s1);
        m = fmaxf(m, m1);
    }
    sm[tid] = m; ss[tid] = s;
    __syncthreads();
    for (int h = 32; h > 0; h >>= 1) {
        if (tid < h) {
            const float m1 = sm[tid + h];
            ss[tid] = lp_merge(sm[tid], ss[tid], m1, ss[tid + h]);
            sm[tid] = fmaxf(sm[tid], m1);
        }
        __syncthreads();
    }
    if (tid == 0) {
        prob[b] = sm[0] == -INFINITY ? 0.0f : expf(probe_v[b] - sm[0] - logf(ss[0]));
        if (b == 0) *pos_p += 1;
    }
}

// ---- language detection ---------------------------------------------------------
// The language head: the logits of the n_lang listed ids of every row at a prompt position, out [x_mpad][WH_LANG_LD] f32 (column j = the id
// listed j-th).  k_lm_head's K walk with the weight rows gathered by id: the same activation tile in LDS, the same LayerNorm statistics
// (quarter sums in the same order), per (id, row) the same MFMA sequence over ascending k-slabs into one accumulator and the same epilogue
// (wh_ln_fold) — so a listed id's logit is bit for bit what k_lm_head / k_lm_head_tile / the split-fp16 forms give that id at that position.
// One wave per 16 listed ids (at most 8 waves over two workgroups per row group); no masks, no argmax partials, no position.
template <typename T, int MT>
__global__ __launch_bounds__(256) void k_lang_head(LangHeadArgs a) {
    extern __shared__ __attribute__((aligned(128))) char smem_raw[];   // 128: h2 tiles find their 32-blocks from the address
    constexpr int EPC = 16 / (int)sizeof(T);
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fl = lane & 15, fg = lane >> 4;
    const int n_tiles = (a.n_lang + 15) >> 4;
    const int m0 = blockIdx.y * MT * 16;
    T* Xs = reinterpret_cast<T*>(smem_raw);
    constexpr int ROWS = MT * 16;
    const int nslab = a.K >> 5, cps = ROWS * 32 / EPC;  // 16-B chunks per slab of this row group
    u32x4 xr[16];
    int xo[16];
    auto stage_load = [&](int c0) {
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const int c = min(c0 + i * 256, nslab * cps - 1), sl = c / cps, o = (c - sl * cps) * EPC;
            xo[i] = sl * ROWS * 32 + o;
            xr[i] = *reinterpret_cast<const u32x4*>((const T*)a.X + ((long)sl * a.x_mpad + m0) * 32 + o);
        }
    };
    auto stage_store = [&](int c0) {
#pragma unroll
        for (int i = 0; i < 16; i++)
            if (c0 + i * 256 < nslab * cps) *reinterpret_cast<u32x4*>(Xs + xo[i]) = xr[i];
    };
    stage_load(tid);
    float* lnstat = reinterpret_cast<float*>(smem_raw + (size_t)nslab * ROWS * 32 * sizeof(T));  // [ROWS][2]
    {   // mean / rstd of this row group: k_lm_head's reduction, term for term
        float* lnq = lnstat + 2 * ROWS;  // [4][ROWS][2]
        if (tid < 4 * ROWS) {
            const int r = tid % ROWS, q = tid / ROWS;
            float s1, s2;
            ln_partial_sum(a.ln_part, a.ln_tiles, a.x_mpad, m0 + r, q, 4, s1, s2);
            ln_part_store<ROWS>(lnq, r, q, s1, s2);
        }
        __syncthreads();
        if (tid < ROWS) {
            float mean, rstd;
            ln_row_stats<ROWS>(lnq, tid, a.K, mean, rstd);
            lnstat[2 * tid] = mean;
            lnstat[2 * tid + 1] = rstd;
        }
    }
    const int iters = a.K >> 5;
    constexpr int DEPTH = sizeof(typename FragT<T>::type) <= 16 ? 16 : 8;   // two register sets of DEPTH weight fragments
    const int nchunk = (iters + DEPTH - 1) / DEPTH;
    const int tile = blockIdx.x * 4 + wave;
    const int units = tile < n_tiles ? nchunk : 0;
    typedef typename FragT<T>::type frag_t;
    frag_t wA[DEPTH], wB[DEPTH];
    f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) acc[t] = f32x4{0, 0, 0, 0};
    // this lane's weight row: the id listed at tile * 16 + fl (the list is padded to WH_LANG_LD entries with valid ids)
    const T* wp = (const T*)a.W + (long)a.ids[min(tile, WH_LANG_LD / 16 - 1) * 16 + fl] * a.K + fg * 8;
    auto load_unit = [&](frag_t (&wq)[DEPTH], int u) {
#pragma unroll
        for (int i = 0; i < DEPTH; i++)
            if (u * DEPTH + i < iters) wq[i] = load_frag<T>(wp + (u * DEPTH + i) * 32);
    };
    auto compute_unit = [&](const frag_t (&wq)[DEPTH], int u) {
#pragma unroll
        for (int i = 0; i < DEPTH; i++) {
            if (u * DEPTH + i < iters) {
#pragma unroll
                for (int t = 0; t < MT; t++) {
                    frag_t xf = load_frag<T>(Xs + ((long)(u * DEPTH + i) * ROWS + t * 16 + fl) * 32 + fg * 8);
                    mma16(acc[t], wq[i], xf);
                }
            }
        }
    };
    if (units > 0) load_unit(wA, 0);   // in flight while the activation tile is staged
    stage_store(tid);
    for (int c0 = tid + 256 * 16; c0 < nslab * cps; c0 += 256 * 16) {  // K > 512
        stage_load(c0);
        stage_store(c0);
    }
    __syncthreads();
    for (int u = 0; u < units; u += 2) {
        const bool hasB = u + 1 < units;
        if (hasB) load_unit(wB, u + 1);
        compute_unit(wA, u);
        if (hasB) {
            if (u + 2 < units) load_unit(wA, u + 2);
            compute_unit(wB, u + 1);
        }
    }
    if (units == 0) return;
    const int j0 = tile * 16 + 4 * fg;   // list positions of this lane's 4 accumulator elements
    float sv[4] = {0, 0, 0, 0}, cv[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int id = a.ids[j0 + e];
        sv[e] = a.ln_s[id];
        cv[e] = a.bias[id];
    }
#pragma unroll
    for (int t = 0; t < MT; t++) {
        const int m = m0 + t * 16 + fl;
        const float mean = lnstat[2 * (t * 16 + fl)], rstd = lnstat[2 * (t * 16 + fl) + 1];
        f32x4 v;
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = wh_ln_fold(acc[t][e], mean, rstd, sv[e], cv[e]);
        if (m < a.M) *reinterpret_cast<f32x4*>(a.out + (long)m * WH_LANG_LD + j0) = v;   // (columns past n_lang hold padding ids' logits, never read)
    }
}

// The language finish: one wave per row.  Over the row's n_lang logits (NaN left out): the maximum and its id (ties to the lowest id, not to
// the lowest list position), the probabilities exp(v - m) / sum in list order, and the chosen id as the row's token at prompt position
// tok_pos (fed there, recorded there).  Nothing finite: the lowest listed id, all probabilities 0.  src_row >= 0 (long-form): every row takes
// that row's result.  pos_p != nullptr: block 0 advances the position (when no other finish kernel of this prompt step does).
__global__ __launch_bounds__(64) void k_lang_finish(const float* __restrict__ logits, const int* __restrict__ ids, int n_lang, int src_row,
                                                    float* __restrict__ probs, int* __restrict__ chosen, int* __restrict__ feed,
                                                    int* __restrict__ out_tokens, int tok_ld, int tok_pos, int* pos_p) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* row = logits + (long)(src_row >= 0 ? src_row : b) * WH_LANG_LD;
    float v[2];
    int id[2];
    float bv = -INFINITY;
    int bi = 0x7fffffff, lo = 0x7fffffff;   // best finite-or-infinite logit's id; lowest listed id
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int j = lane + 64 * k;
        const bool in = j < n_lang;
        v[k] = in ? row[j] : NAN;
        id[k] = in ? ids[j] : 0x7fffffff;
        lo = min(lo, id[k]);
        if (v[k] > bv || (v[k] == bv && id[k] < bi)) { bv = v[k]; bi = id[k]; }   // NaN never wins; -inf only over nothing
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off), ol = __shfl_xor(lo, off);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        lo = min(lo, ol);
    }
    const bool none = bv == -INFINITY;   // every logit NaN or -inf
    float e[2], s = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        // (a +inf maximum: the limit — 1 for the +inf entries, 0 for the others)
        e[k] = (none || !(v[k] == v[k])) ? 0.0f : (bv == INFINITY ? (v[k] == INFINITY ? 1.0f : 0.0f) : ts_exp(v[k] - bv));
        s += e[k];
    }
    s = wave_sum(s);
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int j = lane + 64 * k;
        if (j < n_lang) probs[(long)b * n_lang + j] = none ? 0.0f : e[k] / s;
    }
    if (lane == 0) {
        const int tok = none ? lo : bi;
        chosen[b] = tok;
        feed[(long)b * tok_ld + tok_pos] = tok;
        out_tokens[(long)b * tok_ld + tok_pos] = tok;
        if (pos_p && b == 0) *pos_p += 1;
    }
}

}  // namespace

// off != nullptr (here and in wh_launch_argmax_finish / wh_launch_dec_self_attn): the prefix-aware instantiations
void wh_launch_dec_embed(hipStream_t s, int prec, const void* tok_emb, const float* pos_emb, const int* feed, int feed_ld,
                         const int* pos_p, float* x, void* xslab, float* stats, int rows, int d, int mpad, const float* xgamma, float* shift, const int* off) {
    dim3 grid((rows + 3) / 4);
    wh_with_dtype(prec, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        wh_with_flags([&](auto PFX) {
            hipLaunchKernelGGL((k_dec_embed<T, decltype(PFX)::value>), grid, dim3(256), 0, s, (const T*)tok_emb, pos_emb, feed, feed_ld, pos_p, x, (T*)xslab, stats, rows, d, mpad, xgamma, shift, off);
        }, off != nullptr);
    });
}

// 16-row groups per workgroup (mt) and dynamic LDS of k_lm_head<T, mt, ...> / k_lang_head<T, mt> for M rows of K columns
template <typename T>
static int lm_row_groups(int M, int K, size_t* sm_out) {
    int mt = std::min(wh_dbg_lm_mt, (M + 15) / 16);
    auto lds = [&](int t) { return (size_t)t * 16 * K * sizeof(T) + (size_t)t * 16 * 2 * 4 * 5; };  // X tile + LN stats (+ 4 quarter sums)
    while (mt > 1 && lds(mt) > 150 * 1024) mt--;
    // (128-row groups — two instead of four at 256 clips, half the passes over the 53 MB embedding but one workgroup per CU —
    // measured no faster: 189.5 vs 188.0 ms per 256-clip step)
    if (mt > 4) mt = 4;
    *sm_out = lds(mt);
    return mt;
}

// the same and the grid of k_lm_head for this shape
template <typename T>
static dim3 lm_head_geometry(const SkinnyArgs& a, int* mt_out, size_t* sm_out) {
    const int n_tiles = (a.N + 15) / 16;
    const int mt = *mt_out = lm_row_groups<T>(a.M, a.K, sm_out);
    const size_t sm = *sm_out;
    const int per_cu = std::max<int>(1, (int)(150 * 1024 / sm));
    return dim3(std::min((n_tiles + 3) / 4, 256 * std::min(per_cu, wh_dbg_lm_blocks_per_cu) / ((a.M + 16 * mt - 1) / (16 * mt))), (a.M + 16 * mt - 1) / (16 * mt));
}

// a.X = final-LayerNorm'ed rows [M][K] in the compute dtype
// a.ts_logits != nullptr: the timestamp-rules variants (same logits, same partial count)
// a.part_sum != nullptr: the log-probability variants (same logits, same (max, index) partials)
// a.rep_bits != nullptr: the repetition variants (same logits, same partial count)
template <typename T>
static void launch_lm_head_v(hipStream_t s, const SkinnyArgs& a) {
    int mt;
    size_t sm;
    const dim3 grid = lm_head_geometry<T>(a, &mt, &sm);
    wh_with_flags([&](auto RULES, auto LP, auto REP) {
        wh_with_1to4(mt, [&](auto MT) {
            auto kfn = k_lm_head<T, decltype(MT)::value, decltype(RULES)::value, decltype(LP)::value, decltype(REP)::value>;
            set_max_smem(kfn, sm);
            hipLaunchKernelGGL(kfn, grid, dim3(256), sm, s, a);
        });
    }, a.ts_logits != nullptr, a.part_sum != nullptr, a.rep_bits != nullptr);
}
void wh_launch_lm_head(hipStream_t s, int prec, const SkinnyArgs& a) {
    if (prec == WH_PREC_F32) launch_lm_head_v<float>(s, a);
    else if (prec == WH_PREC_F16X3) {
        if (wh_lm_head_tile_x3_applicable(a)) wh_launch_lm_head_tile_x3(s, a);
        else launch_lm_head_v<h2>(s, a);
    }
    else if (wh_lm_head_tile_applicable(a)) wh_launch_lm_head_tile(s, a);   // hundreds of rows: 256 x 256 tiles (wh_gemm8.hip), same logits
    else launch_lm_head_v<bf16>(s, a);
}

// number of argmax partials per row the LM head writes for this shape (its layout is [part][x_mpad]): k_lm_head's waves per row group
int wh_lm_head_parts(int prec, const SkinnyArgs& a) {
    int mt;
    size_t sm;
    if (prec == WH_PREC_F16X3 && wh_lm_head_tile_x3_applicable(a)) return wh_lm_head_tile_x3_parts(a);
    if (prec == WH_PREC_F32 || prec == WH_PREC_F16X3) return (int)lm_head_geometry<float>(a, &mt, &sm).x * 4;
    if (wh_lm_head_tile_applicable(a)) return wh_lm_head_tile_parts(a);
    return (int)lm_head_geometry<bf16>(a, &mt, &sm).x * 4;
}

void wh_launch_argmax_finish(hipStream_t s, int prec, const float* part_val, const int* part_idx, int n_parts, int mpad, int* pos_p,
                             int* ticket, const DecodeState& st, int B, const NextEmbed& ne, const TsFinish& ts, const float* part_sum, const RepFinish& rp) {
    wh_with_dtype(prec, [&](auto tag) {
        typedef typename decltype(tag)::type T;
        wh_with_flags([&](auto RULES, auto LP, auto PFX, auto REP) {   // REP: the repetition variants
            hipLaunchKernelGGL((k_argmax_finish<T, decltype(RULES)::value, decltype(LP)::value, decltype(PFX)::value, decltype(REP)::value>), dim3(B), dim3(256), 0, s,
                               part_val, part_idx, n_parts, mpad, pos_p, ticket, st, ne, ts, part_sum, rp);
        }, ts.rules, part_sum != nullptr, ne.tok_emb && ne.off, rp.on);
    });
}

void wh_launch_nospeech_finish(hipStream_t s, const float* part_val, const float* part_sum, int n_parts, int mpad, const float* probe_v,
                               float* prob, int B, int* pos_p) {
    hipLaunchKernelGGL(k_nospeech_finish, dim3(B), dim3(64), 0, s, part_val, part_sum, n_parts, mpad, probe_v, prob, pos_p);
}

template <typename T>
static void launch_lang_head_t(hipStream_t s, const LangHeadArgs& a) {
    // row groups as lm_head_geometry forms them (the pitch of the slab covers whole groups)
    size_t sm;
    const int mt = lm_row_groups<T>(a.M, a.K, &sm);
    dim3 grid(((a.n_lang + 15) / 16 + 3) / 4, (a.M + 16 * mt - 1) / (16 * mt));
    wh_with_1to4(mt, [&](auto MT) {
        auto kfn = k_lang_head<T, decltype(MT)::value>;
        set_max_smem(kfn, sm);
        hipLaunchKernelGGL(kfn, grid, dim3(256), sm, s, a);
    });
}

void wh_launch_lang_head(hipStream_t s, int prec, const LangHeadArgs& a) {
    wh_with_dtype(prec, [&](auto tag) { launch_lang_head_t<typename decltype(tag)::type>(s, a); });   // (fp8 mode: the embedding is bf16)
}

void wh_launch_lang_finish(hipStream_t s, const float* logits, const int* ids, int n_lang, int src_row, float* probs, int* chosen, int* feed,
                           int* out_tokens, int tok_ld, int tok_pos, int B, int* pos_p) {
    hipLaunchKernelGGL(k_lang_finish, dim3(B), dim3(64), 0, s, logits, ids, n_lang, src_row, probs, chosen, feed, out_tokens, tok_ld, tok_pos, pos_p);
}
