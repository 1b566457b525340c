// wh_lm_tile.h — what the LM-head tile kernels share: k_lm_head_tile (wh_gemm8.hip: bf16 and fp8 contexts) and k_lm_head_tile_x3
// (wh_gemm8x.hip: WH_PREC_F16X3) differ in their operand format, and with it in their rings, swizzles and main loops.  Everything around the
// main loop is here once: the LDS behind the ring, the final LayerNorm's statistics, the timestamp rules' row state, the repetition bitmap's
// staging, the epilogue (LayerNorm fold, suppress mask, REP / RULES / LP, masked argmax, one partial per (column tile, row)) and the launcher.
//
// A workgroup of 8 waves (WM x WN) owns BM rows x BN = WN * TN * 16 columns of logits; a wave holds TM x TN MFMA tiles of 16 x 16 with the
// weights as the row operand (mma16's D layout: lane l has row fl = l & 15 of the activation tile and columns 4 fg .. 4 fg + 3, fg = l >> 4,
// of each 16-column group).  RING is the bytes of the kernel's LDS-DMA ring, which comes first in LDS and is idle in the epilogue.
//
// Every function is force-inlined into its kernel and takes SkinnyArgs BY VALUE: it is the kernel's own argument, so its fields stay the
// scalar loads from the kernel-argument segment they were (by reference the RULES && REP variants spilled three times as many scalar
// registers).  The kernels' contract (RULES, LP, REP; bit-identical logits to k_lm_head) is stated at k_lm_head_tile, wh_gemm8.hip.
#pragma once
#include <stdlib.h>

#include "wh_common.h"
#include "wh_kernels.h"

template <int BM, int TM, int TN, int WN, int RING>
struct WhLmTile {
    static constexpr int BN = WN * TN * 16;
    static_assert(BN == 256 && TN == 4 && BM == 256, "the bitmap staging (8 words per row, 2 per wave) and the two quarters per thread assume 256 x 256 tiles of 64-column waves");

    // ---- LDS behind the ring -----------------------------------------------------------------------------------------------------------
    struct Lds {
        float* lnstat;   // [BM][2] mean, rstd
        float* lnq;      // [4][BM][2] quarter sums
        int* tsr;        // RULES: [BM][4] the rows' allowed ranges (written after the main loop)
        unsigned* rbw;   // REP: [BM][8] the rows' touched bits of this tile's 256 columns (written after the main loop; behind the ranges' place)
    };
    static __device__ __forceinline__ Lds carve(char* smem) {
        Lds l;
        l.lnstat = reinterpret_cast<float*>(smem + RING);
        l.lnq = l.lnstat + 2 * BM;
        l.tsr = reinterpret_cast<int*>(l.lnq + 4 * BM * 2);
        l.rbw = reinterpret_cast<unsigned*>(l.tsr + 4 * BM);
        return l;
    }
    // dynamic LDS of a launch: a.ts_logits selects the timestamp-rules variants, a.rep_bits the repetition variants
    static size_t lds_bytes(const SkinnyArgs& a) {
        return (size_t)RING + (size_t)BM * 2 * 4 * 5 + ((a.ts_logits || a.rep_bits) ? (size_t)BM * 4 * 4 : 0) + (a.rep_bits ? (size_t)BM * 8 * 4 : 0);
    }

    // ---- before the main loop ------------------------------------------------------------------------------------------------------------
    struct TsRaw { int lo, slo, shi; };
    // final LayerNorm: quarter sums of the producer's per-tile partials, two quarters per thread (row tid & 255) — requested before the ring,
    // so they are the oldest vector-memory requests.  RULES: the rows' state, requested behind them without waiting on the position (gen 0
    // ignores it); it turns into the allowed ranges in LDS after the main loop (stage_rows), so the epilogue reads them from LDS instead of
    // eight dependent global loads.
    template <bool RULES>
    static __device__ __forceinline__ TsRaw prologue(SkinnyArgs a, const Lds l, int m0, int tid) {
        if (a.ln_part) {
            const int r = tid & (BM - 1), h = tid >> 8, row = min(m0 + r, a.x_mpad - 1);
            float s1a, s2a, s1b, s2b;
            ln_partial_sum(a.ln_part, a.ln_tiles, a.x_mpad, row, h, 4, s1a, s2a);
            ln_partial_sum(a.ln_part, a.ln_tiles, a.x_mpad, row, h + 2, 4, s1b, s2b);
            ln_part_store<BM>(l.lnq, r, h, s1a, s2a);
            ln_part_store<BM>(l.lnq, r, h + 2, s1b, s2b);
        }
        TsRaw t = {0, 0, 0};
        if constexpr (RULES) {
            if (tid < BM) {
                const int* r = a.ts_state + 4 * min(m0 + tid, a.M - 1);
                t.lo = r[0]; t.slo = r[1]; t.shi = r[2];
            }
        }
        return t;
    }
    // the quarter sums -> {mean, rstd} per row, in k_lm_head's order; called behind the first barrier after the prologue's LDS writes have
    // left (s_waitcnt lgkmcnt(0) before that barrier), wherever the kernel's loop has it
    static __device__ __forceinline__ void ln_reduce(SkinnyArgs a, const Lds l, int tid) {
        if (a.ln_part && tid < BM) {
            float mean, rstd;
            ln_row_stats<BM>(l.lnq, tid, a.K, mean, rstd);
            l.lnstat[2 * tid] = mean;
            l.lnstat[2 * tid + 1] = rstd;
        }
    }

    // ---- after the main loop, before the barrier that precedes the epilogue -------------------------------------------------------------------
    template <bool RULES, bool REP>
    static __device__ __forceinline__ void stage_rows(SkinnyArgs a, const Lds l, TsRaw t, int m0, int n0, int tid) {
        if constexpr (RULES) {
            if (tid < BM) {
                int lo = t.lo, slo = t.slo, shi = t.shi;
                const int gen0 = *a.pos_p - (a.n_prompt - 1);
                if (gen0 == 0) ts_ranges(nullptr, 0, 0, a.ts_begin, a.ts_max_init, a.N, lo, slo, shi);   // rule 4
                l.tsr[4 * tid] = lo; l.tsr[4 * tid + 1] = slo; l.tsr[4 * tid + 2] = shi;
            }
        }
        if constexpr (REP) {
            if (tid < BM) {   // row m0 + tid's words n0 / 32 .. + 7 (n0 is a multiple of 256: word-aligned); past the row's last word: 0
                const unsigned* src = a.rep_bits + (long)min(m0 + tid, a.M - 1) * a.rep_words;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int w = (n0 >> 5) + k;
                    l.rbw[tid * 8 + k] = w < a.rep_words ? src[w] : 0u;
                }
            }
        }
    }

    // ---- epilogue: final LayerNorm fold + masked argmax, one partial per (column tile, row) --------------------------------------------------
    // Called by every thread behind a __syncthreads() that follows ln_reduce, stage_rows and the last MFMA: the ring is idle and holds the
    // waves' partials ([WN][BM] max, index and, LP, sum of exp).  ct = the column tile (n0 = ct * BN), wm / wn = the wave's place.
    template <bool RULES, bool LP, bool REP>
    static __device__ __forceinline__ void epilogue(SkinnyArgs a, f32x4 (&acc)[TM][TN], char* smem, const Lds l, int ct, int m0, int wm, int wn, int tid) {
        const int lane = tid & 63, fl = lane & 15, fg = lane >> 4, n0 = ct * BN;
        const float* lnstat = l.lnstat;
        const int* tsr = l.tsr;
        const unsigned* rbw = l.rbw;
        const int pos = *a.pos_p;
        const int gen = pos - (a.n_prompt - 1);  // index of the token this row generates
        const int lrow = a.logits_cur ? min(gen, 0) : gen;   // the row of a.logits this position's logits go to
        const unsigned* mask = (gen == 0) ? a.mask_first : a.mask_base;
        const int nw0 = n0 + wn * 64;
        float sv[TN][4], cv[TN][4];
        unsigned mbits[TN];
#pragma unroll
        for (int j = 0; j < TN; j++) {
            const int n = nw0 + j * 16 + 4 * fg;
#pragma unroll
            for (int e = 0; e < 4; e++) { sv[j][e] = 0.0f; cv[j][e] = 0.0f; }
            if (a.ln_part) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (n + e < a.N) { sv[j][e] = a.ln_s[n + e]; cv[j][e] = a.bias[n + e]; }
            }
            mbits[j] = 0;
            if (n < a.N) mbits[j] = mask[n >> 5] >> (n & 31);   // suppress bits of this lane's 4 columns
        }
        float* red_v = reinterpret_cast<float*>(smem);            // [WN][BM] — every wave is past the last barrier of the main loop
        int* red_i = reinterpret_cast<int*>(smem) + WN * BM;
        float* red_s = reinterpret_cast<float*>(smem) + 2 * WN * BM;   // LP: [WN][BM] sum of exp(v - red_v)
        if constexpr (REP) {
            // A lane with a touched id among its 16 columns of a row (rare: a row has at most one per history token) sends the raw logits of those
            // ids (the same expression) to the row's side buffer and replaces their accumulators by NaN, which enters no argmax, no sum of exp and
            // no log-probability pass: the loops below are the REP = false ones.  (With the touched bits as a second, row-dependent suppress mask
            // inside them the rules variants spilled; inside their row loop this pass took the loop past the unroller's size limit and the
            // accumulators went to scratch.)  With the rules on a touched id is never a timestamp, so the timestamp logits are not concerned.
#pragma unroll
            for (int i = 0; i < TM; i++) {
                const int rloc = wm * (TM * 16) + i * 16 + fl, m = m0 + rloc;
                const wh_u32x2 rw = *reinterpret_cast<const wh_u32x2*>(rbw + rloc * 8 + wn * 2);   // the two bitmap words of this wave's 64 columns of row m
                if ((((rw.x | rw.y) >> (4 * fg)) & 0x000f000fu) != 0u && m < a.M) {
                    const float mean = a.ln_part ? lnstat[2 * rloc] : 0.0f, rstd = a.ln_part ? lnstat[2 * rloc + 1] : 1.0f;
                    int nf = nw0 + 4 * fg;   // (through an empty asm per row: the column tests are not hoisted out of the row loop as live lane masks, cf. lp_tile_row)
                    asm volatile("" : "+v"(nf));
#pragma unroll
                    for (int j = 0; j < TN; j++) {
                        const unsigned rb = ((j < 2) ? rw.x : rw.y) >> ((j & 1) * 16 + 4 * fg);
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int nn = nf + j * 16 + e;
                            const bool t = ((rb >> e) & 1u) && nn < a.N;
                            if (t) a.rep_side[(long)m * a.N + nn] = a.ln_part ? wh_ln_fold(acc[i][j][e], mean, rstd, sv[j][e], cv[j][e]) : acc[i][j][e];
                            acc[i][j][e] = t ? __builtin_nanf("") : acc[i][j][e];
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TM; i++) {
            const int rloc = wm * (TM * 16) + i * 16 + fl, m = m0 + rloc;
            const float mean = a.ln_part ? lnstat[2 * rloc] : 0.0f, rstd = a.ln_part ? lnstat[2 * rloc + 1] : 1.0f;
            float bv = -INFINITY;
            int bi = 0x7fffffff;
            int tlo = a.ts_begin, slo = a.N, shi = 0;
            if constexpr (RULES) {
                if (m < a.M) { tlo = tsr[4 * rloc]; slo = tsr[4 * rloc + 1]; shi = tsr[4 * rloc + 2]; }
            }
#pragma unroll
            for (int j = 0; j < TN; j++) {
                const int n = nw0 + j * 16 + 4 * fg;
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const int nn = n + e;
                    const float v = a.ln_part ? wh_ln_fold(acc[i][j][e], mean, rstd, sv[j][e], cv[j][e]) : acc[i][j][e];
                    if (nn < a.N && m < a.M) {
                        if (a.logits && lrow >= 0 && lrow < a.logits_rows) {
                            const int slot = a.logits_sel ? a.logits_sel[m] : m;
                            if (slot >= 0) a.logits[((long)slot * a.logits_rows + lrow) * a.N + nn] = v;
                        }
                        const bool sup = (mbits[j] >> e) & 1u;
                        if constexpr (RULES) {
                            if (nw0 + j * 16 + 16 <= a.ts_begin) { if (!sup && nn >= tlo && v > bv) { bv = v; bi = nn; } }   // text-only column group
                            else ts_take(v, nn, sup, a.ts_begin, tlo, slo, shi, bv, bi, a.ts_logits + (long)m * a.ts_ld);
                        } else if (!sup && v > bv) { bv = v; bi = nn; }  // strict >, columns ascending: lowest index on ties, NaN never wins
                    }
                }
            }
            xrow_argmax(bv, bi);   // over the four lane groups of the row (k_lm_head's reduction)
            if (fg == 0) {   // this wave's (max, index) of row rloc: the WN waves that share the row meet in LDS (the ring is idle now)
                red_v[wn * BM + rloc] = bv;
                red_i[wn * BM + rloc] = bi;
            }
        }
        if constexpr (REP) {
            // parity path: the logits rows keep the raw values (the loop above stored NaN for the touched ids); no accumulator is read, so the
            // row loop stays rolled
            if (a.logits && lrow >= 0 && lrow < a.logits_rows) {
#pragma unroll 1
                for (int i = 0; i < TM; i++) {
                    const int rloc = wm * (TM * 16) + i * 16 + fl, m = m0 + rloc;
                    const wh_u32x2 rw = *reinterpret_cast<const wh_u32x2*>(rbw + rloc * 8 + wn * 2);
                    if ((((rw.x | rw.y) >> (4 * fg)) & 0x000f000fu) == 0u || m >= a.M) continue;
                    const int slot = a.logits_sel ? a.logits_sel[m] : m;
                    if (slot < 0) continue;
                    for (int c = 0; c < 16; c++) {
                        const int j = c >> 2, e = c & 3, nn = nw0 + j * 16 + 4 * fg + e;
                        const unsigned rb = ((j < 2) ? rw.x : rw.y) >> ((j & 1) * 16 + 4 * fg);
                        if (((rb >> e) & 1u) && nn < a.N) a.logits[((long)slot * a.logits_rows + lrow) * a.N + nn] = a.rep_side[(long)m * a.N + nn];
                    }
                }
            }
        }
        if constexpr (LP) {
            // The rows' maxima are known: a second pass over the accumulators adds exp(v - max) over the same ids.  A loop of its own (inside the
            // loop above the two passes of neighbouring rows overlap and the rules variant spills); each row's maximum comes back from LDS, where
            // this wave's own lanes put it (the rules variant has no probe: the probe runs rules-off).
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < TM; i++) {
                const int rloc = wm * (TM * 16) + i * 16 + fl, m = m0 + rloc;
                const float mean = a.ln_part ? lnstat[2 * rloc] : 0.0f, rstd = a.ln_part ? lnstat[2 * rloc + 1] : 1.0f;
                const float bv = red_v[wn * BM + rloc];
                int tlo = 0;
                if constexpr (RULES) tlo = tsr[4 * rloc];
                const float ls = xrow_sum(lp_tile_row<TN, !RULES>(acc[i], a.ln_part != nullptr, mean, rstd, sv, cv, mbits, nw0 + 4 * fg, tlo,
                                                                    RULES ? min(a.ts_begin, a.N) : a.N, bv, m < a.M ? a.probe_id : -1, a.probe_out + m));
                if (fg == 0) red_s[wn * BM + rloc] = ls;
            }
        }
        __syncthreads();
        // one partial per (column tile, row): 203 instead of 812 partials per row for k_argmax_finish to read (strided by the row pitch)
        if (tid < BM && m0 + tid < a.M) {
            float bv = red_v[tid];
            int bi = red_i[tid];
            float ls = LP ? red_s[tid] : 0.0f;
#pragma unroll
            for (int w = 1; w < WN; w++) {
                const float v1 = red_v[w * BM + tid];
                const int i1 = red_i[w * BM + tid];
                if constexpr (LP) ls = lp_merge(bv, ls, v1, red_s[w * BM + tid]);
                const bool take1 = v1 > bv || (v1 == bv && i1 < bi);
                bv = take1 ? v1 : bv;
                bi = take1 ? i1 : bi;
            }
            a.part_val[(long)ct * a.x_mpad + m0 + tid] = bv;
            a.part_idx[(long)ct * a.x_mpad + m0 + tid] = bi;
            if constexpr (LP) a.part_sum[(long)ct * a.x_mpad + m0 + tid] = ls;
        }
    }

    // ---- host side ------------------------------------------------------------------------------------------------------------------------
    // the conditions both kernels share: WH_LM_TILE_MIN_ROWS (default 256; 0 disables: A/B runs and the parity tests flip it between
    // contexts) is read at every launch decision; whole k-steps; the decode slab layout as the activation operand; no per-channel scale.
    // A probe (probe_id >= 0) only without the rules and without the repetition bitmap, which is how the no-speech probe runs: the rules variants
    // have no probe (lp_tile_row<TN, !RULES>), and with the bitmap a touched id's accumulator is NaN by the time the probe is read — k_lm_head,
    // which hands the raw logit out in both, takes those calls (tools/lm_check.cpp holds the dispatch to that).
    static bool applicable(const SkinnyArgs& a, int bk) {
        const char* e = getenv("WH_LM_TILE_MIN_ROWS");
        const int min_rows = e ? atoi(e) : 256;
        if (a.part_sum && a.probe_id >= 0 && (a.ts_logits || a.rep_bits)) return false;
        return min_rows > 0 && a.M >= min_rows && (a.K % bk) == 0 && a.X != nullptr && a.xpart == nullptr && a.wscale == nullptr;
    }
    static int parts(const SkinnyArgs& a) { return (a.N + BN - 1) / BN; }   // argmax partials per row, layout [part][x_mpad]
    // pick(RULES, LP, REP) returns the kernel's instantiation for three std::bool_constant; a.ts_logits selects the timestamp-rules variants,
    // a.part_sum the log-probability variants, a.rep_bits the repetition variants
    template <typename Pick>
    static void launch(hipStream_t s, const SkinnyArgs& a, Pick pick) {
        if (a.part_sum && a.probe_id >= 0 && (a.ts_logits || a.rep_bits)) {   // (see applicable: never launched with a probe it would not write)
            wh_set_error("LM-head tile kernel: a probe needs a launch without timestamp rules and without the repetition bitmap");
            return;
        }
        const size_t sm = lds_bytes(a);
        dim3 grid(parts(a) * ((a.M + BM - 1) / BM));
        wh_with_flags([&](auto RULES, auto LP, auto REP) {
            void (*kfn)(SkinnyArgs) = pick(RULES, LP, REP);
            wh_ensure_dyn_lds((const void*)kfn, sm);
            hipLaunchKernelGGL(kfn, grid, dim3(512), sm, s, a);
        }, a.ts_logits != nullptr, a.part_sum != nullptr, a.rep_bits != nullptr);
    }
};
