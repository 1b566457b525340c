// wh_step.h — what a token-loop position (Step, wh_decode_host.cpp) and the scoring pass (wh_score_host.cpp) share: the operands of the decode
// GEMMs and the launch list of a decoder layer, with the self-attention launch as the one part the caller supplies.
#pragma once
#include "wh_host_shared.h"

namespace wh {

// ---- wh_decode_host.cpp ----
// the suppress lists a and b as a bitmap of vocab / 32 + 1 words (the device masks mask_first / mask_base)
void pack_mask(const int64_t* a, size_t na, const int64_t* b, size_t nb, int vocab, std::vector<unsigned>& out);
// the cross-attention operands of the nb resident clips: K / V of every decoder layer, or the encoder states' final LayerNorm
int project_cross_kv(wh_ctx* c, int nb, const std::function<int()>& after_kv);
// The alignment post-pass that a decode call (rows = clips) and a forced pass (rows = hypotheses) share.
// align_keys: the listed heads' key rows among ncl resident clips, the key pitches and dk into `a`; returns the score kernels' form.
// align_post_pass: scores + softmax, filter, DTW over a.nb rows, in chunks sized so that the workspace `ws` (P, M and the DTW steps of a chunk,
// grown on demand) stays within 1 GiB; the caller has set everything in `a` but P, M, trace and clip0, and has zeroed a.frames.  debug[k] (a
// row, or < 0: not in these rows) keeps that row's whole P and M slots in dbg[k]; the three kernels' times are added to c->al.ms under
// WH_ALIGN_TIMING.
int align_dk(const wh_ctx* c);
int align_keys(const wh_ctx* c, const std::vector<int>& heads, int ncl, AlignArgs& a);
int align_post_pass(wh_ctx* c, AlignArgs a, int form, DevBuf<>& ws, const std::vector<int>& debug, std::vector<wh_ctx::AlignDebug>& dbg);

// LayerNorm never runs as a kernel in the decoder: the kernel that produces a residual-stream row also emits its raw copy in the
// compute dtype (c->dxs, slab layout) and per-column-tile partial sums (c->lnpart); the GEMM that consumes LN(x) has γ folded into
// its weights and applies mean / rstd in its epilogue (wh_model.cpp fold_ln).
// The launches see the context (model, fixed workspace addresses, option buffers) and the step's key, nothing else.
struct StepBase {
    wh_ctx* c;
    const wh_ctx::StepKey& k;
    wh_model* m = c->m;
    const wh_dims& D = m->dims;
    hipStream_t s = c->stream;
    const int prec = m->prec, nb = k.nb, mpad = c->mpad, ln_tiles_d = D.d_model / 16;
    const long d = D.d_model, S = D.n_audio_ctx;
    const bool f8 = prec == WH_PREC_FP8, rules = k.ts_begin >= 0;
    // rows that share a clip: the cross-attention of row b reads clip clip0 + b / rpc of the ncl resident clips.  Beam search: the nb rows are
    // the beams of ncl = nb / rpc clips (rpc == 1: ncl == nb); the scoring pass: the rows of one pass of clips, clip0 its first clip
    const int rpc, ncl, clip0;
    // the cross K/V of all layers are re-read at every position: below ~half the 256 MiB Infinity Cache they are served
    // from it; above, their stream only evicts the decode weights and activations — then they are loaded non-temporally
    const bool kv_nt = (c->cross_es ? 1.0 : (double)D.dec_layers * 2.0) * ncl * S * d * (f8 ? 1 : (double)m->esz) > 128.0 * 1024 * 1024;
    // The row range the launches run on: rows row0 .. row0 + nr - 1 of the nb, on the same workspace (the whole batch unless the split token loop
    // sets a branch's range and stream).  Only the first row of every operand and the row count follow the range: pitches, the
    // cache strides, the kernel variants (SkinnyArgs::m_sel) and kv_nt stay the whole batch's.  es_cus: compute units of the encoder-state
    // cross-attention launch.  A range with row0 > 0 runs with rpc == 1 (no beam search), in bf16 (esz: the slabs' and the caches' element), without
    // per-clip prefixes and on k_dec_gemm / k_dec_gemm_wide only (choose_split, wh_decode_host.cpp)
    int row0 = 0, nr = nb, es_cus = c->dec_cus;
    // the device-side position the launches read and the ticket that advances it: the whole batch's (element 0) unless the range runs free
    // with its own
    int *pos = c->pos, *ticket = c->step_ticket;
    template <typename T> T* rm(T* p, long ld) const { return p + (long)row0 * ld; }                          // row-major rows of ld elements
    void* rm(void* p, long ld, size_t esz) const { return (char*)p + (long)row0 * ld * (long)esz; }
    void* slab(void* p) const { return (char*)p + (long)row0 * 32 * (long)m->esz; }                           // slab layout [K/32][mpad][32]: row r at r * 32
    // the staggering of two branches (null in one chain): q_rec is recorded behind layer 0's cross-attention query — what the other branch's
    // first launch waits for, so that one branch's cross-attention stream runs beside the other's GEMM chain
    hipEvent_t q_rec = nullptr;
    // the forced-alignment pass (wh_score_host.cpp) takes the layer's query here; empty in a token-loop step, which launches
    // what it launched without it
    std::function<void(int)> query_hook;
    void after_query(int l) const {
        if (q_rec && l == 0) hipEventRecord(q_rec, s);
        if (query_hook) query_hook(l);
    }

    StepBase(wh_ctx* ctx, const wh_ctx::StepKey& key) : c(ctx), k(key), rpc(key.beam_k ? key.beam_k : 1), ncl(key.nb / rpc), clip0(0) {}
    StepBase(wh_ctx* ctx, const wh_ctx::StepKey& key, int rows_per_clip, int clips, int first_clip) : c(ctx), k(key), rpc(rows_per_clip), ncl(clips), clip0(first_clip) {}

    // the decode GEMMs: tile GEMMs on contexts of a thousand clips and more (a property of the context, never of the call)
    void gemm(bool out_f32, const SkinnyArgs& a) const {
        if (c->dec_tile && wh_dec_tile_applicable(prec, a)) wh_launch_dec_tile(s, prec, out_f32, a);
        else wh_launch_dec_gemm(s, prec, out_f32, a);
    }
    // a GEMM that consumes LN(x) of the residual stream: out [nb][N], row-major or (slab_out) slab layout; `out` is the range's first row
    SkinnyArgs ln_consumer(const void* W, const float* bias, const float* wscale, const float* ln_s, long N, void* out, int ln_tiles, bool slab_out = false) const {
        SkinnyArgs a;
        a.X = slab(c->dxs); a.x_mpad = mpad; a.W = W; a.bias = bias; a.wscale = wscale; a.C = out;
        if (slab_out) a.c_mpad = mpad; else a.ldc = N;
        a.M = nr; a.m_sel = nb; a.N = (int)N; a.K = (int)d;
        a.ln_part = rm(c->lnpart, 2); a.ln_tiles = ln_tiles; a.ln_s = ln_s; a.shift_io = rm(c->dshift, 1);
        return a;
    }
    // a GEMM that adds to the residual stream: x += X W^T + bias, plus the raw slab copy and the partial sums of the next LayerNorm
    // (next_gamma: that LayerNorm's γ, applied on the activation side in fp8 mode; X: a slab, the range's first row)
    SkinnyArgs residual_producer(const void* W, const float* bias, const float* wscale, const void* X, long K, const float* next_gamma) const {
        SkinnyArgs a;
        a.X = X; a.x_mpad = mpad; a.W = W; a.bias = bias; a.wscale = wscale; a.R = rm(c->dx, d); a.ldr = d; a.C = rm(c->dx, d); a.ldc = d;
        a.M = nr; a.m_sel = nb; a.N = (int)d; a.K = (int)K; a.xslab_out = slab(c->dxs); a.stats_out = rm(c->lnpart, 2); a.row_shift = rm(c->dshift, 1);
        if (f8) a.xgamma = next_gamma;
        return a;
    }
    // final LN ∘ tied LM head: what the emitting step and the no-speech probe share (they differ in the masks and what they record).  On the
    // range's rows; only the plain emitting step runs on a range with row0 > 0 (choose_free, wh_decode_host.cpp: the other per-row buffers of
    // the options do not follow the range)
    SkinnyArgs lm_head_common() const {
        SkinnyArgs a;
        a.W = m->lm_w; a.bias = m->lm_c; a.ln_s = m->lm_s; a.ln_part = rm(c->lnpart, 2); a.ln_tiles = ln_tiles_d;
        a.M = nr; a.N = D.vocab; a.K = (int)d;
        a.X = slab(c->dxs); a.x_mpad = mpad;
        a.pos_p = pos; a.n_prompt = k.n_prompt;
        a.part_val = c->part_val + row0; a.part_idx = c->part_idx + row0;   // [part][mpad]: the range's first row of every partial
        return a;
    }
    // ... with the call's two suppress masks: the LM head of an emitting step.  scratch: the rows' raw logits of this position go there instead of
    // the argmax partials being read (beam search, sampling, scoring)
    SkinnyArgs lm_head_masked(float* scratch = nullptr) const {
        SkinnyArgs a = lm_head_common();
        a.mask_first = c->mask_first; a.mask_base = c->mask_base;
        if (scratch) { a.logits = scratch; a.logits_rows = 1; a.logits_cur = true; }
        return a;
    }

    // One decoder layer on the range's rows (the nb rows unless a range is set).  self_attn(): the launch that turns c->dqkv into c->datt (slab layout) — the cached single-position
    // kernel of the token loop, or the scoring pass's causal kernel over a hypothesis's rows.
    // `advance`: nothing follows the layers at this position (a prompt position without a head), so this fc2 advances the position
    template <typename SelfAttn>
    void layer_with(int l, bool advance, SelfAttn&& self_attn) const {
        layer_head(l, self_attn);
        layer_tail(l, advance);
    }
    // ... its launches up to and including the cross-attention query (and after_query): what runs before the layer's stream over the encoder side
    template <typename SelfAttn>
    void layer_head(int l, SelfAttn&& self_attn) const {
        const DecLayerDev& L = m->dec[l];
        {   // LN1 ∘ Q|K|V projection
            Prof pr(c, WH_KG_DEC_GEMM);
            gemm(false, ln_consumer(L.qkv_w, L.qkv_b, L.qkv_sc, L.qkv_s, 3 * d, rm(c->dqkv, 3 * d, prec == WH_PREC_F16X3 ? 4 : m->esz), (l == 0) ? 1 : ln_tiles_d));
        }
        {
            Prof pr(c, WH_KG_DEC_OTHER);
            self_attn();
        }
        {   // self-attention out-proj + residual → x, raw slab, LN2 partials
            Prof pr(c, WH_KG_DEC_GEMM);
            gemm(true, residual_producer(L.o_w, L.o_b, L.o_sc, slab(c->datt), d, L.ln2_w));
        }
        if (c->cross_es) {
            // the attention runs on the encoder states (wh_cross_es.hip): W_k moves to the query side, W_v behind the attention
            {   // LN2 ∘ cross-attention query, kept in f32
                Prof pr(c, WH_KG_DEC_GEMM);
                gemm(true, ln_consumer(L.cq_w, L.cq_b, L.cq_sc, L.cq_s, d, rm(c->dq32, d), ln_tiles_d));
                // expanded queries qe[h] = W_k,h^T q_h: [nb][H][d] f32
                wh_launch_dec_qexpand(s, prec, rm(c->dq32, d), L.cqx_w, rm(c->dqe, D.n_heads * d), nr, (int)d, D.n_heads);
            }
        } else {   // LN2 ∘ cross-attention query
            Prof pr(c, WH_KG_DEC_GEMM);
            gemm(false, ln_consumer(L.cq_w, L.cq_b, L.cq_sc, L.cq_s, d, rm(c->dq, d, prec == WH_PREC_F16X3 ? 4 : m->esz), ln_tiles_d));
        }
        after_query(l);
    }
    // ... and the rest: cross-attention, its out-projection, the feed-forward block
    void layer_tail(int l, bool advance) const {
        const DecLayerDev& L = m->dec[l];
        const long kv_stride = (long)ncl * S * d;  // elements between consecutive [clips][S][d] planes
        const long kv_clip0 = (long)(clip0 + row0) * S * d; // ... and from the plane's first clip to this launch's first
        if (c->cross_es) {
            if (k.al_q && c->al.layer[l].n) {   // word-level timestamps: the listed heads' expanded queries of this position
                Prof pr(c, WH_KG_DEC_OTHER);
                wh_launch_align_copy(s, false, c->dqe, (long)D.n_heads * d, d, (int)d, c->al.layer[l], c->pos, k.n_prompt - 1, k.al_cap, nb, k.al_q);
            }
            {
                Prof pr(c, WH_KG_DEC_CROSS_ATTN);
                wh_launch_dec_cross_attn_es(s, prec, rm(c->dqe, D.n_heads * d), (const char*)c->es_E + (long)(clip0 + row0) * c->es_rows * d * m->esz, slab(c->dctx), (int)S,
                                            c->es_rows, nr, mpad, kv_nt, es_cus, rpc);
            }
            {   // per head: W_v,h ctx_h + b_v,h → the attention output the out-projection below expects (slab layout)
                Prof pr(c, WH_KG_DEC_GEMM);
                SkinnyArgs a;
                a.X = slab(c->dctx); a.x_mpad = mpad; a.W = L.cv_w; a.bias = L.cv_b; a.C = slab(c->datt); a.c_mpad = mpad;
                a.M = nr; a.m_sel = nb; a.N = WH_HEAD_DIM; a.K = (int)d;
                a.zn = D.n_heads; a.x_zs = (long)(d / 32) * mpad * 32; a.w_zs = (long)WH_HEAD_DIM * d; a.c_zs = (long)(WH_HEAD_DIM / 32) * mpad * 32;
                a.bias_zs = WH_HEAD_DIM;
                if (f8) wh_launch_dec_gemm(s, WH_PREC_BF16, false, a);   // (fp8 mode: cv_w is the quantised model's W_v, code x row scale, as bf16 — wh_model.cpp)
                else gemm(false, a);
            }
        } else {
            if (k.al_q && c->al.layer[l].n) {   // word-level timestamps: the listed heads' queries of this position
                Prof pr(c, WH_KG_DEC_OTHER);
                wh_launch_align_copy(s, m->esz == 2, c->dq, d, WH_HEAD_DIM, WH_HEAD_DIM, c->al.layer[l], c->pos, k.n_prompt - 1, k.al_cap, nb, k.al_q);
            }
            Prof pr(c, WH_KG_DEC_CROSS_ATTN);
            if (f8)
                wh_launch_dec_cross_attn8(s, c->dq, (char*)c->cross_kv8 + (2 * l) * kv_stride, (char*)c->cross_kv8 + (2 * l + 1) * kv_stride,
                                          c->kv_amax + (long)(2 * l) * nb * D.n_heads, c->kv_amax + (long)(2 * l + 1) * nb * D.n_heads,
                                          c->cpart, c->cml, (int)S, (int)d, D.n_heads, c->cross_splits, nb, c->datt, mpad, kv_nt);
            else
                wh_launch_dec_cross_attn(s, prec, rm(c->dq, d, prec == WH_PREC_F16X3 ? 4 : m->esz), (char*)c->cross_kv + ((2 * l) * kv_stride + kv_clip0) * m->esz,
                                         (char*)c->cross_kv + ((2 * l + 1) * kv_stride + kv_clip0) * m->esz,
                                         rm(c->cpart, c->cross_splits * d), rm(c->cml, (long)c->cross_splits * D.n_heads * 2), (int)S, (int)d, D.n_heads, c->cross_splits, nr,
                                         slab(c->datt), mpad, kv_nt, rpc);
        }
        {   // merge of the key ranges ∘ cross-attention out-proj + residual → x, raw slab, LN3 partials
            Prof pr(c, WH_KG_DEC_GEMM);
            const bool merged = c->cross_splits == 1 || c->cross_es;   // one key range per clip: the attention kernel wrote its output itself
            SkinnyArgs a = residual_producer(L.co_w, L.co_b, L.co_sc, merged ? slab(c->datt) : nullptr, d, L.ln3_w);
            if (!merged) { a.xpart = rm(c->cpart, c->cross_splits * d); a.xml = rm(c->cml, (long)c->cross_splits * D.n_heads * 2); a.x_splits = c->cross_splits; a.x_heads = D.n_heads; }
            gemm(true, a);
        }
        {   // LN3 ∘ fc1 + GELU (slab output)
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = ln_consumer(L.fc1_w, L.fc1_b, L.fc1_sc, L.fc1_s, D.ffn, slab(c->dh), ln_tiles_d, true);
            a.act = 1;
            gemm(false, a);
        }
        {   // fc2 + residual → x, raw slab, partials for the next layer's LN1 / the final LN
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = residual_producer(L.fc2_w, L.fc2_b, L.fc2_sc, slab(c->dh), D.ffn, (l + 1 < D.dec_layers) ? m->dec[l + 1].ln1_w : m->dec_ln_w);
            if (advance) { a.ticket = ticket; a.pos_w = pos; }
            gemm(true, a);
        }
    }
};

}  // namespace wh
