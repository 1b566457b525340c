// wh_score_host.cpp — the host side of wh_score_tokens: log p(given tokens | audio) of many hypotheses in one decoder pass
// over all their positions.  Hypothesis g of a pass occupies the T adjacent rows g * T .. g * T + T - 1 of the decode workspace, row g * T + t
// being model position t of prompt ++ tokens (padded with the filler id).  A pass is one token + position embedding, per decoder layer the
// launch list of a token-loop position (StepBase::layer_with) with the causal k_score_self_attn in place of the cached kernel, one LM head
// into the [max_batch][vocab] scratch and k_score_finish.  Nothing is captured; the self-attention caches are not touched.
#include "wh_step.h"

namespace wh {

// everything the call decides before it touches the device
struct ScorePlan {
    int ncl = 0, H = 0, n_hyp = 0, P = 0, Lmax = 0, T = 0, clips_per_pass = 0;
    std::vector<int> len;   // [n_hyp]
};

// all validation; no HIP call
static int plan_score(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, float* logprob_out, size_t cap_tokens, const int32_t* logit_hyps,
                      size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows, ScorePlan& pl) {
    const wh_dims& D = c->m->dims;
    if (!in || in->struct_size != sizeof(wh_score_input))
        return fail(c, WH_ERR_ARG, "wh_score_tokens: struct_size %zu, expected %zu", in ? in->struct_size : (size_t)0, sizeof(wh_score_input));
    if (!c->have_enc) return fail(c, WH_ERR_STATE, "Missing cached decoder input: encoder states (call wh_transcribe_batch or wh_encode first)");
    if (c->pre_valid) return fail(c, WH_ERR_STATE, "the resident encoder states belong to a prefetched batch that has not been transcribed yet");
    if (c->m->prec != WH_PREC_F32 && c->m->prec != WH_PREC_BF16)
        return fail(c, WH_ERR_UNSUPPORTED, "wh_score_tokens: not supported in the %s mode (only the f32 and bf16 cross-attention kernels share a clip between rows)",
                    c->m->prec == WH_PREC_FP8 ? "fp8" : "f16x3");
    const char* opt = c->ts.on ? "timestamp rules" : c->rep.on ? "repetition controls" : c->sm.on ? "sampling" : c->bm.on ? "beam search" : c->al.on ? "alignment"
                      : c->lang.on ? "language detection" : nullptr;
    if (c->pfx.on && !c->pfx.ids.empty()) opt = "a non-empty prefix";
    if (opt) return fail(c, WH_ERR_UNSUPPORTED, "wh_score_tokens: %s set on the ctx is not supported (clear it first)", opt);
    if (p->n_forced != 0) return fail(c, WH_ERR_ARG, "wh_score_tokens: forced tokens are not taken (the hypotheses are the history)");
    const int P = pl.P = (int)p->n_prompt;
    if (P <= 0 || !p->prompt || p->n_prompt > (size_t)D.n_text_ctx) return fail(c, WH_ERR_ARG, "wh_score_tokens: empty prompt, or one beyond %d positions", D.n_text_ctx);
    for (int i = 0; i < P; i++)
        if (p->prompt[i] < 0 || p->prompt[i] >= D.vocab) return fail(c, WH_ERR_ARG, "wh_score_tokens: prompt id %lld outside the vocabulary", (long long)p->prompt[i]);
    const int ncl = pl.ncl = c->enc_batch;
    if (in->hyps_per_clip < 1 || in->hyps_per_clip > (size_t)c->max_batch || in->n_hyp != (size_t)ncl * in->hyps_per_clip)
        return fail(c, WH_ERR_ARG, "wh_score_tokens: n_hyp %zu is not %d resident clips x hyps_per_clip %zu (1 .. max_batch)", in->n_hyp, ncl, in->hyps_per_clip);
    const int H = pl.H = (int)in->hyps_per_clip, n_hyp = pl.n_hyp = ncl * H;
    if (!in->ids || !in->offsets || in->offsets[0] != 0) return fail(c, WH_ERR_ARG, "wh_score_tokens: NULL ids or offsets, or offsets[0] != 0");
    pl.len.resize(n_hyp);
    size_t longest = 0;
    for (int g = 0; g < n_hyp; g++) {
        if (in->offsets[g + 1] <= in->offsets[g]) return fail(c, WH_ERR_ARG, "wh_score_tokens: offsets not strictly increasing at hypothesis %d (every hypothesis has >= 1 token)", g);
        const size_t n = in->offsets[g + 1] - in->offsets[g];
        longest = std::max(longest, n);
        if (P + longest > (size_t)D.n_text_ctx)
            return fail(c, WH_ERR_ARG, "wh_score_tokens: prompt (%d) + hypothesis %d (%zu tokens) exceeds %d positions", P, g, n, D.n_text_ctx);
        pl.len[g] = (int)n;
    }
    for (size_t i = 0; i < in->offsets[n_hyp]; i++)
        if (in->ids[i] < 0 || in->ids[i] >= D.vocab) return fail(c, WH_ERR_ARG, "wh_score_tokens: id %lld outside the vocabulary", (long long)in->ids[i]);
    pl.Lmax = (int)longest;
    pl.T = P + pl.Lmax - 1;
    if (!logprob_out || cap_tokens < longest) return fail(c, WH_ERR_ARG, "wh_score_tokens: logprob_out needs %zu entries per hypothesis", longest);
    if (n_logit_hyps && !logit_hyps) return fail(c, WH_ERR_ARG, "wh_score_tokens: NULL logit_hyps with a non-zero count");
    for (size_t k = 0; k < n_logit_hyps; k++) {
        if (logit_hyps[k] < 0 || logit_hyps[k] >= n_hyp) return fail(c, WH_ERR_ARG, "wh_score_tokens: logit_hyps[%zu] = %d outside the %d hypotheses", k, (int)logit_hyps[k], n_hyp);
        if (logits_out && cap_logits_rows < (size_t)pl.len[logit_hyps[k]])
            return fail(c, WH_ERR_ARG, "wh_score_tokens: logits_out needs %d rows for hypothesis %d", pl.len[logit_hyps[k]], (int)logit_hyps[k]);
    }
    if ((long)H * pl.T > c->max_batch)
        return fail(c, WH_ERR_ARG, "wh_score_tokens: %d hypotheses per clip x %d positions exceed max_batch (%d rows)", H, pl.T, c->max_batch);
    pl.clips_per_pass = c->max_batch / (H * pl.T);
    return WH_OK;
}

// the scoring call's own buffers, allocated by the first call
static int ensure_score_buffers(wh_ctx* c) {
    const size_t B = (size_t)c->max_batch;
    if (int rc = grow(c, c->sc.logits, B * c->m->dims.vocab * 4, false, GROW_FREE_FIRST, "the scoring logits")) return rc;
    Carver cv;
    const size_t o_tok = cv.take((B + c->m->dims.n_text_ctx) * 4), o_off = cv.take(B * 4), o_len = cv.take(B * 4), o_tgt = cv.take(B * 4), o_lp = cv.take(B * 4),
                 o_am = cv.take(B * 4);
    if (!c->sc.buf) {
        if (int rc = grow(c, c->sc.buf, cv.off, false, GROW_FREE_FIRST, "the scoring state")) return rc;
        wh_ctx::Scoring& sc = c->sc;
        sc.tok = at<int>(sc.buf, o_tok); sc.off = at<int>(sc.buf, o_off); sc.len = at<int>(sc.buf, o_len); sc.target = at<int>(sc.buf, o_tgt);
        sc.lp = at<float>(sc.buf, o_lp); sc.am = at<int>(sc.buf, o_am);
        CTX_HIP(c, hipMemset(sc.tok, 0, (B + c->m->dims.n_text_ctx) * 4));
    }
    return WH_OK;
}

// one pass: the hypotheses of clips clip0 .. clip0 + nc - 1, G = nc * H of them, R = G * T rows
static int score_pass(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, const ScorePlan& pl, const wh_ctx::StepKey& key_all, int clip0, int nc,
                      float* logprob_out, int64_t* argmax_out, size_t cap_tokens, const int32_t* logit_hyps, size_t n_logit_hyps, float* logits_out,
                      size_t cap_logits_rows) {
    hipStream_t s = c->stream;
    const wh_dims& D = c->m->dims;
    const int H = pl.H, T = pl.T, P = pl.P, Lmax = pl.Lmax, G = nc * H, R = G * T, g0 = clip0 * H;
    const int filler = p->eot >= 0 && p->eot < D.vocab ? (int)p->eot : 0;
    std::vector<int> tok((size_t)R, filler), off((size_t)R), target((size_t)G * Lmax, 0);
    for (int g = 0; g < G; g++) {
        const int64_t* t = in->ids + in->offsets[g0 + g];
        const int n = pl.len[g0 + g];
        for (int i = 0; i < P; i++) tok[(size_t)g * T + i] = (int)p->prompt[i];
        for (int i = 0; i + 1 < n; i++) tok[(size_t)g * T + P + i] = (int)t[i];   // (the last token is a target only)
        for (int i = 0; i < n; i++) target[(size_t)g * Lmax + i] = (int)t[i];
        for (int i = 0; i < T; i++) off[(size_t)g * T + i] = T - 1 - i;
    }
    wh_ctx::Scoring& sc = c->sc;
    CTX_HIP(c, hipMemcpyAsync(sc.tok + (T - 1), tok.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(sc.off, off.data(), (size_t)R * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(sc.len, pl.len.data() + g0, (size_t)G * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(sc.target, target.data(), target.size() * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipStreamSynchronize(s));   // (pageable host vectors)
    wh_ctx::StepKey key = key_all;
    key.nb = R;
    const StepBase t(c, key, H * T, pl.ncl, clip0);
    {   // every row embeds its own (token, position): k_dec_embed<T, true> at global position T - 1 with the row's offset T - 1 - t
        Prof pr(c, WH_KG_DEC_OTHER);
        wh_launch_dec_embed(s, t.prec, t.m->tok_emb, t.m->dec_pos, sc.tok, 1, c->pos, c->dx, c->dxs, c->lnpart, R, (int)t.d, t.mpad, nullptr, c->dshift, sc.off);
    }
    const bool tm = sc.timing;
    for (int l = 0; l < D.dec_layers; l++)
        t.layer_with(l, false, [&] {
            std::array<hipEvent_t, 2> te = {nullptr, nullptr};
            if (tm) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
            wh_launch_score_self_attn(s, t.prec, c->dqkv, c->datt, (int)t.d, D.n_heads, T, G, t.mpad);
            if (tm) { hipEventRecord(te[1], s); sc.ev_attn.push_back(te); }
        });
    {
        Prof pr(c, WH_KG_DEC_GEMM);
        wh_launch_lm_head(s, t.prec, t.lm_head_masked(sc.logits));
    }
    {
        Prof pr(c, WH_KG_DEC_OTHER);
        std::array<hipEvent_t, 2> te = {nullptr, nullptr};
        if (tm) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
        wh_launch_score_finish(s, sc.logits, D.vocab, c->mask_first, c->mask_base, R, T, P, Lmax, sc.len, sc.target, sc.lp, sc.am);
        if (tm) { hipEventRecord(te[1], s); sc.ev_finish.push_back(te); }
    }
    std::vector<float> lp((size_t)G * Lmax);
    std::vector<int> am((size_t)G * Lmax);
    CTX_HIP(c, hipMemcpyAsync(lp.data(), sc.lp, lp.size() * 4, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipMemcpyAsync(am.data(), sc.am, am.size() * 4, hipMemcpyDeviceToHost, s));
    for (size_t k = 0; logits_out && k < n_logit_hyps; k++) {   // parity rows: entry i of a listed hypothesis is the pass's row g * T + P - 1 + i
        const int g = logit_hyps[k] - g0;
        if (g < 0 || g >= G) continue;
        CTX_HIP(c, hipMemcpyAsync(logits_out + k * cap_logits_rows * D.vocab, sc.logits + ((size_t)g * T + P - 1) * D.vocab, (size_t)pl.len[g0 + g] * D.vocab * 4,
                                  hipMemcpyDeviceToHost, s));
    }
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    for (int g = 0; g < G; g++)
        for (int i = 0; i < pl.len[g0 + g]; i++) {
            logprob_out[(size_t)(g0 + g) * cap_tokens + i] = lp[(size_t)g * Lmax + i];
            if (argmax_out) argmax_out[(size_t)(g0 + g) * cap_tokens + i] = am[(size_t)g * Lmax + i];
        }
    return WH_OK;
}

int run_score(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, float* logprob_out, int64_t* argmax_out, size_t cap_tokens,
              const int32_t* logit_hyps, size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows) {
    ScorePlan pl;
    if (int rc = plan_score(c, p, in, logprob_out, cap_tokens, logit_hyps, n_logit_hyps, logits_out, cap_logits_rows, pl)) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    hipStream_t s = c->stream;
    c->cur = s;
    const wh_dims& D = c->m->dims;
    if (int rc = ensure_score_buffers(c)) return rc;
    // entries past a hypothesis's end are 0
    for (size_t i = 0; i < (size_t)pl.n_hyp * cap_tokens; i++) logprob_out[i] = 0.0f;
    if (argmax_out) for (size_t i = 0; i < (size_t)pl.n_hyp * cap_tokens; i++) argmax_out[i] = 0;
    if (c->s_enc != s) CTX_HIP(c, hipStreamWaitEvent(s, c->ev_enc_done, 0));   // the encoder states come from the encoder stream
    CTX_HIP(c, hipEventRecord(c->ev[5], s));
    std::vector<unsigned> mfirst, mbase;
    pack_mask(p->suppress, p->n_suppress, p->begin_suppress, p->n_begin_suppress, D.vocab, mfirst);
    pack_mask(p->suppress, p->n_suppress, nullptr, 0, D.vocab, mbase);
    CTX_HIP(c, hipMemcpyAsync(c->mask_first, mfirst.data(), mfirst.size() * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->mask_base, mbase.data(), mbase.size() * 4, hipMemcpyHostToDevice, s));
    // every kernel of the pass that reads the position sees T - 1: the embedding's rows are right-aligned to it, and the LM head (n_prompt 1 in
    // the key below) takes it for a generated position, whose raw logits go to row 0 of each row's scratch slot
    const int pos = pl.T - 1;
    CTX_HIP(c, hipMemcpyAsync(c->pos, &pos, 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    if (int rc = project_cross_kv(c, pl.ncl, nullptr)) return rc;
    wh_ctx::StepKey key;   // no option: the plain kernels
    key.n_prompt = 1; key.eot = (int)p->eot;
    for (int clip0 = 0; clip0 < pl.ncl; clip0 += pl.clips_per_pass)
        if (int rc = score_pass(c, p, in, pl, key, clip0, std::min(pl.clips_per_pass, pl.ncl - clip0), logprob_out, argmax_out, cap_tokens, logit_hyps, n_logit_hyps,
                                logits_out, cap_logits_rows))
            return rc;
    CTX_HIP(c, hipEventRecord(c->ev[3], s));
    CTX_HIP(c, hipStreamSynchronize(s));
    c->sc.collect_timing();
    return WH_OK;
}

}  // namespace wh

// measurement hook (tools/score_bench.py; not in the public header): milliseconds of k_score_self_attn (all layers and passes) and k_score_finish of
// the last scoring call — filled when the context was created under WH_SCORE_TIMING=1
extern "C" int wh_debug_score_times(const wh_ctx* c, double* ms2) {
    if (!c || !ms2 || !c->sc.timing) return WH_ERR_ARG;
    ms2[0] = c->sc.ms[0]; ms2[1] = c->sc.ms[1];
    return WH_OK;
}
