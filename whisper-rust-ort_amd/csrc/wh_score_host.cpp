// wh_score_host.cpp — the host side of wh_score_tokens: log p(given tokens | audio) of many hypotheses in one decoder pass
// over all their positions.  Hypothesis g of a pass occupies the T adjacent rows g * T .. g * T + T - 1 of the decode workspace, row g * T + t
// being model position t of prompt ++ tokens (padded with the filler id).  A pass is one token + position embedding, per decoder layer the
// launch list of a token-loop position (StepBase::layer_with) with the causal k_score_self_attn in place of the cached kernel, one LM head
// into the [max_batch][vocab] scratch and k_score_finish.  Nothing is captured; the self-attention caches are not touched.
// wh_align_tokens is the same pass with k_align_gather behind every listed layer's cross-attention query and the alignment
// post-pass over the pass's hypotheses; its LM head and k_score_finish run only when the caller wants the log-probabilities.
#include "wh_step.h"

namespace wh {

// everything the call decides before it touches the device
struct ScorePlan {
    const char* who = "wh_score_tokens";   // the entry, for the messages
    bool align = false;                    // wh_align_tokens: alignment on the ctx is ignored, logprob_out may be NULL
    int ncl = 0, H = 0, n_hyp = 0, P = 0, Lmax = 0, T = 0, clips_per_pass = 0;
    std::vector<int> len;   // [n_hyp]
};

// all validation; no HIP call
static int plan_score(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, float* logprob_out, size_t cap_tokens, const int32_t* logit_hyps,
                      size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows, ScorePlan& pl) {
    const wh_dims& D = c->m->dims;
    if (!in || in->struct_size != sizeof(wh_score_input))
        return fail(c, WH_ERR_ARG, "%s: struct_size %zu, expected %zu", pl.who, in ? in->struct_size : (size_t)0, sizeof(wh_score_input));
    if (!c->have_enc) return fail(c, WH_ERR_STATE, "Missing cached decoder input: encoder states (call wh_transcribe_batch or wh_encode first)");
    if (c->pre_valid) return fail(c, WH_ERR_STATE, "the resident encoder states belong to a prefetched batch that has not been transcribed yet");
    if (c->m->prec != WH_PREC_F32 && c->m->prec != WH_PREC_BF16)
        return fail(c, WH_ERR_UNSUPPORTED, "%s: not supported in the %s mode (only the f32 and bf16 cross-attention kernels share a clip between rows)", pl.who,
                    c->m->prec == WH_PREC_FP8 ? "fp8" : "f16x3");
    const char* opt = c->ts.on ? "timestamp rules" : c->rep.on ? "repetition controls" : c->sm.on ? "sampling" : c->bm.on ? "beam search" : c->al.on && !pl.align ? "alignment"
                      : c->lang.on ? "language detection" : nullptr;
    if (c->pfx.on && !c->pfx.ids.empty()) opt = "a non-empty prefix";
    if (opt) return fail(c, WH_ERR_UNSUPPORTED, "%s: %s set on the ctx is not supported (clear it first)", pl.who, opt);
    if (p->n_forced != 0) return fail(c, WH_ERR_ARG, "%s: forced tokens are not taken (the hypotheses are the history)", pl.who);
    const int P = pl.P = (int)p->n_prompt;
    if (P <= 0 || !p->prompt || p->n_prompt > (size_t)D.n_text_ctx) return fail(c, WH_ERR_ARG, "%s: empty prompt, or one beyond %d positions", pl.who, D.n_text_ctx);
    for (int i = 0; i < P; i++)
        if (p->prompt[i] < 0 || p->prompt[i] >= D.vocab) return fail(c, WH_ERR_ARG, "%s: prompt id %lld outside the vocabulary", pl.who, (long long)p->prompt[i]);
    const int ncl = pl.ncl = c->enc_batch;
    if (in->hyps_per_clip < 1 || in->hyps_per_clip > (size_t)c->max_batch || in->n_hyp != (size_t)ncl * in->hyps_per_clip)
        return fail(c, WH_ERR_ARG, "%s: n_hyp %zu is not %d resident clips x hyps_per_clip %zu (1 .. max_batch)", pl.who, in->n_hyp, ncl, in->hyps_per_clip);
    const int H = pl.H = (int)in->hyps_per_clip, n_hyp = pl.n_hyp = ncl * H;
    if (!in->ids || !in->offsets || in->offsets[0] != 0) return fail(c, WH_ERR_ARG, "%s: NULL ids or offsets, or offsets[0] != 0", pl.who);
    pl.len.resize(n_hyp);
    size_t longest = 0;
    for (int g = 0; g < n_hyp; g++) {
        if (in->offsets[g + 1] <= in->offsets[g]) return fail(c, WH_ERR_ARG, "%s: offsets not strictly increasing at hypothesis %d (every hypothesis has >= 1 token)", pl.who, g);
        const size_t n = in->offsets[g + 1] - in->offsets[g];
        longest = std::max(longest, n);
        if (P + longest > (size_t)D.n_text_ctx)
            return fail(c, WH_ERR_ARG, "%s: prompt (%d) + hypothesis %d (%zu tokens) exceeds %d positions", pl.who, P, g, n, D.n_text_ctx);
        pl.len[g] = (int)n;
    }
    for (size_t i = 0; i < in->offsets[n_hyp]; i++)
        if (in->ids[i] < 0 || in->ids[i] >= D.vocab) return fail(c, WH_ERR_ARG, "%s: id %lld outside the vocabulary", pl.who, (long long)in->ids[i]);
    pl.Lmax = (int)longest;
    pl.T = P + pl.Lmax - 1;
    if ((!logprob_out && !pl.align) || cap_tokens < longest) return fail(c, WH_ERR_ARG, "%s: the outputs need %zu entries per hypothesis", pl.who, longest);
    if (n_logit_hyps && !logit_hyps) return fail(c, WH_ERR_ARG, "%s: NULL logit_hyps with a non-zero count", pl.who);
    for (size_t k = 0; k < n_logit_hyps; k++) {
        if (logit_hyps[k] < 0 || logit_hyps[k] >= n_hyp) return fail(c, WH_ERR_ARG, "%s: logit_hyps[%zu] = %d outside the %d hypotheses", pl.who, k, (int)logit_hyps[k], n_hyp);
        if (logits_out && cap_logits_rows < (size_t)pl.len[logit_hyps[k]])
            return fail(c, WH_ERR_ARG, "%s: logits_out needs %d rows for hypothesis %d", pl.who, pl.len[logit_hyps[k]], (int)logit_hyps[k]);
    }
    if ((long)H * pl.T > c->max_batch)
        return fail(c, WH_ERR_ARG, "%s: %d hypotheses per clip x %d positions exceed max_batch (%d rows)", pl.who, H, pl.T, c->max_batch);
    pl.clips_per_pass = c->max_batch / (H * pl.T);
    return WH_OK;
}

// what wh_align_tokens adds to a scoring call: the head list, the outputs, and what a pass needs of them
struct AlignCall {
    std::vector<int> heads, debug;          // [n][2] (layer, head); the debug hypotheses
    std::vector<AlignLayerHeads> layer;     // [dec_layers]
    int32_t* frames_out = nullptr;
    int32_t* n_frames_out = nullptr;
    std::vector<int> sb;                    // [n_hyp] S_b of each hypothesis's clip
    int *frames = nullptr, *d_sb = nullptr, *n_out = nullptr;   // the carve of wh_ctx::ForcedAlign::ints
};

// the scoring call's own buffers, allocated by the first call (the logits scratch: by the first call that runs the LM head)
static int ensure_score_buffers(wh_ctx* c, bool want_logits) {
    const size_t B = (size_t)c->max_batch;
    if (want_logits)
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
                      size_t cap_logits_rows, AlignCall* ac) {
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
    StepBase t(c, key, H * T, pl.ncl, clip0);
    const bool gather = ac && Lmax > 1;   // (one token per hypothesis: every frame is 0, nothing to launch)
    const int nh = ac ? (int)(ac->heads.size() / 2) : 0;
    if (gather) {
        if (int rc = grow(c, c->fa.q, (size_t)nh * G * Lmax * align_dk(c) * 4, false, GROW_FREE_FIRST, "the forced alignment queries")) return rc;
        const bool tmg = c->al.timing;
        t.query_hook = [&, tmg](int l) {   // the listed heads' queries of every row that is an entry of its hypothesis
            if (!ac->layer[l].n) return;
            Prof pr(c, WH_KG_DEC_OTHER);
            std::array<hipEvent_t, 2> te = {nullptr, nullptr};
            if (tmg) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
            if (c->cross_es) wh_launch_align_gather(s, false, c->dqe, (long)D.n_heads * t.d, t.d, (int)t.d, ac->layer[l], R, T, P, Lmax, c->sc.len, G, c->fa.q);
            else wh_launch_align_gather(s, t.m->esz == 2, c->dq, t.d, WH_HEAD_DIM, WH_HEAD_DIM, ac->layer[l], R, T, P, Lmax, c->sc.len, G, c->fa.q);
            if (tmg) { hipEventRecord(te[1], s); c->fa.ev_gather.push_back(te); }
        };
    }
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
    if (gather) {   // the post-pass over the pass's hypotheses: row g reads the keys of clip clip0 + g / H
        std::vector<int> nout((size_t)G);
        for (int g = 0; g < G; g++) nout[g] = P + pl.len[g0 + g];
        CTX_HIP(c, hipMemcpyAsync(ac->n_out, nout.data(), (size_t)G * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(ac->d_sb, ac->sb.data() + g0, (size_t)G * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemsetAsync(ac->frames, 0, (size_t)G * Lmax * 4, s));
        CTX_HIP(c, hipStreamSynchronize(s));   // (pageable host vector)
        AlignArgs a;
        a.q = c->fa.q;
        const int form = align_keys(c, ac->heads, pl.ncl, a);
        a.k_div = H; a.k_clip0 = clip0;
        a.n_out = ac->n_out; a.n_prompt = P; a.cap = Lmax; a.sb = ac->d_sb;
        a.nb = G; a.n_heads = nh; a.S = D.n_audio_ctx; a.Sp = (D.n_audio_ctx + 3) / 4 * 4;
        a.frames = ac->frames; a.frames_ld = Lmax;
        std::vector<int> dbg_rows(ac->debug.size());
        for (size_t k = 0; k < ac->debug.size(); k++) dbg_rows[k] = ac->debug[k] >= g0 && ac->debug[k] < g0 + G ? ac->debug[k] - g0 : -1;
        if (int rc = align_post_pass(c, a, form, c->fa.ws, dbg_rows, c->al.dbg)) return rc;
        std::vector<int> fr((size_t)G * Lmax);
        CTX_HIP(c, hipMemcpyAsync(fr.data(), ac->frames, fr.size() * 4, hipMemcpyDeviceToHost, s));
        CTX_HIP(c, hipStreamSynchronize(s));
        for (int g = 0; g < G; g++)
            for (int i = 0; i < pl.len[g0 + g]; i++) ac->frames_out[(size_t)(g0 + g) * cap_tokens + i] = fr[(size_t)g * Lmax + i];
    }
    for (size_t k = 0; ac && k < ac->debug.size(); k++) {   // the debug hypotheses' slots cut to [n_heads][n_h][S_b] and [n_h][S_b] (zeros for n_h == 1)
        const int h = ac->debug[k];
        if (h < g0 || h >= g0 + G) continue;
        wh_ctx::AlignDebug& dbg = c->al.dbg[k];
        const int n = pl.len[h], sb = ac->sb[h], Sp = (D.n_audio_ctx + 3) / 4 * 4;
        std::vector<float> pr((size_t)nh * n * sb, 0.0f), mt((size_t)n * sb, 0.0f);
        if (!dbg.probs.empty() && n > 1)
            for (int hd = 0; hd < nh; hd++)
                for (int i = 0; i < n; i++) std::copy_n(dbg.probs.begin() + ((size_t)hd * Lmax + i) * Sp, sb, pr.begin() + ((size_t)hd * n + i) * sb);
        if (!dbg.matrix.empty() && n > 1)
            for (int i = 0; i < n; i++) std::copy_n(dbg.matrix.begin() + (size_t)i * Sp, sb, mt.begin() + (size_t)i * sb);
        dbg.n_heads = nh; dbg.n_gen = n; dbg.sb = sb;
        dbg.probs.swap(pr);
        dbg.matrix.swap(mt);
    }
    if (!logprob_out) {   // (wh_align_tokens without log-probabilities: no LM head, no k_score_finish)
        CTX_HIP(c, hipStreamSynchronize(s));
        CTX_HIP(c, hipGetLastError());
        return WH_OK;
    }
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

// the planned call: the passes over the resident clips (ac: with the alignment of wh_align_tokens)
static int run_passes(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, const ScorePlan& pl, float* logprob_out, int64_t* argmax_out, size_t cap_tokens,
                      const int32_t* logit_hyps, size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows, AlignCall* ac) {
    CTX_HIP(c, hipSetDevice(c->m->device));
    hipStream_t s = c->stream;
    c->cur = s;
    const wh_dims& D = c->m->dims;
    if (int rc = ensure_score_buffers(c, logprob_out != nullptr)) return rc;
    if (ac) {
        const size_t B = (size_t)c->max_batch;   // frames: G * Lmax <= G * T <= max_batch
        if (int rc = grow(c, c->fa.ints, 3 * B * 4, false, GROW_FREE_FIRST, "the forced alignment state")) return rc;
        ac->frames = c->fa.ints; ac->d_sb = ac->frames + B; ac->n_out = ac->d_sb + B;
        for (size_t i = 0; i < (size_t)pl.n_hyp * cap_tokens; i++) ac->frames_out[i] = 0;
        for (int g = 0; ac->n_frames_out && g < pl.n_hyp; g++) ac->n_frames_out[g] = ac->sb[g];
        c->al.dbg.assign(ac->debug.size(), wh_ctx::AlignDebug());
        c->al.ms[0] = c->al.ms[1] = c->al.ms[2] = 0;
    }
    // entries past a hypothesis's end are 0
    for (size_t i = 0; logprob_out && i < (size_t)pl.n_hyp * cap_tokens; i++) logprob_out[i] = 0.0f;
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
                                logits_out, cap_logits_rows, ac))
            return rc;
    CTX_HIP(c, hipEventRecord(c->ev[3], s));
    CTX_HIP(c, hipStreamSynchronize(s));
    c->sc.collect_timing();
    if (ac) {
        c->fa.ms_gather = 0;
        wh_drain_events(c->fa.ev_gather, &c->fa.ms_gather);
        c->al.have_dbg = !ac->debug.empty();
    }
    return WH_OK;
}

int run_score(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, float* logprob_out, int64_t* argmax_out, size_t cap_tokens,
              const int32_t* logit_hyps, size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows) {
    ScorePlan pl;
    if (int rc = plan_score(c, p, in, logprob_out, cap_tokens, logit_hyps, n_logit_hyps, logits_out, cap_logits_rows, pl)) return rc;
    return run_passes(c, p, in, pl, logprob_out, argmax_out, cap_tokens, logit_hyps, n_logit_hyps, logits_out, cap_logits_rows, nullptr);
}

// wh_align_tokens: everything wh_score_tokens refuses (but alignment set on the ctx, which is ignored), then the head list's own argument errors
int run_align_tokens(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, const wh_alignment_opts* heads, int32_t* frames_out, int32_t* n_frames_out,
                     float* logprob_out, size_t cap_tokens) {
    ScorePlan pl;
    pl.who = "wh_align_tokens"; pl.align = true;
    if (int rc = plan_score(c, p, in, logprob_out, cap_tokens, nullptr, 0, nullptr, 0, pl)) return rc;
    if (!heads) return fail(c, WH_ERR_ARG, "wh_align_tokens: NULL alignment heads");
    if (int rc = alignment_opts_check(c, heads, "wh_align_tokens")) return rc;
    for (size_t k = 0; k < heads->n_debug_rows; k++)
        if (heads->debug_rows[k] >= pl.n_hyp) return fail(c, WH_ERR_ARG, "wh_align_tokens: debug hypothesis %d outside the %d hypotheses", (int)heads->debug_rows[k], pl.n_hyp);
    if (!frames_out) return fail(c, WH_ERR_ARG, "wh_align_tokens: frames_out is NULL");
    if (c->cross_es && !wh_align_scores_supported(WH_ALIGN_ES_BF16, c->m->dims.d_model))
        return fail(c, WH_ERR_UNSUPPORTED, "wh_align_tokens: no score kernel for encoder states %d wide", c->m->dims.d_model);
    AlignCall ac;
    ac.heads.assign(heads->heads, heads->heads + 2 * heads->n_heads);
    ac.debug.assign(heads->debug_rows, heads->debug_rows + heads->n_debug_rows);
    alignment_layers(c->m->dims, heads, ac.layer);
    ac.frames_out = frames_out; ac.n_frames_out = n_frames_out;
    ac.sb.resize(pl.n_hyp);
    for (int g = 0; g < pl.n_hyp; g++) {   // frames of the hypothesis's clip, as a decode call counts them (upload_token_state)
        const int b = g / pl.H, nf = (size_t)b < c->enc_nframes.size() ? c->enc_nframes[b] : WH_N_FRAMES;
        ac.sb[g] = std::min(c->m->dims.n_audio_ctx, std::max(8, (nf + 1) / 2));
    }
    return run_passes(c, p, in, pl, logprob_out, nullptr, cap_tokens, nullptr, 0, nullptr, 0, &ac);
}

}  // namespace wh

// measurement hook (tools/score_bench.py; not in the public header): milliseconds of k_score_self_attn (all layers and passes) and k_score_finish of
// the last scoring call — filled when the context was created under WH_SCORE_TIMING=1
extern "C" int wh_debug_score_times(const wh_ctx* c, double* ms2) {
    if (!c || !ms2 || !c->sc.timing) return WH_ERR_ARG;
    ms2[0] = c->sc.ms[0]; ms2[1] = c->sc.ms[1];
    return WH_OK;
}

// measurement hook (tools/forced_align_bench.py; not in the public header): milliseconds of k_align_gather (all layers and passes) and of the three
// post-pass kernels of the last wh_align_tokens call — filled when the context was created under WH_ALIGN_TIMING=1
extern "C" int wh_debug_forced_align_times(const wh_ctx* c, double* ms4) {
    if (!c || !ms4 || !c->al.timing) return WH_ERR_ARG;
    ms4[0] = c->fa.ms_gather;
    for (int i = 0; i < 3; i++) ms4[1 + i] = c->al.ms[i];
    return WH_OK;
}
