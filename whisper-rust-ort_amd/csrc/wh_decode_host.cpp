// wh_decode_host.cpp — the host side of a decode call (greedy_decode_with_past, reference src/main.rs:753-829): run_decode and its stages — the
// plan, the token state, the cross-K/V projection, one decoder position (Step), the captured step and the token loop, the alignment post-pass
// and the two read-backs.
#include "wh_step.h"

namespace wh {

void pack_mask(const int64_t* a, size_t na, const int64_t* b, size_t nb, int vocab, std::vector<unsigned>& out) {
    out.assign((size_t)vocab / 32 + 1, 0u);
    for (size_t i = 0; i < na; i++)
        if (a[i] >= 0 && a[i] < vocab) out[a[i] >> 5] |= 1u << (a[i] & 31);
    for (size_t i = 0; i < nb; i++)
        if (b[i] >= 0 && b[i] < vocab) out[b[i] >> 5] |= 1u << (b[i] & 31);
}

// ---- cross-KV + greedy loop for the nb clips whose encoder states are resident ------------------
// run_decode (below) is a sequence of stages: plan_decode -> upload_token_state -> prepare_logits -> project_cross_kv -> the prompt
// positions (launch_step, eagerly) -> run_token_loop (the captured step) -> read_back.

// Everything a decode call decides before it touches the device: the step's key (but for the logits addresses) and what only the host needs.
struct DecodePlan {
    wh_ctx::StepKey key;   // key.n_prompt = PP, key.pfx: see below
    int P = 0, NEW = 0;
    // per-clip prefixes: row b is idle for Nmax - plen[b] global positions, then runs prefix_b ++ prompt; every row reaches prompt[0] at
    // global position Nmax, so on the device the prompt is simply PP = Nmax + P positions long.  key.pfx = Nmax > 0
    // (all prefixes empty: exactly the launches of a context without prefixes)
    int Nmax = 0;
    std::vector<int> plen;
    std::vector<const int64_t*> pids;
    // language detection: per-row detection at prompt position lang_sot_index (lang_det), or — later batches of a long-form call — the
    // language of the file's first window as an ordinary prompt token (lang_fix).  Either way the caller's prompt[lang_slot] is a placeholder.
    bool lang_det = false, lang_fix = false, lp_probe = false;
    int lang_slot = -1;
    int lang_pos = -1, probe_pos = -1;   // global positions whose logits language detection / the no-speech probe read (-1: none)
    // logits kept for the parity harness: n_lrows rows of the batch (sel_map[b] = slot of row b, when the caller selects rows)
    bool want_logits = false;
    size_t n_lrows = 0;
    std::vector<int> sel_map;
    // beam search: key.nb rows = ncl clips x K beams (off: K == 1, ncl == key.nb)
    int K = 1, ncl = 0;
};

static int choose_split(const wh_ctx* c, const wh_ctx::StepKey& key);   // (the split token loop, below)
static bool choose_free(wh_ctx* c, const wh_ctx::StepKey& key, bool want_logits);   // (the free-running halves, below)

// all validation; no HIP call
static int plan_decode(wh_ctx* c, int ncl, const wh_decode_params* p, bool want_logits, size_t logits_rows, const int32_t* sel, size_t n_sel, DecodePlan& pl) {
    const wh_dims& D = c->m->dims;
    if (int rc = options_check(c, p, ncl, c->pfx.win_base >= 0)) return rc;
    const int K = pl.K = c->bm.on ? c->bm.k : 1, nb = ncl * K;   // the rows of the device batch
    pl.ncl = ncl;
    const int P = pl.P = (int)p->n_prompt, NEW = pl.NEW = (int)p->max_new_tokens;
    if (P <= 0 || NEW <= 0 || !p->prompt) return fail(c, WH_ERR_ARG, "decode: empty prompt or max_new_tokens == 0");
    if (P + NEW > D.n_text_ctx) return fail(c, WH_ERR_ARG, "decode: prompt (%d) + max_new_tokens (%d) exceeds %d positions", P, NEW, D.n_text_ctx);
    if (p->n_forced > (size_t)NEW) return fail(c, WH_ERR_ARG, "decode: more forced tokens than max_new_tokens");
    pl.lang_fix = c->lang.on && c->lang.fixed >= 0;
    pl.lang_det = c->lang.on && !pl.lang_fix;
    const int lang_slot = pl.lang_slot = c->lang.on ? c->lang.sot_index + 1 : -1;
    if (c->lang.on && lang_slot >= P)
        return fail(c, WH_ERR_ARG, "decode: language detection's sot_index %d + 1 is not below n_prompt (%d)", c->lang.sot_index, P);
    for (int i = 0; i < P; i++)
        if (i != lang_slot && (p->prompt[i] < 0 || p->prompt[i] >= D.vocab)) return fail(c, WH_ERR_ARG, "decode: prompt id %lld outside the vocabulary", (long long)p->prompt[i]);
    for (size_t i = 0; i < p->n_forced; i++)
        if (p->forced[i] < 0 || p->forced[i] >= D.vocab) return fail(c, WH_ERR_ARG, "decode: forced id outside the vocabulary");
    if (c->ts.on) {   // timestamp rules: <|0.00|> must lie above EOT (so EOT and the specials are text ids) and inside the vocabulary
        if (c->ts.begin <= p->eot || c->ts.begin >= D.vocab)
            return fail(c, WH_ERR_ARG, "decode: timestamp_begin %lld outside (eot %lld, vocab %d)", (long long)c->ts.begin, (long long)p->eot, D.vocab);
        for (int i = 0; i < P; i++)
            if (i != lang_slot && c->ts.no_ts >= 0 && p->prompt[i] == c->ts.no_ts) return fail(c, WH_ERR_ARG, "decode: the prompt holds <|notimestamps|> while timestamp rules are on");
    }
    pl.lp_probe = c->lp.on && c->lp.no_speech >= 0;
    if (pl.lp_probe && c->lp.sot_index >= P - 1)   // the probe reads a prompt position that emits nothing
        return fail(c, WH_ERR_ARG, "decode: the no-speech probe's sot_index %d is not below n_prompt - 1 (%d)", c->lp.sot_index, P - 1);
    pl.plen.assign(nb, 0);
    pl.pids.assign(nb, nullptr);
    if (c->pfx.on)
        for (int b = 0; b < nb; b++) {
            pl.pids[b] = prefix_of(c, c->pfx.win_base, b / K, &pl.plen[b]);
            pl.Nmax = std::max(pl.Nmax, pl.plen[b]);
        }
    if (pl.lang_det) pl.lang_pos = pl.Nmax + c->lang.sot_index;
    if (pl.lp_probe) pl.probe_pos = pl.Nmax + c->lp.sot_index;
    pl.want_logits = want_logits;
    pl.n_lrows = sel ? n_sel : (size_t)nb;
    if (want_logits && sel) {
        pl.sel_map.assign(nb, -1);
        for (size_t i = 0; i < n_sel; i++) {
            if (sel[i] < 0 || sel[i] >= nb || pl.sel_map[sel[i]] >= 0) return fail(c, WH_ERR_ARG, "decode: logits row %d outside the batch or listed twice", (int)sel[i]);
            pl.sel_map[sel[i]] = (int)i;
        }
    }
    wh_ctx::StepKey& key = pl.key;
    key.nb = nb; key.n_prompt = pl.Nmax + P; key.pfx = pl.Nmax > 0; key.eot = (int)p->eot; key.n_forced = (int)p->n_forced;
    key.logits_rows = (int)logits_rows;
    if (c->ts.on) { key.ts_begin = (int)c->ts.begin; key.ts_max_init = c->ts.max_init; }
    if (c->lp.on) key.lp_sum = c->lp.part_sum;
    if (c->rep.on) { key.rep = true; key.rep_p = c->rep.p; key.rep_n = c->rep.n; }
    if (c->al.on) { key.al_cap = NEW; key.al_gen = c->al.gen; }   // (prepare_alignment completes it with the side buffer's address)
    if (c->bm.on) { key.beam_k = c->bm.k; key.beam_c = c->bm.c; key.beam_buf = c->bm.buf; }
    if (c->sm.on && !sample_trivial(c)) key.sample_buf = c->sm.buf;
    key.split = choose_split(c, key);
    key.split_cus = key.split ? std::min(c->split_cus, c->dec_cus) : 0;
    key.free = choose_free(c, key, want_logits);
    return WH_OK;
}

// feed, out_tokens, n_out, done, pos, ticket, repetition bits, forced ids, the two suppress masks, the prefix offsets
static int upload_token_state(wh_ctx* c, const wh_decode_params* p, const DecodePlan& pl) {
    hipStream_t s = c->stream;
    const int nb = pl.key.nb, ld = c->tok_ld, Nmax = pl.Nmax, vocab = c->m->dims.vocab;
    std::vector<int> feed((size_t)nb * ld, 0);
    for (int b = 0; b < nb; b++) {
        for (int i = 0; i < pl.plen[b]; i++) feed[(size_t)b * ld + Nmax - pl.plen[b] + i] = (int)pl.pids[b][i];   // (columns below Nmax - n_b: filler id 0 of an idle row)
        for (int i = 0; i < pl.P; i++) feed[(size_t)b * ld + Nmax + i] = i == pl.lang_slot ? (pl.lang_fix ? (int)c->lang.fixed : 0) : (int)p->prompt[i];
    }
    if (pl.key.pfx) {
        std::vector<int> off(nb);
        for (int b = 0; b < nb; b++) off[b] = Nmax - pl.plen[b];
        CTX_HIP(c, hipMemcpyAsync(c->pfx.off, off.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipStreamSynchronize(s));
    }
    CTX_HIP(c, hipMemcpyAsync(c->feed, feed.data(), feed.size() * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->out_tokens, feed.data(), feed.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<int> nout(nb, pl.key.n_prompt);
    CTX_HIP(c, hipMemcpyAsync(c->n_out, nout.data(), nb * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemsetAsync(c->done, 0, nb * 4, s));
    std::vector<int> sm_done;
    std::vector<float> sm_t;
    std::vector<unsigned long long> sm_id;
    if (pl.key.sample_buf) {   // this call's rows: temperatures, random streams, and the inactive rows start done (a long-form call: row 0 for every window, the window index as its id)
        const bool lf = c->pfx.win_base >= 0;
        sm_done.resize(nb); sm_t.resize(nb); sm_id.resize(nb);
        for (int b = 0; b < nb; b++) {
            sm_done[b] = c->sm.active[lf ? 0 : b] ? 0 : 1;
            sm_t[b] = c->sm.temp[lf ? 0 : b];
            sm_id[b] = lf ? (unsigned long long)(c->pfx.win_base + b) : (unsigned long long)c->sm.ids[b];
        }
        const unsigned long long seed = c->sm.seed;
        CTX_HIP(c, hipMemcpyAsync(c->done, sm_done.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->sm.d_temp, sm_t.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->sm.d_ids, sm_id.data(), nb * 8, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->sm.d_seed, &seed, 8, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipStreamSynchronize(s));   // (`seed` goes out of scope)
    }
    CTX_HIP(c, hipMemsetAsync(c->pos, 0, 2 * 4, s));           // (both elements: the whole batch's and the second range's)
    CTX_HIP(c, hipMemsetAsync(c->step_ticket, 0, 2 * 4, s));
    if (c->rep.on) CTX_HIP(c, hipMemsetAsync(c->rep.bits, 0, (size_t)nb * c->rep.words * 4, s));   // no history yet: nothing is touched
    if (pl.key.beam_k) {   // no position has run (the first one starts the scores and the pool itself)
        CTX_HIP(c, hipMemsetAsync(c->bm.n_steps, 0, (size_t)pl.ncl * 4, s));
        CTX_HIP(c, hipMemsetAsync(c->bm.pool_n, 0, (size_t)pl.ncl * 4, s));
    }
    std::vector<int> forced(p->n_forced);
    for (size_t i = 0; i < p->n_forced; i++) forced[i] = (int)p->forced[i];
    if (!forced.empty()) CTX_HIP(c, hipMemcpyAsync(c->forced, forced.data(), forced.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<unsigned> mfirst, mbase;
    pack_mask(p->suppress, p->n_suppress, p->begin_suppress, p->n_begin_suppress, vocab, mfirst);  // :765-768
    pack_mask(p->suppress, p->n_suppress, nullptr, 0, vocab, mbase);
    if (c->ts.on && c->ts.no_ts >= 0 && c->ts.no_ts < vocab) {   // timestamp rule 1: <|notimestamps|> at every step
        mfirst[c->ts.no_ts >> 5] |= 1u << (c->ts.no_ts & 31);
        mbase[c->ts.no_ts >> 5] |= 1u << (c->ts.no_ts & 31);
    }
    CTX_HIP(c, hipMemcpyAsync(c->mask_first, mfirst.data(), mfirst.size() * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->mask_base, mbase.data(), mbase.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<int> sb;
    if (c->al.on) {   // frames of each clip: half its mel frames (the conv stride), at least 8, at most the audio context
        sb.resize(nb);
        for (int b = 0; b < nb; b++) {
            const int nf = (size_t)b < c->enc_nframes.size() ? c->enc_nframes[b] : WH_N_FRAMES;
            sb[b] = std::min(c->m->dims.n_audio_ctx, std::max(8, (nf + 1) / 2));
        }
        CTX_HIP(c, hipMemcpyAsync(c->al.sb, sb.data(), nb * 4, hipMemcpyHostToDevice, s));
    }
    CTX_HIP(c, hipStreamSynchronize(s));  // host vectors above go out of scope
    return WH_OK;
}

// the parity buffer of a call that keeps logits: the row selection goes to the device, the buffer grows on demand; completes the key
static int prepare_logits(wh_ctx* c, DecodePlan& pl) {
    if (!pl.want_logits) return WH_OK;
    if (!pl.sel_map.empty()) {
        CTX_HIP(c, hipMemcpy(c->logits_sel, pl.sel_map.data(), pl.key.nb * 4, hipMemcpyHostToDevice));
        pl.key.d_sel = c->logits_sel;
    }
    if (int rc = grow(c, c->logits, pl.n_lrows * pl.key.logits_rows * c->m->dims.vocab * 4, true, GROW_FREE_FIRST, "the kept logits")) return rc;
    pl.key.d_logits = c->logits;
    return WH_OK;
}

// Word-level timestamps: the side buffer the captured step copies the alignment heads' queries into, [heads][nb][max_new_tokens][dk] f32 — sized
// by the call, grown on demand; completes the key
int align_dk(const wh_ctx* c) { return c->cross_es ? c->m->dims.d_model : WH_HEAD_DIM; }
static int prepare_alignment(wh_ctx* c, DecodePlan& pl) {
    if (!c->al.on) return WH_OK;
    if (int rc = grow(c, c->al.q, c->al.heads.size() / 2 * (size_t)pl.key.nb * pl.NEW * align_dk(c) * 4, true, GROW_FREE_FIRST, "the alignment queries")) return rc;
    pl.key.al_q = c->al.q;
    return WH_OK;
}

// the listed heads' key rows of clip 0 among ncl resident clips (wh_step.h)
int align_keys(const wh_ctx* c, const std::vector<int>& heads, int ncl, AlignArgs& a) {
    const wh_dims& D = c->m->dims;
    const int S = D.n_audio_ctx;
    a.dk = align_dk(c);
    const long kv_stride = (long)ncl * S * D.d_model;
    for (size_t i = 0; i < heads.size() / 2; i++) {
        const int l = heads[2 * i], h = heads[2 * i + 1];
        a.k_base[i] = c->cross_es ? c->es_E : (const void*)((const char*)c->cross_kv + ((long)(2 * l) * kv_stride + (long)h * WH_HEAD_DIM) * c->m->esz);
    }
    a.k_clip_pitch = (long)(c->cross_es ? c->es_rows : S) * D.d_model; a.k_row_pitch = D.d_model;
    return c->cross_es ? WH_ALIGN_ES_BF16 : c->m->prec == WH_PREC_F32 ? WH_ALIGN_KV_F32 : WH_ALIGN_KV_BF16;
}

// The post-pass over a.nb rows (wh_step.h): scores + softmax, filter, DTW for chunks of rows sized so that the workspace (P, M and the DTW steps
// of a chunk) stays within WH_ALIGN_WS_BYTES; keeps the debug rows' P and M.
constexpr size_t WH_ALIGN_WS_BYTES = (size_t)1 << 30;
int align_post_pass(wh_ctx* c, AlignArgs a, int form, DevBuf<>& ws, const std::vector<int>& debug, std::vector<wh_ctx::AlignDebug>& dbg) {
    hipStream_t s = c->stream;
    const int nb = a.nb, NEW = a.cap, nh = a.n_heads, S = a.S, Sp = a.Sp;
    const size_t b_p = (size_t)nh * NEW * Sp * 4, b_m = (size_t)NEW * Sp * 4, b_t = (size_t)(NEW + 1) * (S + 1), per_clip = b_p + b_m + b_t;
    const int chunk = (int)std::min<size_t>((size_t)nb, std::max<size_t>(1, WH_ALIGN_WS_BYTES / per_clip));
    Carver cv;
    const size_t o_p = cv.take(chunk * b_p), o_m = cv.take(chunk * b_m), o_t = cv.take(chunk * b_t);
    if (int rc = grow(c, ws, cv.off, false, GROW_FREE_FIRST, "the alignment workspace")) return rc;   // (only the post-pass reads it: no captured step to drop)
    a.P = at<float>(ws, o_p); a.M = at<float>(ws, o_m); a.trace = at<unsigned char>(ws, o_t);
    const bool tm = c->al.timing && !c->capturing;
    hipEvent_t te[4] = {nullptr, nullptr, nullptr, nullptr};
    if (tm) for (auto& e : te) CTX_HIP(c, hipEventCreate(&e));
    struct TeGuard { hipEvent_t* te; ~TeGuard() { for (int i = 0; i < 4; i++) if (te[i]) hipEventDestroy(te[i]); } } te_guard{te};
    for (int c0 = 0; c0 < nb; c0 += chunk) {
        const int nc = std::min(chunk, nb - c0);
        a.clip0 = c0;
        Prof pr(c, WH_KG_DEC_OTHER);
        if (tm) CTX_HIP(c, hipEventRecord(te[0], s));
        CTX_LAUNCH(c, wh_launch_align_scores(s, form, a, nc));
        if (tm) CTX_HIP(c, hipEventRecord(te[1], s));
        wh_launch_align_filter(s, a, nc);
        if (tm) CTX_HIP(c, hipEventRecord(te[2], s));
        wh_launch_align_dtw(s, a, nc);
        if (tm) {   // (measurement runs only: the host waits for every chunk)
            CTX_HIP(c, hipEventRecord(te[3], s));
            CTX_HIP(c, hipEventSynchronize(te[3]));
            for (int i = 0; i < 3; i++) { float ms = 0; hipEventElapsedTime(&ms, te[i], te[i + 1]); c->al.ms[i] += ms; }
        }
        for (size_t k = 0; k < debug.size(); k++) {   // parity harness: the whole slot; the caller cuts it to the row's own rows and S_b
            const int r = debug[k];
            if (r < c0 || r >= c0 + nc) continue;
            wh_ctx::AlignDebug& d = dbg[k];
            d.probs.resize((size_t)nh * NEW * Sp);
            d.matrix.resize((size_t)NEW * Sp);
            CTX_HIP(c, hipMemcpyAsync(d.probs.data(), a.P + (size_t)(r - c0) * nh * NEW * Sp, d.probs.size() * 4, hipMemcpyDeviceToHost, s));
            CTX_HIP(c, hipMemcpyAsync(d.matrix.data(), a.M + (size_t)(r - c0) * NEW * Sp, d.matrix.size() * 4, hipMemcpyDeviceToHost, s));
            CTX_HIP(c, hipStreamSynchronize(s));
        }
    }
    return WH_OK;
}

// The post-pass of a call with word-level timestamps, on the decode stream after the token loop.
static int run_alignment(wh_ctx* c, const DecodePlan& pl) {
    if (!c->al.on) return WH_OK;
    hipStream_t s = c->stream;
    const wh_dims& D = c->m->dims;
    const int nb = pl.key.nb, NEW = pl.NEW, nh = (int)(c->al.heads.size() / 2), S = D.n_audio_ctx, Sp = (S + 3) / 4 * 4;
    c->al.dbg.clear();
    CTX_HIP(c, hipMemsetAsync(c->al.frames, 0, (size_t)nb * D.n_text_ctx * 4, s));
    if (NEW == 1) return WH_OK;   // one row per clip: frame 0, nothing to launch
    AlignArgs a;
    a.q = c->al.q;
    const int form = align_keys(c, c->al.heads, nb, a);
    a.n_out = c->n_out; a.n_prompt = pl.key.n_prompt; a.cap = NEW; a.sb = c->al.sb;
    a.nb = nb; a.n_heads = nh; a.S = S; a.Sp = Sp;
    a.frames = c->al.frames; a.frames_ld = D.n_text_ctx;
    c->al.dbg.resize(c->al.debug.size());
    c->al.ms[0] = c->al.ms[1] = c->al.ms[2] = 0;
    return align_post_pass(c, a, form, c->al.ws, c->al.debug, c->al.dbg);
}

// cross-attention K/V of every decoder layer, once per clip: present.{i}.encoder.{key,value} of the step-0 decoder run (src/main.rs:771-787).
// `after_kv` (optional) runs on the host right after the projection has been enqueued and its completion event recorded: the place where
// the NEXT batch's encoder pass is put on the encoder stream, before the host is tied up in the token loop.
int project_cross_kv(wh_ctx* c, int nb, const std::function<int()>& after_kv) {
    wh_model* m = c->m;
    const wh_dims& D = m->dims;
    hipStream_t s = c->stream;
    const int prec = m->prec;
    const long d = D.d_model, S = D.n_audio_ctx;
    if (c->cross_es) {
        // no projection: the token loop attends over the encoder states themselves (wh_cross_es.hip).  Their final LayerNorm runs
        // here, on the decode stream, into decode-side storage — the encoder-side workspace is free for the next pass afterwards
        Prof pr(c, WH_KG_DEC_GEMM);
        if (prec == WH_PREC_F16X3 && wh_es3_enabled()) wh_launch_layernorm_es3(s, c->x, m->enc_ln_w, m->enc_ln_b, c->es_E, (long)nb * S, (int)S, c->es_rows);   // fp16 + e4m3 remainder rows
        else if (prec == WH_PREC_F16X3) wh_launch_layernorm_es2(s, c->x, m->enc_ln_w, m->enc_ln_b, c->es_E, (long)nb * S, (int)S, c->es_rows);   // fp16 limb planes
        else if (prec == WH_PREC_FP8) wh_launch_layernorm_es8(s, c->x, m->enc_ln_w, m->enc_ln_b, c->es_E, (long)nb * S, (int)S, c->es_rows);                 // e4m3 rows
        else wh_launch_layernorm_blocks(s, prec, c->x, m->enc_ln_w, m->enc_ln_b, c->es_E, (long)nb * S, (int)d, c->es_rows == (int)S ? 0 : (int)S, c->es_rows);
    } else {
        Prof pr(c, WH_KG_DEC_GEMM);
        GemmArgs g;
        g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
        g.A = c->enc_out; g.lda = d; g.W = m->cross_kv_w; g.ldw = d;
        g.C = c->cross_kv; g.ldc = d; g.n_per = (int)d; g.c_ns = (long)nb * S * d;   // elements between consecutive [nb][S][d] planes
        g.bias = m->cross_kv_b; g.bias_mode = 1; g.wscale = m->cross_kv_sc;
        g.M = nb * (int)S; g.N = (int)(D.dec_layers * 2 * d); g.K = (int)d;
        if (c->enc_fold) {   // encoder's final LayerNorm folded in: raw bf16 rows, statistics from the last fc2's epilogue
            g.A = c->xb; g.W = m->cross_kv_wf; g.bias = m->cross_kv_c; g.ln_mode = 1; g.ln_stat = c->enc_stat; g.ln_s = m->cross_kv_s;
        }
        if (c->mx_ok) { g.A = c->xn8; g.a_sc = c->xn8_sc; g.W = m->cross_kv_w8; CTX_LAUNCH(c, wh_launch_gemm8_mx(s, 0, g)); }   // xn8 = MX(final LN), run_encoder
        else CTX_LAUNCH(c, wh_launch_gemm(s, prec, prec == WH_PREC_F16X3, g));   // (split-fp16 mode: K and V as f32 rows — their consumer is the f32 attention kernel, no matrix-core operand)
        if (prec == WH_PREC_FP8) {  // bf16 projection → e4m3 codes, one scale per (layer, K|V, clip, head)
            const long planes = (long)D.dec_layers * 2 * nb;
            CTX_HIP(c, hipMemsetAsync(c->kv_amax, 0, planes * D.n_heads * 4, s));
            wh_launch_kv_quant(s, c->cross_kv, (unsigned*)c->kv_amax, c->cross_kv8, planes, (int)S, (int)d, D.n_heads);
        }
    }
    CTX_HIP(c, hipEventRecord(c->ev_kv_done, s));   // the encoder-side workspace may be overwritten from here on
    c->kv_done_armed = true;
    if (after_kv) {
        int rc = after_kv();
        if (rc) return rc;
        c->cur = s;
    }
    return WH_OK;
}

// ---- one decoder position (~50 kernel launches) ---------------------------------------------------
// (the operands of the decode GEMMs and the layer's launch list: StepBase, wh_step.h)
// What a prompt position does besides the layers.  It embeds its own input token (a generated position's input was embedded by the
// previous position's argmax finish); only the last prompt position emits.
struct PromptStep {
    bool emits = false;
    bool lang = false;    // language detection reads this position's logits; the chosen id goes to column lang_col
    int lang_col = 0;
    bool probe = false;   // the no-speech probe reads this position's logits
};

// The launches of a position see the context (model, fixed workspace addresses, option buffers) and the step's key, nothing else.
struct Step : StepBase {
    using StepBase::StepBase;
    const int* d_off = k.pfx ? c->pfx.off : nullptr;

    // the token bookkeeping of the kernel that ends an emitting step, from the range's first row on; log-probabilities go to the sampling call's
    // own buffer or, when they are on, to lp.tok (whole batch only: a range with row0 > 0 records none, choose_free)
    DecodeState decode_state() const {
        DecodeState st;
        st.feed = rm(c->feed, c->tok_ld); st.out_tokens = rm(c->out_tokens, c->tok_ld); st.n_out = rm(c->n_out, 1); st.done = rm(c->done, 1);
        st.forced = c->forced; st.n_forced = k.n_forced; st.n_prompt = k.n_prompt; st.eot = k.eot; st.tok_ld = c->tok_ld;
        st.logprob = k.sample_buf ? c->sm.lp : k.lp_sum ? c->lp.tok : nullptr;
        return st;
    }
    // the embedding of the next position's input token (and of a prompt position's own).  Beam search gets the same values it used to fill in by
    // hand without xgamma and off: it is refused in fp8 mode (f8 false: xgamma nullptr) and with a non-empty prefix (k.pfx false: d_off nullptr).
    NextEmbed next_embed() const {
        NextEmbed ne;
        ne.tok_emb = m->tok_emb; ne.pos_emb = m->dec_pos; ne.x = rm(c->dx, d); ne.xslab = slab(c->dxs); ne.stats = rm(c->lnpart, 2);
        ne.xgamma = f8 ? m->dec[0].ln1_w : nullptr; ne.d = (int)d; ne.mpad = mpad; ne.shift = rm(c->dshift, 1); ne.off = d_off;
        return ne;
    }

    // one decoder layer at the current position: self-attention over the row's cache, with this position's k / v appended
    void layer(int l, bool advance) const {
        layer_to_query(l);
        layer_tail(l, advance);
    }
    // ... up to and including its cross-attention query: the first segment of a free-running range is layer 0's
    void layer_to_query(int l) const {
        const long cache_row = (long)D.n_heads * D.n_text_ctx * WH_HEAD_DIM * m->esz;   // bytes per row
        const long cache_l = (long)nb * cache_row;                                      // ... and per layer: the whole batch's, whatever the range
        const long cache_0 = l * cache_l + row0 * cache_row;
        layer_head(l, [&] {
            wh_launch_dec_self_attn(s, prec, rm(c->dqkv, 3 * d, prec == WH_PREC_F16X3 ? 4 : m->esz), (char*)c->self_k + cache_0, (char*)c->self_v + cache_0, slab(c->datt), pos,
                                    (int)d, D.n_heads, D.n_text_ctx, nr, mpad, d_off);   // (a range with row0 > 0 has no prefixes: d_off == nullptr)
        });
    }

    // final LN ∘ tied LM head + masked argmax; the finish kernel records the token, advances the position and embeds the next one.  The plain
    // variant runs on the range's rows with the range's position and ticket (the partials' count is this launch's: two ranges may differ); the
    // rules', the log-probabilities', the repetition bitmap's and the kept logits' per-row buffers are the whole batch's (row0 == 0)
    void emit() const {
        if (k.beam_k) return emit_beam();
        if (k.sample_buf) return emit_sample();
        int lm_parts;
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = lm_head_masked();
            a.logits = k.d_logits; a.logits_rows = k.logits_rows; a.logits_sel = k.d_sel;
            if (rules) {
                a.ts_state = c->ts.state; a.ts_logits = c->ts.logits; a.ts_ld = D.vocab - k.ts_begin;
                a.ts_begin = k.ts_begin; a.ts_max_init = k.ts_max_init;
            }
            a.part_sum = k.lp_sum;
            if (k.rep) { a.rep_bits = c->rep.bits; a.rep_side = c->rep.side; a.rep_words = c->rep.words; }
            wh_launch_lm_head(s, prec, a);
            lm_parts = wh_lm_head_parts(prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);   // argmax finish + greedy bookkeeping + the next position's embedding
        TsFinish tf;
        if (rules) {
            tf.rules = true; tf.ts_logits = c->ts.logits; tf.ts_ld = D.vocab - k.ts_begin; tf.state = c->ts.state;
            tf.ts_begin = k.ts_begin; tf.vocab = D.vocab;
        }
        RepFinish rf;
        if (k.rep) {
            rf.on = true; rf.bits = c->rep.bits; rf.side = c->rep.side; rf.words = c->rep.words; rf.vocab = D.vocab;
            rf.p = k.rep_p; rf.inv = 1.0f / k.rep_p; rf.ngram = k.rep_n;
            if (rules) rf.exempt_from = k.ts_begin;   // timestamps repeat in pairs and the rules own them
            rf.mask_first = c->mask_first; rf.mask_base = c->mask_base;
        }
        wh_launch_argmax_finish(s, prec, c->part_val + row0, c->part_idx + row0, lm_parts, mpad, pos, ticket, decode_state(), nr, next_embed(), tf, k.lp_sum, rf);
    }

    // Beam search: the LM head leaves the rows' raw logits of this position in the scratch (its argmax partials are not read);
    // k_beam_select chooses the next beams of every clip and embeds their tokens; k_beam_reorder permutes the self-attention caches and
    // advances the position.  One chain, no parallel branches.
    void emit_beam() const {
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            wh_launch_lm_head(s, prec, lm_head_masked(c->bm.logits));
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        BeamArgs b;
        b.K = k.beam_k; b.C = k.beam_c; b.n_clips = ncl; b.vocab = D.vocab;
        b.logits = c->bm.logits; b.pos_p = c->pos; b.n_prompt = k.n_prompt; b.eot = k.eot; b.tok_ld = c->tok_ld;
        b.mask_first = c->mask_first; b.mask_base = c->mask_base;
        if (rules) { b.ts_begin = k.ts_begin; b.ts_max_init = k.ts_max_init; }
        b.scores = c->bm.scores; b.parent = c->bm.parent; b.state = c->bm.state; b.pool_n = c->bm.pool_n; b.n_steps = c->bm.n_steps; b.pool = c->bm.pool;
        b.tr_parent = c->bm.tr_parent; b.tr_token = c->bm.tr_token; b.tr_score = c->bm.tr_score; b.tr_lp = c->bm.tr_lp; b.tr_pool = c->bm.tr_pool;
        b.rows_ld = c->max_batch; b.done = c->done; b.feed = c->feed;
        b.logits_out = k.d_logits; b.logits_rows = k.logits_rows; b.logits_sel = k.d_sel;
        const bool tm = c->bm.timing && !c->capturing;   // (measurement runs only: positions launched eagerly)
        std::array<hipEvent_t, 3> te = {nullptr, nullptr, nullptr};
        if (tm) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
        wh_launch_beam_select(s, prec, b, next_embed());
        if (tm) hipEventRecord(te[1], s);
        wh_launch_beam_reorder(s, (int)m->esz, c->self_k, c->self_v, c->bm.parent, c->done, k.beam_k, ncl, D.dec_layers, D.n_heads, D.n_text_ctx, c->pos, c->step_ticket);
        if (tm) { hipEventRecord(te[2], s); c->bm.events.push_back(te); }
    }

    // Temperature sampling: the LM head leaves the rows' raw logits of this position in the scratch (its argmax partials are not
    // read; k_argmax_finish is not launched); k_sample_select chooses every row's token, does the finish kernel's bookkeeping, embeds the next
    // position and advances.  One chain, no parallel branches.
    void emit_sample() const {
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            wh_launch_lm_head(s, prec, lm_head_masked(c->sm.logits));
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        SampleArgs a;
        a.logits = c->sm.logits; a.vocab = D.vocab; a.mask_first = c->mask_first; a.mask_base = c->mask_base;
        if (rules) { a.ts_begin = k.ts_begin; a.ts_max_init = k.ts_max_init; a.ts_state = c->sm.state; }
        a.temperature = c->sm.d_temp; a.row_ids = c->sm.d_ids; a.seed = c->sm.d_seed;
        a.logits_out = k.d_logits; a.logits_rows = k.logits_rows; a.logits_sel = k.d_sel;
        const bool tm = c->sm.timing && !c->capturing;   // (measurement runs only: positions launched eagerly)
        std::array<hipEvent_t, 2> te = {nullptr, nullptr};
        if (tm) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
        wh_launch_sample_select(s, prec, a, decode_state(), next_embed(), nb, c->pos, c->step_ticket);
        if (tm) { hipEventRecord(te[1], s); c->sm.events.push_back(te); }
    }

    // the listed ids' unfiltered logits of this prompt position -> each row's language token in column tok_col of the next one; the
    // finish advances the position unless the probe's finish will
    void lang(int tok_col, bool advance) const {
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            const SkinnyArgs h = lm_head_common();   // the LM head's operands, the weight rows gathered by id
            LangHeadArgs a;
            a.X = h.X; a.x_mpad = h.x_mpad; a.W = h.W; a.bias = h.bias; a.ln_s = h.ln_s; a.ln_part = h.ln_part; a.ln_tiles = h.ln_tiles; a.M = h.M; a.K = h.K;
            a.ids = c->lang.d_ids; a.n_lang = (int)c->lang.ids.size(); a.out = c->lang.logits;
            wh_launch_lang_head(s, prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        wh_launch_lang_finish(s, c->lang.logits, c->lang.d_ids, (int)c->lang.ids.size(), c->lang.bcast ? 0 : -1, c->lang.probs, c->lang.chosen,
                              c->feed, c->out_tokens, c->tok_ld, tok_col, nb, advance ? c->pos : nullptr);
    }

    // softmax(v)[no_speech] over this prompt position's unfiltered logits: the LM head's log-probability variant with an all-zero mask,
    // no rules, nothing recorded; the probe's finish kernel advances the position
    void probe() const {
        int parts;
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = lm_head_common();
            a.mask_first = c->lp.mask_zero; a.mask_base = c->lp.mask_zero;
            a.part_sum = c->lp.part_sum;
            a.probe_id = (int)c->lp.no_speech; a.probe_out = c->lp.probe_v;
            wh_launch_lm_head(s, prec, a);
            parts = wh_lm_head_parts(prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        wh_launch_nospeech_finish(s, c->part_val, c->lp.part_sum, parts, mpad, c->lp.probe_v, c->lp.ns, nb, c->pos);
    }
};

// ---- the split token loop ----------------------------------------------------------
// Whether a call's generated positions run as two row ranges, and the first range's rows (0: one chain).  The rows of a greedy batch are
// independent until the argmax finish, and no kernel of a layer mixes rows, so a range computes what it computes in the whole batch.
//  * only the plain greedy key in bf16: no beam search (rows share clips and are permuted), no sampling, no alignment copies; what only acts in
//    emit() — timestamp rules, log-probabilities, repetition controls — is allowed;
//  * per-clip prefixes with a non-empty one in the batch fall back to one chain, and so do contexts whose decode GEMMs are k_dec_tile;
//  * k_dec_gemm / k_dec_gemm_wide read whole row groups of G = min(64, nb rounded up to 16) rows whose tail is masked, not clamped: the second
//    range's groups must end inside the slab pitch.
constexpr bool WH_DEC_SPLIT_DEFAULT = true;    // (the rule below applies without WH_DEC_SPLIT=1)
static int choose_split(const wh_ctx* c, const wh_ctx::StepKey& key) {
    const int nb = key.nb;
    if (c->split_mode == 0 || c->m->prec != WH_PREC_BF16 || c->dec_tile || nb < 2) return 0;   // (k_dec_tile takes no row range)
    if (key.beam_k || key.sample_buf || c->al.on || key.pfx) return 0;
    int r0 = 0;
    if (c->dbg_split > 0) r0 = c->dbg_split;                                                       // the tests' hook: any context
    else if ((c->split_mode == 1 || (c->split_mode < 0 && WH_DEC_SPLIT_DEFAULT)) && c->cross_es && nb >= 1024) {
        r0 = c->split_rows > 0 ? c->split_rows : nb / 2 / 64 * 64;                                  // halves, on a row-group boundary of the decode GEMMs
    }
    if (r0 <= 0 || r0 >= nb) return 0;
    const int G = std::min(64, (nb + 15) / 16 * 16);
    if (r0 + (nb - r0 + G - 1) / G * G > c->mpad) return 0;
    return r0;
}

// the events of the free-running halves (below): A / B behind the first segment of a range's position, fork / join around a run of free positions
enum { FREE_EV_A = 0, FREE_EV_B, FREE_EV_FORK, FREE_EV_JOIN, FREE_EVENTS };
// the second decode stream and the events of a split step: created outside any capture, at the first call that splits
static int ensure_split_stream(wh_ctx* c) {
    if (!c->s_split) {
        hipError_t he = c->dec_mask.empty() ? hipStreamCreateWithFlags(&c->s_split, hipStreamNonBlocking)
                                            : hipExtStreamCreateWithCUMask(&c->s_split, (uint32_t)c->dec_mask.size(), c->dec_mask.data());
        if (he != hipSuccess) { c->s_split = nullptr; return fail(c, WH_ERR_HIP, "the second decode stream: %s", hipGetErrorString(he)); }
    }
    const size_t want = 3;   // fork, join, the first range's first cross-attention query
    while (c->split_ev.size() < want) {
        hipEvent_t e = nullptr;
        CTX_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->split_ev.push_back(e);
    }
    while (c->free_ev.size() < FREE_EVENTS) {   // the free-running halves' own (never captured)
        hipEvent_t e = nullptr;
        CTX_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->free_ev.push_back(e);
    }
    return WH_OK;
}

// ---- the free-running halves -------------------------------------------------------
// The rows of a greedy batch are independent across positions too: clip b's position p + 1 needs nothing of another clip's position p.  So the
// two ranges of a split call need not meet before the LM head: each runs whole positions — layers, LM head, finish — on its own stream, with its
// own device-side position and ticket (element 1 of c->pos / c->step_ticket: the second range's), and the skew between them survives from one
// position to the next: one range's LM head, finish and first GEMMs run beside the other's stream over the encoder side.
// A range's position is two segments, each a single chain (captured: a graph without branches, replayed on the range's stream only):
//   segment 0: layer 0 up to and including its cross-attention query;   segment 1: the rest of layer 0, the other layers, LM head, finish.
// Applies where the call splits and its key is the plain one: timestamp rules, log-probabilities, the repetition bitmap and kept logits carry
// per-row buffers that do not follow a range.  The LM head reads whole row groups past the range's last row (k_lm_head: masked; the tile
// kernels: clamped to the slab pitch counted from the range's first row), so both ranges' groups must end inside the slab pitch.
constexpr bool WH_DEC_FREE_DEFAULT = true;    // (where choose_split splits by its rule; WH_DEC_FREE=0 turns it off)
// rows from a range's first one that its LM head launch may read
static int lm_head_reach(const Step& r) {
    const SkinnyArgs a = r.lm_head_masked();
    if (wh_lm_head_tile_applicable(a)) return (r.nr + 255) / 256 * 256;
    int reach = 0;   // k_lm_head: groups of 16 * mt rows, mt <= 4 as the launcher chooses it (any of them here)
    for (int mt = 1; mt <= std::min(4, (r.nr + 15) / 16); mt++) reach = std::max(reach, (r.nr + 16 * mt - 1) / (16 * mt) * (16 * mt));
    return reach;
}
// the two ranges of a free-running call: which = 0: rows [0, split) on the decode stream, position and ticket 0; 1: the rest on the second stream
static Step free_range(wh_ctx* c, const wh_ctx::StepKey& k, int which) {
    Step r{c, k};
    r.es_cus = k.split_cus;
    if (which == 0) { r.nr = k.split; return r; }
    r.row0 = k.split; r.nr = k.nb - k.split; r.s = c->s_split;
    r.pos = c->pos + 1; r.ticket = c->step_ticket + 1;
    return r;
}
static bool choose_free(wh_ctx* c, const wh_ctx::StepKey& key, bool want_logits) {
    if (!key.split || c->free_mode == 0) return false;
    if (!(c->dbg_split > 0 ? c->dbg_free != 0 : (c->free_mode == 1 || WH_DEC_FREE_DEFAULT))) return false;
    if (key.ts_begin >= 0 || key.lp_sum || key.rep || want_logits || key.d_logits) return false;
    for (int which = 0; which < 2; which++) {
        const Step r = free_range(c, key, which);
        if (r.row0 + lm_head_reach(r) > c->mpad) return false;
    }
    return true;
}
static void launch_free_segment(const Step& r, int seg) {
    if (seg == 0) return r.layer_to_query(0);
    r.layer_tail(0, false);
    for (int l = 1; l < r.D.dec_layers; l++) r.layer(l, false);
    r.emit();
}

// The decoder layers of a generated position as two branches: rows [0, split) on the decode stream, the rest on the second one, forked behind
// the embedding (the previous position's finish) and joined before emit().  Captured, the events become the edges of a graph with two
// parallel branches; launched eagerly they order the two streams.  The layers are issued alternately, so that the stagger's event is
// recorded before the launch that waits for it is issued.
static void launch_layers_split(wh_ctx* c, const Step& t) {
    const int L = t.D.dec_layers, r0 = t.k.split;
    hipEvent_t* ev = c->split_ev.data();
    hipEvent_t e_fork = ev[0], e_join = ev[1];
    Step a = t, b = t;
    a.nr = r0; a.es_cus = t.k.split_cus;
    b.row0 = r0; b.nr = t.nb - r0; b.es_cus = t.k.split_cus; b.s = c->s_split;
    a.q_rec = ev[2];   // the stagger: B starts behind A's first cross-attention query (left alone, both reach their cross-attention together)
    hipEventRecord(e_fork, t.s);
    hipStreamWaitEvent(c->s_split, e_fork, 0);
    for (int l = 0; l < L; l++) {
        a.layer(l, false);
        if (l == 0 && a.q_rec) hipStreamWaitEvent(c->s_split, a.q_rec, 0);
        b.layer(l, false);
    }
    hipEventRecord(e_join, c->s_split);
    hipStreamWaitEvent(t.s, e_join, 0);
}

// One decoder position.  prompt == nullptr: a generated position — the emitting step that is captured into the graph; it sees the
// context and its key, nothing else (wh_ctx::StepKey).
static void launch_step(wh_ctx* c, const wh_ctx::StepKey& k, const PromptStep* prompt = nullptr) {
    const Step t{c, k};
    const bool emits = !prompt || prompt->emits, lang = prompt && prompt->lang, probe = prompt && prompt->probe;
    if (prompt) {   // token + position embedding → x, raw slab, row sums (one "tile")
        Prof pr(c, WH_KG_DEC_OTHER);
        const NextEmbed ne = t.next_embed();
        wh_launch_dec_embed(t.s, t.prec, ne.tok_emb, ne.pos_emb, c->feed, c->tok_ld, c->pos, ne.x, ne.xslab, ne.stats, t.nb, ne.d, ne.mpad, ne.xgamma, ne.shift, ne.off);
    }
    if (!prompt && k.split) launch_layers_split(c, t);
    else for (int l = 0; l < t.D.dec_layers; l++) t.layer(l, l == t.D.dec_layers - 1 && !emits && !lang && !probe);
    if (emits) t.emit();
    if (lang) t.lang(prompt->lang_col, !probe);   // (before the probe, if the probe sits at the same position)
    if (probe) t.probe();
}

// captures what launches() puts on stream s into the step's graph `slot` and instantiates it
template <typename F>
static int capture_step_graph(wh_ctx* c, hipStream_t s, int slot, F&& launches) {
    c->capturing = true;  // no event records inside the captured step
    hipGraph_t graph = nullptr;
    hipError_t ce = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (ce == hipSuccess) {
        launches();
        ce = hipStreamEndCapture(s, &graph);
    }
    c->capturing = false;
    if (ce != hipSuccess) {
        if (graph) hipGraphDestroy(graph);
        return fail(c, WH_ERR_HIP, "graph capture of the decode step failed: %s", hipGetErrorString(ce));
    }
    hipGraphExec_t gexec = nullptr;
    ce = hipGraphInstantiate(&gexec, graph, nullptr, nullptr, 0);
    if (ce != hipSuccess) {
        hipGraphDestroy(graph);
        return fail(c, WH_ERR_HIP, "hipGraphInstantiate of the decode step failed: %s", hipGetErrorString(ce));
    }
    c->step_graph[slot] = graph;
    c->step_exec[slot] = gexec;
    return WH_OK;
}

// the instantiated graph of launch_step(c, key): kept from the last call if the key is the same, else captured now.  A free-running key
// (DESIGN.md §5t): the four segments A1, A2, B1, B2 instead, each a single chain captured on the stream that replays it
static int ensure_step_graph(wh_ctx* c, const wh_ctx::StepKey& key) {
    if (c->step_exec[0] && c->step_key == key) return WH_OK;
    drop_step_graph(c);   // nothing of it is in flight: every call ends with a stream synchronisation
    int rc = WH_OK;
    if (key.free) {
        for (int i = 0; i < 4 && !rc; i++) {
            const Step r = free_range(c, key, i / 2);
            rc = capture_step_graph(c, r.s, i, [&] { launch_free_segment(r, i % 2); });
        }
    } else {
        rc = capture_step_graph(c, c->stream, 0, [&] { launch_step(c, key); });
    }
    if (rc) {
        drop_step_graph(c);   // (the segments captured before the one that failed)
        return rc;
    }
    c->step_key = key;
    return WH_OK;
}

// The `remaining` generated positions after the prompt replay ONE captured hipGraph of an emitting step — every kernel reads the
// position from device memory, so the graph is position-independent.  The host then pays one graph launch per token instead of ~50
// kernel launches (src/main.rs:793-826 is one ORT Run per token in the reference).
// A free-running key replays four single-chain graphs per position, two on each stream, ordered by two events; the halves
// meet only where the host needs the whole batch: the done poll, an event-timed position, sync_every_pos and the end of the loop.
static int run_token_loop(wh_ctx* c, const wh_ctx::StepKey& key, int remaining, bool poll_eot) {
    hipStream_t s = c->stream, s2 = c->s_split;
    // with event timing on: every position is launched eagerly (stride 0/1), or only every stride-th one
    // (sampled live timing) while the others replay the graph
    const int stride = c->prof ? c->prof_stride : 0;
    const bool use_graph = remaining > 1 && !c->no_graph && (!c->prof || stride > 1);
    if (use_graph) {
        int rc = ensure_step_graph(c, key);
        if (rc) return rc;
    }
    std::vector<int> done_h(key.nb);
    wh_ctx::StepKey one_chain = key;   // event-timed positions run unsplit: their kernel-group brackets describe the one-chain form
    one_chain.split = one_chain.split_cus = 0;
    one_chain.free = false;
    const Step ra = free_range(c, key, 0), rb = free_range(c, key, key.free ? 1 : 0);   // (the ranges of a free-running key)
    hipEvent_t* fe = c->free_ev.data();
    bool forked = false, have_eb = false;   // forked: the second stream runs its range; have_eb: it has recorded FREE_EV_B since the fork
    hipError_t he = hipSuccess;
    auto note = [&](hipError_t e) { if (he == hipSuccess) he = e; };
    // the halves meet: everything the second stream has been given is ordered before what the decode stream is given next
    auto join = [&] {
        if (!forked) return;
        note(hipEventRecord(fe[FREE_EV_JOIN], s2));
        note(hipStreamWaitEvent(s, fe[FREE_EV_JOIN], 0));
        forked = false;
    };
    auto fail_loop = [&](const char* what) {
        hipStreamSynchronize(s);
        if (forked) hipStreamSynchronize(s2);
        drop_step_graph(c);
        return fail(c, WH_ERR_HIP, "%s failed: %s", what, hipGetErrorString(he));
    };
    for (int r = 0; r < remaining; r++) {
        const bool sampled = c->prof && stride > 1 && (r % stride) == stride / 2;
        const bool timed = c->prof && (!use_graph || sampled);   // an event-timed position: eagerly, as the one chain on the whole batch
        if (key.free && !timed) {
            // One free-running position.  Issue order (every wait is issued after the record it refers to, in program order; the edges are
            // ordered by (position, segment) and cannot form a cycle — a wait issued before its record is how this would hang):
            //   [resume: copy pos[0] -> pos[1] on s, record FORK on s, s2 waits FORK]
            //   1. s waits B(p-1)   2. A1(p) on s   3. record A on s   4. A2(p) on s
            //   5. s2 waits A       6. B1(p) on s2  7. record B on s2  8. B2(p) on s2
            // A: B starts behind A's first query expansion (the stagger of §5s).  B: A is never more than one position ahead.
            if (!forked) {   // after whole-batch work (the prompt, a timed position, a poll): the second range's position is the batch's again
                note(hipMemcpyAsync(c->pos + 1, c->pos, 4, hipMemcpyDeviceToDevice, s));
                note(hipEventRecord(fe[FREE_EV_FORK], s));
                note(hipStreamWaitEvent(s2, fe[FREE_EV_FORK], 0));
                forked = true;
                have_eb = false;
            }
            if (have_eb && c->free_eb) note(hipStreamWaitEvent(s, fe[FREE_EV_B], 0));
            if (use_graph) note(hipGraphLaunch(c->step_exec[0], s)); else launch_free_segment(ra, 0);
            note(hipEventRecord(fe[FREE_EV_A], s));
            if (use_graph) note(hipGraphLaunch(c->step_exec[1], s)); else launch_free_segment(ra, 1);
            note(hipStreamWaitEvent(s2, fe[FREE_EV_A], 0));
            if (use_graph) note(hipGraphLaunch(c->step_exec[2], s2)); else launch_free_segment(rb, 0);
            note(hipEventRecord(fe[FREE_EV_B], s2));
            have_eb = true;
            if (use_graph) note(hipGraphLaunch(c->step_exec[3], s2)); else launch_free_segment(rb, 1);
            if (he != hipSuccess) return fail_loop("a free-running decode position");
            c->last_split = key.split;
            c->last_free = 1;
        } else {
            join();
            if (use_graph && !sampled) note(hipGraphLaunch(c->step_exec[0], s));
            else launch_step(c, c->prof ? one_chain : key);
            if (he != hipSuccess) return fail_loop("hipGraphLaunch");
            if (!timed) c->last_split = key.split;   // a position ran as two branches
        }
        // diagnostic (profiles/README.md, rocprofv3 --pmc at whisper-large-v3 size): bound the number of dispatches in flight
        if (c->sync_every_pos) { join(); hipStreamSynchronize(s); }
        // EOT early-out (src/main.rs:781-783, 820-822): poll the done flags every 16 generated tokens
        const int gen = r + 1;
        if ((gen & 15) == 15 && r + 1 < remaining && poll_eot) {
            join();
            hipError_t e1 = hipMemcpyAsync(done_h.data(), c->done, key.nb * 4, hipMemcpyDeviceToHost, s);
            hipError_t e2 = hipStreamSynchronize(s);
            if (e1 != hipSuccess || e2 != hipSuccess || he != hipSuccess)
                return fail(c, WH_ERR_HIP, "decode: polling the done flags failed: %s", hipGetErrorString(he != hipSuccess ? he : e1 != hipSuccess ? e1 : e2));
            bool all = true;
            for (int b = 0; b < key.nb; b++) all = all && done_h[b];
            if (all) break;
        }
    }
    join();   // what follows (alignment, the read-back) is the decode stream's
    if (he != hipSuccess) return fail_loop("joining the free-running halves");
    return WH_OK;
}

// ---- what the two read-backs share ----
// n 4-byte elements from the device into v, on the decode stream (the caller synchronises)
template <typename V>
static hipError_t fetch(wh_ctx* c, V& v, const void* src, size_t n) {
    v.resize(n);
    return hipMemcpyAsync(v.data(), src, n * 4, hipMemcpyDeviceToHost, c->stream);
}
// keeps the languages of this batch's n clips for wh_get_languages; clip b's values are those of row b * stride (beam search: its first beam).
// Later batches of a long-form call (lang_fix): the file's language and window 0's probabilities (the first rows kept), once per window
static void keep_languages(wh_ctx* c, const DecodePlan& pl, int n, int stride, const std::vector<int>& chosen, const std::vector<float>& probs) {
    const size_t n_lang = c->lang.ids.size();
    if (pl.lang_fix) {
        for (int b = 0; b < n; b++) {
            c->lang.rows.push_back(c->lang.fixed);
            for (size_t j = 0; j < n_lang; j++) { const float pj = c->lang.prob_rows[j]; c->lang.prob_rows.push_back(pj); }
        }
    } else if (pl.lang_det) {
        for (int b = 0; b < n; b++) {
            c->lang.rows.push_back(chosen[(size_t)b * stride]);
            c->lang.prob_rows.insert(c->lang.prob_rows.end(), probs.begin() + (size_t)b * stride * n_lang, probs.begin() + ((size_t)b * stride + 1) * n_lang);
        }
        c->lang.have = true;
        c->lang.have_n = n_lang;
    }
}
// the kept logits of the selected rows to the caller; rows_of(r): the positions batch row r produced
template <typename F>
static int copy_kept_logits(wh_ctx* c, const DecodePlan& pl, float* logits_out, const int32_t* sel, F rows_of) {
    const size_t logits_rows = pl.key.logits_rows, vocab = c->m->dims.vocab;
    for (size_t i = 0; i < pl.n_lrows; i++) {
        const size_t rows = rows_of(sel ? sel[i] : (int)i);
        CTX_HIP(c, hipMemcpy(logits_out + i * logits_rows * vocab, pl.key.d_logits + i * logits_rows * vocab, std::min(rows, logits_rows) * vocab * 4,
                             hipMemcpyDeviceToHost));
    }
    return WH_OK;
}

// tokens, counts, log-probabilities, no-speech, languages, logits; keeps what wh_get_logprobs / wh_get_languages return
static int read_back(wh_ctx* c, const DecodePlan& pl, int64_t* tokens_out, size_t tok_stride, size_t* n_tokens_out, float* logits_out, const int32_t* sel) {
    hipStream_t s = c->stream;
    const int nb = pl.key.nb, ld = c->tok_ld, Nmax = pl.Nmax, PP = pl.key.n_prompt;
    const bool lp = c->lp.on || pl.key.sample_buf;   // (a sampling call records log-probabilities itself, in its own buffer)
    const size_t n_lang = c->lang.ids.size();
    std::vector<int> toks, nout, lch, afr, asb;
    std::vector<float> lps, nsp, lpr;
    const double t0 = now_s();
    CTX_HIP(c, fetch(c, toks, c->out_tokens, (size_t)nb * ld));
    CTX_HIP(c, fetch(c, nout, c->n_out, nb));
    if (lp) CTX_HIP(c, fetch(c, lps, pl.key.sample_buf ? c->sm.lp : c->lp.tok, (size_t)nb * ld));
    if (pl.lp_probe) CTX_HIP(c, fetch(c, nsp, c->lp.ns, nb));
    if (pl.lang_det) {
        CTX_HIP(c, fetch(c, lch, c->lang.chosen, nb));
        CTX_HIP(c, fetch(c, lpr, c->lang.probs, (size_t)nb * n_lang));
    }
    if (c->al.on) {
        CTX_HIP(c, fetch(c, afr, c->al.frames, (size_t)nb * c->m->dims.n_text_ctx));
        CTX_HIP(c, fetch(c, asb, c->al.sb, nb));
    }
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    c->sm.collect_timing();
    if (c->al.on) {   // kept for wh_get_token_frames / wh_get_alignment_debug
        const int tc = c->m->dims.n_text_ctx, nh = (int)(c->al.heads.size() / 2), Sp = (c->m->dims.n_audio_ctx + 3) / 4 * 4, NEW = pl.NEW;
        for (int b = 0; b < nb; b++) {
            c->al.rows.emplace_back(afr.begin() + (size_t)b * tc, afr.begin() + (size_t)b * tc + (nout[b] - PP));
            c->al.nframes.push_back(asb[b]);
        }
        c->al.have = true;
        c->al.dbg.resize(c->al.debug.size());
        for (size_t k = 0; k < c->al.debug.size(); k++) {   // the debug rows' slots cut to [n_heads][n_gen][S_b] and [n_gen][S_b]
            wh_ctx::AlignDebug& dbg = c->al.dbg[k];
            const int r = c->al.debug[k], n = nout[r] - PP, sb = asb[r];
            std::vector<float> pr((size_t)nh * n * sb, 0.0f), mt((size_t)n * sb, 0.0f);
            if (!dbg.probs.empty() && n > 1)
                for (int h = 0; h < nh; h++)
                    for (int g = 0; g < n; g++) std::copy_n(dbg.probs.begin() + ((size_t)h * NEW + g) * Sp, sb, pr.begin() + ((size_t)h * n + g) * sb);
            if (!dbg.matrix.empty() && n > 1)
                for (int g = 0; g < n; g++) std::copy_n(dbg.matrix.begin() + (size_t)g * Sp, sb, mt.begin() + (size_t)g * sb);
            dbg.n_heads = nh; dbg.n_gen = n; dbg.sb = sb;
            dbg.probs.swap(pr);
            dbg.matrix.swap(mt);
        }
    }
    keep_languages(c, pl, nb, 1, lch, lpr);
    if (lp) {   // kept for wh_get_logprobs: each clip's generated positions
        for (int b = 0; b < nb; b++) c->lp.rows.emplace_back(lps.begin() + (size_t)b * ld + PP, lps.begin() + (size_t)b * ld + nout[b]);
        c->lp.ns_rows.insert(c->lp.ns_rows.end(), nsp.begin(), nsp.end());
        c->lp.have = true;
        c->lp.have_ns = pl.lp_probe;
    }
    for (int b = 0; b < nb; b++) {
        n_tokens_out[b] = (size_t)(nout[b] - Nmax);   // the prefix columns are not echoed: shared prompt ++ generated, as without prefixes
        for (int i = Nmax; i < nout[b]; i++) tokens_out[(size_t)b * tok_stride + i - Nmax] = toks[(size_t)b * ld + i];
    }
    if (logits_out)
        if (int rc = copy_kept_logits(c, pl, logits_out, sel, [&](int b) { return (size_t)nout[b] - PP; })) return rc;
    c->timing.d2h_s = now_s() - t0;
    return WH_OK;
}

// read_back of a call with beam search: the pool and the trace come back, the parents are walked back into hypotheses, the
// hypotheses are ranked (f32), and the best one of each clip is returned as its tokens (and log-probabilities); keeps what wh_get_beams /
// wh_get_beam_trace return.  Language detection and the no-speech probe: the clip's first row.
static int read_back_beam(wh_ctx* c, const DecodePlan& pl, int64_t* tokens_out, size_t tok_stride, size_t* n_tokens_out, float* logits_out, const int32_t* sel) {
    hipStream_t s = c->stream;
    const int R = pl.key.nb, K = pl.K, ncl = pl.ncl, ld = c->max_batch, PP = pl.key.n_prompt, NEW = pl.NEW;
    const size_t n_lang = c->lang.ids.size();
    std::vector<int> trp, trt, trpool, pool, pool_n, nsteps, feed, lch;
    std::vector<float> trs, trl, nsp, lpr;
    const double t0 = now_s();
    const size_t ntr = (size_t)NEW * ld;   // (the trace is [position][max_batch]: the call's positions are its first NEW rows)
    CTX_HIP(c, fetch(c, trp, c->bm.tr_parent, ntr));
    CTX_HIP(c, fetch(c, trt, c->bm.tr_token, ntr));
    CTX_HIP(c, fetch(c, trs, c->bm.tr_score, ntr));
    CTX_HIP(c, fetch(c, trl, c->bm.tr_lp, ntr));
    CTX_HIP(c, fetch(c, trpool, c->bm.tr_pool, ntr));
    CTX_HIP(c, fetch(c, pool, c->bm.pool, (size_t)ncl * WH_MAX_BEAM_CANDIDATES * 4));
    CTX_HIP(c, fetch(c, pool_n, c->bm.pool_n, ncl));
    CTX_HIP(c, fetch(c, nsteps, c->bm.n_steps, ncl));
    CTX_HIP(c, fetch(c, feed, c->feed, (size_t)R * c->tok_ld));   // (the prompt as it was fed: the detected language token)
    if (pl.lp_probe) CTX_HIP(c, fetch(c, nsp, c->lp.ns, R));
    if (pl.lang_det) {
        CTX_HIP(c, fetch(c, lch, c->lang.chosen, R));
        CTX_HIP(c, fetch(c, lpr, c->lang.probs, (size_t)R * n_lang));
    }
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    c->bm.collect_timing();
    keep_languages(c, pl, ncl, K, lch, lpr);
    c->bm.traces.assign(c->bm.trace_clips.size(), wh_ctx::BeamTrace());
    for (int clip = 0; clip < ncl; clip++) {
        const int ns = nsteps[clip], r0 = clip * K;
        // the history of beam j after position g (g == -1: empty), newest token last
        auto chain = [&](int g, int j, std::vector<int>& toks, std::vector<float>& lps) {
            for (; g >= 0; g--) {
                const size_t t = (size_t)g * ld + r0 + j;
                toks.push_back(trt[t]);
                lps.push_back(trl[t]);
                j = trp[t];
            }
            std::reverse(toks.begin(), toks.end());
            std::reverse(lps.begin(), lps.end());
        };
        std::vector<wh_ctx::BeamHyp> hyps;
        for (int e = 0; e < pool_n[clip]; e++) {   // the pool, in insertion order
            const int* pe = pool.data() + ((size_t)clip * WH_MAX_BEAM_CANDIDATES + e) * 4;
            wh_ctx::BeamHyp h;
            chain(pe[0] - 1, pe[1], h.tokens, h.lps);
            float lp;
            memcpy(&h.sum, &pe[2], 4);
            memcpy(&lp, &pe[3], 4);
            h.tokens.push_back(pl.key.eot);
            h.lps.push_back(lp);
            h.finished = true;
            hyps.push_back(std::move(h));
        }
        if ((int)hyps.size() < K && ns > 0) {   // fewer than K: the live, non-dead beams by descending score (ties: the lower beam)
            std::vector<int> live;
            for (int j = 0; j < K; j++)
                if (trs[(size_t)(ns - 1) * ld + r0 + j] > -INFINITY) live.push_back(j);
            std::stable_sort(live.begin(), live.end(), [&](int x, int y) { return trs[(size_t)(ns - 1) * ld + r0 + x] > trs[(size_t)(ns - 1) * ld + r0 + y]; });
            for (int j : live) {
                if ((int)hyps.size() >= K) break;
                wh_ctx::BeamHyp h;
                chain(ns - 1, j, h.tokens, h.lps);
                h.sum = trs[(size_t)(ns - 1) * ld + r0 + j];
                hyps.push_back(std::move(h));
            }
        }
        for (auto& h : hyps) {
            const float len = (float)std::max<size_t>(1, h.tokens.size() - (h.finished ? 1 : 0));
            h.rank = c->bm.length_penalty < 0.0f ? h.sum / len : h.sum / powf((5.0f + len) / 6.0f, c->bm.length_penalty);
        }
        std::stable_sort(hyps.begin(), hyps.end(), [](const wh_ctx::BeamHyp& x, const wh_ctx::BeamHyp& y) { return x.rank > y.rank; });
        // the clip's tokens: the prompt as fed, then the best hypothesis
        for (int i = pl.Nmax; i < PP; i++) tokens_out[(size_t)clip * tok_stride + i - pl.Nmax] = feed[(size_t)r0 * c->tok_ld + i];
        size_t n = (size_t)(PP - pl.Nmax);
        if (!hyps.empty())
            for (int t : hyps[0].tokens) tokens_out[(size_t)clip * tok_stride + n++] = t;
        n_tokens_out[clip] = n;
        if (c->lp.on) {
            c->lp.rows.emplace_back(hyps.empty() ? std::vector<float>() : hyps[0].lps);
            if (pl.lp_probe) c->lp.ns_rows.push_back(nsp[r0]);
        }
        for (size_t k = 0; k < c->bm.trace_clips.size(); k++) {
            if (c->bm.trace_clips[k] != clip) continue;
            wh_ctx::BeamTrace& tr = c->bm.traces[k];
            tr.K = K; tr.n_steps = ns;
            tr.parents.clear(); tr.tokens.clear(); tr.scores.clear(); tr.pool.clear();
            for (int g = 0; g < ns; g++) {
                for (int j = 0; j < K; j++) {
                    const size_t t = (size_t)g * ld + r0 + j;
                    tr.parents.push_back(trp[t]); tr.tokens.push_back(trt[t]); tr.scores.push_back(trs[t]);
                }
                tr.pool.push_back(trpool[(size_t)g * ld + clip]);
            }
        }
        c->bm.hyps.push_back(std::move(hyps));
    }
    c->bm.have = true;
    if (c->lp.on) { c->lp.have = true; c->lp.have_ns = pl.lp_probe; }
    if (logits_out)   // physical rows: what each produced at the positions its clip ran
        if (int rc = copy_kept_logits(c, pl, logits_out, sel, [&](int r) { return (size_t)nsteps[r / K]; })) return rc;
    c->timing.d2h_s = now_s() - t0;
    return WH_OK;
}

// `sel` (optional, with logits_out): the n_sel batch rows whose logits are read back — logits_out is then [n_sel][logits_rows][vocab]
int run_decode(wh_ctx* c, int nb, const wh_decode_params* p, int64_t* tokens_out, size_t tok_stride, size_t* n_tokens_out, float* logits_out,
               size_t logits_rows, const std::function<int()>& after_kv, const int32_t* sel, size_t n_sel) {
    hipStream_t s = c->stream;
    c->cur = s;
    DecodePlan pl;
    int rc = plan_decode(c, nb, p, logits_out != nullptr, logits_rows, sel, n_sel, pl);
    if (rc) return rc;
    const wh_ctx::StepKey& key = pl.key;
    c->last_split = c->last_free = 0;   // (run_token_loop sets them to what it launched)
    if (key.split && (rc = ensure_split_stream(c))) return rc;
    // the encoder states come from the encoder stream
    if (c->s_enc != s) CTX_HIP(c, hipStreamWaitEvent(s, c->ev_enc_done, 0));
    CTX_HIP(c, hipEventRecord(c->ev[5], s));   // decode start (stage timing)
    if ((rc = upload_token_state(c, p, pl)) || (rc = prepare_logits(c, pl)) || (rc = prepare_alignment(c, pl)) || (rc = project_cross_kv(c, nb, after_kv))) return rc;
    // Positions 0 .. PP-1 (the prompt, the last of which emits the first token) are launched eagerly; the rest is the token loop's
    const int PP = key.n_prompt, total_pos = PP + pl.NEW - 1;
    for (int step = 0; step < std::min(PP, total_pos); step++) {
        PromptStep ps;
        ps.emits = step >= PP - 1;
        ps.lang = step == pl.lang_pos; ps.lang_col = pl.Nmax + pl.lang_slot;
        ps.probe = step == pl.probe_pos;
        launch_step(c, key, &ps);
    }
    if ((rc = run_token_loop(c, key, total_pos - PP, p->n_forced == 0)) || (rc = run_alignment(c, pl))) return rc;
    CTX_HIP(c, hipEventRecord(c->ev[3], s));
    if (key.beam_k) return read_back_beam(c, pl, tokens_out, tok_stride, n_tokens_out, logits_out, sel);
    return read_back(c, pl, tokens_out, tok_stride, n_tokens_out, logits_out, sel);
}

}  // namespace wh
