// wh_options.cpp — the decode options of a context (include/whisper_hip.h): the eight setters and their getters, the gate
// every decode entry passes before it launches anything (options_check), and the measurement hooks.
#include "wh_host_shared.h"

using namespace wh;

namespace wh {

// An option setter's buffer: `bytes` zeroed bytes on the context's device into `out`, or false with the setter's error recorded (the caller
// returns WH_ERR_NOMEM) and `out` as it was.
template <typename T>
static bool setter_alloc(wh_ctx* c, const char* setter, size_t bytes, DevBuf<T>& out) {
    hipSetDevice(c->m->device);
    DevBuf<T> b;
    hipError_t e = hipMalloc(&b.p, bytes);
    if (e == hipSuccess) e = hipMemset(b.p, 0, bytes);
    if (e != hipSuccess) {
        fail(c, WH_ERR_NOMEM, "%s: hipMalloc: %s", setter, hipGetErrorString(e));
        return false;
    }
    b.bytes = bytes;
    out = std::move(b);
    return true;
}

// An option whose buffers the captured step may hold is cleared: the step graph is dropped if one of them is set, then the struct is reset — its
// owners free the buffers, and its getters have nothing to return until the next call with the option on.
template <typename Opt>
static void clear_option(wh_ctx* c, Opt& o) {
    hipSetDevice(c->m->device);
    if (o.held()) drop_step_graph(c);
    o.reset_results();
    o = Opt();
}

// Per-clip prefixes: the prefix of row b of a device batch (its length in *len), and what a decode entry refuses because of the
// prefixes, checked through options_check.  first_row = index of the batch's first window in a long-form call (-1: the rows are the call's clips).
const int64_t* prefix_of(const wh_ctx* c, long first_row, int b, int* len) {
    size_t clip = (size_t)b;
    if (first_row >= 0) {   // long-form: one prefix for the file, for window 0 or for every window
        if (c->pfx.scope == WH_PREFIX_FIRST_WINDOW && first_row + b != 0) { *len = 0; return c->pfx.ids.data(); }
        clip = 0;
    }
    *len = (int)(c->pfx.offsets[clip + 1] - c->pfx.offsets[clip]);
    return c->pfx.ids.data() + c->pfx.offsets[clip];
}
static int prefix_check(wh_ctx* c, const wh_decode_params* p, int nb, bool longform) {
    if (!c->pfx.on) return WH_OK;
    const size_t n_clips = c->pfx.offsets.size() - 1;
    if (longform ? n_clips != 1 : n_clips != (size_t)nb)
        return fail(c, WH_ERR_ARG, "decode: wh_ctx_set_prefixes was given %zu clips, this call has %d", n_clips, longform ? 1 : nb);
    int nmax = 0;
    for (size_t b = 0; b < n_clips; b++) nmax = std::max(nmax, (int)(c->pfx.offsets[b + 1] - c->pfx.offsets[b]));
    if (nmax == 0) return WH_OK;
    if ((size_t)nmax + p->n_prompt + p->max_new_tokens > (size_t)c->m->dims.n_text_ctx)
        return fail(c, WH_ERR_ARG, "decode: longest prefix (%d) + prompt (%zu) + max_new_tokens (%zu) exceeds %d positions", nmax, p->n_prompt, p->max_new_tokens,
                    c->m->dims.n_text_ctx);
    if (c->lang.on)
        return fail(c, WH_ERR_UNSUPPORTED, "decode: language detection with a non-empty prefix is not supported (the logits at <|startoftranscript|> depend on the "
                                           "prefix): detect the language with an un-prefixed call first, then decode with that language in the prompt");
    return WH_OK;
}

// Word-level timestamps: what a decode entry refuses because of them, checked by every entry before it launches anything and
// again by run_decode.
static int align_check(wh_ctx* c, int nb) {
    if (!c->al.on) return WH_OK;
    if (c->m->prec == WH_PREC_FP8 || c->m->prec == WH_PREC_F16X3)
        return fail(c, WH_ERR_UNSUPPORTED, "decode: word-level timestamps are not supported in the %s mode (no score kernel for its keys and queries)",
                    c->m->prec == WH_PREC_FP8 ? "fp8" : "f16x3");
    if (c->cross_es && !wh_align_scores_supported(WH_ALIGN_ES_BF16, c->m->dims.d_model))
        return fail(c, WH_ERR_UNSUPPORTED, "decode: word-level timestamps have no score kernel for encoder states %d wide", c->m->dims.d_model);
    for (int r : c->al.debug)
        if (r >= nb) return fail(c, WH_ERR_ARG, "decode: alignment debug row %d outside the batch (%d clips)", r, nb);
    return WH_OK;
}

// Beam search: what a decode entry refuses because of it, checked by every entry before it launches anything and again by
// run_decode.  nb = the call's clips (a long-form call: one device batch never holds more than max_batch / K windows).
static int beam_check(wh_ctx* c, const wh_decode_params* p, int nb) {
    if (!c->bm.on) return WH_OK;
    if ((long)nb * c->bm.k > c->max_batch)
        return fail(c, WH_ERR_ARG, "decode: %d clips x beam_size %d exceed max_batch (%d rows)", nb, c->bm.k, c->max_batch);
    if (c->m->prec == WH_PREC_FP8 || c->m->prec == WH_PREC_F16X3)
        return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search is not supported in the %s mode", c->m->prec == WH_PREC_FP8 ? "fp8" : "f16x3");
    if (p->n_forced) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with forced tokens is not supported");
    if (c->rep.on) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with repetition controls is not supported");
    if (c->al.on) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with word-level timestamps is not supported");
    if (c->pfx.on && c->pfx.offsets.back() != 0) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with a non-empty prefix is not supported");
    return WH_OK;
}

// Temperature sampling: what a decode entry refuses because of it, checked by every entry before it launches anything and again
// by run_decode.  nb = the call's clips (a long-form call: the setter's one row stands for every window).
static int sample_check(wh_ctx* c, int nb, bool longform) {
    if (!c->sm.on) return WH_OK;
    if (c->sm.temp.size() != (size_t)(longform ? 1 : nb))
        return fail(c, WH_ERR_ARG, "decode: wh_ctx_set_sampling was given %zu rows, this call has %d", c->sm.temp.size(), longform ? 1 : nb);
    if (c->bm.on) return fail(c, WH_ERR_UNSUPPORTED, "decode: sampling with beam search is not supported (the search runs at temperature 0 only)");
    if (c->rep.on) return fail(c, WH_ERR_UNSUPPORTED, "decode: sampling with repetition controls is not supported");
    if (c->al.on) return fail(c, WH_ERR_UNSUPPORTED, "decode: sampling with word-level timestamps is not supported");
    return WH_OK;
}
// The one gate of the decode options: every entry passes it before it launches anything, and plan_decode again.  The order — prefixes, alignment,
// beam search, sampling — decides which message a call gets that two options refuse.  al_rows: the batch rows that alignment's debug rows must
// exist in, where that is not n_clips (the long-form entry: its last, smallest device batch).
int options_check(wh_ctx* c, const wh_decode_params* p, int n_clips, bool longform, int al_rows) {
    int rc;
    if ((rc = prefix_check(c, p, n_clips, longform)) || (rc = align_check(c, al_rows >= 0 ? al_rows : n_clips)) || (rc = beam_check(c, p, n_clips)) ||
        (rc = sample_check(c, n_clips, longform)))
        return rc;
    return WH_OK;
}
// the argument errors of a wh_alignment_opts, for the setter and for wh_align_tokens (`who`, for the message): WH_ERR_ARG, nothing changed
int alignment_opts_check(wh_ctx* c, const wh_alignment_opts* o, const char* who) {
    if (o->struct_size != sizeof(wh_alignment_opts)) return fail(c, WH_ERR_ARG, "%s: struct_size %zu, expected %zu", who, o->struct_size, sizeof(wh_alignment_opts));
    const wh_dims& D = c->m->dims;
    if (o->n_heads < 1 || o->n_heads > WH_MAX_ALIGN_HEADS || !o->heads) return fail(c, WH_ERR_ARG, "%s: n_heads %zu outside 1..%d (or a NULL list)", who, o->n_heads, WH_MAX_ALIGN_HEADS);
    if (o->n_debug_rows > WH_MAX_ALIGN_DEBUG_ROWS || (o->n_debug_rows && !o->debug_rows)) return fail(c, WH_ERR_ARG, "%s: more than %d debug rows (or a NULL list)", who, WH_MAX_ALIGN_DEBUG_ROWS);
    for (size_t i = 0; i < o->n_heads; i++) {
        const int l = o->heads[2 * i], h = o->heads[2 * i + 1];
        if (l < 0 || l >= D.dec_layers || h < 0 || h >= D.n_heads) return fail(c, WH_ERR_ARG, "%s: (layer %d, head %d) outside the model (%d layers, %d heads)", who, l, h, D.dec_layers, D.n_heads);
        for (size_t j = 0; j < i; j++)
            if (o->heads[2 * j] == l && o->heads[2 * j + 1] == h) return fail(c, WH_ERR_ARG, "%s: (layer %d, head %d) listed twice", who, l, h);
    }
    for (size_t i = 0; i < o->n_debug_rows; i++)
        if (o->debug_rows[i] < 0) return fail(c, WH_ERR_ARG, "%s: negative debug row", who);
    return WH_OK;
}
// the listed heads of each decoder layer, with their slots in the caller's list
void alignment_layers(const wh_dims& D, const wh_alignment_opts* o, std::vector<AlignLayerHeads>& layer) {
    layer.assign(D.dec_layers, AlignLayerHeads());
    for (size_t i = 0; i < o->n_heads; i++) {
        AlignLayerHeads& lh = layer[o->heads[2 * i]];
        lh.slot[lh.n] = (unsigned char)i;
        lh.head[lh.n] = (unsigned char)o->heads[2 * i + 1];
        lh.n++;
    }
}
// every temperature 0 and every row active: the plain kernels are launched
bool sample_trivial(const wh_ctx* c) {
    for (size_t i = 0; i < c->sm.temp.size(); i++)
        if (c->sm.temp[i] != 0.0f || !c->sm.active[i]) return false;
    return true;
}

}  // namespace wh

extern "C" {

// Whisper's timestamp rules on every decode entry of the ctx.  The buffers — the rows' timestamp logits and a per-row state —
// are allocated when rules are turned on (the logits again for another timestamp_begin); the captured decode step is recaptured when the
// key changes (and before a buffer it holds is freed).
int wh_ctx_set_timestamp_rules(wh_ctx* c, const wh_timestamp_rules* r) {
    if (!c) return WH_ERR_ARG;
    if (!r) {
        c->ts.on = false;
        return WH_OK;
    }
    if (r->struct_size != sizeof(wh_timestamp_rules)) return fail(c, WH_ERR_ARG, "wh_ctx_set_timestamp_rules: struct_size %zu, expected %zu", r->struct_size, sizeof(wh_timestamp_rules));
    const int vocab = c->m->dims.vocab;
    if (r->timestamp_begin <= 0 || r->timestamp_begin >= vocab)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_timestamp_rules: timestamp_begin %lld outside the vocabulary (%d)", (long long)r->timestamp_begin, vocab);
    if (r->no_timestamps >= vocab || r->no_timestamps < -1)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_timestamp_rules: no_timestamps %lld outside the vocabulary", (long long)r->no_timestamps);
    const int ld = vocab - (int)r->timestamp_begin;
    if (!c->ts.logits || c->ts.ld != ld) {   // the new logits exist before the old ones go: a failed allocation leaves the context as it was
        DevBuf<float> tl;
        DevBuf<int> st;
        if (!setter_alloc(c, "wh_ctx_set_timestamp_rules", (size_t)c->mpad * ld * 4, tl)) return WH_ERR_NOMEM;
        if (!c->ts.state && !setter_alloc(c, "wh_ctx_set_timestamp_rules", (size_t)c->mpad * 16, st)) return WH_ERR_NOMEM;
        drop_step_graph(c);   // (a captured step may hold the old buffer's address)
        c->ts.logits = std::move(tl);
        c->ts.ld = ld;
        if (st) c->ts.state = std::move(st);
    }
    c->ts.on = true;
    c->ts.begin = r->timestamp_begin;
    c->ts.no_ts = r->no_timestamps;
    // (a bound past the vocabulary is no bound: clamped to the last timestamp, so tb + max_init never overflows in the kernels)
    c->ts.max_init = r->max_initial_timestamp_index < 0 ? -1 : std::min<int>(r->max_initial_timestamp_index, vocab - 1 - (int)r->timestamp_begin);
    return WH_OK;
}

// Token log-probabilities and the no-speech probe on every decode entry of the ctx.  The buffers are allocated the first
// time it is turned on; the captured decode step is keyed on the setting (other kernels, one more argument).
int wh_ctx_set_logprobs(wh_ctx* c, const wh_logprob_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->lp.on = false;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_logprob_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_logprobs: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_logprob_opts));
    const int vocab = c->m->dims.vocab;
    if (o->no_speech < -1 || o->no_speech >= vocab) return fail(c, WH_ERR_ARG, "wh_ctx_set_logprobs: no_speech %lld outside the vocabulary (%d)", (long long)o->no_speech, vocab);
    if (o->sot_index < 0) return fail(c, WH_ERR_ARG, "wh_ctx_set_logprobs: negative sot_index");
    if (!c->lp.buf) {
        const size_t MP = (size_t)c->mpad, B = (size_t)c->max_batch, n_tiles = ((size_t)vocab + 15) / 16;
        Carver cv;
        const size_t o_sum = cv.take(MP * (n_tiles + 4) * 4), o_tok = cv.take(B * c->tok_ld * 4), o_mask = cv.take(((size_t)vocab / 32 + 1) * 4);
        const size_t o_pv = cv.take(MP * 4), o_ns = cv.take(B * 4);
        if (!setter_alloc(c, "wh_ctx_set_logprobs", cv.off, c->lp.buf)) return WH_ERR_NOMEM;
        char* buf = c->lp.buf;
        c->lp.part_sum = at<float>(buf, o_sum);
        c->lp.tok = at<float>(buf, o_tok);
        c->lp.mask_zero = at<unsigned>(buf, o_mask);
        c->lp.probe_v = at<float>(buf, o_pv);
        c->lp.ns = at<float>(buf, o_ns);
    }
    c->lp.on = true;
    c->lp.no_speech = o->no_speech;
    c->lp.sot_index = o->sot_index;
    return WH_OK;
}

// Repetition penalty and no-repeat n-grams on every decode entry of the ctx.  The bitmap and the side buffer are allocated when
// the option is turned on and freed when it is cleared ({1.0f, 0} clears it); the captured decode step is keyed on the setting and dropped
// before a buffer it holds is freed.
int wh_ctx_set_repetition(wh_ctx* c, const wh_repetition_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (o) {
        if (o->struct_size != sizeof(wh_repetition_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_repetition: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_repetition_opts));
        if (!std::isfinite(o->repetition_penalty) || !(o->repetition_penalty > 0.0f))
            return fail(c, WH_ERR_ARG, "wh_ctx_set_repetition: repetition_penalty %g is not a finite value above 0", (double)o->repetition_penalty);
        if (o->no_repeat_ngram_size < 0 || o->no_repeat_ngram_size > WH_MAX_NGRAM)
            return fail(c, WH_ERR_ARG, "wh_ctx_set_repetition: no_repeat_ngram_size %d outside 0 .. %d", (int)o->no_repeat_ngram_size, WH_MAX_NGRAM);
    }
    if (!o || (o->repetition_penalty == 1.0f && o->no_repeat_ngram_size == 0)) {
        clear_option(c, c->rep);
        return WH_OK;
    }
    if (!c->rep.bits) {
        const size_t vocab = (size_t)c->m->dims.vocab, words = (vocab + 31) / 32, B = (size_t)c->max_batch;
        DevBuf<unsigned> bits;
        DevBuf<float> side;
        if (!setter_alloc(c, "wh_ctx_set_repetition", B * words * 4, bits) || !setter_alloc(c, "wh_ctx_set_repetition", B * vocab * 4, side)) return WH_ERR_NOMEM;
        c->rep.bits = std::move(bits); c->rep.side = std::move(side); c->rep.words = (int)words;
    }
    c->rep.on = true;
    c->rep.p = o->repetition_penalty;
    c->rep.n = o->no_repeat_ngram_size;
    return WH_OK;
}

// Language detection on every decode entry of the ctx.  The buffers are allocated the first time it is turned on; nothing of
// it enters the captured decode step.
int wh_ctx_set_language_detection(wh_ctx* c, const wh_language_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->lang.on = false;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_language_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_language_detection: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_language_opts));
    const int vocab = c->m->dims.vocab;
    if (o->n_lang < 1 || o->n_lang > WH_MAX_LANGUAGES || !o->lang_ids) return fail(c, WH_ERR_ARG, "wh_ctx_set_language_detection: n_lang %zu outside 1..%d (or a NULL list)", o->n_lang, WH_MAX_LANGUAGES);
    if (o->sot_index < 0) return fail(c, WH_ERR_ARG, "wh_ctx_set_language_detection: negative sot_index");
    for (size_t i = 0; i < o->n_lang; i++) {
        if (o->lang_ids[i] < 0 || o->lang_ids[i] >= vocab) return fail(c, WH_ERR_ARG, "wh_ctx_set_language_detection: id %lld outside the vocabulary (%d)", (long long)o->lang_ids[i], vocab);
        for (size_t j = 0; j < i; j++)
            if (o->lang_ids[j] == o->lang_ids[i]) return fail(c, WH_ERR_ARG, "wh_ctx_set_language_detection: id %lld listed twice", (long long)o->lang_ids[i]);
    }
    hipSetDevice(c->m->device);
    const size_t MP = (size_t)c->mpad, B = (size_t)c->max_batch;
    Carver cv;
    const size_t o_ids = cv.take(WH_LANG_LD * 4), o_log = cv.take(MP * WH_LANG_LD * 4), o_pr = cv.take(B * WH_LANG_LD * 4), o_ch = cv.take(B * 4);
    DevBuf<> fresh;   // (the first call's allocation: the context's only once the id list is on the device)
    if (!c->lang.buf && !setter_alloc(c, "wh_ctx_set_language_detection", cv.off, fresh)) return WH_ERR_NOMEM;
    char* buf = fresh ? (char*)fresh : (char*)c->lang.buf;
    int ids[WH_LANG_LD];
    for (int i = 0; i < WH_LANG_LD; i++) ids[i] = (int)o->lang_ids[(size_t)i < o->n_lang ? i : 0];
    hipError_t e = hipMemcpy(at<int>(buf, o_ids), ids, sizeof ids, hipMemcpyHostToDevice);   // (nothing of the ctx is in flight: every call ends with a stream synchronisation)
    if (e != hipSuccess) {
        if (!fresh && c->lang.on) {   // put the list in force back
            for (int i = 0; i < WH_LANG_LD; i++) ids[i] = (int)c->lang.ids[(size_t)i < c->lang.ids.size() ? i : 0];
            hipMemcpy(at<int>(buf, o_ids), ids, sizeof ids, hipMemcpyHostToDevice);
        }
        return fail(c, WH_ERR_HIP, "wh_ctx_set_language_detection: hipMemcpy: %s", hipGetErrorString(e));
    }
    if (fresh) c->lang.buf = std::move(fresh);
    c->lang.d_ids = at<int>(buf, o_ids);
    c->lang.logits = at<float>(buf, o_log);
    c->lang.probs = at<float>(buf, o_pr);
    c->lang.chosen = at<int>(buf, o_ch);
    c->lang.ids.assign(o->lang_ids, o->lang_ids + o->n_lang);
    c->lang.sot_index = o->sot_index;
    c->lang.on = true;
    return WH_OK;
}

// Per-clip prompt prefixes on every decode entry of the ctx.  The setter copies the ids; the per-row offsets are computed and
// uploaded by each call (run_decode).
int wh_ctx_set_prefixes(wh_ctx* c, const wh_prefix_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->pfx.on = false;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_prefix_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_prefix_opts));
    if (o->n_clips < 1 || o->n_clips > (size_t)c->max_batch || !o->offsets) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: n_clips %zu outside 1..max_batch (%d) (or NULL offsets)", o->n_clips, c->max_batch);
    if (o->longform_scope != WH_PREFIX_FIRST_WINDOW && o->longform_scope != WH_PREFIX_ALL_WINDOWS) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: unknown longform_scope %d", (int)o->longform_scope);
    if (o->offsets[0] != 0) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: offsets[0] must be 0");
    for (size_t b = 0; b < o->n_clips; b++)
        if (o->offsets[b + 1] < o->offsets[b]) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: offsets decrease at clip %zu", b);
    const size_t n_ids = o->offsets[o->n_clips];
    if (n_ids && !o->ids) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: ids is NULL");
    const int vocab = c->m->dims.vocab;
    for (size_t i = 0; i < n_ids; i++)
        if (o->ids[i] < 0 || o->ids[i] >= vocab) return fail(c, WH_ERR_ARG, "wh_ctx_set_prefixes: id %lld outside the vocabulary (%d)", (long long)o->ids[i], vocab);
    if (!c->pfx.off && !setter_alloc(c, "wh_ctx_set_prefixes", (size_t)c->max_batch * 4, c->pfx.off)) return WH_ERR_NOMEM;
    c->pfx.ids.assign(o->ids, o->ids + n_ids);
    c->pfx.offsets.assign(o->offsets, o->offsets + o->n_clips + 1);
    c->pfx.scope = o->longform_scope;
    c->pfx.on = true;
    return WH_OK;
}

// Word-level timestamps on every decode entry of the ctx.  The setter copies the head list and allocates the frames; the side
// buffer of the queries and the post-pass workspace are sized by the calls.  The captured decode step is keyed on the list's identity.
int wh_ctx_set_alignment(wh_ctx* c, const wh_alignment_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->al.on = false;
        return WH_OK;
    }
    if (int rc = alignment_opts_check(c, o, "wh_ctx_set_alignment")) return rc;
    const wh_dims& D = c->m->dims;
    if (!c->al.frames) {
        DevBuf<int> fr, sb;
        if (!setter_alloc(c, "wh_ctx_set_alignment", (size_t)c->max_batch * D.n_text_ctx * 4, fr) || !setter_alloc(c, "wh_ctx_set_alignment", (size_t)c->max_batch * 4, sb)) return WH_ERR_NOMEM;
        c->al.frames = std::move(fr); c->al.sb = std::move(sb);
    }
    c->al.heads.assign(o->heads, o->heads + 2 * o->n_heads);
    c->al.debug.assign(o->debug_rows, o->debug_rows + o->n_debug_rows);
    alignment_layers(D, o, c->al.layer);
    c->al.gen++;
    c->al.on = true;
    return WH_OK;
}

// Beam search on every decode entry of the ctx.  The logits scratch and the search state are allocated when the option is turned
// on and freed when it is cleared; the captured decode step is keyed on the setting and dropped before a buffer it holds is freed.
int wh_ctx_set_beam_search(wh_ctx* c, const wh_beam_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        const bool timing = c->bm.timing;   // (a property of the context, read at its creation)
        clear_option(c, c->bm);
        c->bm.timing = timing;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_beam_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_beam_opts));
    if (o->beam_size < 1 || o->beam_size > WH_MAX_BEAMS) return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: beam_size %d outside 1 .. %d", (int)o->beam_size, WH_MAX_BEAMS);
    if (!std::isfinite(o->patience) || !(o->patience > 0.0f)) return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: patience %g is not a finite value above 0", (double)o->patience);
    const long cand = lroundf((float)o->beam_size * o->patience);
    if (cand < 1 || cand > WH_MAX_BEAM_CANDIDATES)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: round(beam_size * patience) = %ld outside 1 .. %d", cand, WH_MAX_BEAM_CANDIDATES);
    if (std::isnan(o->length_penalty)) return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: length_penalty is NaN");
    if (o->n_trace_clips > WH_MAX_BEAM_TRACE_CLIPS || (o->n_trace_clips && !o->trace_clips))
        return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: more than %d trace clips (or a NULL list)", WH_MAX_BEAM_TRACE_CLIPS);
    for (size_t i = 0; i < o->n_trace_clips; i++)
        if (o->trace_clips[i] < 0) return fail(c, WH_ERR_ARG, "wh_ctx_set_beam_search: negative trace clip");
    if (!c->bm.logits) {
        const size_t B = (size_t)c->max_batch, vocab = (size_t)c->m->dims.vocab, b_row = B * 4, b_tr = (size_t)c->tok_ld * B * 4;
        Carver cv;
        const size_t o_scores = cv.take(b_row), o_parent = cv.take(b_row), o_pool_n = cv.take(b_row), o_n_steps = cv.take(b_row);
        const size_t o_state = cv.take(B * WH_BEAM_STATE * 4), o_pool = cv.take(B * WH_MAX_BEAM_CANDIDATES * 4 * 4);
        const size_t o_trp = cv.take(b_tr), o_trt = cv.take(b_tr), o_trpool = cv.take(b_tr), o_trs = cv.take(b_tr), o_trl = cv.take(b_tr);
        DevBuf<float> lg;
        DevBuf<> st;
        if (!setter_alloc(c, "wh_ctx_set_beam_search", B * vocab * 4, lg) || !setter_alloc(c, "wh_ctx_set_beam_search", cv.off, st)) return WH_ERR_NOMEM;
        c->bm.logits = std::move(lg); c->bm.buf = std::move(st);
        char* buf = c->bm.buf;
        c->bm.scores = at<float>(buf, o_scores); c->bm.parent = at<int>(buf, o_parent); c->bm.pool_n = at<int>(buf, o_pool_n); c->bm.n_steps = at<int>(buf, o_n_steps);
        c->bm.state = at<int>(buf, o_state); c->bm.pool = at<int>(buf, o_pool);
        c->bm.tr_parent = at<int>(buf, o_trp); c->bm.tr_token = at<int>(buf, o_trt); c->bm.tr_pool = at<int>(buf, o_trpool);
        c->bm.tr_score = at<float>(buf, o_trs); c->bm.tr_lp = at<float>(buf, o_trl);
    }
    c->bm.on = true;
    c->bm.k = o->beam_size;
    c->bm.c = (int)cand;
    c->bm.length_penalty = o->length_penalty;
    c->bm.trace_clips.assign(o->trace_clips, o->trace_clips + o->n_trace_clips);
    return WH_OK;
}

// Temperature sampling on every decode entry of the ctx.  The logits scratch and the per-row buffers are allocated when the option
// is turned on and freed when it is cleared; the captured decode step is keyed on the buffers' identity and dropped before they are freed.  The
// per-row values reach the kernel through those buffers (upload_token_state), so another rung of a ladder replays the same captured step.
int wh_ctx_set_sampling(wh_ctx* c, const wh_sampling_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        const bool timing = c->sm.timing;   // (a property of the context, read at its creation)
        clear_option(c, c->sm);
        c->sm.timing = timing;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_sampling_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_sampling: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_sampling_opts));
    if (o->n_rows < 1 || o->n_rows > (size_t)c->max_batch || !o->temperature)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_sampling: n_rows %zu outside 1 .. max_batch (%d) (or a NULL temperature list)", o->n_rows, c->max_batch);
    for (size_t i = 0; i < o->n_rows; i++)
        if (!std::isfinite(o->temperature[i]) || o->temperature[i] < 0.0f)
            return fail(c, WH_ERR_ARG, "wh_ctx_set_sampling: temperature[%zu] = %g is negative or not finite", i, (double)o->temperature[i]);
    if (!c->sm.logits) {
        const size_t B = (size_t)c->max_batch, vocab = (size_t)c->m->dims.vocab;
        Carver cv;
        const size_t o_ids = cv.take(B * 8), o_seed = cv.take(8), o_temp = cv.take(B * 4), o_state = cv.take(B * 16), o_lp = cv.take(B * c->tok_ld * 4);
        DevBuf<float> lg;
        DevBuf<> rows;
        if (!setter_alloc(c, "wh_ctx_set_sampling", B * vocab * 4, lg) || !setter_alloc(c, "wh_ctx_set_sampling", cv.off, rows)) return WH_ERR_NOMEM;
        c->sm.logits = std::move(lg); c->sm.buf = std::move(rows);
        char* buf = c->sm.buf;
        c->sm.d_ids = at<unsigned long long>(buf, o_ids); c->sm.d_seed = at<unsigned long long>(buf, o_seed); c->sm.d_temp = at<float>(buf, o_temp);
        c->sm.state = at<int>(buf, o_state); c->sm.lp = at<float>(buf, o_lp);
    }
    c->sm.on = true;
    c->sm.seed = o->seed;
    c->sm.temp.assign(o->temperature, o->temperature + o->n_rows);
    c->sm.active.assign(o->n_rows, 1);
    if (o->active) c->sm.active.assign(o->active, o->active + o->n_rows);
    c->sm.ids.resize(o->n_rows);
    for (size_t i = 0; i < o->n_rows; i++) c->sm.ids[i] = o->row_ids ? o->row_ids[i] : (uint64_t)i;
    return WH_OK;
}

int wh_get_beams(const wh_ctx* c, int64_t* tokens, size_t cap_tokens, size_t* n_tokens, float* sum_logprob, float* rank_score, int32_t* finished,
                 size_t cap_hyp, size_t* n_hyp, size_t cap_clips, size_t* n_clips_out) {
    if (!c) return WH_ERR_ARG;
    if (!c->bm.have) return WH_ERR_STATE;
    const size_t n = c->bm.hyps.size();
    if (n_clips_out) *n_clips_out = n;
    if (!tokens && !n_hyp) return WH_OK;
    if (cap_clips < n) return WH_ERR_ARG;
    for (size_t b = 0; b < n; b++) {
        const size_t nh = std::min(cap_hyp, c->bm.hyps[b].size());
        if (tokens)
            for (size_t h = 0; h < nh; h++)
                if (c->bm.hyps[b][h].tokens.size() > cap_tokens) return WH_ERR_ARG;
    }
    for (size_t b = 0; b < n; b++) {
        const size_t nh = std::min(cap_hyp, c->bm.hyps[b].size());
        if (n_hyp) n_hyp[b] = nh;
        for (size_t h = 0; h < cap_hyp; h++) {
            const size_t at = b * cap_hyp + h;
            const wh_ctx::BeamHyp* hy = h < nh ? &c->bm.hyps[b][h] : nullptr;
            if (tokens) {
                std::fill(tokens + at * cap_tokens, tokens + (at + 1) * cap_tokens, (int64_t)0);
                if (hy) std::copy(hy->tokens.begin(), hy->tokens.end(), tokens + at * cap_tokens);
            }
            if (n_tokens) n_tokens[at] = hy ? hy->tokens.size() : 0;
            if (sum_logprob) sum_logprob[at] = hy ? hy->sum : 0.0f;
            if (rank_score) rank_score[at] = hy ? hy->rank : 0.0f;
            if (finished) finished[at] = hy && hy->finished ? 1 : 0;
        }
    }
    return WH_OK;
}

int wh_get_beam_trace(const wh_ctx* c, size_t k, int32_t* parents, int32_t* tokens, float* scores, int32_t* pool_size, size_t cap_steps, size_t* n_steps) {
    if (!c) return WH_ERR_ARG;
    if (!c->bm.have || c->bm.traces.empty()) return WH_ERR_STATE;
    if (k >= c->bm.traces.size()) return WH_ERR_ARG;
    const wh_ctx::BeamTrace& t = c->bm.traces[k];
    if (n_steps) *n_steps = (size_t)t.n_steps;
    if ((parents || tokens || scores || pool_size) && cap_steps < (size_t)t.n_steps) return WH_ERR_ARG;
    if (parents) std::copy(t.parents.begin(), t.parents.end(), parents);
    if (tokens) std::copy(t.tokens.begin(), t.tokens.end(), tokens);
    if (scores) std::copy(t.scores.begin(), t.scores.end(), scores);
    if (pool_size) std::copy(t.pool.begin(), t.pool.end(), pool_size);
    return WH_OK;
}

int wh_get_token_frames(const wh_ctx* c, int32_t* frames, size_t cap_tokens, int32_t* n_frames, size_t cap_clips, size_t* n_clips_out) {
    if (!c) return WH_ERR_ARG;
    if (!c->al.have) return WH_ERR_STATE;
    const size_t n = c->al.rows.size();
    if (n_clips_out) *n_clips_out = n;
    if ((frames || n_frames) && cap_clips < n) return WH_ERR_ARG;
    if (frames) {
        for (size_t b = 0; b < n; b++)
            if (c->al.rows[b].size() > cap_tokens) return WH_ERR_ARG;
        for (size_t b = 0; b < n; b++) {
            std::fill(frames + b * cap_tokens, frames + (b + 1) * cap_tokens, 0);
            std::copy(c->al.rows[b].begin(), c->al.rows[b].end(), frames + b * cap_tokens);
        }
    }
    if (n_frames) std::copy(c->al.nframes.begin(), c->al.nframes.end(), n_frames);
    return WH_OK;
}

int wh_get_alignment_debug(const wh_ctx* c, size_t k, float* probs, float* matrix, size_t cap_floats, int32_t* shape3) {
    if (!c) return WH_ERR_ARG;
    if (!(c->al.have || c->al.have_dbg) || c->al.dbg.empty()) return WH_ERR_STATE;
    if (k >= c->al.dbg.size()) return WH_ERR_ARG;
    const wh_ctx::AlignDebug& d = c->al.dbg[k];
    if (shape3) { shape3[0] = d.n_heads; shape3[1] = d.n_gen; shape3[2] = d.sb; }
    if (probs) {
        if (cap_floats < d.probs.size()) return WH_ERR_ARG;
        std::copy(d.probs.begin(), d.probs.end(), probs);
    }
    if (matrix) {
        if (cap_floats < d.matrix.size()) return WH_ERR_ARG;
        std::copy(d.matrix.begin(), d.matrix.end(), matrix);
    }
    return WH_OK;
}

int wh_get_languages(const wh_ctx* c, int64_t* lang_out, float* probs, size_t cap_clips, size_t* n_clips_out) {
    if (!c) return WH_ERR_ARG;
    if (!c->lang.have) return WH_ERR_STATE;
    const size_t n = c->lang.rows.size();
    if (n_clips_out) *n_clips_out = n;
    if (!lang_out) return WH_OK;
    if (cap_clips < n) return WH_ERR_ARG;
    std::copy(c->lang.rows.begin(), c->lang.rows.end(), lang_out);
    if (probs) std::copy(c->lang.prob_rows.begin(), c->lang.prob_rows.end(), probs);
    return WH_OK;
}

int wh_get_logprobs(const wh_ctx* c, float* token_logprobs, size_t cap_tokens, float* no_speech_prob, size_t cap_clips, size_t* n_clips_out) {
    if (!c) return WH_ERR_ARG;
    if (!c->lp.have) return WH_ERR_STATE;
    const size_t n = c->lp.rows.size();
    if (n_clips_out) *n_clips_out = n;
    if (no_speech_prob && !c->lp.have_ns) return WH_ERR_STATE;
    if ((token_logprobs || no_speech_prob) && cap_clips < n) return WH_ERR_ARG;
    if (token_logprobs) {
        for (size_t b = 0; b < n; b++)
            if (c->lp.rows[b].size() > cap_tokens) return WH_ERR_ARG;
        for (size_t b = 0; b < n; b++) {
            std::fill(token_logprobs + b * cap_tokens, token_logprobs + (b + 1) * cap_tokens, 0.0f);
            std::copy(c->lp.rows[b].begin(), c->lp.rows[b].end(), token_logprobs + b * cap_tokens);
        }
    }
    if (no_speech_prob) std::copy(c->lp.ns_rows.begin(), c->lp.ns_rows.end(), no_speech_prob);
    return WH_OK;
}

// measurement hook (tools/ingest_bench.py; not in the public header): the conversion of the last wh_transcribe_batch_raw* batch (its raw bytes and
// descriptors are still resident) launched `reps` more times, each between two events on the encoder stream: microseconds per launch in us[reps].
// The rows it writes are the rows it wrote before.
extern "C" int wh_debug_ingest_times(wh_ctx* c, int reps, float* us) {
    if (!c || !us || reps < 1 || c->ing_last_n == 0 || c->h2d_valid) return WH_ERR_ARG;
    CTX_HIP(c, hipSetDevice(c->m->device));
    hipEvent_t a, b;
    CTX_HIP(c, hipEventCreate(&a));
    CTX_HIP(c, hipEventCreate(&b));
    int rc = WH_OK;
    for (int i = 0; i < reps && rc == WH_OK; i++) {
        hipEventRecord(a, c->s_enc);
        wh_launch_ingest(c->s_enc, c->ing_raw[c->ing_last_buf], c->ing_desc, c->ing_last_n, c->ing_last_max_out, c->pcm);
        hipEventRecord(b, c->s_enc);
        float ms = 0;
        if (hipEventSynchronize(b) != hipSuccess || hipEventElapsedTime(&ms, a, b) != hipSuccess) rc = fail(c, WH_ERR_HIP, "wh_debug_ingest_times: %s", hipGetErrorString(hipGetLastError()));
        us[i] = ms * 1e3f;
    }
    hipEventDestroy(a);
    hipEventDestroy(b);
    return rc;
}

// measurement hook (tools/align_bench.py; not in the public header): milliseconds of the three post-pass kernels of the last call, summed over
// its chunks — filled when the context was created under WH_ALIGN_TIMING=1
extern "C" int wh_debug_align_times(const wh_ctx* c, double* ms3) {
    if (!c || !ms3 || !c->al.timing) return WH_ERR_ARG;
    for (int i = 0; i < 3; i++) ms3[i] = c->al.ms[i];
    return WH_OK;
}

// measurement hook (tools/beam_bench.py; not in the public header): milliseconds of k_beam_select and k_beam_reorder of the last call, summed over
// the positions that were launched eagerly (their count in *positions) — filled when the context was created under WH_BEAM_TIMING=1
extern "C" int wh_debug_beam_times(const wh_ctx* c, double* ms2, long* positions) {
    if (!c || !ms2 || !positions || !c->bm.timing) return WH_ERR_ARG;
    ms2[0] = c->bm.ms[0]; ms2[1] = c->bm.ms[1];
    *positions = c->bm.timed;
    return WH_OK;
}

// measurement hook (tools/sample_bench.py; not in the public header): milliseconds of k_sample_select of the last call, summed over the positions
// that were launched eagerly (their count in *positions) — filled when the context was created under WH_SAMPLE_TIMING=1
extern "C" int wh_debug_sample_times(const wh_ctx* c, double* ms, long* positions) {
    if (!c || !ms || !positions || !c->sm.timing) return WH_ERR_ARG;
    *ms = c->sm.ms;
    *positions = c->sm.timed;
    return WH_OK;
}

}  // extern "C"
