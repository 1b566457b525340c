// wh_api.cpp — the C ABI of include/whisper_hip.h: context lifecycle and the orchestration of
// log-mel → encoder → cross-KV → batched greedy decode on one HIP stream.
//
// Mirrors, per entry point: whisper_log_mel_80 (reference src/main.rs:407-509), run_encoder
// (:698-707), greedy_decode_with_past (:753-829) and the per-window body of
// transcribe_longform_chunked (:870-915, 946-967).
#include <hip/hip_runtime.h>
#include <math.h>
#include <cmath>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>

#include "wh_common.h"
#include "wh_ingest_desc.h"
#include "wh_internal.h"

const std::string& wh_global_error();

namespace {

constexpr int RAW_LD = 3008;   // raw log-mel row stride (frames), multiple of 16
constexpr int TOK_ROWS = 3002; // conv1 operand rows per clip: zero row, 3000 frames, zero row
constexpr int H1_ROWS = 3001;  // conv2 operand rows per clip: zero row, 3000 positions

double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int fail(wh_ctx* c, int code, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    wh_set_error("%s", buf);
    return code;
}

#define CTX_HIP(c, expr)                                                                          \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess)                                                                     \
            return fail(c, WH_ERR_HIP, "HIP error %d (%s) at %s:%d: %s", (int)_e, hipGetErrorString(_e), __FILE__, \
                        __LINE__, #expr);                                                         \
    } while (0)

// a kernel launcher that reports a launch it cannot run (GEMM geometry / mode checks): surface it as this call's error
#define CTX_LAUNCH(c, expr)                                                                       \
    do {                                                                                          \
        const int _rc = (expr);                                                                   \
        if (_rc != WH_OK) return fail(c, _rc, "%s", wh_global_error().c_str());                   \
    } while (0)

// ---- profiling scope: brackets the launches of one kernel group with events -------------------
struct Prof {
    wh_ctx* c;
    int g;
    size_t slot = 0;
    bool on;
    Prof(wh_ctx* ctx, int group) : c(ctx), g(group), on(ctx->prof && !ctx->capturing && ((ctx->prof_mask >> group) & 1)) {
        if (!on) return;
        c->prof_launches[g]++;  // launches that are bracketed by events
        auto& v = c->prof_events[g];
        if (c->prof_used[g] == v.size()) {
            hipEvent_t a, b;
            hipEventCreate(&a);
            hipEventCreate(&b);
            v.push_back({a, b});
        }
        slot = c->prof_used[g]++;
        hipEventRecord(v[slot].first, c->cur);
    }
    ~Prof() {
        if (on) hipEventRecord(c->prof_events[g][slot].second, c->cur);
    }
};

void prof_reset(wh_ctx* c) {
    for (int g = 0; g < WH_KG_COUNT; g++) { c->prof_used[g] = 0; c->prof_ms[g] = 0; c->prof_launches[g] = 0; }
}
void prof_collect(wh_ctx* c) {
    if (!c->prof) return;
    for (int g = 0; g < WH_KG_COUNT; g++) {
        double ms = 0;
        for (size_t i = 0; i < c->prof_used[g]; i++) {
            float t = 0;
            // (events of a prefetched encoder pass may still be pending on the encoder stream: hipErrorNotReady — not counted)
            if (hipEventElapsedTime(&t, c->prof_events[g][i].first, c->prof_events[g][i].second) == hipSuccess) ms += t;
        }
        c->prof_ms[g] = ms;
    }
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    }
};

// ---- encoder for nb clips whose conv1 operand already sits in c->melT ---------------------------
// An encoder pass (log-mel included) is about to overwrite the encoder-side workspace: it must not start before the
// cross-K/V projection of the previous batch has read the encoder states.  No-op when both phases share one stream.
int enc_begin(wh_ctx* c) {
    c->cur = c->s_enc;
    if (c->kv_done_armed && c->s_enc != c->stream) CTX_HIP(c, hipStreamWaitEvent(c->s_enc, c->ev_kv_done, 0));
    return WH_OK;
}

int run_encoder(wh_ctx* c, int nb, bool want_f32) {
    wh_model* m = c->m;
    const wh_dims& D = m->dims;
    hipStream_t s = c->s_enc;
    c->cur = s;
    const int prec = m->prec;
    const long d = D.d_model, S = D.n_audio_ctx, F = D.ffn, C = D.n_mels;
    const size_t esz = m->esz;
    {   // conv1 (k3,p1) + GELU: GEMM over overlapping rows of the token-major mel
        Prof p(c, WH_KG_ENC_GEMM);
        GemmArgs g;
        g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
        g.A = c->melT; g.lda = C; g.a_bs = (long)TOK_ROWS * C; g.m_per = WH_N_FRAMES;
        g.W = m->conv1_w; g.ldw = m->conv1_k;
        g.C = (char*)c->h1 + d * esz; g.ldc = d; g.c_bs = (long)H1_ROWS * d;
        g.bias = m->conv1_b; g.bias_mode = 1; g.act = 1;
        g.f32_operands = true;   // (WH_PREC_F16X3: the only GEMM whose operands stay f32 rows, see GemmArgs)
        g.M = nb * WH_N_FRAMES; g.N = (int)d; g.K = m->conv1_k;
        CTX_LAUNCH(c, wh_launch_gemm(s, prec, false, g));
    }
    const long rows = (long)nb * S;
    // LayerNorm fold (bf16, c->enc_fold): every GEMM that produces the residual stream also writes it as bf16 plus per-row
    // partial sums; k_ln_stats turns those into {mean, rstd}; the GEMMs that consume LN(x) read the raw bf16 rows with
    // gamma folded into their weights and apply rstd (acc - mean s) + c in the epilogue.  No LayerNorm kernel, no normalised
    // copy: 3.1 GB less read and one launch less per LayerNorm at 1024 clips.
    const bool fold = c->enc_fold;
    const int n_grp = (int)(d / 64);
    // `first`: conv2, the first producer of a pass — its rows are shifted by what is known before they exist, the row means of the
    // positional table it adds (enc_shift0); later producers by the row's true mean at the previous LayerNorm (enc_shift)
    auto producer = [&](GemmArgs& g, bool first = false) {
        if (!fold) return;
        g.xb_out = c->xb; g.stats_out = c->enc_part; g.stats_rows = rows;
        g.row_shift = first ? c->enc_shift0 : c->enc_shift;
    };
    auto finish_stats = [&](bool first = false) {
        if (fold) wh_launch_ln_stats(s, c->enc_part, n_grp, rows, (int)d, c->enc_stat, c->enc_shift, first ? c->enc_shift0 : c->enc_shift);
    };
    {   // conv2 (k3,s2,p1) + GELU + sinusoid positions → f32 residual stream
        Prof p(c, WH_KG_ENC_GEMM);
        GemmArgs g;
        g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
        g.A = c->h1; g.lda = 2 * d; g.a_bs = (long)H1_ROWS * d; g.m_per = (int)S;
        g.W = m->conv2_w; g.ldw = 3 * d;
        g.C = c->x; g.ldc = d; g.c_bs = S * d;
        g.bias = m->conv2_b; g.bias_mode = 1; g.act = 1;
        g.R = m->enc_pos; g.ldr = d; g.r_bs = 0;
        g.M = nb * (int)S; g.N = (int)d; g.K = (int)(3 * d);
        producer(g, true);
        CTX_LAUNCH(c, wh_launch_gemm(s, prec, true, g));
        finish_stats(true);
    }
    for (int l = 0; l < D.enc_layers; l++) {
        const EncLayerDev& L = m->enc[l];
        // WH_PREC_FP8 with MX activations: LayerNorm writes e4m3 codes + block exponents and the three GEMMs it feeds run
        // on the fp8 matrix cores (e4m3 weights x MX activations); otherwise bf16 operands (fp8 weights as code values)
        const bool mx = c->mx_ok;
        if (!fold) {
            Prof p(c, WH_KG_ENC_GEMM);
            if (mx) CTX_LAUNCH(c, wh_launch_layernorm_mx(s, c->x, L.ln1_w, L.ln1_b, c->xn8, c->xn8_sc, rows, (int)d));
            else wh_launch_layernorm(s, prec, c->x, L.ln1_w, L.ln1_b, c->xn, rows, (int)d);
        }
        {   // Q|K projection (q pre-scaled, k has no bias)
            Prof p(c, WH_KG_ENC_GEMM);
            GemmArgs g;
            g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
            g.A = c->xn; g.lda = d; g.W = L.qk_w; g.ldw = d; g.C = c->qk; g.ldc = 2 * d;
            g.bias = L.qk_b; g.bias_mode = 1; g.wscale = L.qk_sc; g.M = (int)rows; g.N = (int)(2 * d); g.K = (int)d;
            if (fold) { g.A = c->xb; g.W = L.qk_wf; g.bias = L.qk_c; g.ln_mode = 1; g.ln_stat = c->enc_stat; g.ln_s = L.qk_s; }
            if (mx) { g.A = c->xn8; g.a_sc = c->xn8_sc; g.W = L.qk_w8; CTX_LAUNCH(c, wh_launch_gemm8_mx(s, 0, g)); }
            else CTX_LAUNCH(c, wh_launch_gemm(s, prec, false, g));
        }
        {   // V^T[e][key] = W_v x^T + b_v: per-clip product with the weight as the row operand
            Prof p(c, WH_KG_ENC_GEMM);
            GemmArgs g;
            g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
            g.A = L.v_w; g.lda = d; g.a_zs = 0;
            g.W = c->xn; g.ldw = d; g.w_zs = S * d;
            g.C = c->vT; g.ldc = c->ldv; g.c_zs = d * c->ldv;
            g.bias = L.v_b; g.bias_mode = 2; g.wscale = L.v_sc; g.M = (int)d; g.N = (int)S; g.K = (int)d; g.batch = nb;
            if (fold) {   // the LayerNorm statistics belong to the COLUMNS here (keys), s and c to the rows (features)
                g.A = L.v_wf; g.W = c->xb; g.bias = L.v_c; g.ln_mode = 2; g.ln_stat = c->enc_stat; g.ln_stat_zs = 2 * S; g.ln_s = L.v_s;
            }
            if (mx && d >= 256) { g.A = L.v_w8; g.W = c->xn8; g.w_sc8 = c->xn8_sc; g.w_sc_zs = S * 4 * wh_mx_nkp((int)d); CTX_LAUNCH(c, wh_launch_gemm8_mx(s, 0, g)); }
            else if (mx) return fail(c, WH_ERR_UNSUPPORTED, "MX activations need d_model >= 256");
            else CTX_LAUNCH(c, wh_launch_gemm(s, prec, false, g));
        }
        {
            Prof p(c, WH_KG_ENC_ATTN);
            wh_launch_enc_attn(s, prec, c->qk, c->vT, c->att, nb, (int)S, (int)d, D.n_heads, c->ldv);
        }
        {   // out-proj + bias + residual (in place on the f32 stream)
            Prof p(c, WH_KG_ENC_GEMM);
            GemmArgs g;
            g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
            g.A = c->att; g.lda = d; g.W = L.o_w; g.ldw = d; g.C = c->x; g.ldc = d;
            g.bias = L.o_b; g.bias_mode = 1; g.wscale = L.o_sc; g.R = c->x; g.ldr = d; g.M = (int)rows; g.N = (int)d; g.K = (int)d;
            producer(g);
            CTX_LAUNCH(c, wh_launch_gemm(s, prec, true, g));
            finish_stats();
        }
        if (!fold) {
            Prof p(c, WH_KG_ENC_GEMM);
            if (mx) CTX_LAUNCH(c, wh_launch_layernorm_mx(s, c->x, L.ln2_w, L.ln2_b, c->xn8, c->xn8_sc, rows, (int)d));
            else wh_launch_layernorm(s, prec, c->x, L.ln2_w, L.ln2_b, c->xn, rows, (int)d);
        }
        if (c->enc_mlp) {   // the feed-forward block in one launch (wh_mlp.hip; decided with the context — the two-launch form's hidden-activation buffer does not exist then)
            Prof p(c, WH_KG_ENC_GEMM);
            MlpArgs ma;
            ma.X = c->xb; ma.ldx = d; ma.ln_stat = c->enc_stat; ma.W1 = L.fc1_wf; ma.s1 = L.fc1_s; ma.c1 = L.fc1_c; ma.W2 = L.fc2_w; ma.b2 = L.fc2_b;
            ma.Xres = c->x; ma.ldr = d; ma.xb_out = c->xb; ma.stats_out = c->enc_part; ma.stats_rows = rows; ma.row_shift = c->enc_shift;
            ma.M = (int)rows; ma.d = (int)d; ma.F = (int)F;
            CTX_LAUNCH(c, wh_launch_enc_mlp(s, ma));
            finish_stats();
            continue;
        }
        {   // fc1 + GELU (MX: the output leaves as e4m3 codes + block exponents, fc2's operand)
            Prof p(c, WH_KG_ENC_GEMM);
            GemmArgs g;
            g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
            g.A = c->xn; g.lda = d; g.W = L.fc1_w; g.ldw = d; g.C = c->hbuf; g.ldc = F;
            g.bias = L.fc1_b; g.bias_mode = 1; g.wscale = L.fc1_sc; g.act = 1; g.M = (int)rows; g.N = (int)F; g.K = (int)d;
            if (fold) { g.A = c->xb; g.W = L.fc1_wf; g.bias = L.fc1_c; g.ln_mode = 1; g.ln_stat = c->enc_stat; g.ln_s = L.fc1_s; }
            if (mx) { g.A = c->xn8; g.a_sc = c->xn8_sc; g.W = L.fc1_w8; g.C = c->h8; g.c_sc = c->h8_sc; CTX_LAUNCH(c, wh_launch_gemm8_mx(s, 2, g)); }
            else CTX_LAUNCH(c, wh_launch_gemm(s, prec, false, g));
        }
        {
            Prof p(c, WH_KG_ENC_GEMM);
            GemmArgs g;
            g.small_ctx = c->max_batch <= WH_SMALL_CTX_CLIPS;
            g.A = c->hbuf; g.lda = F; g.W = L.fc2_w; g.ldw = F; g.C = c->x; g.ldc = d;
            g.bias = L.fc2_b; g.bias_mode = 1; g.wscale = L.fc2_sc; g.R = c->x; g.ldr = d; g.M = (int)rows; g.N = (int)d; g.K = (int)F;
            if (mx) { g.A = c->h8; g.a_sc = c->h8_sc; g.W = L.fc2_w8; CTX_LAUNCH(c, wh_launch_gemm8_mx(s, 1, g)); }
            else { producer(g); CTX_LAUNCH(c, wh_launch_gemm(s, prec, true, g)); finish_stats(); }
        }
    }
    {
        Prof p(c, WH_KG_ENC_GEMM);
        // the cross K/V projection's operand: MX form when that GEMM runs on the fp8 matrix cores, else the compute dtype
        // (fold: the final LayerNorm lives in the cross K/V projection's weights; its statistics are in c->enc_stat already)
        if (c->mx_ok && !c->cross_es) CTX_LAUNCH(c, wh_launch_layernorm_mx(s, c->x, m->enc_ln_w, m->enc_ln_b, c->xn8, c->xn8_sc, rows, (int)d));   // (encoder-state form: the final LayerNorm runs at decode step 0, into e4m3 rows)
        else if (!fold) wh_launch_layernorm(s, prec, c->x, m->enc_ln_w, m->enc_ln_b, c->enc_out, rows, (int)d);
        if (want_f32) {
            if (prec == WH_PREC_F32) hipMemcpyAsync(c->enc_out_f32, c->enc_out, rows * d * 4, hipMemcpyDeviceToDevice, s);
            else wh_launch_layernorm(s, WH_PREC_F32, c->x, m->enc_ln_w, m->enc_ln_b, c->enc_out_f32, rows, (int)d);
        }
    }
    CTX_HIP(c, hipEventRecord(c->ev_enc_done, s));
    c->have_enc = true;
    c->enc_batch = nb;
    return WH_OK;
}

void drop_step_graph(wh_ctx* c) {
    if (c->step_exec && c->stream) hipStreamSynchronize(c->stream);  // an error path may have left replays in flight
    if (c->step_exec) hipGraphExecDestroy(c->step_exec);
    if (c->step_graph) hipGraphDestroy(c->step_graph);
    c->step_exec = nullptr;
    c->step_graph = nullptr;
    c->step_key = wh_ctx::StepKey();
}

void pack_mask(const int64_t* a, size_t na, const int64_t* b, size_t nb, int vocab, std::vector<unsigned>& out) {
    out.assign((size_t)vocab / 32 + 1, 0u);
    for (size_t i = 0; i < na; i++)
        if (a[i] >= 0 && a[i] < vocab) out[a[i] >> 5] |= 1u << (a[i] & 31);
    for (size_t i = 0; i < nb; i++)
        if (b[i] >= 0 && b[i] < vocab) out[b[i] >> 5] |= 1u << (b[i] & 31);
}

// Per-clip prefixes: the prefix lengths of the nb rows of a device batch and what a decode entry refuses because of them,
// checked by every entry before it launches anything and again by run_decode.  first_row = index of the batch's first window in a long-form
// call (-1: the rows are the call's clips).  len_out (optional) [nb]; the return value of prefix_max is the longest one.
const int64_t* prefix_of(const wh_ctx* c, long first_row, int b, int* len) {
    size_t clip = (size_t)b;
    if (first_row >= 0) {   // long-form: one prefix for the file, for window 0 or for every window
        if (c->pfx_scope == WH_PREFIX_FIRST_WINDOW && first_row + b != 0) { *len = 0; return c->pfx_ids.data(); }
        clip = 0;
    }
    *len = (int)(c->pfx_offsets[clip + 1] - c->pfx_offsets[clip]);
    return c->pfx_ids.data() + c->pfx_offsets[clip];
}
int prefix_check(wh_ctx* c, const wh_decode_params* p, int nb, bool longform) {
    if (!c->pfx_on) return WH_OK;
    const size_t n_clips = c->pfx_offsets.size() - 1;
    if (longform ? n_clips != 1 : n_clips != (size_t)nb)
        return fail(c, WH_ERR_ARG, "decode: wh_ctx_set_prefixes was given %zu clips, this call has %d", n_clips, longform ? 1 : nb);
    int nmax = 0;
    for (size_t b = 0; b < n_clips; b++) nmax = std::max(nmax, (int)(c->pfx_offsets[b + 1] - c->pfx_offsets[b]));
    if (nmax == 0) return WH_OK;
    if ((size_t)nmax + p->n_prompt + p->max_new_tokens > (size_t)c->m->dims.n_text_ctx)
        return fail(c, WH_ERR_ARG, "decode: longest prefix (%d) + prompt (%zu) + max_new_tokens (%zu) exceeds %d positions", nmax, p->n_prompt, p->max_new_tokens,
                    c->m->dims.n_text_ctx);
    if (c->lang_on)
        return fail(c, WH_ERR_UNSUPPORTED, "decode: language detection with a non-empty prefix is not supported (the logits at <|startoftranscript|> depend on the "
                                           "prefix): detect the language with an un-prefixed call first, then decode with that language in the prompt");
    return WH_OK;
}

// Word-level timestamps: what a decode entry refuses because of them, checked by every entry before it launches anything and
// again by run_decode.
int align_check(wh_ctx* c, int nb) {
    if (!c->al_on) return WH_OK;
    if (c->m->prec == WH_PREC_FP8 || c->m->prec == WH_PREC_F16X3)
        return fail(c, WH_ERR_UNSUPPORTED, "decode: word-level timestamps are not supported in the %s mode (no score kernel for its keys and queries)",
                    c->m->prec == WH_PREC_FP8 ? "fp8" : "f16x3");
    if (c->cross_es && !wh_align_scores_supported(WH_ALIGN_ES_BF16, c->m->dims.d_model))
        return fail(c, WH_ERR_UNSUPPORTED, "decode: word-level timestamps have no score kernel for encoder states %d wide", c->m->dims.d_model);
    for (int r : c->al_debug)
        if (r >= nb) return fail(c, WH_ERR_ARG, "decode: alignment debug row %d outside the batch (%d clips)", r, nb);
    return WH_OK;
}

// Beam search: what a decode entry refuses because of it, checked by every entry before it launches anything and again by
// run_decode.  nb = the call's clips (a long-form call: one device batch never holds more than max_batch / K windows).
int beam_check(wh_ctx* c, const wh_decode_params* p, int nb) {
    if (!c->bm_on) return WH_OK;
    if ((long)nb * c->bm_k > c->max_batch)
        return fail(c, WH_ERR_ARG, "decode: %d clips x beam_size %d exceed max_batch (%d rows)", nb, c->bm_k, c->max_batch);
    if (c->m->prec == WH_PREC_FP8 || c->m->prec == WH_PREC_F16X3)
        return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search is not supported in the %s mode", c->m->prec == WH_PREC_FP8 ? "fp8" : "f16x3");
    if (p->n_forced) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with forced tokens is not supported");
    if (c->rep_on) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with repetition controls is not supported");
    if (c->al_on) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with word-level timestamps is not supported");
    if (c->pfx_on && c->pfx_offsets.back() != 0) return fail(c, WH_ERR_UNSUPPORTED, "decode: beam search with a non-empty prefix is not supported");
    return WH_OK;
}

// Temperature sampling: what a decode entry refuses because of it, checked by every entry before it launches anything and again
// by run_decode.  nb = the call's clips (a long-form call: the setter's one row stands for every window).
int sample_check(wh_ctx* c, int nb, bool longform) {
    if (!c->sm_on) return WH_OK;
    if (c->sm_temp.size() != (size_t)(longform ? 1 : nb))
        return fail(c, WH_ERR_ARG, "decode: wh_ctx_set_sampling was given %zu rows, this call has %d", c->sm_temp.size(), longform ? 1 : nb);
    if (c->bm_on) return fail(c, WH_ERR_UNSUPPORTED, "decode: sampling with beam search is not supported (the search runs at temperature 0 only)");
    if (c->rep_on) return fail(c, WH_ERR_UNSUPPORTED, "decode: sampling with repetition controls is not supported");
    if (c->al_on) return fail(c, WH_ERR_UNSUPPORTED, "decode: sampling with word-level timestamps is not supported");
    return WH_OK;
}
// every temperature 0 and every row active: the plain kernels are launched
bool sample_trivial(const wh_ctx* c) {
    for (size_t i = 0; i < c->sm_temp.size(); i++)
        if (c->sm_temp[i] != 0.0f || !c->sm_active[i]) return false;
    return true;
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

// all validation; no HIP call
int plan_decode(wh_ctx* c, int ncl, const wh_decode_params* p, bool want_logits, size_t logits_rows, const int32_t* sel, size_t n_sel, DecodePlan& pl) {
    const wh_dims& D = c->m->dims;
    if (int rc = beam_check(c, p, ncl)) return rc;
    if (int rc = sample_check(c, ncl, c->pfx_win_base >= 0)) return rc;
    const int K = pl.K = c->bm_on ? c->bm_k : 1, nb = ncl * K;   // the rows of the device batch
    pl.ncl = ncl;
    const int P = pl.P = (int)p->n_prompt, NEW = pl.NEW = (int)p->max_new_tokens;
    if (P <= 0 || NEW <= 0 || !p->prompt) return fail(c, WH_ERR_ARG, "decode: empty prompt or max_new_tokens == 0");
    if (P + NEW > D.n_text_ctx) return fail(c, WH_ERR_ARG, "decode: prompt (%d) + max_new_tokens (%d) exceeds %d positions", P, NEW, D.n_text_ctx);
    if (p->n_forced > (size_t)NEW) return fail(c, WH_ERR_ARG, "decode: more forced tokens than max_new_tokens");
    pl.lang_fix = c->lang_on && c->lang_fixed >= 0;
    pl.lang_det = c->lang_on && !pl.lang_fix;
    const int lang_slot = pl.lang_slot = c->lang_on ? c->lang_sot_index + 1 : -1;
    if (c->lang_on && lang_slot >= P)
        return fail(c, WH_ERR_ARG, "decode: language detection's sot_index %d + 1 is not below n_prompt (%d)", c->lang_sot_index, P);
    for (int i = 0; i < P; i++)
        if (i != lang_slot && (p->prompt[i] < 0 || p->prompt[i] >= D.vocab)) return fail(c, WH_ERR_ARG, "decode: prompt id %lld outside the vocabulary", (long long)p->prompt[i]);
    for (size_t i = 0; i < p->n_forced; i++)
        if (p->forced[i] < 0 || p->forced[i] >= D.vocab) return fail(c, WH_ERR_ARG, "decode: forced id outside the vocabulary");
    if (c->ts_on) {   // timestamp rules: <|0.00|> must lie above EOT (so EOT and the specials are text ids) and inside the vocabulary
        if (c->ts_begin <= p->eot || c->ts_begin >= D.vocab)
            return fail(c, WH_ERR_ARG, "decode: timestamp_begin %lld outside (eot %lld, vocab %d)", (long long)c->ts_begin, (long long)p->eot, D.vocab);
        for (int i = 0; i < P; i++)
            if (i != lang_slot && c->ts_no_ts >= 0 && p->prompt[i] == c->ts_no_ts) return fail(c, WH_ERR_ARG, "decode: the prompt holds <|notimestamps|> while timestamp rules are on");
    }
    pl.lp_probe = c->lp_on && c->lp_no_speech >= 0;
    if (pl.lp_probe && c->lp_sot_index >= P - 1)   // the probe reads a prompt position that emits nothing
        return fail(c, WH_ERR_ARG, "decode: the no-speech probe's sot_index %d is not below n_prompt - 1 (%d)", c->lp_sot_index, P - 1);
    if (int rc = prefix_check(c, p, ncl, c->pfx_win_base >= 0)) return rc;
    if (int rc = align_check(c, ncl)) return rc;
    pl.plen.assign(nb, 0);
    pl.pids.assign(nb, nullptr);
    if (c->pfx_on)
        for (int b = 0; b < nb; b++) {
            pl.pids[b] = prefix_of(c, c->pfx_win_base, b / K, &pl.plen[b]);
            pl.Nmax = std::max(pl.Nmax, pl.plen[b]);
        }
    if (pl.lang_det) pl.lang_pos = pl.Nmax + c->lang_sot_index;
    if (pl.lp_probe) pl.probe_pos = pl.Nmax + c->lp_sot_index;
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
    if (c->ts_on) { key.ts_begin = (int)c->ts_begin; key.ts_max_init = c->ts_max_init; }
    if (c->lp_on) key.lp_sum = c->lp_part_sum;
    if (c->rep_on) { key.rep = true; key.rep_p = c->rep_p; key.rep_n = c->rep_n; }
    if (c->al_on) { key.al_cap = NEW; key.al_gen = c->al_gen; }   // (prepare_alignment completes it with the side buffer's address)
    if (c->bm_on) { key.beam_k = c->bm_k; key.beam_c = c->bm_c; key.beam_buf = c->bm_buf; }
    if (c->sm_on && !sample_trivial(c)) key.sample_buf = c->sm_buf;
    return WH_OK;
}

// feed, out_tokens, n_out, done, pos, ticket, repetition bits, forced ids, the two suppress masks, the prefix offsets
int upload_token_state(wh_ctx* c, const wh_decode_params* p, const DecodePlan& pl) {
    hipStream_t s = c->stream;
    const int nb = pl.key.nb, ld = c->tok_ld, Nmax = pl.Nmax, vocab = c->m->dims.vocab;
    std::vector<int> feed((size_t)nb * ld, 0);
    for (int b = 0; b < nb; b++) {
        for (int i = 0; i < pl.plen[b]; i++) feed[(size_t)b * ld + Nmax - pl.plen[b] + i] = (int)pl.pids[b][i];   // (columns below Nmax - n_b: filler id 0 of an idle row)
        for (int i = 0; i < pl.P; i++) feed[(size_t)b * ld + Nmax + i] = i == pl.lang_slot ? (pl.lang_fix ? (int)c->lang_fixed : 0) : (int)p->prompt[i];
    }
    if (pl.key.pfx) {
        std::vector<int> off(nb);
        for (int b = 0; b < nb; b++) off[b] = Nmax - pl.plen[b];
        CTX_HIP(c, hipMemcpyAsync(c->pfx_off, off.data(), nb * 4, hipMemcpyHostToDevice, s));
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
        const bool lf = c->pfx_win_base >= 0;
        sm_done.resize(nb); sm_t.resize(nb); sm_id.resize(nb);
        for (int b = 0; b < nb; b++) {
            sm_done[b] = c->sm_active[lf ? 0 : b] ? 0 : 1;
            sm_t[b] = c->sm_temp[lf ? 0 : b];
            sm_id[b] = lf ? (unsigned long long)(c->pfx_win_base + b) : (unsigned long long)c->sm_ids[b];
        }
        const unsigned long long seed = c->sm_seed;
        CTX_HIP(c, hipMemcpyAsync(c->done, sm_done.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->sm_d_temp, sm_t.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->sm_d_ids, sm_id.data(), nb * 8, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->sm_d_seed, &seed, 8, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipStreamSynchronize(s));   // (`seed` goes out of scope)
    }
    CTX_HIP(c, hipMemsetAsync(c->pos, 0, 4, s));
    CTX_HIP(c, hipMemsetAsync(c->step_ticket, 0, 4, s));
    if (c->rep_on) CTX_HIP(c, hipMemsetAsync(c->rep_bits, 0, (size_t)nb * c->rep_words * 4, s));   // no history yet: nothing is touched
    if (pl.key.beam_k) {   // no position has run (the first one starts the scores and the pool itself)
        CTX_HIP(c, hipMemsetAsync(c->bm_n_steps, 0, (size_t)pl.ncl * 4, s));
        CTX_HIP(c, hipMemsetAsync(c->bm_pool_n, 0, (size_t)pl.ncl * 4, s));
    }
    std::vector<int> forced(p->n_forced);
    for (size_t i = 0; i < p->n_forced; i++) forced[i] = (int)p->forced[i];
    if (!forced.empty()) CTX_HIP(c, hipMemcpyAsync(c->forced, forced.data(), forced.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<unsigned> mfirst, mbase;
    pack_mask(p->suppress, p->n_suppress, p->begin_suppress, p->n_begin_suppress, vocab, mfirst);  // :765-768
    pack_mask(p->suppress, p->n_suppress, nullptr, 0, vocab, mbase);
    if (c->ts_on && c->ts_no_ts >= 0 && c->ts_no_ts < vocab) {   // timestamp rule 1: <|notimestamps|> at every step
        mfirst[c->ts_no_ts >> 5] |= 1u << (c->ts_no_ts & 31);
        mbase[c->ts_no_ts >> 5] |= 1u << (c->ts_no_ts & 31);
    }
    CTX_HIP(c, hipMemcpyAsync(c->mask_first, mfirst.data(), mfirst.size() * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->mask_base, mbase.data(), mbase.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<int> sb;
    if (c->al_on) {   // frames of each clip: half its mel frames (the conv stride), at least 8, at most the audio context
        sb.resize(nb);
        for (int b = 0; b < nb; b++) {
            const int nf = (size_t)b < c->enc_nframes.size() ? c->enc_nframes[b] : WH_N_FRAMES;
            sb[b] = std::min(c->m->dims.n_audio_ctx, std::max(8, (nf + 1) / 2));
        }
        CTX_HIP(c, hipMemcpyAsync(c->al_sb, sb.data(), nb * 4, hipMemcpyHostToDevice, s));
    }
    CTX_HIP(c, hipStreamSynchronize(s));  // host vectors above go out of scope
    return WH_OK;
}

// the parity buffer of a call that keeps logits: the row selection goes to the device, the buffer grows on demand; completes the key
int prepare_logits(wh_ctx* c, DecodePlan& pl) {
    if (!pl.want_logits) return WH_OK;
    if (!pl.sel_map.empty()) {
        CTX_HIP(c, hipMemcpy(c->logits_sel, pl.sel_map.data(), pl.key.nb * 4, hipMemcpyHostToDevice));
        pl.key.d_sel = c->logits_sel;
    }
    const size_t need = pl.n_lrows * pl.key.logits_rows * c->m->dims.vocab;
    if (need > c->logits_cap) {
        drop_step_graph(c);  // the captured step holds the old buffer's address
        if (c->logits) CTX_HIP(c, hipFree(c->logits));
        c->logits = nullptr;
        c->logits_cap = 0;
        CTX_HIP(c, hipMalloc((void**)&c->logits, need * 4));
        c->logits_cap = need;
    }
    pl.key.d_logits = c->logits;
    return WH_OK;
}

// Word-level timestamps: the side buffer the captured step copies the alignment heads' queries into, [heads][nb][max_new_tokens][dk] f32 — sized
// by the call, grown on demand; completes the key
int align_dk(const wh_ctx* c) { return c->cross_es ? c->m->dims.d_model : WH_HEAD_DIM; }
int prepare_alignment(wh_ctx* c, DecodePlan& pl) {
    if (!c->al_on) return WH_OK;
    const size_t need = c->al_heads.size() / 2 * (size_t)pl.key.nb * pl.NEW * align_dk(c);
    if (need > c->al_q_cap) {
        drop_step_graph(c);  // the captured step holds the old buffer's address
        if (c->al_q) CTX_HIP(c, hipFree(c->al_q));
        c->al_q = nullptr;
        c->al_q_cap = 0;
        CTX_HIP(c, hipMalloc((void**)&c->al_q, need * 4));
        c->al_q_cap = need;
    }
    pl.key.al_q = c->al_q;
    return WH_OK;
}

// The post-pass of a call with word-level timestamps, on the decode stream after the token loop: scores + softmax, filter, DTW for chunks of
// clips sized so that the workspace (P, M and the DTW steps of a chunk) stays within WH_ALIGN_WS_BYTES; keeps the debug rows' P and M.
constexpr size_t WH_ALIGN_WS_BYTES = (size_t)1 << 30;
int run_alignment(wh_ctx* c, const DecodePlan& pl) {
    if (!c->al_on) return WH_OK;
    hipStream_t s = c->stream;
    const wh_dims& D = c->m->dims;
    const int nb = pl.key.nb, NEW = pl.NEW, nh = (int)(c->al_heads.size() / 2), S = D.n_audio_ctx, Sp = (S + 3) / 4 * 4;
    c->al_dbg.clear();
    CTX_HIP(c, hipMemsetAsync(c->al_frames, 0, (size_t)nb * D.n_text_ctx * 4, s));
    if (NEW == 1) return WH_OK;   // one row per clip: frame 0, nothing to launch
    auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t b_p = (size_t)nh * NEW * Sp * 4, b_m = (size_t)NEW * Sp * 4, b_t = (size_t)(NEW + 1) * (S + 1), per_clip = b_p + b_m + b_t;
    const int chunk = (int)std::min<size_t>((size_t)nb, std::max<size_t>(1, WH_ALIGN_WS_BYTES / per_clip));
    const size_t ws_need = up(chunk * b_p) + up(chunk * b_m) + up(chunk * b_t);
    if (ws_need > c->al_ws_cap) {
        if (c->al_ws) CTX_HIP(c, hipFree(c->al_ws));
        c->al_ws = nullptr;
        c->al_ws_cap = 0;
        CTX_HIP(c, hipMalloc((void**)&c->al_ws, ws_need));
        c->al_ws_cap = ws_need;
    }
    AlignArgs a;
    a.q = c->al_q; a.dk = align_dk(c);
    const long kv_stride = (long)nb * S * D.d_model;
    for (int i = 0; i < nh; i++) {
        const int l = c->al_heads[2 * i], h = c->al_heads[2 * i + 1];
        a.k_base[i] = c->cross_es ? c->es_E : (const void*)((const char*)c->cross_kv + ((long)(2 * l) * kv_stride + (long)h * WH_HEAD_DIM) * c->m->esz);
    }
    a.k_clip_pitch = (long)(c->cross_es ? c->es_rows : S) * D.d_model; a.k_row_pitch = D.d_model;
    a.n_out = c->n_out; a.n_prompt = pl.key.n_prompt; a.cap = NEW; a.sb = c->al_sb;
    a.nb = nb; a.n_heads = nh; a.S = S; a.Sp = Sp;
    a.P = (float*)c->al_ws; a.M = (float*)(c->al_ws + up(chunk * b_p)); a.trace = (unsigned char*)(c->al_ws + up(chunk * b_p) + up(chunk * b_m));
    a.frames = c->al_frames; a.frames_ld = D.n_text_ctx;
    const int form = c->cross_es ? WH_ALIGN_ES_BF16 : c->m->prec == WH_PREC_F32 ? WH_ALIGN_KV_F32 : WH_ALIGN_KV_BF16;
    c->al_dbg.resize(c->al_debug.size());
    const bool tm = c->al_timing && !c->capturing;
    hipEvent_t te[4] = {nullptr, nullptr, nullptr, nullptr};
    if (tm) for (auto& e : te) CTX_HIP(c, hipEventCreate(&e));
    struct TeGuard { hipEvent_t* te; ~TeGuard() { for (int i = 0; i < 4; i++) if (te[i]) hipEventDestroy(te[i]); } } te_guard{te};
    c->al_ms[0] = c->al_ms[1] = c->al_ms[2] = 0;
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
            for (int i = 0; i < 3; i++) { float ms = 0; hipEventElapsedTime(&ms, te[i], te[i + 1]); c->al_ms[i] += ms; }
        }
        for (size_t k = 0; k < c->al_debug.size(); k++) {   // parity harness: the whole slot; read_back cuts it to the row's n_gen and S_b
            const int r = c->al_debug[k];
            if (r < c0 || r >= c0 + nc) continue;
            wh_ctx::AlignDebug& dbg = c->al_dbg[k];
            dbg.probs.resize((size_t)nh * NEW * Sp);
            dbg.matrix.resize((size_t)NEW * Sp);
            CTX_HIP(c, hipMemcpyAsync(dbg.probs.data(), a.P + (size_t)(r - c0) * nh * NEW * Sp, dbg.probs.size() * 4, hipMemcpyDeviceToHost, s));
            CTX_HIP(c, hipMemcpyAsync(dbg.matrix.data(), a.M + (size_t)(r - c0) * NEW * Sp, dbg.matrix.size() * 4, hipMemcpyDeviceToHost, s));
            CTX_HIP(c, hipStreamSynchronize(s));
        }
    }
    return WH_OK;
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
// LayerNorm never runs as a kernel in the decoder: the kernel that produces a residual-stream row also emits its raw copy in the
// compute dtype (c->dxs, slab layout) and per-column-tile partial sums (c->lnpart); the GEMM that consumes LN(x) has γ folded into
// its weights and applies mean / rstd in its epilogue (wh_model.cpp fold_ln).
// What a prompt position does besides the layers.  It embeds its own input token (a generated position's input was embedded by the
// previous position's argmax finish); only the last prompt position emits.
struct PromptStep {
    bool emits = false;
    bool lang = false;    // language detection reads this position's logits; the chosen id goes to column lang_col
    int lang_col = 0;
    bool probe = false;   // the no-speech probe reads this position's logits
};

// The launches of a position see the context (model, fixed workspace addresses, option buffers) and the step's key, nothing else.
struct Step {
    wh_ctx* c;
    const wh_ctx::StepKey& k;
    wh_model* m = c->m;
    const wh_dims& D = m->dims;
    hipStream_t s = c->stream;
    const int prec = m->prec, nb = k.nb, mpad = c->mpad, ln_tiles_d = D.d_model / 16;
    const long d = D.d_model, S = D.n_audio_ctx;
    const bool f8 = prec == WH_PREC_FP8, rules = k.ts_begin >= 0;
    // beam search: the nb rows are the beams of ncl = nb / rpc clips, and the cross-attention of row b reads clip b / rpc (rpc == 1: ncl == nb)
    const int rpc = k.beam_k ? k.beam_k : 1, ncl = nb / rpc;
    // the cross K/V of all layers are re-read at every position: below ~half the 256 MiB Infinity Cache they are served
    // from it; above, their stream only evicts the decode weights and activations — then they are loaded non-temporally
    const bool kv_nt = (c->cross_es ? 1.0 : (double)D.dec_layers * 2.0) * ncl * S * d * (f8 ? 1 : (double)m->esz) > 128.0 * 1024 * 1024;
    const int* d_off = k.pfx ? c->pfx_off : nullptr;

    // the decode GEMMs: tile GEMMs on contexts of a thousand clips and more (a property of the context, never of the call)
    void gemm(bool out_f32, const SkinnyArgs& a) const {
        if (c->dec_tile && wh_dec_tile_applicable(prec, a)) wh_launch_dec_tile(s, prec, out_f32, a);
        else wh_launch_dec_gemm(s, prec, out_f32, a);
    }
    // a GEMM that consumes LN(x) of the residual stream: out [nb][N], row-major or (slab_out) slab layout
    SkinnyArgs ln_consumer(const void* W, const float* bias, const float* wscale, const float* ln_s, long N, void* out, int ln_tiles, bool slab_out = false) const {
        SkinnyArgs a;
        a.X = c->dxs; a.x_mpad = mpad; a.W = W; a.bias = bias; a.wscale = wscale; a.C = out;
        if (slab_out) a.c_mpad = mpad; else a.ldc = N;
        a.M = nb; a.N = (int)N; a.K = (int)d;
        a.ln_part = c->lnpart; a.ln_tiles = ln_tiles; a.ln_s = ln_s; a.shift_io = c->dshift;
        return a;
    }
    // a GEMM that adds to the residual stream: x += X W^T + bias, plus the raw slab copy and the partial sums of the next LayerNorm
    // (next_gamma: that LayerNorm's γ, applied on the activation side in fp8 mode)
    SkinnyArgs residual_producer(const void* W, const float* bias, const float* wscale, const void* X, long K, const float* next_gamma) const {
        SkinnyArgs a;
        a.X = X; a.x_mpad = mpad; a.W = W; a.bias = bias; a.wscale = wscale; a.R = c->dx; a.ldr = d; a.C = c->dx; a.ldc = d;
        a.M = nb; a.N = (int)d; a.K = (int)K; a.xslab_out = c->dxs; a.stats_out = c->lnpart; a.row_shift = c->dshift;
        if (f8) a.xgamma = next_gamma;
        return a;
    }
    // final LN ∘ tied LM head: what the emitting step and the no-speech probe share (they differ in the masks and what they record)
    SkinnyArgs lm_head_common() const {
        SkinnyArgs a;
        a.W = m->lm_w; a.bias = m->lm_c; a.ln_s = m->lm_s; a.ln_part = c->lnpart; a.ln_tiles = ln_tiles_d;
        a.M = nb; a.N = D.vocab; a.K = (int)d;
        a.X = c->dxs; a.x_mpad = mpad;
        a.pos_p = c->pos; a.n_prompt = k.n_prompt;
        a.part_val = c->part_val; a.part_idx = c->part_idx;
        return a;
    }

    // `advance`: nothing follows the layers at this position (a prompt position without a head), so this fc2 advances the position
    void layer(int l, bool advance) const {
        const DecLayerDev& L = m->dec[l];
        const long cache_l = (long)nb * D.n_heads * D.n_text_ctx * WH_HEAD_DIM * m->esz;   // bytes per layer
        const long kv_stride = (long)ncl * S * d;  // elements between consecutive [clips][S][d] planes
        {   // LN1 ∘ Q|K|V projection
            Prof pr(c, WH_KG_DEC_GEMM);
            gemm(false, ln_consumer(L.qkv_w, L.qkv_b, L.qkv_sc, L.qkv_s, 3 * d, c->dqkv, (l == 0) ? 1 : ln_tiles_d));
        }
        {
            Prof pr(c, WH_KG_DEC_OTHER);
            wh_launch_dec_self_attn(s, prec, c->dqkv, (char*)c->self_k + l * cache_l, (char*)c->self_v + l * cache_l, c->datt, c->pos, (int)d, D.n_heads,
                                    D.n_text_ctx, nb, mpad, d_off);
        }
        {   // self-attention out-proj + residual → x, raw slab, LN2 partials
            Prof pr(c, WH_KG_DEC_GEMM);
            gemm(true, residual_producer(L.o_w, L.o_b, L.o_sc, c->datt, d, L.ln2_w));
        }
        if (c->cross_es) {
            // the attention runs on the encoder states (wh_cross_es.hip): W_k moves to the query side, W_v behind the attention
            {   // LN2 ∘ cross-attention query, kept in f32
                Prof pr(c, WH_KG_DEC_GEMM);
                gemm(true, ln_consumer(L.cq_w, L.cq_b, L.cq_sc, L.cq_s, d, c->dq32, ln_tiles_d));
                // expanded queries qe[h] = W_k,h^T q_h: [nb][H][d] f32
                wh_launch_dec_qexpand(s, prec, c->dq32, L.cqx_w, c->dqe, nb, (int)d, D.n_heads);
            }
            if (k.al_q && c->al_layer[l].n) {   // word-level timestamps: the listed heads' expanded queries of this position
                Prof pr(c, WH_KG_DEC_OTHER);
                wh_launch_align_copy(s, false, c->dqe, (long)D.n_heads * d, d, (int)d, c->al_layer[l], c->pos, k.n_prompt - 1, k.al_cap, nb, k.al_q);
            }
            {
                Prof pr(c, WH_KG_DEC_CROSS_ATTN);
                wh_launch_dec_cross_attn_es(s, prec, c->dqe, c->es_E, c->dctx, (int)S, c->es_rows, nb, mpad, kv_nt, c->dec_cus, rpc);
            }
            {   // per head: W_v,h ctx_h + b_v,h → the attention output the out-projection below expects (slab layout)
                Prof pr(c, WH_KG_DEC_GEMM);
                SkinnyArgs a;
                a.X = c->dctx; a.x_mpad = mpad; a.W = L.cv_w; a.bias = L.cv_b; a.C = c->datt; a.c_mpad = mpad;
                a.M = nb; a.N = WH_HEAD_DIM; a.K = (int)d;
                a.zn = D.n_heads; a.x_zs = (long)(d / 32) * mpad * 32; a.w_zs = (long)WH_HEAD_DIM * d; a.c_zs = (long)(WH_HEAD_DIM / 32) * mpad * 32;
                a.bias_zs = WH_HEAD_DIM;
                if (f8) wh_launch_dec_gemm(s, WH_PREC_BF16, false, a);   // (fp8 mode: cv_w is the quantised model's W_v, code x row scale, as bf16 — wh_model.cpp)
                else gemm(false, a);
            }
        } else {
            {   // LN2 ∘ cross-attention query
                Prof pr(c, WH_KG_DEC_GEMM);
                gemm(false, ln_consumer(L.cq_w, L.cq_b, L.cq_sc, L.cq_s, d, c->dq, ln_tiles_d));
            }
            if (k.al_q && c->al_layer[l].n) {   // word-level timestamps: the listed heads' queries of this position
                Prof pr(c, WH_KG_DEC_OTHER);
                wh_launch_align_copy(s, m->esz == 2, c->dq, d, WH_HEAD_DIM, WH_HEAD_DIM, c->al_layer[l], c->pos, k.n_prompt - 1, k.al_cap, nb, k.al_q);
            }
            Prof pr(c, WH_KG_DEC_CROSS_ATTN);
            if (f8)
                wh_launch_dec_cross_attn8(s, c->dq, (char*)c->cross_kv8 + (2 * l) * kv_stride, (char*)c->cross_kv8 + (2 * l + 1) * kv_stride,
                                          c->kv_amax + (long)(2 * l) * nb * D.n_heads, c->kv_amax + (long)(2 * l + 1) * nb * D.n_heads,
                                          c->cpart, c->cml, (int)S, (int)d, D.n_heads, c->cross_splits, nb, c->datt, mpad, kv_nt);
            else
                wh_launch_dec_cross_attn(s, prec, c->dq, (char*)c->cross_kv + (2 * l) * kv_stride * m->esz, (char*)c->cross_kv + (2 * l + 1) * kv_stride * m->esz,
                                         c->cpart, c->cml, (int)S, (int)d, D.n_heads, c->cross_splits, nb, c->datt, mpad, kv_nt, rpc);
        }
        {   // merge of the key ranges ∘ cross-attention out-proj + residual → x, raw slab, LN3 partials
            Prof pr(c, WH_KG_DEC_GEMM);
            const bool merged = c->cross_splits == 1 || c->cross_es;   // one key range per clip: the attention kernel wrote its output itself
            SkinnyArgs a = residual_producer(L.co_w, L.co_b, L.co_sc, merged ? c->datt : nullptr, d, L.ln3_w);
            if (!merged) { a.xpart = c->cpart; a.xml = c->cml; a.x_splits = c->cross_splits; a.x_heads = D.n_heads; }
            gemm(true, a);
        }
        {   // LN3 ∘ fc1 + GELU (slab output)
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = ln_consumer(L.fc1_w, L.fc1_b, L.fc1_sc, L.fc1_s, D.ffn, c->dh, ln_tiles_d, true);
            a.act = 1;
            gemm(false, a);
        }
        {   // fc2 + residual → x, raw slab, partials for the next layer's LN1 / the final LN
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = residual_producer(L.fc2_w, L.fc2_b, L.fc2_sc, c->dh, D.ffn, (l + 1 < D.dec_layers) ? m->dec[l + 1].ln1_w : m->dec_ln_w);
            if (advance) { a.ticket = c->step_ticket; a.pos_w = c->pos; }
            gemm(true, a);
        }
    }

    // final LN ∘ tied LM head + masked argmax; the finish kernel records the token, advances the position and embeds the next one
    void emit() const {
        if (k.beam_k) return emit_beam();
        if (k.sample_buf) return emit_sample();
        int lm_parts;
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = lm_head_common();
            a.mask_first = c->mask_first; a.mask_base = c->mask_base;
            a.logits = k.d_logits; a.logits_rows = k.logits_rows; a.logits_sel = k.d_sel;
            if (rules) {
                a.ts_state = c->ts_state; a.ts_logits = c->ts_logits; a.ts_ld = D.vocab - k.ts_begin;
                a.ts_begin = k.ts_begin; a.ts_max_init = k.ts_max_init;
            }
            a.part_sum = k.lp_sum;
            if (k.rep) { a.rep_bits = c->rep_bits; a.rep_side = c->rep_side; a.rep_words = c->rep_words; }
            wh_launch_lm_head(s, prec, a);
            lm_parts = wh_lm_head_parts(prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);   // argmax finish + greedy bookkeeping + the next position's embedding
        DecodeState st;
        st.feed = c->feed; st.out_tokens = c->out_tokens; st.n_out = c->n_out; st.done = c->done;
        st.forced = c->forced; st.n_forced = k.n_forced; st.n_prompt = k.n_prompt; st.eot = k.eot; st.tok_ld = c->tok_ld;
        if (k.lp_sum) st.logprob = c->lp_tok;
        NextEmbed ne;
        ne.tok_emb = m->tok_emb; ne.pos_emb = m->dec_pos; ne.x = c->dx; ne.xslab = c->dxs; ne.stats = c->lnpart;
        ne.xgamma = f8 ? m->dec[0].ln1_w : nullptr; ne.d = (int)d; ne.mpad = mpad; ne.shift = c->dshift; ne.off = d_off;
        TsFinish tf;
        if (rules) {
            tf.rules = true; tf.ts_logits = c->ts_logits; tf.ts_ld = D.vocab - k.ts_begin; tf.state = c->ts_state;
            tf.ts_begin = k.ts_begin; tf.vocab = D.vocab;
        }
        RepFinish rf;
        if (k.rep) {
            rf.on = true; rf.bits = c->rep_bits; rf.side = c->rep_side; rf.words = c->rep_words; rf.vocab = D.vocab;
            rf.p = k.rep_p; rf.inv = 1.0f / k.rep_p; rf.ngram = k.rep_n;
            if (rules) rf.exempt_from = k.ts_begin;   // timestamps repeat in pairs and the rules own them
            rf.mask_first = c->mask_first; rf.mask_base = c->mask_base;
        }
        wh_launch_argmax_finish(s, prec, c->part_val, c->part_idx, lm_parts, mpad, c->pos, c->step_ticket, st, nb, ne, tf, k.lp_sum, rf);
    }

    // Beam search: the LM head leaves the rows' raw logits of this position in the scratch (its argmax partials are not read);
    // k_beam_select chooses the next beams of every clip and embeds their tokens; k_beam_reorder permutes the self-attention caches and
    // advances the position.  One chain, no parallel branches.
    void emit_beam() const {
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = lm_head_common();
            a.mask_first = c->mask_first; a.mask_base = c->mask_base;
            a.logits = c->bm_logits; a.logits_rows = 1; a.logits_cur = true;
            wh_launch_lm_head(s, prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        BeamArgs b;
        b.K = k.beam_k; b.C = k.beam_c; b.n_clips = ncl; b.vocab = D.vocab;
        b.logits = c->bm_logits; b.pos_p = c->pos; b.n_prompt = k.n_prompt; b.eot = k.eot; b.tok_ld = c->tok_ld;
        b.mask_first = c->mask_first; b.mask_base = c->mask_base;
        if (rules) { b.ts_begin = k.ts_begin; b.ts_max_init = k.ts_max_init; }
        b.scores = c->bm_scores; b.parent = c->bm_parent; b.state = c->bm_state; b.pool_n = c->bm_pool_n; b.n_steps = c->bm_n_steps; b.pool = c->bm_pool;
        b.tr_parent = c->bm_tr_parent; b.tr_token = c->bm_tr_token; b.tr_score = c->bm_tr_score; b.tr_lp = c->bm_tr_lp; b.tr_pool = c->bm_tr_pool;
        b.rows_ld = c->max_batch; b.done = c->done; b.feed = c->feed;
        b.logits_out = k.d_logits; b.logits_rows = k.logits_rows; b.logits_sel = k.d_sel;
        NextEmbed ne;
        ne.tok_emb = m->tok_emb; ne.pos_emb = m->dec_pos; ne.x = c->dx; ne.xslab = c->dxs; ne.stats = c->lnpart;
        ne.d = (int)d; ne.mpad = mpad; ne.shift = c->dshift;
        const bool tm = c->bm_timing && !c->capturing;   // (measurement runs only: positions launched eagerly)
        std::array<hipEvent_t, 3> te = {nullptr, nullptr, nullptr};
        if (tm) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
        wh_launch_beam_select(s, prec, b, ne);
        if (tm) hipEventRecord(te[1], s);
        wh_launch_beam_reorder(s, (int)m->esz, c->self_k, c->self_v, c->bm_parent, c->done, k.beam_k, ncl, D.dec_layers, D.n_heads, D.n_text_ctx, c->pos, c->step_ticket);
        if (tm) { hipEventRecord(te[2], s); c->bm_events.push_back(te); }
    }

    // Temperature sampling: the LM head leaves the rows' raw logits of this position in the scratch (its argmax partials are not
    // read; k_argmax_finish is not launched); k_sample_select chooses every row's token, does the finish kernel's bookkeeping, embeds the next
    // position and advances.  One chain, no parallel branches.
    void emit_sample() const {
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = lm_head_common();
            a.mask_first = c->mask_first; a.mask_base = c->mask_base;
            a.logits = c->sm_logits; a.logits_rows = 1; a.logits_cur = true;
            wh_launch_lm_head(s, prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        SampleArgs a;
        a.logits = c->sm_logits; a.vocab = D.vocab; a.mask_first = c->mask_first; a.mask_base = c->mask_base;
        if (rules) { a.ts_begin = k.ts_begin; a.ts_max_init = k.ts_max_init; a.ts_state = c->sm_state; }
        a.temperature = c->sm_d_temp; a.row_ids = c->sm_d_ids; a.seed = c->sm_d_seed;
        a.logits_out = k.d_logits; a.logits_rows = k.logits_rows; a.logits_sel = k.d_sel;
        DecodeState st;
        st.feed = c->feed; st.out_tokens = c->out_tokens; st.n_out = c->n_out; st.done = c->done;
        st.forced = c->forced; st.n_forced = k.n_forced; st.n_prompt = k.n_prompt; st.eot = k.eot; st.tok_ld = c->tok_ld;
        st.logprob = c->sm_lp;
        NextEmbed ne;
        ne.tok_emb = m->tok_emb; ne.pos_emb = m->dec_pos; ne.x = c->dx; ne.xslab = c->dxs; ne.stats = c->lnpart;
        ne.xgamma = f8 ? m->dec[0].ln1_w : nullptr; ne.d = (int)d; ne.mpad = mpad; ne.shift = c->dshift; ne.off = d_off;
        const bool tm = c->sm_timing && !c->capturing;   // (measurement runs only: positions launched eagerly)
        std::array<hipEvent_t, 2> te = {nullptr, nullptr};
        if (tm) { for (auto& e : te) hipEventCreate(&e); hipEventRecord(te[0], s); }
        wh_launch_sample_select(s, prec, a, st, ne, nb, c->pos, c->step_ticket);
        if (tm) { hipEventRecord(te[1], s); c->sm_events.push_back(te); }
    }

    // the listed ids' unfiltered logits of this prompt position -> each row's language token in column tok_col of the next one; the
    // finish advances the position unless the probe's finish will
    void lang(int tok_col, bool advance) const {
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            const SkinnyArgs h = lm_head_common();   // the LM head's operands, the weight rows gathered by id
            LangHeadArgs a;
            a.X = h.X; a.x_mpad = h.x_mpad; a.W = h.W; a.bias = h.bias; a.ln_s = h.ln_s; a.ln_part = h.ln_part; a.ln_tiles = h.ln_tiles; a.M = h.M; a.K = h.K;
            a.ids = c->lang_d_ids; a.n_lang = (int)c->lang_ids.size(); a.out = c->lang_logits;
            wh_launch_lang_head(s, prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        wh_launch_lang_finish(s, c->lang_logits, c->lang_d_ids, (int)c->lang_ids.size(), c->lang_bcast ? 0 : -1, c->lang_probs, c->lang_chosen,
                              c->feed, c->out_tokens, c->tok_ld, tok_col, nb, advance ? c->pos : nullptr);
    }

    // softmax(v)[no_speech] over this prompt position's unfiltered logits: the LM head's log-probability variant with an all-zero mask,
    // no rules, nothing recorded; the probe's finish kernel advances the position
    void probe() const {
        int parts;
        {
            Prof pr(c, WH_KG_DEC_GEMM);
            SkinnyArgs a = lm_head_common();
            a.mask_first = c->lp_mask_zero; a.mask_base = c->lp_mask_zero;
            a.part_sum = c->lp_part_sum;
            a.probe_id = (int)c->lp_no_speech; a.probe_out = c->lp_probe_v;
            wh_launch_lm_head(s, prec, a);
            parts = wh_lm_head_parts(prec, a);
        }
        Prof pr(c, WH_KG_DEC_OTHER);
        wh_launch_nospeech_finish(s, c->part_val, c->lp_part_sum, parts, mpad, c->lp_probe_v, c->lp_ns, nb, c->pos);
    }
};

// One decoder position.  prompt == nullptr: a generated position — the emitting step that is captured into the graph; it sees the
// context and its key, nothing else (wh_ctx::StepKey).
void launch_step(wh_ctx* c, const wh_ctx::StepKey& k, const PromptStep* prompt = nullptr) {
    const Step t{c, k};
    const bool emits = !prompt || prompt->emits, lang = prompt && prompt->lang, probe = prompt && prompt->probe;
    if (prompt) {   // token + position embedding → x, raw slab, row sums (one "tile")
        Prof pr(c, WH_KG_DEC_OTHER);
        wh_launch_dec_embed(t.s, t.prec, t.m->tok_emb, t.m->dec_pos, c->feed, c->tok_ld, c->pos, c->dx, c->dxs, c->lnpart, t.nb, (int)t.d, t.mpad,
                            t.f8 ? t.m->dec[0].ln1_w : nullptr, c->dshift, t.d_off);
    }
    for (int l = 0; l < t.D.dec_layers; l++) t.layer(l, l == t.D.dec_layers - 1 && !emits && !lang && !probe);
    if (emits) t.emit();
    if (lang) t.lang(prompt->lang_col, !probe);   // (before the probe, if the probe sits at the same position)
    if (probe) t.probe();
}

// the instantiated graph of launch_step(c, key): kept from the last call if the key is the same, else captured now
int ensure_step_graph(wh_ctx* c, const wh_ctx::StepKey& key) {
    if (c->step_exec && c->step_key == key) return WH_OK;
    hipStream_t s = c->stream;
    drop_step_graph(c);   // nothing of it is in flight: every call ends with a stream synchronisation
    c->capturing = true;  // no event records inside the captured step
    hipGraph_t graph = nullptr;
    hipError_t ce = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (ce == hipSuccess) {
        launch_step(c, key);
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
    c->step_graph = graph;
    c->step_exec = gexec;
    c->step_key = key;
    return WH_OK;
}

// The `remaining` generated positions after the prompt replay ONE captured hipGraph of an emitting step — every kernel reads the
// position from device memory, so the graph is position-independent.  The host then pays one graph launch per token instead of ~50
// kernel launches (src/main.rs:793-826 is one ORT Run per token in the reference).
int run_token_loop(wh_ctx* c, const wh_ctx::StepKey& key, int remaining, bool poll_eot) {
    hipStream_t s = c->stream;
    // with event timing on: every position is launched eagerly (stride 0/1), or only every stride-th one
    // (sampled live timing) while the others replay the graph
    const int stride = c->prof ? c->prof_stride : 0;
    const bool use_graph = remaining > 1 && !c->no_graph && (!c->prof || stride > 1);
    if (use_graph) {
        int rc = ensure_step_graph(c, key);
        if (rc) return rc;
    }
    std::vector<int> done_h(key.nb);
    for (int r = 0; r < remaining; r++) {
        const bool sampled = c->prof && stride > 1 && (r % stride) == stride / 2;
        if (use_graph && !sampled) {
            hipError_t ge = hipGraphLaunch(c->step_exec, s);
            if (ge != hipSuccess) {
                hipStreamSynchronize(s);
                drop_step_graph(c);
                return fail(c, WH_ERR_HIP, "hipGraphLaunch failed: %s", hipGetErrorString(ge));
            }
        } else {
            launch_step(c, key);
        }
        // diagnostic (profiles/README.md, rocprofv3 --pmc at whisper-large-v3 size): bound the number of dispatches in flight
        if (c->sync_every_pos) hipStreamSynchronize(s);
        // EOT early-out (src/main.rs:781-783, 820-822): poll the done flags every 16 generated tokens
        const int gen = r + 1;
        if ((gen & 15) == 15 && r + 1 < remaining && poll_eot) {
            hipError_t e1 = hipMemcpyAsync(done_h.data(), c->done, key.nb * 4, hipMemcpyDeviceToHost, s);
            hipError_t e2 = hipStreamSynchronize(s);
            if (e1 != hipSuccess || e2 != hipSuccess)
                return fail(c, WH_ERR_HIP, "decode: polling the done flags failed: %s", hipGetErrorString(e1 != hipSuccess ? e1 : e2));
            bool all = true;
            for (int b = 0; b < key.nb; b++) all = all && done_h[b];
            if (all) break;
        }
    }
    return WH_OK;
}

// tokens, counts, log-probabilities, no-speech, languages, logits; keeps what wh_get_logprobs / wh_get_languages return
int read_back(wh_ctx* c, const DecodePlan& pl, int64_t* tokens_out, size_t tok_stride, size_t* n_tokens_out, float* logits_out, const int32_t* sel) {
    hipStream_t s = c->stream;
    const int nb = pl.key.nb, ld = c->tok_ld, Nmax = pl.Nmax, PP = pl.key.n_prompt, vocab = c->m->dims.vocab;
    const size_t logits_rows = pl.key.logits_rows;
    const bool lp = c->lp_on || pl.key.sample_buf;   // (a sampling call records log-probabilities itself, in its own buffer)
    const size_t n_lang = c->lang_ids.size();
    std::vector<int> toks, nout, lch, afr, asb;
    std::vector<float> lps, nsp, lpr;
    const double t0 = now_s();
    auto fetch = [&](auto& v, const void* src, size_t n) {   // (4-byte elements)
        v.resize(n);
        return hipMemcpyAsync(v.data(), src, n * 4, hipMemcpyDeviceToHost, s);
    };
    CTX_HIP(c, fetch(toks, c->out_tokens, (size_t)nb * ld));
    CTX_HIP(c, fetch(nout, c->n_out, nb));
    if (lp) CTX_HIP(c, fetch(lps, pl.key.sample_buf ? c->sm_lp : c->lp_tok, (size_t)nb * ld));
    if (pl.lp_probe) CTX_HIP(c, fetch(nsp, c->lp_ns, nb));
    if (pl.lang_det) {
        CTX_HIP(c, fetch(lch, c->lang_chosen, nb));
        CTX_HIP(c, fetch(lpr, c->lang_probs, (size_t)nb * n_lang));
    }
    if (c->al_on) {
        CTX_HIP(c, fetch(afr, c->al_frames, (size_t)nb * c->m->dims.n_text_ctx));
        CTX_HIP(c, fetch(asb, c->al_sb, nb));
    }
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    c->sm_ms = 0;
    c->sm_timed = (long)c->sm_events.size();
    for (auto& te : c->sm_events) {
        float ms = 0;
        hipEventElapsedTime(&ms, te[0], te[1]);
        c->sm_ms += ms;
        for (auto& e : te) hipEventDestroy(e);
    }
    c->sm_events.clear();
    if (c->al_on) {   // kept for wh_get_token_frames / wh_get_alignment_debug
        const int tc = c->m->dims.n_text_ctx, nh = (int)(c->al_heads.size() / 2), Sp = (c->m->dims.n_audio_ctx + 3) / 4 * 4, NEW = pl.NEW;
        for (int b = 0; b < nb; b++) {
            c->al_rows.emplace_back(afr.begin() + (size_t)b * tc, afr.begin() + (size_t)b * tc + (nout[b] - PP));
            c->al_nframes.push_back(asb[b]);
        }
        c->al_have = true;
        c->al_dbg.resize(c->al_debug.size());
        for (size_t k = 0; k < c->al_debug.size(); k++) {   // the debug rows' slots cut to [n_heads][n_gen][S_b] and [n_gen][S_b]
            wh_ctx::AlignDebug& dbg = c->al_dbg[k];
            const int r = c->al_debug[k], n = nout[r] - PP, sb = asb[r];
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
    if (pl.lang_fix) {   // the file's language and window 0's probabilities (the first rows kept), once per window of this batch
        for (int b = 0; b < nb; b++) {
            c->lang_rows.push_back(c->lang_fixed);
            for (size_t j = 0; j < n_lang; j++) { const float pj = c->lang_prob_rows[j]; c->lang_prob_rows.push_back(pj); }
        }
    } else if (pl.lang_det) {
        for (int b = 0; b < nb; b++) c->lang_rows.push_back(lch[b]);
        c->lang_prob_rows.insert(c->lang_prob_rows.end(), lpr.begin(), lpr.end());
        c->lang_have = true;
        c->lang_have_n = n_lang;
    }
    if (lp) {   // kept for wh_get_logprobs: each clip's generated positions
        for (int b = 0; b < nb; b++) c->lp_rows.emplace_back(lps.begin() + (size_t)b * ld + PP, lps.begin() + (size_t)b * ld + nout[b]);
        c->lp_ns_rows.insert(c->lp_ns_rows.end(), nsp.begin(), nsp.end());
        c->lp_have = true;
        c->lp_have_ns = pl.lp_probe;
    }
    for (int b = 0; b < nb; b++) {
        n_tokens_out[b] = (size_t)(nout[b] - Nmax);   // the prefix columns are not echoed: shared prompt ++ generated, as without prefixes
        for (int i = Nmax; i < nout[b]; i++) tokens_out[(size_t)b * tok_stride + i - Nmax] = toks[(size_t)b * ld + i];
    }
    if (logits_out) {
        for (size_t i = 0; i < pl.n_lrows; i++) {
            const int b = sel ? sel[i] : (int)i;
            const size_t rows = (size_t)nout[b] - PP;
            CTX_HIP(c, hipMemcpy(logits_out + i * logits_rows * vocab, pl.key.d_logits + i * logits_rows * vocab, std::min(rows, logits_rows) * vocab * 4,
                                 hipMemcpyDeviceToHost));
        }
    }
    c->timing.d2h_s = now_s() - t0;
    return WH_OK;
}

// read_back of a call with beam search: the pool and the trace come back, the parents are walked back into hypotheses, the
// hypotheses are ranked (f32), and the best one of each clip is returned as its tokens (and log-probabilities); keeps what wh_get_beams /
// wh_get_beam_trace return.  Language detection and the no-speech probe: the clip's first row.
int read_back_beam(wh_ctx* c, const DecodePlan& pl, int64_t* tokens_out, size_t tok_stride, size_t* n_tokens_out, float* logits_out, const int32_t* sel) {
    hipStream_t s = c->stream;
    const int R = pl.key.nb, K = pl.K, ncl = pl.ncl, ld = c->max_batch, PP = pl.key.n_prompt, vocab = c->m->dims.vocab, NEW = pl.NEW;
    const size_t n_lang = c->lang_ids.size();
    std::vector<int> trp, trt, trpool, pool, pool_n, nsteps, feed, lch;
    std::vector<float> trs, trl, nsp, lpr;
    const double t0 = now_s();
    auto fetch = [&](auto& v, const void* src, size_t n) {   // (4-byte elements)
        v.resize(n);
        return hipMemcpyAsync(v.data(), src, n * 4, hipMemcpyDeviceToHost, s);
    };
    const size_t ntr = (size_t)NEW * ld;   // (the trace is [position][max_batch]: the call's positions are its first NEW rows)
    CTX_HIP(c, fetch(trp, c->bm_tr_parent, ntr));
    CTX_HIP(c, fetch(trt, c->bm_tr_token, ntr));
    CTX_HIP(c, fetch(trs, c->bm_tr_score, ntr));
    CTX_HIP(c, fetch(trl, c->bm_tr_lp, ntr));
    CTX_HIP(c, fetch(trpool, c->bm_tr_pool, ntr));
    CTX_HIP(c, fetch(pool, c->bm_pool, (size_t)ncl * WH_MAX_BEAM_CANDIDATES * 4));
    CTX_HIP(c, fetch(pool_n, c->bm_pool_n, ncl));
    CTX_HIP(c, fetch(nsteps, c->bm_n_steps, ncl));
    CTX_HIP(c, fetch(feed, c->feed, (size_t)R * c->tok_ld));   // (the prompt as it was fed: the detected language token)
    if (pl.lp_probe) CTX_HIP(c, fetch(nsp, c->lp_ns, R));
    if (pl.lang_det) {
        CTX_HIP(c, fetch(lch, c->lang_chosen, R));
        CTX_HIP(c, fetch(lpr, c->lang_probs, (size_t)R * n_lang));
    }
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    c->bm_ms[0] = c->bm_ms[1] = 0;
    c->bm_timed = (long)c->bm_events.size();
    for (auto& te : c->bm_events) {
        for (int i = 0; i < 2; i++) { float ms = 0; hipEventElapsedTime(&ms, te[i], te[i + 1]); c->bm_ms[i] += ms; }
        for (auto& e : te) hipEventDestroy(e);
    }
    c->bm_events.clear();
    if (pl.lang_fix) {
        for (int b = 0; b < ncl; b++) {
            c->lang_rows.push_back(c->lang_fixed);
            for (size_t j = 0; j < n_lang; j++) { const float pj = c->lang_prob_rows[j]; c->lang_prob_rows.push_back(pj); }
        }
    } else if (pl.lang_det) {
        for (int b = 0; b < ncl; b++) {
            c->lang_rows.push_back(lch[(size_t)b * K]);
            c->lang_prob_rows.insert(c->lang_prob_rows.end(), lpr.begin() + (size_t)b * K * n_lang, lpr.begin() + ((size_t)b * K + 1) * n_lang);
        }
        c->lang_have = true;
        c->lang_have_n = n_lang;
    }
    c->bm_traces.assign(c->bm_trace_clips.size(), wh_ctx::BeamTrace());
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
            h.rank = c->bm_length_penalty < 0.0f ? h.sum / len : h.sum / powf((5.0f + len) / 6.0f, c->bm_length_penalty);
        }
        std::stable_sort(hyps.begin(), hyps.end(), [](const wh_ctx::BeamHyp& x, const wh_ctx::BeamHyp& y) { return x.rank > y.rank; });
        // the clip's tokens: the prompt as fed, then the best hypothesis
        for (int i = pl.Nmax; i < PP; i++) tokens_out[(size_t)clip * tok_stride + i - pl.Nmax] = feed[(size_t)r0 * c->tok_ld + i];
        size_t n = (size_t)(PP - pl.Nmax);
        if (!hyps.empty())
            for (int t : hyps[0].tokens) tokens_out[(size_t)clip * tok_stride + n++] = t;
        n_tokens_out[clip] = n;
        if (c->lp_on) {
            c->lp_rows.emplace_back(hyps.empty() ? std::vector<float>() : hyps[0].lps);
            if (pl.lp_probe) c->lp_ns_rows.push_back(nsp[r0]);
        }
        for (size_t k = 0; k < c->bm_trace_clips.size(); k++) {
            if (c->bm_trace_clips[k] != clip) continue;
            wh_ctx::BeamTrace& tr = c->bm_traces[k];
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
        c->bm_hyps.push_back(std::move(hyps));
    }
    c->bm_have = true;
    if (c->lp_on) { c->lp_have = true; c->lp_have_ns = pl.lp_probe; }
    if (logits_out) {
        const size_t logits_rows = pl.key.logits_rows;
        for (size_t i = 0; i < pl.n_lrows; i++) {   // physical rows: what each produced at the positions its clip ran
            const int r = sel ? sel[i] : (int)i;
            const size_t rows = (size_t)nsteps[r / K];
            CTX_HIP(c, hipMemcpy(logits_out + i * logits_rows * vocab, pl.key.d_logits + i * logits_rows * vocab, std::min(rows, logits_rows) * vocab * 4,
                                 hipMemcpyDeviceToHost));
        }
    }
    c->timing.d2h_s = now_s() - t0;
    return WH_OK;
}

// `sel` (optional, with logits_out): the n_sel batch rows whose logits are read back — logits_out is then [n_sel][logits_rows][vocab]
int run_decode(wh_ctx* c, int nb, const wh_decode_params* p, int64_t* tokens_out, size_t tok_stride,
               size_t* n_tokens_out, float* logits_out, size_t logits_rows, const std::function<int()>& after_kv = nullptr,
               const int32_t* sel = nullptr, size_t n_sel = 0) {
    hipStream_t s = c->stream;
    c->cur = s;
    DecodePlan pl;
    int rc = plan_decode(c, nb, p, logits_out != nullptr, logits_rows, sel, n_sel, pl);
    if (rc) return rc;
    const wh_ctx::StepKey& key = pl.key;
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

// mel of nb clips resident at `pcm` ([nb][480000] f32, n samples each in c->d_nsamp) → conv1 operand in c->melT
int run_mel_batch(wh_ctx* c, const float* pcm, int nb) {
    wh_model* m = c->m;
    hipStream_t s = c->s_enc;
    c->cur = s;
    CTX_HIP(c, hipMemsetAsync(c->d_gmax, 0, nb * 4, s));
    {
        Prof p(c, WH_KG_MEL);
        wh_launch_mel_stft(s, pcm, WH_CLIP_SAMPLES, c->d_nsamp, nb, WH_N_FRAMES, m->mel_tw, m->mel_win, m->mel_fbT,
                           m->dims.n_mels, c->raw, (long)m->dims.n_mels * RAW_LD, RAW_LD, c->d_gmax);
    }
    {
        Prof p(c, WH_KG_MEL);
        if (m->esz == 4)
            wh_launch_mel_tokens<float>(s, c->raw, (long)m->dims.n_mels * RAW_LD, RAW_LD, nullptr, nullptr, c->d_nframes,
                                        c->d_gmax, 0, m->dims.n_mels, nb, (float*)c->melT, (long)TOK_ROWS * m->dims.n_mels);
        else
            wh_launch_mel_tokens<bf16>(s, c->raw, (long)m->dims.n_mels * RAW_LD, RAW_LD, nullptr, nullptr, c->d_nframes,
                                       c->d_gmax, 0, m->dims.n_mels, nb, (bf16*)c->melT, (long)TOK_ROWS * m->dims.n_mels);
    }
    return WH_OK;
}

// log-mel + encoder of nb resident clips as one pass on the encoder stream, stage events into set `set`
int run_encoder_pass(wh_ctx* c, const float* pcm, int nb, int set) {
    int rc = enc_begin(c);
    if (rc) return rc;
    hipStream_t s = c->s_enc;
    CTX_HIP(c, hipEventRecord(c->enc_ev[set][0], s));
    if (c->ing_n) {   // a raw entry: the clips' bytes in ing_raw[ing_buf] become the PCM rows first (part of the pass's preprocess time)
        c->cur = s;
        Prof p(c, WH_KG_MEL);
        wh_launch_ingest(s, c->ing_raw[c->ing_buf], c->ing_desc, c->ing_n, c->ing_max_out, c->pcm);
        c->ing_last_n = c->ing_n; c->ing_last_buf = c->ing_buf; c->ing_last_max_out = c->ing_max_out;
        c->ing_n = 0;
    }
    rc = run_mel_batch(c, pcm, nb);
    if (rc) return rc;
    CTX_HIP(c, hipEventRecord(c->enc_ev[set][1], s));
    rc = run_encoder(c, nb, false);
    if (rc) return rc;
    CTX_HIP(c, hipEventRecord(c->enc_ev[set][2], s));
    return WH_OK;
}

// stage times of the batch whose encoder pass is in event set c->enc_set and whose decode ran between ev[5] and ev[3]
int finish_timing(wh_ctx* c, double t_start) {
    float a = 0, b = 0, d = 0;
    hipEventElapsedTime(&a, c->enc_ev[c->enc_set][0], c->enc_ev[c->enc_set][1]);
    hipEventElapsedTime(&b, c->enc_ev[c->enc_set][1], c->enc_ev[c->enc_set][2]);
    hipEventElapsedTime(&d, c->ev[5], c->ev[3]);
    c->timing.preprocess_s = a * 1e-3;
    c->timing.encode_s = b * 1e-3;
    c->timing.decode_s = d * 1e-3;
    c->timing.total_s = now_s() - t_start;
    prof_collect(c);
    return WH_OK;
}

int check_params(wh_ctx* c, const wh_decode_params* p) {
    // (every decode entry passes here once, first: what wh_get_logprobs returns belongs to the call that starts now)
    c->lp_have = c->lp_have_ns = false;
    c->lp_rows.clear();
    c->lp_ns_rows.clear();
    c->lang_have = false;
    c->lang_rows.clear();
    c->lang_prob_rows.clear();
    c->al_have = false;
    c->al_rows.clear();
    c->al_nframes.clear();
    c->al_dbg.clear();
    c->bm_have = false;
    c->bm_hyps.clear();
    c->bm_traces.clear();
    for (auto& te : c->bm_events)   // (timing events of a call that failed before its read-back)
        for (auto& e : te) hipEventDestroy(e);
    c->bm_events.clear();
    for (auto& te : c->sm_events)
        for (auto& e : te) hipEventDestroy(e);
    c->sm_events.clear();
    if (!p) return fail(c, WH_ERR_ARG, "decode params are NULL");
    if ((p->n_suppress && !p->suppress) || (p->n_begin_suppress && !p->begin_suppress) || (p->n_forced && !p->forced))
        return fail(c, WH_ERR_ARG, "decode params: NULL list with non-zero length");
    return WH_OK;
}

}  // namespace

// =================================================================================================
extern "C" {

int wh_abi_version(void) { return WH_ABI_VERSION; }

int wh_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int wh_synthetic_weights(const char* preset, uint64_t seed, float* out, size_t cap, size_t* n_out) {
    wh_dims dims{};
    if (!preset || !wh_preset_dims(preset, &dims)) { wh_set_error("unknown synthetic preset"); return WH_ERR_ARG; }
    std::vector<float> w;
    wh_synth_weights(dims, seed, w);
    if (n_out) *n_out = w.size();
    if (out) {
        if (cap < w.size()) { wh_set_error("buffer too small"); return WH_ERR_ARG; }
        memcpy(out, w.data(), w.size() * 4);
    }
    return WH_OK;
}

size_t wh_mel_frames(size_t n) {  // src/main.rs:444-452
    size_t nf = 1 + n / 160;
    if (nf > 1) nf -= 1;
    return nf;
}

int wh_model_load(const char* spec, int device, int precision, wh_model** out) {
    if (!spec || !out) { wh_set_error("wh_model_load: NULL argument"); return WH_ERR_ARG; }
    *out = nullptr;
    std::string s(spec);
    wh_dims dims{};
    std::vector<float> master;
    WhPreQuant pre;
    if (s.rfind("synthetic:", 0) == 0) {
        size_t c2 = s.find(':', 10);
        std::string preset = s.substr(10, c2 == std::string::npos ? std::string::npos : c2 - 10);
        uint64_t seed = c2 == std::string::npos ? 0 : strtoull(s.c_str() + c2 + 1, nullptr, 10);
        if (!wh_preset_dims(preset, &dims)) { wh_set_error("unknown synthetic preset '%s'", preset.c_str()); return WH_ERR_ARG; }
        wh_synth_weights(dims, seed, master);
    } else {
        int rc = wh_load_model_dir(s, &dims, master, &pre);
        if (rc) return rc;
    }
    return wh_model_build(dims, std::move(master), device, precision, out, &pre);
}

int wh_model_create(const wh_dims* dims, const float* weights, size_t n, int device, int precision, wh_model** out) {
    if (!dims || !weights || !out) { wh_set_error("wh_model_create: NULL argument"); return WH_ERR_ARG; }
    *out = nullptr;
    std::vector<float> master(weights, weights + n);
    return wh_model_build(*dims, std::move(master), device, precision, out);
}

void wh_model_free(wh_model* m) {
    if (!m) return;
    if (m->arena) hipFree(m->arena);
    delete m;
}

int wh_model_get_dims(const wh_model* m, wh_dims* out) {
    if (!m || !out) return WH_ERR_ARG;
    *out = m->dims;
    return WH_OK;
}
int wh_model_precision(const wh_model* m) { return m ? m->prec : -1; }

void wh_e4m3_quantize(const float* x, size_t n, uint8_t* codes) { for (size_t i = 0; i < n; i++) codes[i] = wh_e4m3_from_f32(x[i]); }
void wh_e4m3_dequantize(const uint8_t* codes, size_t n, float* x) { for (size_t i = 0; i < n; i++) x[i] = wh_e4m3_to_f32(codes[i]); }

int wh_model_export_tensor(const wh_model* m, const char* name, float* out, size_t cap, size_t* n_out) {
    if (!m || !name) return WH_ERR_ARG;
    auto it = m->index.find(name);
    if (it == m->index.end()) { wh_set_error("no tensor named %s", name); return WH_ERR_ARG; }
    if (n_out) *n_out = it->second.second;
    if (out) {
        if (cap < it->second.second) { wh_set_error("export buffer too small"); return WH_ERR_ARG; }
        memcpy(out, m->master.data() + it->second.first, it->second.second * 4);
    }
    return WH_OK;
}

int wh_ctx_create(wh_model* m, int max_batch, wh_ctx** out) {
    wh_ctx_opts o{};
    o.struct_size = sizeof o;
    o.max_batch = max_batch;
    return wh_ctx_create_ex(m, &o, out);
}

static int ctx_create_impl(wh_model* m, const wh_ctx_opts* opts, wh_ctx** out) {
    if (!m || !out || !opts) { wh_set_error("wh_ctx_create: NULL argument"); return WH_ERR_ARG; }
    *out = nullptr;
    if (opts->struct_size != sizeof(wh_ctx_opts)) { wh_set_error("wh_ctx_create_ex: wh_ctx_opts.struct_size does not match this library"); return WH_ERR_ARG; }
    const int max_batch = opts->max_batch;
    if (max_batch < 1 || max_batch > WH_MAX_BATCH) { wh_set_error("max_batch must be 1..2048"); return WH_ERR_ARG; }
    if ((opts->enc_cu_mask_words && !opts->enc_cu_mask) || (opts->dec_cu_mask_words && !opts->dec_cu_mask)) {
        wh_set_error("wh_ctx_create_ex: NULL CU mask with a non-zero word count");
        return WH_ERR_ARG;
    }
    auto mask_bits = [](const uint32_t* w, size_t n) { size_t k = 0; for (size_t i = 0; i < n; i++) k += (size_t)__builtin_popcount(w[i]); return k; };
    if ((opts->enc_cu_mask_words && mask_bits(opts->enc_cu_mask, opts->enc_cu_mask_words) == 0) ||
        (opts->dec_cu_mask_words && mask_bits(opts->dec_cu_mask, opts->dec_cu_mask_words) == 0)) {
        wh_set_error("wh_ctx_create_ex: a CU mask with no bit set would leave its stream without compute units");
        return WH_ERR_ARG;
    }
    // A mask must restrict every XCD it is meant to restrict: bit i is compute unit i / 8 of XCD i % 8, and an XCD none of
    // whose bits is set is not restricted at all (measured, tools/cu_mask_probe.hip) — refuse such a mask instead of silently
    // running on compute units the caller meant to leave to the other stream.  A mask naming every compute unit is no mask.
    auto xcds_covered = [](const uint32_t* w, size_t n) { unsigned seen = 0; for (size_t i = 0; i < n * 32; i++) if (w[i >> 5] >> (i & 31) & 1) seen |= 1u << (i & 7); return seen == 0xFFu; };
    if ((opts->enc_cu_mask_words && !xcds_covered(opts->enc_cu_mask, opts->enc_cu_mask_words)) ||
        (opts->dec_cu_mask_words && !xcds_covered(opts->dec_cu_mask, opts->dec_cu_mask_words))) {
        wh_set_error("wh_ctx_create_ex: a CU mask must select at least one compute unit of every XCD (bit i = compute unit i / 8 of XCD i %% 8)");
        return WH_ERR_ARG;
    }
    WH_HIP_CHECK(hipSetDevice(m->device));
    int n_cus = 0;
    WH_HIP_CHECK(hipDeviceGetAttribute(&n_cus, hipDeviceAttributeMultiprocessorCount, m->device));
    const bool enc_masked = opts->enc_cu_mask_words && (int)mask_bits(opts->enc_cu_mask, opts->enc_cu_mask_words) < n_cus;
    const bool dec_masked = opts->dec_cu_mask_words && (int)mask_bits(opts->dec_cu_mask, opts->dec_cu_mask_words) < n_cus;
    auto* c = new wh_ctx();
    c->m = m;
    c->max_batch = max_batch;
    c->dec_cus = dec_masked ? (int)mask_bits(opts->dec_cu_mask, opts->dec_cu_mask_words) : n_cus;   // compute units the token-loop stream may use
    c->no_graph = getenv("WH_NO_GRAPH") != nullptr;
    c->sync_every_pos = getenv("WH_SYNC_EVERY_POS") != nullptr;
    c->al_timing = getenv("WH_ALIGN_TIMING") != nullptr;
    c->bm_timing = getenv("WH_BEAM_TIMING") != nullptr;
    c->sm_timing = getenv("WH_SAMPLE_TIMING") != nullptr;
    const wh_dims& D = m->dims;
    const size_t B = max_batch, d = D.d_model, S = D.n_audio_ctx, F = D.ffn, C = D.n_mels, esz = m->esz;
    const size_t Ld = D.dec_layers, H = D.n_heads, TC = D.n_text_ctx;
    c->ldv = (int)align_up(S, 64);
    c->tok_ld = D.n_text_ctx + 1;
    // row pitch of the slab-layout decode activations: the decode GEMMs read whole 32- / 64-row groups (k_dec_gemm MT = 2,
    // k_dec_gemm_wide MT = 4) whose tail rows are masked, not clamped — the pitch covers them
    c->mpad = (int)align_up(B, B > 16 ? 64 : 16);
    // enough workgroups to cover the chip at small batch, no more than 16 key ranges
    c->cross_splits = (int)std::min<size_t>(32, std::max<size_t>(1, 256 / B));  // measured: ~256 workgroups streams best
    if (m->prec == WH_PREC_BF16 && d > 512 && d % 256 == 0)   // wide models: a workgroup per 256-column group as well (k_dec_cross_attn_cg)
        c->cross_splits = (int)std::min<size_t>(32, std::max<size_t>(1, 512 / (B * (d / 256))));
    const size_t n_tiles = (D.vocab + 15) / 16;
    Carver cv;
    const size_t o_pcm = cv.take(B * WH_CLIP_SAMPLES * 4), o_raw = cv.take(B * C * RAW_LD * 4);
    const size_t o_melstage = cv.take(C * WH_N_FRAMES * 4);
    const size_t o_melT = cv.take((B * TOK_ROWS * C + 256) * esz), o_h1 = cv.take((B * H1_ROWS * d + 256) * esz);
    const size_t o_x = cv.take(B * S * d * 4), o_xn = cv.take(B * S * d * esz), o_qk = cv.take(B * S * 2 * d * esz);
    // WH_PREC_BF16 on the LDS-DMA GEMM (contexts beyond a few clips, widths it has tiles for): the encoder's LayerNorms are
    // folded into their consumer GEMMs — decided from the model and the context, never from a call's clip count
    // (every folded GEMM must pass wh_gemm8_applicable: rows = clips x S >= 256, V^T with M = d_model >= 256 and N = S % 4 == 0, producers
    // with N = d_model % 64 == 0; WH_GEMM8=0 sends every GEMM to k_gemm, which has no fold — then the LayerNorm kernels run)
    c->enc_fold = m->prec == WH_PREC_BF16 && max_batch > WH_SMALL_CTX_CLIPS && d >= 256 && (d % 64) == 0 && (F % 64) == 0 && S >= 256 && (S % 4) == 0 &&
                  m->cross_kv_wf != nullptr && wh_gemm8_enabled() && getenv("WH_NO_ENC_FOLD") == nullptr;
    // ... and a layer's feed-forward block runs as one launch (wh_mlp.hip: d_model 512, ffn a multiple of 128); the 2048-wide hidden activations
    // then never exist in HBM and their buffer (12.6 GB at 2048 clips) is not carved.  WH_ENC_MLP=0: the two k_gemm8 launches (A/B runs)
    c->enc_mlp = c->enc_fold && d == 512 && F >= 128 && (F % 128) == 0 && !(getenv("WH_ENC_MLP") && atoi(getenv("WH_ENC_MLP")) == 0);
    const size_t o_vT = cv.take(B * d * c->ldv * esz), o_att = cv.take(B * S * d * esz), o_h = c->enc_mlp ? 0 : cv.take(B * S * F * esz);
    const size_t o_enc = cv.take(B * S * d * esz), o_encf = cv.take(B * S * d * 4);
    // Cross-attention on the encoder states (bf16, whisper-base geometry, contexts of at least one workgroup per CU): the token
    // loop streams the S x d states themselves instead of the projected K and V of every layer — no cross-K/V cache.  Decided
    // from the model and the context only (WH_CTX_CROSS_ES_ON / _OFF or WH_CROSS_ES=1 / 0 override the size rule).
    c->cross_es = m->cross_es && max_batch >= 256;
    if (opts->flags & WH_CTX_CROSS_ES_ON) c->cross_es = m->cross_es;
    if (opts->flags & WH_CTX_CROSS_ES_OFF) c->cross_es = false;
    if (const char* e = getenv("WH_CROSS_ES")) c->cross_es = m->cross_es && atoi(e) != 0;
    if ((opts->flags & WH_CTX_CROSS_ES_ON) && !m->cross_es) {
        delete c;
        wh_set_error("wh_ctx_create_ex: WH_CTX_CROSS_ES_ON needs a bf16 or f16x3 model of whisper-base geometry (d_model 512, 8 heads)");
        return WH_ERR_UNSUPPORTED;
    }
    // decode GEMMs on LDS-DMA tiles (wh_dec_tile.hip) where a batch is a thousand rows and more, in the split-fp16 mode: measured against
    // k_dec_gemm_wide at 2048 clips — f16x3 224 -> 193 ms of decode GEMMs per step; bf16 130 -> 133 ms (both forms sit
    // on the per-CU L2 -> LDS rate there: 256 KB of operands per 128 x 128 tile), so bf16 keeps k_dec_gemm_wide.  WH_DEC_TILE=0 / 1 forces
    // it off / on for A/B runs
    c->dec_tile = m->prec == WH_PREC_F16X3 && max_batch >= 1024;
    if (const char* e = getenv("WH_DEC_TILE")) c->dec_tile = (m->prec == WH_PREC_BF16 || m->prec == WH_PREC_F16X3) && atoi(e) != 0;
    // rows from one clip's encoder states to the next: 20 rows (20 KiB) of padding, so that the lock-step streams of the persistent
    // workgroups (clip i, i + 256, ...) do not all sit on the same 4 KiB phase of the 1,536,000-byte clip pitch: 491 -> 480-485 us per
    // 2048-clip launch (tools/es_state_probe.py, WH_ES_PAD = 0 / 12 / 20 / 28 / 44 / 84: 491 / 487 / 482 / 484 / 485 / 490)
    c->es_rows = (int)S + 20;
    if (const char* e = getenv("WH_ES_PAD")) c->es_rows = (int)S + std::max(0, atoi(e));   // (A/B runs)
    c->es_rows_cap = c->es_rows;
    if (const char* e = getenv("WH_ES_PAD_MAX")) c->es_rows_cap = std::max(c->es_rows, (int)S + atoi(e));   // (probe runs: room for wh_debug_set_es_pad)
    const size_t o_ckv = cv.take(c->cross_es ? B * (size_t)c->es_rows_cap * d * esz : Ld * 2 * B * S * d * esz);
    const bool f8 = m->prec == WH_PREC_FP8;
    const bool f8kv = f8 && !c->cross_es;   // (the encoder-state form of the fp8 mode keeps no projected K / V at all)
    const size_t o_ckv8 = f8kv ? cv.take(Ld * 2 * B * S * d) : 0, o_kvam = f8kv ? cv.take(Ld * 2 * B * H * 4) : 0;
    // fp8-MFMA encoder (wh_gemm8_mx.hip): MX activations when every contraction length is one the kernel takes
    // (decided from the model and the context only, never from a call's clip count: S >= 256 rows is one full tile even for one clip)
    // contraction lengths: any multiple of 128 from 256 on (whisper-large-v3: 1280, 5120); d_model must be a width k_layernorm_mx exists for
    auto mx_k = [](size_t k) { return k >= 256 && (k % 128) == 0; };
    // (the same predicates wh_gemm8_mx_applicable applies to every shape of the path: Q|K / fc1 / fc2 / cross-K/V rows = clips x S >= one tile,
    // the per-clip V^T product with M = d_model rows and N = S columns in groups of four)
    c->mx_ok = f8 && mx_k(d) && mx_k(F) && wh_mx_ln_width((int)d) && S >= 256 && (S % 4) == 0 && getenv("WH_NO_MX") == nullptr;
    const size_t o_xn8 = c->mx_ok ? cv.take(B * S * d) : 0, o_xn8s = c->mx_ok ? cv.take(B * S * 4 * wh_mx_nkp((int)d)) : 0;
    const size_t o_h8 = c->mx_ok ? cv.take(B * S * F) : 0, o_h8s = c->mx_ok ? cv.take(B * S * 4 * wh_mx_nkp((int)F)) : 0;
    const size_t o_xb = c->enc_fold ? cv.take(B * S * d * 2) : 0, o_epart = c->enc_fold ? cv.take((d / 64) * B * S * 2 * 4) : 0;
    const size_t o_estat = c->enc_fold ? cv.take(B * S * 2 * 4) : 0, o_eshift = c->enc_fold ? cv.take(B * S * 4) : 0, o_eshift0 = c->enc_fold ? cv.take(B * S * 4) : 0;
    const size_t o_sk = cv.take(Ld * B * H * TC * WH_HEAD_DIM * esz), o_sv = cv.take(Ld * B * H * TC * WH_HEAD_DIM * esz);
    const size_t MP = (size_t)c->mpad;  // slab-layout activations: [K/32][MP][32]
    const size_t o_dx = cv.take(B * d * 4), o_dxn = cv.take(MP * d * esz), o_dqkv = cv.take(B * 3 * d * esz);
    const size_t o_dxs = cv.take(MP * d * esz), o_lnp = cv.take((d / 16) * MP * 2 * 4), o_dsh = cv.take(MP * 4);
    const size_t o_datt = cv.take(MP * d * esz), o_dq = cv.take(B * d * esz), o_dh = cv.take(MP * F * esz);
    const size_t o_dqe = c->cross_es ? cv.take(B * H * d * 4) : 0, o_dctx = c->cross_es ? cv.take(MP * H * d * esz) : 0;
    const size_t o_dq32 = c->cross_es ? cv.take(B * d * 4) : 0;
    const size_t o_cpart = cv.take(B * c->cross_splits * d * 4), o_cml = cv.take(B * c->cross_splits * H * 2 * 4);
    const size_t o_pv = cv.take(MP * (n_tiles + 4) * 4), o_pi = cv.take(MP * (n_tiles + 4) * 4);  // [part][mpad]
    const size_t o_feed = cv.take(B * c->tok_ld * 4), o_out = cv.take(B * c->tok_ld * 4);
    const size_t o_nout = cv.take(B * 4), o_done = cv.take(B * 4), o_forced = cv.take(TC * 4), o_pos = cv.take(4);
    const size_t o_stk = cv.take(4);
    const size_t o_m1 = cv.take((D.vocab / 32 + 1) * 4), o_m2 = cv.take((D.vocab / 32 + 1) * 4);
    const size_t o_ns = cv.take(B * 4), o_nf = cv.take(B * 4), o_si = cv.take(B * 4), o_fs = cv.take(B * 4), o_gm = cv.take(B * 4);
    const size_t o_lsel = cv.take(B * 4);
    c->ws_bytes = cv.off;
    hipError_t he = hipMalloc((void**)&c->ws, c->ws_bytes);
    if (he != hipSuccess) { delete c; return wh_fail_hip(he, "hipMalloc(workspace)", __FILE__, __LINE__); }
    he = hipMemset(c->ws, 0, c->ws_bytes);  // conv zero rows, V^T key padding, caches
    if (he != hipSuccess) { hipFree(c->ws); delete c; return wh_fail_hip(he, "hipMemset(workspace)", __FILE__, __LINE__); }
    char* w = c->ws;
    c->pcm = (float*)(w + o_pcm); c->raw = (float*)(w + o_raw); c->mel_stage = (float*)(w + o_melstage);
    c->melT = w + o_melT; c->h1 = w + o_h1; c->x = (float*)(w + o_x); c->xn = w + o_xn; c->qk = w + o_qk;
    c->vT = w + o_vT; c->att = w + o_att; c->hbuf = c->enc_mlp ? nullptr : w + o_h; c->enc_out = w + o_enc; c->enc_out_f32 = (float*)(w + o_encf);
    c->cross_kv = w + o_ckv; c->self_k = w + o_sk; c->self_v = w + o_sv;
    if (f8kv) { c->cross_kv8 = w + o_ckv8; c->kv_amax = (float*)(w + o_kvam); }
    if (c->cross_es) { c->es_E = w + o_ckv; c->cross_kv = nullptr; c->dqe = (float*)(w + o_dqe); c->dctx = w + o_dctx; c->dq32 = (float*)(w + o_dq32); }
    if (c->enc_fold) { c->xb = w + o_xb; c->enc_part = (float*)(w + o_epart); c->enc_stat = (float*)(w + o_estat); c->enc_shift = (float*)(w + o_eshift); c->enc_shift0 = (float*)(w + o_eshift0); }
    if (c->enc_fold) {   // the first producer's row offsets: the mean of each position's row of the positional table, for every clip of a batch
        std::vector<float> pm(S), all(B * S);
        const float* pos = m->master.data() + m->index.at("model.encoder.embed_positions.weight").first;
        for (size_t r = 0; r < S; r++) {
            double acc = 0.0;
            for (size_t k = 0; k < d; k++) acc += (double)pos[r * d + k];
            pm[r] = (float)(acc / (double)d);
        }
        for (size_t b = 0; b < B; b++) memcpy(all.data() + b * S, pm.data(), S * 4);
        he = hipMemcpy(c->enc_shift0, all.data(), all.size() * 4, hipMemcpyHostToDevice);
        if (he != hipSuccess) { hipFree(c->ws); delete c; return wh_fail_hip(he, "hipMemcpy(row offsets)", __FILE__, __LINE__); }
    }
    if (c->mx_ok) {
        c->xn8 = (unsigned char*)(w + o_xn8); c->xn8_sc = (unsigned char*)(w + o_xn8s);
        c->h8 = (unsigned char*)(w + o_h8); c->h8_sc = (unsigned char*)(w + o_h8s);
    }
    c->dx = (float*)(w + o_dx); c->dxn = w + o_dxn; c->dxs = w + o_dxs; c->lnpart = (float*)(w + o_lnp); c->dshift = (float*)(w + o_dsh); c->dqkv = w + o_dqkv; c->datt = w + o_datt; c->dq = w + o_dq; c->dh = w + o_dh;
    c->cpart = (float*)(w + o_cpart); c->cml = (float*)(w + o_cml); c->part_val = (float*)(w + o_pv); c->part_idx = (int*)(w + o_pi);
    c->feed = (int*)(w + o_feed); c->out_tokens = (int*)(w + o_out); c->n_out = (int*)(w + o_nout); c->done = (int*)(w + o_done);
    c->forced = (int*)(w + o_forced); c->pos = (int*)(w + o_pos);
    c->step_ticket = (int*)(w + o_stk);
    c->mask_first = (unsigned*)(w + o_m1); c->mask_base = (unsigned*)(w + o_m2);
    c->d_nsamp = (int*)(w + o_ns); c->d_nframes = (int*)(w + o_nf); c->d_src_index = (int*)(w + o_si);
    c->d_frame_start = (int*)(w + o_fs); c->d_gmax = (unsigned*)(w + o_gm);
    c->logits_sel = (int*)(w + o_lsel);
    // streams: one for everything, or — chip partition — the token loop on `stream` and log-mel + encoder on `s_enc`, each
    // optionally confined to a set of compute units (hipExtStreamCreateWithCUMask: bit i of the mask is compute unit
    // i / 8 of XCD i % 8 on this part, tools/cu_mask_probe.hip)
    if (dec_masked) he = hipExtStreamCreateWithCUMask(&c->stream, (uint32_t)opts->dec_cu_mask_words, opts->dec_cu_mask);
    else he = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (he != hipSuccess) { hipFree(c->ws); delete c; return wh_fail_hip(he, "hipStreamCreate", __FILE__, __LINE__); }
    c->s_enc = c->stream;
    if (opts->enc_cu_mask_words || (opts->flags & WH_CTX_TWO_STREAMS)) {
        if (enc_masked) he = hipExtStreamCreateWithCUMask(&c->s_enc, (uint32_t)opts->enc_cu_mask_words, opts->enc_cu_mask);
        else he = hipStreamCreateWithFlags(&c->s_enc, hipStreamNonBlocking);
        if (he != hipSuccess) { hipStreamDestroy(c->stream); hipFree(c->ws); delete c; return wh_fail_hip(he, "hipStreamCreate(encoder stream)", __FILE__, __LINE__); }
    }
    c->cur = c->stream;
    for (auto& e : c->ev) hipEventCreate(&e);
    for (auto& set : c->enc_ev)
        for (auto& e : set) hipEventCreate(&e);
    hipEventCreateWithFlags(&c->ev_enc_done, hipEventDisableTiming);
    hipEventCreateWithFlags(&c->ev_kv_done, hipEventDisableTiming);
    *out = c;
    return WH_OK;
}

// ---- where the workspace lies -------------------------------------------------------------------------------------------------------------------
// The token loop's dominant kernel (cross-attention on the encoder states: 256 workgroups, each streaming its clips' states) runs in one of
// two states that differ by ~9 % — 474-483 or 515-528 us per 2048-clip bf16 launch — and the state follows the PLACEMENT of the workspace, not the
// process, the context or the virtual address: consecutive processes of a box alternate, and inside one process a context re-created while a
// placeholder holds the old one's memory flips every time (tools/es_place_probe.py, profiles/r04_cross_es_placement.txt).  User space cannot ask
// for a placement, but it can look and move: contexts that run that kernel at a thousand clips and more time it on their fresh (zeroed) workspace
// and, when its stream rate reads below WH_PLACE_FRAC (default 0.80; 0.835 in the split-fp16 mode) of 8 TB/s, build further contexts (up to
// WH_PLACE_TRIES = 3 in all) while the earlier ones still hold their memory, time each and keep the fastest.  Costs the extra workspaces for a
// moment (a try that does not fit ends the search) and about a second of start-up each.  WH_PLACE=0 turns the step off.
static float probe_cross_es_us(wh_ctx* c) {
    const wh_dims& D = c->m->dims;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return -1.0f;
    const int nb = c->max_batch, reps = 8;
    hipDeviceSynchronize();   // the workspace's zero fill (null stream; c->stream does not wait for it) must not share HBM with the launches timed here
    for (int i = 0; i < 3; i++) wh_launch_dec_cross_attn_es(c->stream, c->m->prec, c->dqe, c->es_E, c->dctx, D.n_audio_ctx, c->es_rows, nb, c->mpad, true, c->dec_cus);
    hipEventRecord(e0, c->stream);
    for (int i = 0; i < reps; i++) wh_launch_dec_cross_attn_es(c->stream, c->m->prec, c->dqe, c->es_E, c->dctx, D.n_audio_ctx, c->es_rows, nb, c->mpad, true, c->dec_cus);
    hipEventRecord(e1, c->stream);
    float ms = -1.0f;
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) ms = -1.0f;
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    return ms < 0.0f ? -1.0f : ms * 1e3f / reps;
}

int wh_ctx_create_ex(wh_model* m, const wh_ctx_opts* opts, wh_ctx** out) {
    const int rc = ctx_create_impl(m, opts, out);
    if (rc != WH_OK) return rc;
    wh_ctx* c = *out;
    c->place_tries = 0;
    const char* off = getenv("WH_PLACE");
    if (!c->cross_es || c->max_batch < 1024 || (off && atoi(off) == 0)) return WH_OK;
    const float t1 = probe_cross_es_us(c);
    if (t1 <= 0.0f) return WH_OK;
    c->place_tries = 1;
    c->place_us_first = c->place_us_kept = t1;
    const bool es3 = m->prec == WH_PREC_F16X3 && wh_es3_enabled();
    const double bytes = (double)c->max_batch * c->es_rows * m->dims.d_model * (es3 ? 3.0 : m->prec == WH_PREC_F16X3 ? 4.0 : m->prec == WH_PREC_FP8 ? 1.0 : 2.0);
    const char* fe = getenv("WH_PLACE_FRAC");
    // (between the two states as the probe sees them: bf16 0.75-0.77 / 0.82-0.84 of the roof, fp16 limb planes 0.79-0.82 / 0.84-0.86)
    // (e4m3 states: 251 us per 2048-clip launch in one state, 268-270 in the other: 0.79 / 0.74 of the roof as the probe sees them)
    // (fp16 + e4m3 states: 745-770 us per 2048-clip launch in one state, ~836 in the other: 0.78-0.80 / 0.715 of the roof as the probe sees them)
    const double want = fe ? atof(fe) : (es3 ? 0.75 : m->prec == WH_PREC_F16X3 ? 0.835 : m->prec == WH_PREC_FP8 ? 0.77 : 0.80);
    if (bytes / (t1 * 1e-6) >= want * 8e12) return WH_OK;
    // further workspaces, each built while all earlier ones still hold their memory (so it lies somewhere else), until one reads fast or
    // WH_PLACE_TRIES (default 3) are timed or the next one does not fit; the fastest stays
    const char* te = getenv("WH_PLACE_TRIES");
    const int max_tries = te ? std::max(1, atoi(te)) : 3;
    wh_ctx* best = c;
    float t_best = t1;
    int tries = 1;
    std::vector<wh_ctx*> others;
    while (tries < max_tries) {
        wh_ctx* cn = nullptr;
        if (ctx_create_impl(m, opts, &cn) != WH_OK) {   // no room: what we have stays — and the failed allocation must not be found by a later hipGetLastError()
            (void)hipGetLastError();
            wh_set_error("%s", "");
            break;
        }
        const float tn = probe_cross_es_us(cn);
        tries++;
        if (tn > 0.0f && tn < 0.98f * t_best) {
            others.push_back(best);
            best = cn;
            t_best = tn;
        } else {
            others.push_back(cn);
        }
        if (bytes / (t_best * 1e-6) >= want * 8e12) break;
    }
    for (wh_ctx* o : others) wh_ctx_free(o);
    best->place_tries = tries;
    best->place_us_first = t1;
    best->place_us_kept = t_best;
    *out = best;
    return WH_OK;
}

int wh_ctx_placement(const wh_ctx* c, float* first_us, float* kept_us) {
    if (!c) return -1;
    if (first_us) *first_us = c->place_us_first;
    if (kept_us) *kept_us = c->place_us_kept;
    return c->place_tries;
}

// An option setter's buffer: `bytes` zeroed bytes on the context's device, or nullptr with the setter's error recorded (the caller returns
// WH_ERR_NOMEM).
static void* setter_alloc(wh_ctx* c, const char* setter, size_t bytes) {
    hipSetDevice(c->m->device);
    void* buf = nullptr;
    hipError_t e = hipMalloc(&buf, bytes);
    if (e == hipSuccess) e = hipMemset(buf, 0, bytes);
    if (e == hipSuccess) return buf;
    if (buf) hipFree(buf);
    fail(c, WH_ERR_NOMEM, "%s: hipMalloc: %s", setter, hipGetErrorString(e));
    return nullptr;
}

// Whisper's timestamp rules on every decode entry of the ctx.  The buffers — the rows' timestamp logits and a per-row state —
// are allocated when rules are turned on (the logits again for another timestamp_begin); the captured decode step is recaptured when the
// key changes (and before a buffer it holds is freed).
int wh_ctx_set_timestamp_rules(wh_ctx* c, const wh_timestamp_rules* r) {
    if (!c) return WH_ERR_ARG;
    if (!r) {
        c->ts_on = false;
        return WH_OK;
    }
    if (r->struct_size != sizeof(wh_timestamp_rules)) return fail(c, WH_ERR_ARG, "wh_ctx_set_timestamp_rules: struct_size %zu, expected %zu", r->struct_size, sizeof(wh_timestamp_rules));
    const int vocab = c->m->dims.vocab;
    if (r->timestamp_begin <= 0 || r->timestamp_begin >= vocab)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_timestamp_rules: timestamp_begin %lld outside the vocabulary (%d)", (long long)r->timestamp_begin, vocab);
    if (r->no_timestamps >= vocab || r->no_timestamps < -1)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_timestamp_rules: no_timestamps %lld outside the vocabulary", (long long)r->no_timestamps);
    const int ld = vocab - (int)r->timestamp_begin;
    if (!c->ts_logits || c->ts_ld != ld) {
        float* tl = (float*)setter_alloc(c, "wh_ctx_set_timestamp_rules", (size_t)c->mpad * ld * 4);
        int* st = c->ts_state ? c->ts_state : (int*)(tl ? setter_alloc(c, "wh_ctx_set_timestamp_rules", (size_t)c->mpad * 16) : nullptr);
        if (!tl || !st) {
            if (tl) hipFree(tl);
            return WH_ERR_NOMEM;
        }
        drop_step_graph(c);   // (a captured step may hold the old buffer's address)
        if (c->ts_logits) hipFree(c->ts_logits);
        c->ts_logits = tl; c->ts_ld = ld; c->ts_state = st;
    }
    c->ts_on = true;
    c->ts_begin = r->timestamp_begin;
    c->ts_no_ts = r->no_timestamps;
    // (a bound past the vocabulary is no bound: clamped to the last timestamp, so tb + max_init never overflows in the kernels)
    c->ts_max_init = r->max_initial_timestamp_index < 0 ? -1 : std::min<int>(r->max_initial_timestamp_index, vocab - 1 - (int)r->timestamp_begin);
    return WH_OK;
}

// Token log-probabilities and the no-speech probe on every decode entry of the ctx.  The buffers are allocated the first
// time it is turned on; the captured decode step is keyed on the setting (other kernels, one more argument).
int wh_ctx_set_logprobs(wh_ctx* c, const wh_logprob_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->lp_on = false;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_logprob_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_logprobs: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_logprob_opts));
    const int vocab = c->m->dims.vocab;
    if (o->no_speech < -1 || o->no_speech >= vocab) return fail(c, WH_ERR_ARG, "wh_ctx_set_logprobs: no_speech %lld outside the vocabulary (%d)", (long long)o->no_speech, vocab);
    if (o->sot_index < 0) return fail(c, WH_ERR_ARG, "wh_ctx_set_logprobs: negative sot_index");
    if (!c->lp_buf) {
        auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
        const size_t MP = (size_t)c->mpad, B = (size_t)c->max_batch, n_tiles = ((size_t)vocab + 15) / 16;
        const size_t b_sum = up(MP * (n_tiles + 4) * 4), b_tok = up(B * c->tok_ld * 4), b_mask = up(((size_t)vocab / 32 + 1) * 4), b_pv = up(MP * 4), b_ns = up(B * 4);
        char* buf = (char*)setter_alloc(c, "wh_ctx_set_logprobs", b_sum + b_tok + b_mask + b_pv + b_ns);
        if (!buf) return WH_ERR_NOMEM;
        c->lp_buf = buf;
        c->lp_part_sum = (float*)buf;
        c->lp_tok = (float*)(buf + b_sum);
        c->lp_mask_zero = (unsigned*)(buf + b_sum + b_tok);
        c->lp_probe_v = (float*)(buf + b_sum + b_tok + b_mask);
        c->lp_ns = (float*)(buf + b_sum + b_tok + b_mask + b_pv);
    }
    c->lp_on = true;
    c->lp_no_speech = o->no_speech;
    c->lp_sot_index = o->sot_index;
    return WH_OK;
}

// Repetition penalty and no-repeat n-grams on every decode entry of the ctx.  The bitmap and the side buffer are allocated when
// the option is turned on and freed when it is cleared ({1.0f, 0} clears it); the captured decode step is keyed on the setting and dropped
// before a buffer it holds is freed.
static void rep_release(wh_ctx* c) {
    if (c->rep_bits || c->rep_side) drop_step_graph(c);   // (a captured step may hold the buffers' addresses)
    if (c->rep_bits) hipFree(c->rep_bits);
    if (c->rep_side) hipFree(c->rep_side);
    c->rep_bits = nullptr; c->rep_side = nullptr;
    c->rep_on = false; c->rep_p = 1.0f; c->rep_n = 0;
}
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
        hipSetDevice(c->m->device);
        rep_release(c);
        return WH_OK;
    }
    if (!c->rep_bits) {
        const size_t vocab = (size_t)c->m->dims.vocab, words = (vocab + 31) / 32, B = (size_t)c->max_batch;
        unsigned* bits = (unsigned*)setter_alloc(c, "wh_ctx_set_repetition", B * words * 4);
        float* side = (float*)(bits ? setter_alloc(c, "wh_ctx_set_repetition", B * vocab * 4) : nullptr);
        if (!side) {
            if (bits) hipFree(bits);
            return WH_ERR_NOMEM;
        }
        c->rep_bits = bits; c->rep_side = side; c->rep_words = (int)words;
    }
    c->rep_on = true;
    c->rep_p = o->repetition_penalty;
    c->rep_n = o->no_repeat_ngram_size;
    return WH_OK;
}

// Language detection on every decode entry of the ctx.  The buffers are allocated the first time it is turned on; nothing of
// it enters the captured decode step.
int wh_ctx_set_language_detection(wh_ctx* c, const wh_language_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->lang_on = false;
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
    char* buf = c->lang_buf;
    auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    const size_t MP = (size_t)c->mpad, B = (size_t)c->max_batch;
    const size_t b_ids = up(WH_LANG_LD * 4), b_log = up(MP * WH_LANG_LD * 4), b_pr = up(B * WH_LANG_LD * 4), b_ch = up(B * 4);
    if (!buf && !(buf = (char*)setter_alloc(c, "wh_ctx_set_language_detection", b_ids + b_log + b_pr + b_ch))) return WH_ERR_NOMEM;
    int ids[WH_LANG_LD];
    for (int i = 0; i < WH_LANG_LD; i++) ids[i] = (int)o->lang_ids[(size_t)i < o->n_lang ? i : 0];
    hipError_t e = hipMemcpy(buf, ids, sizeof ids, hipMemcpyHostToDevice);   // (nothing of the ctx is in flight: every call ends with a stream synchronisation)
    if (e != hipSuccess) {
        if (!c->lang_buf) hipFree(buf);
        else if (c->lang_on) {   // put the list in force back
            for (int i = 0; i < WH_LANG_LD; i++) ids[i] = (int)c->lang_ids[(size_t)i < c->lang_ids.size() ? i : 0];
            hipMemcpy(buf, ids, sizeof ids, hipMemcpyHostToDevice);
        }
        return fail(c, WH_ERR_HIP, "wh_ctx_set_language_detection: hipMemcpy: %s", hipGetErrorString(e));
    }
    c->lang_buf = buf;
    c->lang_d_ids = (int*)buf;
    c->lang_logits = (float*)(buf + b_ids);
    c->lang_probs = (float*)(buf + b_ids + b_log);
    c->lang_chosen = (int*)(buf + b_ids + b_log + b_pr);
    c->lang_ids.assign(o->lang_ids, o->lang_ids + o->n_lang);
    c->lang_sot_index = o->sot_index;
    c->lang_on = true;
    return WH_OK;
}

// Per-clip prompt prefixes on every decode entry of the ctx.  The setter copies the ids; the per-row offsets are computed and
// uploaded by each call (run_decode).
int wh_ctx_set_prefixes(wh_ctx* c, const wh_prefix_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->pfx_on = false;
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
    if (!c->pfx_off) {
        if (!(c->pfx_off = (int*)setter_alloc(c, "wh_ctx_set_prefixes", (size_t)c->max_batch * 4))) return WH_ERR_NOMEM;
    }
    c->pfx_ids.assign(o->ids, o->ids + n_ids);
    c->pfx_offsets.assign(o->offsets, o->offsets + o->n_clips + 1);
    c->pfx_scope = o->longform_scope;
    c->pfx_on = true;
    return WH_OK;
}

// Word-level timestamps on every decode entry of the ctx.  The setter copies the head list and allocates the frames; the side
// buffer of the queries and the post-pass workspace are sized by the calls.  The captured decode step is keyed on the list's identity.
int wh_ctx_set_alignment(wh_ctx* c, const wh_alignment_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        c->al_on = false;
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_alignment_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_alignment: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_alignment_opts));
    const wh_dims& D = c->m->dims;
    if (o->n_heads < 1 || o->n_heads > WH_MAX_ALIGN_HEADS || !o->heads) return fail(c, WH_ERR_ARG, "wh_ctx_set_alignment: n_heads %zu outside 1..%d (or a NULL list)", o->n_heads, WH_MAX_ALIGN_HEADS);
    if (o->n_debug_rows > WH_MAX_ALIGN_DEBUG_ROWS || (o->n_debug_rows && !o->debug_rows)) return fail(c, WH_ERR_ARG, "wh_ctx_set_alignment: more than %d debug rows (or a NULL list)", WH_MAX_ALIGN_DEBUG_ROWS);
    for (size_t i = 0; i < o->n_heads; i++) {
        const int l = o->heads[2 * i], h = o->heads[2 * i + 1];
        if (l < 0 || l >= D.dec_layers || h < 0 || h >= D.n_heads) return fail(c, WH_ERR_ARG, "wh_ctx_set_alignment: (layer %d, head %d) outside the model (%d layers, %d heads)", l, h, D.dec_layers, D.n_heads);
        for (size_t j = 0; j < i; j++)
            if (o->heads[2 * j] == l && o->heads[2 * j + 1] == h) return fail(c, WH_ERR_ARG, "wh_ctx_set_alignment: (layer %d, head %d) listed twice", l, h);
    }
    for (size_t i = 0; i < o->n_debug_rows; i++)
        if (o->debug_rows[i] < 0) return fail(c, WH_ERR_ARG, "wh_ctx_set_alignment: negative debug row");
    if (!c->al_frames) {
        int* fr = (int*)setter_alloc(c, "wh_ctx_set_alignment", (size_t)c->max_batch * D.n_text_ctx * 4);
        int* sb = (int*)(fr ? setter_alloc(c, "wh_ctx_set_alignment", (size_t)c->max_batch * 4) : nullptr);
        if (!sb) {
            if (fr) hipFree(fr);
            return WH_ERR_NOMEM;
        }
        c->al_frames = fr; c->al_sb = sb;
    }
    c->al_heads.assign(o->heads, o->heads + 2 * o->n_heads);
    c->al_debug.assign(o->debug_rows, o->debug_rows + o->n_debug_rows);
    c->al_layer.assign(D.dec_layers, AlignLayerHeads());
    for (size_t i = 0; i < o->n_heads; i++) {
        AlignLayerHeads& lh = c->al_layer[o->heads[2 * i]];
        lh.slot[lh.n] = (unsigned char)i;
        lh.head[lh.n] = (unsigned char)o->heads[2 * i + 1];
        lh.n++;
    }
    c->al_gen++;
    c->al_on = true;
    return WH_OK;
}

// Beam search on every decode entry of the ctx.  The logits scratch and the search state are allocated when the option is turned
// on and freed when it is cleared; the captured decode step is keyed on the setting and dropped before a buffer it holds is freed.
static void beam_release(wh_ctx* c) {
    if (c->bm_logits || c->bm_buf) drop_step_graph(c);   // (a captured step may hold the buffers' addresses)
    if (c->bm_logits) hipFree(c->bm_logits);
    if (c->bm_buf) hipFree(c->bm_buf);
    c->bm_logits = nullptr; c->bm_buf = nullptr;
    c->bm_on = false; c->bm_k = c->bm_c = 0;
    c->bm_trace_clips.clear();
}
int wh_ctx_set_beam_search(wh_ctx* c, const wh_beam_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        hipSetDevice(c->m->device);
        beam_release(c);
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
    if (!c->bm_logits) {
        auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
        const size_t B = (size_t)c->max_batch, vocab = (size_t)c->m->dims.vocab, TL = (size_t)c->tok_ld;
        const size_t b_row = up(B * 4), b_state = up(B * WH_BEAM_STATE * 4), b_pool = up(B * WH_MAX_BEAM_CANDIDATES * 4 * 4), b_tr = up(TL * B * 4);
        float* lg = (float*)setter_alloc(c, "wh_ctx_set_beam_search", B * vocab * 4);
        char* buf = (char*)(lg ? setter_alloc(c, "wh_ctx_set_beam_search", 4 * b_row + b_state + b_pool + 5 * b_tr) : nullptr);
        if (!buf) {
            if (lg) hipFree(lg);
            return WH_ERR_NOMEM;
        }
        c->bm_logits = lg; c->bm_buf = buf;
        char* q = buf;
        c->bm_scores = (float*)q; q += b_row;
        c->bm_parent = (int*)q; q += b_row;
        c->bm_pool_n = (int*)q; q += b_row;
        c->bm_n_steps = (int*)q; q += b_row;
        c->bm_state = (int*)q; q += b_state;
        c->bm_pool = (int*)q; q += b_pool;
        c->bm_tr_parent = (int*)q; q += b_tr;
        c->bm_tr_token = (int*)q; q += b_tr;
        c->bm_tr_pool = (int*)q; q += b_tr;
        c->bm_tr_score = (float*)q; q += b_tr;
        c->bm_tr_lp = (float*)q;
    }
    c->bm_on = true;
    c->bm_k = o->beam_size;
    c->bm_c = (int)cand;
    c->bm_length_penalty = o->length_penalty;
    c->bm_trace_clips.assign(o->trace_clips, o->trace_clips + o->n_trace_clips);
    return WH_OK;
}

// Temperature sampling on every decode entry of the ctx.  The logits scratch and the per-row buffers are allocated when the option
// is turned on and freed when it is cleared; the captured decode step is keyed on the buffers' identity and dropped before they are freed.  The
// per-row values reach the kernel through those buffers (upload_token_state), so another rung of a ladder replays the same captured step.
static void sample_release(wh_ctx* c) {
    if (c->sm_logits || c->sm_buf) drop_step_graph(c);   // (a captured step may hold the buffers' addresses)
    if (c->sm_logits) hipFree(c->sm_logits);
    if (c->sm_buf) hipFree(c->sm_buf);
    c->sm_logits = nullptr; c->sm_buf = nullptr;
    c->sm_on = false;
    c->sm_temp.clear(); c->sm_active.clear(); c->sm_ids.clear();
}
int wh_ctx_set_sampling(wh_ctx* c, const wh_sampling_opts* o) {
    if (!c) return WH_ERR_ARG;
    if (!o) {
        hipSetDevice(c->m->device);
        sample_release(c);
        return WH_OK;
    }
    if (o->struct_size != sizeof(wh_sampling_opts)) return fail(c, WH_ERR_ARG, "wh_ctx_set_sampling: struct_size %zu, expected %zu", o->struct_size, sizeof(wh_sampling_opts));
    if (o->n_rows < 1 || o->n_rows > (size_t)c->max_batch || !o->temperature)
        return fail(c, WH_ERR_ARG, "wh_ctx_set_sampling: n_rows %zu outside 1 .. max_batch (%d) (or a NULL temperature list)", o->n_rows, c->max_batch);
    for (size_t i = 0; i < o->n_rows; i++)
        if (!std::isfinite(o->temperature[i]) || o->temperature[i] < 0.0f)
            return fail(c, WH_ERR_ARG, "wh_ctx_set_sampling: temperature[%zu] = %g is negative or not finite", i, (double)o->temperature[i]);
    if (!c->sm_logits) {
        auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
        const size_t B = (size_t)c->max_batch, vocab = (size_t)c->m->dims.vocab, TL = (size_t)c->tok_ld;
        const size_t b_t = up(B * 4), b_id = up(B * 8), b_seed = up(8), b_state = up(B * 16), b_lp = up(B * TL * 4);
        float* lg = (float*)setter_alloc(c, "wh_ctx_set_sampling", B * vocab * 4);
        char* buf = (char*)(lg ? setter_alloc(c, "wh_ctx_set_sampling", b_t + b_id + b_seed + b_state + b_lp) : nullptr);
        if (!buf) {
            if (lg) hipFree(lg);
            return WH_ERR_NOMEM;
        }
        c->sm_logits = lg; c->sm_buf = buf;
        char* q = buf;
        c->sm_d_ids = (unsigned long long*)q; q += b_id;
        c->sm_d_seed = (unsigned long long*)q; q += b_seed;
        c->sm_d_temp = (float*)q; q += b_t;
        c->sm_state = (int*)q; q += b_state;
        c->sm_lp = (float*)q;
    }
    c->sm_on = true;
    c->sm_seed = o->seed;
    c->sm_temp.assign(o->temperature, o->temperature + o->n_rows);
    c->sm_active.assign(o->n_rows, 1);
    if (o->active) c->sm_active.assign(o->active, o->active + o->n_rows);
    c->sm_ids.resize(o->n_rows);
    for (size_t i = 0; i < o->n_rows; i++) c->sm_ids[i] = o->row_ids ? o->row_ids[i] : (uint64_t)i;
    return WH_OK;
}

int wh_get_beams(const wh_ctx* c, int64_t* tokens, size_t cap_tokens, size_t* n_tokens, float* sum_logprob, float* rank_score, int32_t* finished,
                 size_t cap_hyp, size_t* n_hyp, size_t cap_clips, size_t* n_clips_out) {
    if (!c) return WH_ERR_ARG;
    if (!c->bm_have) return WH_ERR_STATE;
    const size_t n = c->bm_hyps.size();
    if (n_clips_out) *n_clips_out = n;
    if (!tokens && !n_hyp) return WH_OK;
    if (cap_clips < n) return WH_ERR_ARG;
    for (size_t b = 0; b < n; b++) {
        const size_t nh = std::min(cap_hyp, c->bm_hyps[b].size());
        if (tokens)
            for (size_t h = 0; h < nh; h++)
                if (c->bm_hyps[b][h].tokens.size() > cap_tokens) return WH_ERR_ARG;
    }
    for (size_t b = 0; b < n; b++) {
        const size_t nh = std::min(cap_hyp, c->bm_hyps[b].size());
        if (n_hyp) n_hyp[b] = nh;
        for (size_t h = 0; h < cap_hyp; h++) {
            const size_t at = b * cap_hyp + h;
            const wh_ctx::BeamHyp* hy = h < nh ? &c->bm_hyps[b][h] : nullptr;
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
    if (!c->bm_have || c->bm_traces.empty()) return WH_ERR_STATE;
    if (k >= c->bm_traces.size()) return WH_ERR_ARG;
    const wh_ctx::BeamTrace& t = c->bm_traces[k];
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
    if (!c->al_have) return WH_ERR_STATE;
    const size_t n = c->al_rows.size();
    if (n_clips_out) *n_clips_out = n;
    if ((frames || n_frames) && cap_clips < n) return WH_ERR_ARG;
    if (frames) {
        for (size_t b = 0; b < n; b++)
            if (c->al_rows[b].size() > cap_tokens) return WH_ERR_ARG;
        for (size_t b = 0; b < n; b++) {
            std::fill(frames + b * cap_tokens, frames + (b + 1) * cap_tokens, 0);
            std::copy(c->al_rows[b].begin(), c->al_rows[b].end(), frames + b * cap_tokens);
        }
    }
    if (n_frames) std::copy(c->al_nframes.begin(), c->al_nframes.end(), n_frames);
    return WH_OK;
}

int wh_get_alignment_debug(const wh_ctx* c, size_t k, float* probs, float* matrix, size_t cap_floats, int32_t* shape3) {
    if (!c) return WH_ERR_ARG;
    if (!c->al_have || c->al_dbg.empty()) return WH_ERR_STATE;
    if (k >= c->al_dbg.size()) return WH_ERR_ARG;
    const wh_ctx::AlignDebug& d = c->al_dbg[k];
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
    if (!c->lang_have) return WH_ERR_STATE;
    const size_t n = c->lang_rows.size();
    if (n_clips_out) *n_clips_out = n;
    if (!lang_out) return WH_OK;
    if (cap_clips < n) return WH_ERR_ARG;
    std::copy(c->lang_rows.begin(), c->lang_rows.end(), lang_out);
    if (probs) std::copy(c->lang_prob_rows.begin(), c->lang_prob_rows.end(), probs);
    return WH_OK;
}

int wh_get_logprobs(const wh_ctx* c, float* token_logprobs, size_t cap_tokens, float* no_speech_prob, size_t cap_clips, size_t* n_clips_out) {
    if (!c) return WH_ERR_ARG;
    if (!c->lp_have) return WH_ERR_STATE;
    const size_t n = c->lp_rows.size();
    if (n_clips_out) *n_clips_out = n;
    if (no_speech_prob && !c->lp_have_ns) return WH_ERR_STATE;
    if ((token_logprobs || no_speech_prob) && cap_clips < n) return WH_ERR_ARG;
    if (token_logprobs) {
        for (size_t b = 0; b < n; b++)
            if (c->lp_rows[b].size() > cap_tokens) return WH_ERR_ARG;
        for (size_t b = 0; b < n; b++) {
            std::fill(token_logprobs + b * cap_tokens, token_logprobs + (b + 1) * cap_tokens, 0.0f);
            std::copy(c->lp_rows[b].begin(), c->lp_rows[b].end(), token_logprobs + b * cap_tokens);
        }
    }
    if (no_speech_prob) std::copy(c->lp_ns_rows.begin(), c->lp_ns_rows.end(), no_speech_prob);
    return WH_OK;
}

void wh_ctx_free(wh_ctx* c) {
    if (!c) return;
    hipSetDevice(c->m->device);
    if (c->s_enc && c->s_enc != c->stream) hipStreamSynchronize(c->s_enc);   // a prefetched encoder pass may be in flight
    if (c->stream) hipStreamSynchronize(c->stream);
    drop_step_graph(c);
    for (int g = 0; g < WH_KG_COUNT; g++)
        for (auto& e : c->prof_events[g]) { hipEventDestroy(e.first); hipEventDestroy(e.second); }
    for (auto& e : c->ev)
        if (e) hipEventDestroy(e);
    for (auto& set : c->enc_ev)
        for (auto& e : set)
            if (e) hipEventDestroy(e);
    if (c->ev_enc_done) hipEventDestroy(c->ev_enc_done);
    if (c->ev_kv_done) hipEventDestroy(c->ev_kv_done);
    if (c->s_enc && c->s_enc != c->stream) hipStreamDestroy(c->s_enc);
    if (c->stream) hipStreamDestroy(c->stream);
    if (c->ws) hipFree(c->ws);
    if (c->pcm_long) hipFree(c->pcm_long);
    if (c->raw_long) hipFree(c->raw_long);
    if (c->mel_out_long) hipFree(c->mel_out_long);
    if (c->logits) hipFree(c->logits);
    if (c->ts_logits) hipFree(c->ts_logits);
    if (c->ts_state) hipFree(c->ts_state);
    if (c->lp_buf) hipFree(c->lp_buf);
    if (c->lang_buf) hipFree(c->lang_buf);
    if (c->pfx_off) hipFree(c->pfx_off);
    if (c->rep_bits) hipFree(c->rep_bits);
    if (c->rep_side) hipFree(c->rep_side);
    if (c->al_q) hipFree(c->al_q);
    if (c->al_ws) hipFree(c->al_ws);
    if (c->al_frames) hipFree(c->al_frames);
    if (c->al_sb) hipFree(c->al_sb);
    if (c->bm_logits) hipFree(c->bm_logits);
    if (c->bm_buf) hipFree(c->bm_buf);
    for (auto& te : c->bm_events)
        for (auto& e : te) hipEventDestroy(e);
    if (c->sm_logits) hipFree(c->sm_logits);
    if (c->sm_buf) hipFree(c->sm_buf);
    for (auto& te : c->sm_events)
        for (auto& e : te) hipEventDestroy(e);
    if (c->s_copy) { hipStreamSynchronize(c->s_copy); hipStreamDestroy(c->s_copy); }
    if (c->ev_h2d) hipEventDestroy(c->ev_h2d);
    if (c->pcm2) hipFree(c->pcm2);
    for (void* r : c->ing_raw)
        if (r) hipFree(r);
    if (c->ing_desc) hipFree(c->ing_desc);
    delete c;
}

int wh_ctx_cross_mode(const wh_ctx* c) { return c ? (c->cross_es ? 1 : 0) : -1; }

// probe hook (tools/es_pitch_probe.py; not in the public header): rows of padding between the clips' encoder states, within the room
// WH_ES_PAD_MAX reserved at creation.  Addresses only — results do not depend on it.
extern "C" int wh_debug_set_es_pad(wh_ctx* c, int pad_rows) {
    if (!c || !c->cross_es || pad_rows < 0 || c->m->dims.n_audio_ctx + pad_rows > c->es_rows_cap) return WH_ERR_ARG;
    c->es_rows = c->m->dims.n_audio_ctx + pad_rows;
    c->have_enc = false;
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
    if (!c || !ms3 || !c->al_timing) return WH_ERR_ARG;
    for (int i = 0; i < 3; i++) ms3[i] = c->al_ms[i];
    return WH_OK;
}

// measurement hook (tools/beam_bench.py; not in the public header): milliseconds of k_beam_select and k_beam_reorder of the last call, summed over
// the positions that were launched eagerly (their count in *positions) — filled when the context was created under WH_BEAM_TIMING=1
extern "C" int wh_debug_beam_times(const wh_ctx* c, double* ms2, long* positions) {
    if (!c || !ms2 || !positions || !c->bm_timing) return WH_ERR_ARG;
    ms2[0] = c->bm_ms[0]; ms2[1] = c->bm_ms[1];
    *positions = c->bm_timed;
    return WH_OK;
}

// measurement hook (tools/sample_bench.py; not in the public header): milliseconds of k_sample_select of the last call, summed over the positions
// that were launched eagerly (their count in *positions) — filled when the context was created under WH_SAMPLE_TIMING=1
extern "C" int wh_debug_sample_times(const wh_ctx* c, double* ms, long* positions) {
    if (!c || !ms || !positions || !c->sm_timing) return WH_ERR_ARG;
    *ms = c->sm_ms;
    *positions = c->sm_timed;
    return WH_OK;
}

const char* wh_last_error(const wh_ctx* c) { return c ? c->err.c_str() : wh_global_error().c_str(); }

int wh_get_timings(const wh_ctx* c, wh_timing* out) {
    if (!c || !out) return WH_ERR_ARG;
    *out = c->timing;
    return WH_OK;
}

int wh_profile_enable(wh_ctx* c, int group_mask) {
    if (!c) return WH_ERR_ARG;
    c->prof = (group_mask & 0xFFFF) != 0;
    c->prof_mask = group_mask & 0xFFFF;
    c->prof_stride = (group_mask >> 16) & 0xFFFF;
    return WH_OK;
}
int wh_profile_get(const wh_ctx* c, double* ms, int64_t* launches) {
    if (!c || !ms || !launches) return WH_ERR_ARG;
    for (int g = 0; g < WH_KG_COUNT; g++) { ms[g] = c->prof_ms[g]; launches[g] = c->prof_launches[g]; }
    return WH_OK;
}

// grow the whole-file buffers to hold n samples / nf frames
static int ensure_long(wh_ctx* c, size_t n, size_t nf) {
    const size_t C = c->m->dims.n_mels;
    if (n > c->pcm_cap) {
        if (c->pcm_long) hipFree(c->pcm_long);
        c->pcm_long = nullptr; c->pcm_cap = 0;
        CTX_HIP(c, hipMalloc((void**)&c->pcm_long, n * 4));
        c->pcm_cap = n;
    }
    const size_t nfp = align_up(nf, 16);
    if (nfp > c->raw_long_cap) {
        if (c->raw_long) hipFree(c->raw_long);
        if (c->mel_out_long) hipFree(c->mel_out_long);
        c->raw_long = c->mel_out_long = nullptr; c->raw_long_cap = 0;
        CTX_HIP(c, hipMalloc((void**)&c->raw_long, C * nfp * 4));
        CTX_HIP(c, hipMalloc((void**)&c->mel_out_long, C * nfp * 4));
        c->raw_long_cap = nfp;
    }
    return WH_OK;
}

// grow raw staging buffer `k` to `bytes`.  A failed allocation leaves the ctx as it was, with no sticky HIP error.
static int ensure_ingest(wh_ctx* c, int k, size_t bytes) {
    if (!c->ing_desc) {
        void* d = nullptr;
        const hipError_t e = hipMalloc(&d, (size_t)c->max_batch * sizeof(WhIngestDesc));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, WH_ERR_NOMEM, "raw audio descriptors: hipMalloc: %s", hipGetErrorString(e));
        }
        c->ing_desc = (WhIngestDesc*)d;
    }
    if (bytes <= c->ing_raw_cap[k]) return WH_OK;
    void* nb = nullptr;
    const hipError_t e = hipMalloc(&nb, bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();   // (the old, smaller buffer is kept)
        return fail(c, WH_ERR_NOMEM, "raw audio staging (%zu bytes): hipMalloc: %s", bytes, hipGetErrorString(e));
    }
    if (c->ing_raw[k]) hipFree(c->ing_raw[k]);
    c->ing_raw[k] = nb;
    c->ing_raw_cap[k] = bytes;
    return WH_OK;
}

// the refusals of the raw entries (include/whisper_hip.h), before anything is launched; max_out: the longest resampled clip allowed
static int check_raw_clips(wh_ctx* c, const wh_raw_clip* clips, size_t n, size_t max_out, const char* too_long) {
    for (size_t i = 0; i < n; i++) {
        if (const char* why = wh_raw_clip_problem(clips[i])) return fail(c, WH_ERR_ARG, "clip %zu: %s", i, why);
        if (clips[i].n_frames > ((size_t)1 << 40)) return fail(c, WH_ERR_ARG, "clip %zu: more than 2^40 frames", i);
    }
    for (size_t i = 0; i < n; i++) {
        const size_t no = wh_resampled_len(clips[i].n_frames, clips[i].sample_rate);
        if (clips[i].n_frames == 0 || no == 0) return fail(c, WH_ERR_EMPTY_AUDIO, "Empty audio");   // src/main.rs:414-416
        if (no > max_out) return fail(c, WH_ERR_ARG, "clip %zu %s", i, too_long);
    }
    return WH_OK;
}

// the batch's raw bytes -> staging buffer k on stream s
static int copy_raw_clips(wh_ctx* c, const wh_raw_clip* clips, const WhIngestPlan& plan, int k, hipStream_t s) {
    for (size_t i = 0; i < plan.desc.size(); i++)
        CTX_HIP(c, hipMemcpyAsync((char*)c->ing_raw[k] + plan.desc[i].raw_off, clips[i].data, plan.bytes[i], hipMemcpyHostToDevice, s));
    return WH_OK;
}

// whole-file raw log-mel into c->raw_long (row stride = align16(frames)); returns frames
// `raw` (optional): the file as it was read; it is converted into c->pcm_long on the device instead of copying `pcm`
static int whole_file_mel(wh_ctx* c, const float* pcm, size_t n, size_t* nf_out, size_t* ld_out, const wh_raw_clip* raw = nullptr,
                          double* h2d_s_out = nullptr) {
    if (n == 0) return fail(c, WH_ERR_EMPTY_AUDIO, "Empty audio");  // src/main.rs:414-416
    if (!pcm && !raw) return fail(c, WH_ERR_ARG, "pcm is NULL");
    if (n > 0x7fffffffu) return fail(c, WH_ERR_ARG, "audio longer than 2^31 samples");
    const size_t nf = wh_mel_frames(n), ld = align_up(nf, 16);
    int rc = ensure_long(c, n, nf);
    if (rc) return rc;
    rc = enc_begin(c);
    if (rc) return rc;
    hipStream_t s = c->s_enc;
    const int ni = (int)n, nfi = (int)nf;
    const double t_copy = now_s();
    WhIngestPlan plan;
    if (raw) {
        wh_ingest_pack(raw, 1, 0, plan);
        CTX_HIP(c, hipMemcpyAsync(c->ing_raw[0], raw->data, plan.bytes[0], hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->ing_desc, plan.desc.data(), sizeof(WhIngestDesc), hipMemcpyHostToDevice, s));
    } else {
        CTX_HIP(c, hipMemcpyAsync(c->pcm_long, pcm, n * 4, hipMemcpyHostToDevice, s));
    }
    CTX_HIP(c, hipMemcpyAsync(c->d_nsamp, &ni, 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->d_nframes, &nfi, 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemsetAsync(c->d_gmax, 0, 4, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    if (h2d_s_out) *h2d_s_out = now_s() - t_copy;
    if (raw) {
        Prof p(c, WH_KG_MEL);
        wh_launch_ingest(s, c->ing_raw[0], c->ing_desc, 1, plan.max_out, c->pcm_long);
    }
    {
        Prof p(c, WH_KG_MEL);
        wh_launch_mel_stft(s, c->pcm_long, 0, c->d_nsamp, 1, (long)nf, c->m->mel_tw, c->m->mel_win, c->m->mel_fbT,
                           c->m->dims.n_mels, c->raw_long, 0, (long)ld, c->d_gmax);
    }
    *nf_out = nf;
    *ld_out = ld;
    return WH_OK;
}

int wh_log_mel(wh_ctx* c, const float* pcm, size_t n, float* mel_out, size_t cap_frames, size_t* n_frames_out) {
    if (!c) return WH_ERR_ARG;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    size_t nf = 0, ld = 0;
    int rc = whole_file_mel(c, pcm, n, &nf, &ld);
    if (rc) return rc;
    if (n_frames_out) *n_frames_out = nf;
    if (!mel_out || cap_frames < nf) return fail(c, WH_ERR_ARG, "mel_out too small: %zu frames needed", nf);
    hipStream_t s = c->s_enc;
    wh_launch_mel_norm(s, c->raw_long, (long)ld, c->d_gmax, c->m->dims.n_mels, (long)nf, c->mel_out_long);
    CTX_HIP(c, hipMemcpyAsync(mel_out, c->mel_out_long, (size_t)c->m->dims.n_mels * nf * 4, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    c->timing = wh_timing{};
    c->timing.preprocess_s = c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

int wh_encode(wh_ctx* c, const float* mel, float* enc_out) {
    if (!c) return WH_ERR_ARG;
    if (!mel) return fail(c, WH_ERR_BAD_SHAPE, "wh_encode: mel is NULL (expected [n_mels][3000])");
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    const wh_dims& D = c->m->dims;
    int rc = enc_begin(c);
    if (rc) return rc;
    hipStream_t s = c->s_enc;
    c->pre_valid = false;   // the resident encoder states are replaced
    const int nf = WH_N_FRAMES;
    CTX_HIP(c, hipMemcpyAsync(c->mel_stage, mel, (size_t)D.n_mels * WH_N_FRAMES * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->d_nframes, &nf, 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipEventRecord(c->ev[1], s));
    if (c->m->esz == 4)
        wh_launch_mel_tokens<float>(s, c->mel_stage, 0, WH_N_FRAMES, nullptr, nullptr, c->d_nframes, nullptr, 1, D.n_mels, 1,
                                    (float*)c->melT, (long)TOK_ROWS * D.n_mels);
    else
        wh_launch_mel_tokens<bf16>(s, c->mel_stage, 0, WH_N_FRAMES, nullptr, nullptr, c->d_nframes, nullptr, 1, D.n_mels, 1,
                                   (bf16*)c->melT, (long)TOK_ROWS * D.n_mels);
    rc = run_encoder(c, 1, enc_out != nullptr);
    if (rc) return rc;
    c->enc_nframes.assign(1, WH_N_FRAMES);
    CTX_HIP(c, hipEventRecord(c->ev[2], s));
    if (enc_out)
        CTX_HIP(c, hipMemcpyAsync(enc_out, c->enc_out_f32, (size_t)D.n_audio_ctx * D.d_model * 4, hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[1], c->ev[2]);
    c->timing = wh_timing{};
    c->timing.encode_s = ms * 1e-3;
    c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

// stage times of a decode-only call (run_decode brackets the decode with ev[5] .. ev[3])
static void decode_only_timing(wh_ctx* c, double t0) {
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[5], c->ev[3]);
    const double d2h = c->timing.d2h_s;
    c->timing = wh_timing{};
    c->timing.decode_s = ms * 1e-3;
    c->timing.d2h_s = d2h;
    c->timing.total_s = now_s() - t0;
    prof_collect(c);
}

int wh_decode_greedy(wh_ctx* c, const wh_decode_params* p, int64_t* tokens_out, size_t cap_tokens, size_t* n_tokens_out,
                     float* logits_out, size_t cap_logits_rows) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!c->have_enc) return fail(c, WH_ERR_STATE, "Missing cached decoder input: encoder states (call wh_encode first)");
    if (c->pre_valid) return fail(c, WH_ERR_STATE, "the resident encoder states belong to a prefetched batch that has not been transcribed yet");
    if (!tokens_out || !n_tokens_out || cap_tokens < p->n_prompt + p->max_new_tokens)
        return fail(c, WH_ERR_ARG, "tokens_out needs capacity n_prompt + max_new_tokens");
    if (logits_out && cap_logits_rows < p->max_new_tokens) return fail(c, WH_ERR_ARG, "logits_out needs max_new_tokens rows");
    // (beam search: the logits belong to beam_size physical rows, and this entry's logits_out holds one — read them through wh_decode_greedy_rows)
    if (logits_out && c->bm_on && c->bm_k > 1)
        return fail(c, WH_ERR_ARG, "wh_decode_greedy: logits_out holds one row's logits, beam search has %d rows per clip; use wh_decode_greedy_rows", c->bm_k);
    rc = prefix_check(c, p, 1, false);
    if (rc) return rc;
    if ((rc = align_check(c, 1)) || (rc = beam_check(c, p, 1)) || (rc = sample_check(c, 1, false))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    rc = run_decode(c, 1, p, tokens_out, cap_tokens, n_tokens_out, logits_out, p->max_new_tokens);
    if (rc) return rc;
    decode_only_timing(c, t0);
    return WH_OK;
}

int wh_decode_greedy_batch(wh_ctx* c, const wh_decode_params* p, int64_t* tokens_out, size_t cap_tokens, size_t* n_tokens_out,
                           size_t cap_clips, size_t* n_clips_out, float* logits_out, size_t cap_logits_rows) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!c->have_enc) return fail(c, WH_ERR_STATE, "Missing cached decoder input: encoder states (call wh_transcribe_batch or wh_encode first)");
    if (c->pre_valid) return fail(c, WH_ERR_STATE, "the resident encoder states belong to a prefetched batch that has not been transcribed yet");
    const int nb = c->enc_batch;
    if (n_clips_out) *n_clips_out = (size_t)nb;
    if (!tokens_out || !n_tokens_out || cap_clips < (size_t)nb || cap_tokens < p->n_prompt + p->max_new_tokens)
        return fail(c, WH_ERR_ARG, "tokens_out needs %d rows of capacity n_prompt + max_new_tokens", nb);
    if (logits_out && cap_logits_rows < p->max_new_tokens) return fail(c, WH_ERR_ARG, "logits_out needs max_new_tokens rows per clip");
    // (beam search: logits_out is [n * beam_size][cap_logits_rows][vocab], one block per physical row — cap_clips must cover them)
    if (logits_out && c->bm_on && cap_clips < (size_t)nb * c->bm_k)
        return fail(c, WH_ERR_ARG, "wh_decode_greedy_batch: with beam search logits_out holds %d clips x %d beams: cap_clips must be at least %d", nb, c->bm_k, nb * c->bm_k);
    rc = prefix_check(c, p, nb, false);
    if (rc) return rc;
    if ((rc = align_check(c, nb)) || (rc = beam_check(c, p, nb)) || (rc = sample_check(c, nb, false))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    rc = run_decode(c, nb, p, tokens_out, cap_tokens, n_tokens_out, logits_out, logits_out ? cap_logits_rows : 0);
    if (rc) return rc;
    decode_only_timing(c, t0);
    return WH_OK;
}

int wh_decode_greedy_rows(wh_ctx* c, const wh_decode_params* p, const int32_t* rows, size_t n_rows, int64_t* tokens_out, size_t cap_tokens,
                          size_t* n_tokens_out, size_t cap_clips, size_t* n_clips_out, float* logits_out, size_t cap_logits_rows) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!c->have_enc) return fail(c, WH_ERR_STATE, "Missing cached decoder input: encoder states (call wh_transcribe_batch or wh_encode first)");
    if (c->pre_valid) return fail(c, WH_ERR_STATE, "the resident encoder states belong to a prefetched batch that has not been transcribed yet");
    const int nb = c->enc_batch;
    if (n_clips_out) *n_clips_out = (size_t)nb;
    const size_t phys = (size_t)nb * (c->bm_on ? c->bm_k : 1);   // (beam search: rows address the physical rows, clip * K + beam)
    if (!rows || n_rows == 0 || n_rows > phys || !logits_out) return fail(c, WH_ERR_ARG, "wh_decode_greedy_rows: need 1..%zu rows and a logits buffer", phys);
    if (!tokens_out || !n_tokens_out || cap_clips < (size_t)nb || cap_tokens < p->n_prompt + p->max_new_tokens)
        return fail(c, WH_ERR_ARG, "tokens_out needs %d rows of capacity n_prompt + max_new_tokens", nb);
    if (cap_logits_rows < p->max_new_tokens) return fail(c, WH_ERR_ARG, "logits_out needs max_new_tokens rows per selected clip");
    rc = prefix_check(c, p, nb, false);
    if (rc) return rc;
    if ((rc = align_check(c, nb)) || (rc = beam_check(c, p, nb)) || (rc = sample_check(c, nb, false))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    rc = run_decode(c, nb, p, tokens_out, cap_tokens, n_tokens_out, logits_out, cap_logits_rows, nullptr, rows, n_rows);
    if (rc) return rc;
    decode_only_timing(c, t0);
    return WH_OK;
}

// Clips resident at `pcm` on the device → tokens.  The encoder pass of this batch runs now unless `prefetched`; if
// `next_pcm` is given, the NEXT batch's log-mel + encoder are put on the encoder stream as soon as this batch's cross-K/V
// projection has been enqueued, i.e. they run beside this batch's token loop.
static int transcribe_resident(wh_ctx* c, const float* pcm, int nb, bool prefetched, const float* next_pcm, int next_nb,
                               const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out, double t_start,
                               const std::function<int()>& after_enqueue = nullptr) {
    int rc;
    if (!prefetched) {
        c->pre_valid = false;
        rc = run_encoder_pass(c, pcm, nb, c->enc_set);
        if (rc) return rc;
    }
    std::function<int()> hook = after_enqueue;   // (host work to run once this batch's encoder and cross-K/V step are enqueued)
    if (next_pcm) {
        hook = [c, next_pcm, next_nb]() -> int {
            // every clip of a device-resident batch is exactly 30 s: fill the per-clip sample / frame counts on the stream
            hipStream_t se = c->s_enc;
            int rc2 = enc_begin(c);
            if (rc2) return rc2;
            CTX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_nsamp, WH_CLIP_SAMPLES, next_nb, se));
            CTX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_nframes, WH_N_FRAMES, next_nb, se));
            rc2 = run_encoder_pass(c, next_pcm, next_nb, c->enc_set ^ 1);
            if (rc2) return rc2;
            c->pre_pcm = next_pcm;
            c->pre_n = next_nb;
            c->pre_valid = true;
            return WH_OK;
        };
    }
    rc = run_decode(c, nb, p, tokens_out, p->n_prompt + p->max_new_tokens, n_tokens_out, nullptr, 0, hook);
    if (rc) {   // the prefetched pass (if the hook got that far) is not adopted: the next call recomputes its encoder states
        c->pre_valid = false;
        if (c->s_enc != c->stream) hipStreamSynchronize(c->s_enc);
        return rc;
    }
    rc = finish_timing(c, t_start);
    if (c->pre_valid) {          // the resident states are now the prefetched batch's
        c->enc_set ^= 1;
        c->enc_batch = c->pre_n;
    }
    return rc;
}

// A prefetch of wh_transcribe_batch_next / wh_transcribe_batch_raw_next that the call now starting does not take over: wait for its copies
// (they write c->pcm, c->pcm2 or a raw staging buffer this call may reuse) and forget it.
static int drop_pending_h2d(wh_ctx* c) {
    if (c->h2d_valid) CTX_HIP(c, hipStreamSynchronize(c->s_copy));
    c->h2d_valid = false;
    return WH_OK;
}

int wh_transcribe_batch(wh_ctx* c, const wh_clip* clips, size_t n_clips, const wh_decode_params* p, int64_t* tokens_out,
                        size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!clips || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    rc = prefix_check(c, p, (int)n_clips, false);
    if (rc) return rc;
    if ((rc = align_check(c, (int)n_clips)) || (rc = beam_check(c, p, (int)n_clips)) || (rc = sample_check(c, (int)n_clips, false))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    rc = drop_pending_h2d(c);   // (a prefetch of wh_transcribe_batch*_next may be on its way into c->pcm)
    if (rc) return rc;
    rc = enc_begin(c);
    if (rc) return rc;
    hipStream_t s = c->s_enc;
    std::vector<int> ns(n_clips), nf(n_clips);
    for (size_t i = 0; i < n_clips; i++) {
        if (clips[i].n_samples == 0) return fail(c, WH_ERR_EMPTY_AUDIO, "Empty audio");
        if (!clips[i].pcm) return fail(c, WH_ERR_ARG, "clip %zu: pcm is NULL", i);
        if (clips[i].n_samples > WH_CLIP_SAMPLES) return fail(c, WH_ERR_ARG, "clip %zu longer than one 30 s window; use wh_transcribe_longform", i);
        ns[i] = (int)clips[i].n_samples;
        nf[i] = (int)wh_mel_frames(clips[i].n_samples);
        CTX_HIP(c, hipMemcpyAsync(c->pcm + i * WH_CLIP_SAMPLES, clips[i].pcm, clips[i].n_samples * 4, hipMemcpyHostToDevice, s));
    }
    CTX_HIP(c, hipMemcpyAsync(c->d_nsamp, ns.data(), n_clips * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->d_nframes, nf.data(), n_clips * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    c->timing = wh_timing{};
    c->timing.h2d_s = now_s() - t0;
    c->enc_nframes = nf;
    return transcribe_resident(c, c->pcm, (int)n_clips, false, nullptr, 0, p, tokens_out, n_tokens_out, t0);
}

// the copy stream and its event (shared by the f32 and the raw prefetch)
static int ensure_copy_stream(wh_ctx* c) {
    if (!c->s_copy) CTX_HIP(c, hipStreamCreateWithFlags(&c->s_copy, hipStreamNonBlocking));
    if (!c->ev_h2d) CTX_HIP(c, hipEventCreateWithFlags(&c->ev_h2d, hipEventDisableTiming));
    return WH_OK;
}

// per-clip checks + counts of a host batch (wh_transcribe_batch*)
static int host_batch_counts(wh_ctx* c, const wh_clip* clips, size_t n_clips, std::vector<int>& ns, std::vector<int>& nf) {
    ns.resize(n_clips);
    nf.resize(n_clips);
    for (size_t i = 0; i < n_clips; i++) {
        if (clips[i].n_samples == 0) return fail(c, WH_ERR_EMPTY_AUDIO, "Empty audio");
        if (!clips[i].pcm) return fail(c, WH_ERR_ARG, "clip %zu: pcm is NULL", i);
        if (clips[i].n_samples > WH_CLIP_SAMPLES) return fail(c, WH_ERR_ARG, "clip %zu longer than one 30 s window; use wh_transcribe_longform", i);
        ns[i] = (int)clips[i].n_samples;
        nf[i] = (int)wh_mel_frames(clips[i].n_samples);
    }
    return WH_OK;
}

int wh_transcribe_batch_next(wh_ctx* c, const wh_clip* clips, size_t n_clips, const wh_clip* next_clips, size_t n_next,
                             const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!clips || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    rc = prefix_check(c, p, (int)n_clips, false);
    if (rc) return rc;
    if ((rc = align_check(c, (int)n_clips)) || (rc = beam_check(c, p, (int)n_clips)) || (rc = sample_check(c, (int)n_clips, false))) return rc;
    if (next_clips && (n_next == 0 || n_next > (size_t)c->max_batch)) return fail(c, WH_ERR_ARG, "n_next must be 1..max_batch (%d)", c->max_batch);
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    if (!c->pcm2) {   // second PCM buffer, copy stream and its event: only contexts that use this entry pay for them
        CTX_HIP(c, hipMalloc((void**)&c->pcm2, (size_t)c->max_batch * WH_CLIP_SAMPLES * 4));
        if ((rc = ensure_copy_stream(c))) return rc;
    }
    std::vector<int> ns, nf;
    rc = host_batch_counts(c, clips, n_clips, ns, nf);
    if (rc) return rc;
    rc = enc_begin(c);
    if (rc) return rc;
    hipStream_t s = c->s_enc;
    c->pre_valid = false;
    // this batch's PCM: already on its way (copied beside the previous call's work), or copied now
    const bool hit = c->h2d_valid && !c->h2d_is_raw && c->h2d_src == clips[0].pcm && c->h2d_n == (int)n_clips && c->h2d_ns == ns;
    int buf = hit ? c->h2d_buf : 0;
    float* d_pcm = buf ? c->pcm2 : c->pcm;
    c->timing = wh_timing{};
    if (hit) {
        CTX_HIP(c, hipStreamWaitEvent(s, c->ev_h2d, 0));
    } else {
        if (c->h2d_valid) CTX_HIP(c, hipStreamSynchronize(c->s_copy));   // a prefetch nobody asked for: let it finish before its buffer is reused
        for (size_t i = 0; i < n_clips; i++)
            CTX_HIP(c, hipMemcpyAsync(d_pcm + i * WH_CLIP_SAMPLES, clips[i].pcm, clips[i].n_samples * 4, hipMemcpyHostToDevice, s));
    }
    c->h2d_valid = false;
    CTX_HIP(c, hipMemcpyAsync(c->d_nsamp, ns.data(), n_clips * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->d_nframes, nf.data(), n_clips * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    c->timing.h2d_s = now_s() - t0;   // (a prefetched batch: what was left of its copy)
    std::function<int()> copy_next;
    if (next_clips) {
        // the next batch's copy goes to the other buffer on the copy stream.  Its (thousands of) copy calls are issued from the hook below,
        // i.e. after this batch's log-mel, encoder and cross-K/V step have been enqueued: the host-side issue cost (~8 us per clip) then falls
        // into time the device is busy anyway instead of delaying this batch's first kernel
        std::vector<int> ns2, nf2;
        rc = host_batch_counts(c, next_clips, n_next, ns2, nf2);
        if (rc) return rc;
        float* d_next = buf ? c->pcm : c->pcm2;
        const int nbuf = buf ^ 1;
        copy_next = [c, next_clips, n_next, d_next, nbuf, ns2, nf2]() -> int {
            for (size_t i = 0; i < n_next; i++)
                CTX_HIP(c, hipMemcpyAsync(d_next + i * WH_CLIP_SAMPLES, next_clips[i].pcm, next_clips[i].n_samples * 4, hipMemcpyHostToDevice, c->s_copy));
            CTX_HIP(c, hipEventRecord(c->ev_h2d, c->s_copy));
            c->h2d_is_raw = false;
            c->h2d_buf = nbuf; c->h2d_src = next_clips[0].pcm; c->h2d_n = (int)n_next; c->h2d_ns = ns2; c->h2d_nf = nf2; c->h2d_valid = true;
            return WH_OK;
        };
    }
    c->enc_nframes = nf;
    return transcribe_resident(c, d_pcm, (int)n_clips, false, nullptr, 0, p, tokens_out, n_tokens_out, t0, copy_next);
}

int wh_transcribe_batch_device_next(wh_ctx* c, const float* d_pcm, size_t n_clips, const float* d_pcm_next, size_t n_clips_next,
                                    const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!d_pcm || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    rc = prefix_check(c, p, (int)n_clips, false);
    if (rc) return rc;
    if ((rc = align_check(c, (int)n_clips)) || (rc = beam_check(c, p, (int)n_clips)) || (rc = sample_check(c, (int)n_clips, false))) return rc;
    if (d_pcm_next && (n_clips_next == 0 || n_clips_next > (size_t)c->max_batch))
        return fail(c, WH_ERR_ARG, "n_clips_next must be 1..max_batch (%d)", c->max_batch);
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    // encoder states of exactly this batch already resident (prefetched by the previous call)?
    const bool prefetched = c->pre_valid && c->pre_pcm == d_pcm && c->pre_n == (int)n_clips;
    if (!prefetched) {
        rc = enc_begin(c);
        if (rc) return rc;
        CTX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_nsamp, WH_CLIP_SAMPLES, n_clips, c->s_enc));
        CTX_HIP(c, hipMemsetD32Async((hipDeviceptr_t)c->d_nframes, WH_N_FRAMES, n_clips, c->s_enc));
    }
    c->pre_valid = false;
    c->timing = wh_timing{};
    c->enc_nframes.assign(std::max(n_clips, n_clips_next), WH_N_FRAMES);   // (device-resident clips are exactly 30 s, this batch's and the prefetched one's)
    return transcribe_resident(c, d_pcm, (int)n_clips, prefetched, d_pcm_next, (int)n_clips_next, p, tokens_out, n_tokens_out, t0);
}

int wh_transcribe_batch_device(wh_ctx* c, const float* d_pcm, size_t n_clips, const wh_decode_params* p,
                               int64_t* tokens_out, size_t* n_tokens_out) {
    return wh_transcribe_batch_device_next(c, d_pcm, n_clips, nullptr, 0, p, tokens_out, n_tokens_out);
}

int wh_longform_plan(size_t n_samples, double chunk_length_s, double overlap_s, size_t* offsets, size_t cap,
                     size_t* n_chunks) {  // src/main.rs:858-861, 875-882
    if (!n_chunks) return WH_ERR_ARG;
    const size_t sr = 16000;
    const size_t chunk_len = (size_t)llround((double)(float)chunk_length_s * (double)sr);
    const size_t overlap = (size_t)llround((double)(float)overlap_s * (double)sr);
    size_t step = chunk_len > overlap ? chunk_len - overlap : 0;
    if (step < 1) step = 1;
    size_t n = 0, pos = 0;
    while (pos < n_samples) {
        size_t end = std::min(pos + chunk_len, n_samples);
        if (offsets && n < cap) offsets[n] = pos;
        n++;
        if (end == n_samples) break;
        pos += step;
    }
    *n_chunks = n;
    return (offsets && n > cap) ? WH_ERR_ARG : WH_OK;
}

// wh_transcribe_longform on `pcm`, or (raw != NULL) on the file `raw` converted on the device: n_samples is then its resampled length
static int longform_impl(wh_ctx* c, const float* pcm, const wh_raw_clip* raw, size_t n_samples, double chunk_length_s, double overlap_s,
                         const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out, size_t cap_chunks, size_t* n_chunks_out) {
    int rc;
    rc = prefix_check(c, p, 1, true);
    if (rc) return rc;
    {   // (alignment debug rows are rows of a device batch: they must exist in every batch of the call, so in its last, smallest one)
        size_t nw = 0;
        wh_longform_plan(n_samples, chunk_length_s, overlap_s, nullptr, 0, &nw);
        if ((rc = align_check(c, nw ? (int)(nw - (nw - 1) / c->max_batch * c->max_batch) : 1))) return rc;
    }
    if ((rc = beam_check(c, p, 1)) || (rc = sample_check(c, 1, true))) return rc;
    const size_t win_batch = (size_t)(c->bm_on ? c->max_batch / c->bm_k : c->max_batch);   // windows per device batch (beam search: K rows each)
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    hipStream_t s = c->s_enc;   // whole-file mel, window cut and encoder; run_decode uses the decode stream
    c->pre_valid = false;
    size_t nch = 0;
    wh_longform_plan(n_samples, chunk_length_s, overlap_s, nullptr, 0, &nch);
    *n_chunks_out = nch;
    if (n_samples == 0) return fail(c, WH_ERR_EMPTY_AUDIO, "Empty audio");
    if (nch > cap_chunks) return fail(c, WH_ERR_ARG, "need room for %zu chunks", nch);
    std::vector<size_t> offs(nch);
    wh_longform_plan(n_samples, chunk_length_s, overlap_s, offs.data(), nch, &nch);
    // whole-file mel once: the normalisation max is global over the FILE (src/main.rs:870-872)
    CTX_HIP(c, hipEventRecord(c->ev[0], s));
    size_t nf = 0, ld = 0;
    double h2d_s = 0;
    rc = whole_file_mel(c, pcm, n_samples, &nf, &ld, raw, &h2d_s);
    if (rc) return rc;
    CTX_HIP(c, hipEventRecord(c->ev[1], s));
    const size_t stride = p->n_prompt + p->max_new_tokens;
    const wh_dims& D = c->m->dims;
    double enc_s = 0, dec_s = 0;
    // language detection: the language of the file is the language of its first window (openai-whisper's transcribe()) — the first device
    // batch broadcasts its row 0's choice, later batches take that id as an ordinary prompt token
    struct LangScope {
        wh_ctx* c;
        ~LangScope() { c->lang_bcast = false; c->lang_fixed = -1; c->pfx_win_base = -1; }   // (and the prefix's window scope)
    } lang_scope{c};
    c->lang_bcast = true;
    for (size_t base = 0; base < nch; base += win_batch) {
        const int nb = (int)std::min<size_t>(win_batch, nch - base);
        std::vector<int> src(nb, 0), fs(nb), nfs(1, (int)nf);
        for (int i = 0; i < nb; i++) fs[i] = (int)(offs[base + i] / 160);  // frame_start = pos / hop (:895, 950)
        rc = enc_begin(c);
        if (rc) return rc;
        CTX_HIP(c, hipMemcpyAsync(c->d_src_index, src.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->d_frame_start, fs.data(), nb * 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipMemcpyAsync(c->d_nframes, nfs.data(), 4, hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipStreamSynchronize(s));
        CTX_HIP(c, hipEventRecord(c->ev[4], s));
        if (c->m->esz == 4)
            wh_launch_mel_tokens<float>(s, c->raw_long, 0, (long)ld, c->d_src_index, c->d_frame_start, c->d_nframes, c->d_gmax, 0,
                                        D.n_mels, nb, (float*)c->melT, (long)TOK_ROWS * D.n_mels);
        else
            wh_launch_mel_tokens<bf16>(s, c->raw_long, 0, (long)ld, c->d_src_index, c->d_frame_start, c->d_nframes, c->d_gmax, 0,
                                       D.n_mels, nb, (bf16*)c->melT, (long)TOK_ROWS * D.n_mels);
        rc = run_encoder(c, nb, false);
        if (rc) return rc;
        CTX_HIP(c, hipEventRecord(c->ev[2], s));
        c->enc_nframes.resize(nb);   // each window's valid mel frames
        for (int i = 0; i < nb; i++) c->enc_nframes[i] = (int)std::min<size_t>(WH_N_FRAMES, nf - std::min<size_t>(nf, (size_t)fs[i]));
        c->pfx_win_base = (long)base;   // per-clip prefixes: which rows of this batch are window 0
        rc = run_decode(c, nb, p, tokens_out + base * stride, stride, n_tokens_out + base, nullptr, 0);
        if (rc) return rc;
        if (c->lang_on && base == 0) c->lang_fixed = c->lang_rows[0];
        float a = 0, b = 0;
        hipEventElapsedTime(&a, c->ev[4], c->ev[2]);
        hipEventElapsedTime(&b, c->ev[5], c->ev[3]);
        enc_s += a * 1e-3;
        dec_s += b * 1e-3;
    }
    float a = 0;
    hipEventElapsedTime(&a, c->ev[0], c->ev[1]);
    c->timing = wh_timing{};
    if (raw) c->timing.h2d_s = h2d_s;
    c->timing.preprocess_s = a * 1e-3;
    c->timing.encode_s = enc_s;
    c->timing.decode_s = dec_s;
    c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

int wh_transcribe_longform(wh_ctx* c, const float* pcm, size_t n_samples, double chunk_length_s, double overlap_s,
                           const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out, size_t cap_chunks,
                           size_t* n_chunks_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!tokens_out || !n_tokens_out || !n_chunks_out) return fail(c, WH_ERR_ARG, "NULL argument");
    return longform_impl(c, pcm, nullptr, n_samples, chunk_length_s, overlap_s, p, tokens_out, n_tokens_out, cap_chunks, n_chunks_out);
}

// ---- raw audio in (src/main.rs:207-316 run on the device) ----

size_t wh_resampled_samples(size_t n_frames, uint32_t sample_rate) { return wh_resampled_len(n_frames, sample_rate); }

// the common front of the raw entries that write rows of c->pcm: stage `clips` in buffer k (copied on the encoder stream unless `resident`),
// upload descriptors and per-clip counts, and arm the conversion for the next encoder pass
static int stage_raw_batch(wh_ctx* c, const wh_raw_clip* clips, size_t n_clips, int k, bool resident, std::vector<int>& nf) {
    WhIngestPlan plan;
    wh_ingest_pack(clips, n_clips, WH_CLIP_SAMPLES, plan);
    hipStream_t s = c->s_enc;
    if (!resident) {
        int rc = ensure_ingest(c, k, plan.total_bytes);
        if (rc) return rc;
        if ((rc = copy_raw_clips(c, clips, plan, k, s))) return rc;
    }
    std::vector<int> ns(n_clips);
    nf.resize(n_clips);
    for (size_t i = 0; i < n_clips; i++) {
        ns[i] = (int)plan.desc[i].n_out;
        nf[i] = (int)wh_mel_frames(plan.desc[i].n_out);
    }
    CTX_HIP(c, hipMemcpyAsync(c->ing_desc, plan.desc.data(), n_clips * sizeof(WhIngestDesc), hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->d_nsamp, ns.data(), n_clips * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipMemcpyAsync(c->d_nframes, nf.data(), n_clips * 4, hipMemcpyHostToDevice, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    c->ing_n = (int)n_clips;
    c->ing_buf = k;
    c->ing_max_out = plan.max_out;
    return WH_OK;
}

static const char* const RAW_TOO_LONG = "longer than one 30 s window; use wh_transcribe_longform_raw";

int wh_ingest_raw(wh_ctx* c, const wh_raw_clip* clips, size_t n_clips, float* pcm_out, size_t cap_samples, size_t* n_samples_out) {
    if (!c) return WH_ERR_ARG;
    if (!clips || !pcm_out || !n_samples_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    int rc = check_raw_clips(c, clips, n_clips, n_clips == 1 ? (size_t)0x7fffffffu : (size_t)WH_CLIP_SAMPLES, RAW_TOO_LONG);
    if (rc) return rc;
    for (size_t i = 0; i < n_clips; i++)
        if (wh_resampled_len(clips[i].n_frames, clips[i].sample_rate) > cap_samples)
            return fail(c, WH_ERR_ARG, "pcm_out too small: clip %zu needs %zu samples", i, wh_resampled_len(clips[i].n_frames, clips[i].sample_rate));
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    if ((rc = drop_pending_h2d(c)) || (rc = enc_begin(c))) return rc;
    hipStream_t s = c->s_enc;
    c->timing = wh_timing{};
    if (n_clips == 1) {   // one clip of any length: converted where wh_transcribe_longform_raw converts a file
        const size_t n = wh_resampled_len(clips[0].n_frames, clips[0].sample_rate);
        WhIngestPlan plan;
        wh_ingest_pack(clips, 1, 0, plan);
        if ((rc = ensure_ingest(c, 0, plan.total_bytes)) || (rc = ensure_long(c, n, wh_mel_frames(n)))) return rc;
        if ((rc = copy_raw_clips(c, clips, plan, 0, s))) return rc;
        CTX_HIP(c, hipMemcpyAsync(c->ing_desc, plan.desc.data(), sizeof(WhIngestDesc), hipMemcpyHostToDevice, s));
        CTX_HIP(c, hipStreamSynchronize(s));
        c->timing.h2d_s = now_s() - t0;
        {
            Prof p(c, WH_KG_MEL);
            wh_launch_ingest(s, c->ing_raw[0], c->ing_desc, 1, plan.max_out, c->pcm_long);
        }
        CTX_HIP(c, hipMemcpyAsync(pcm_out, c->pcm_long, n * 4, hipMemcpyDeviceToHost, s));
        n_samples_out[0] = n;
    } else {
        std::vector<int> nf;
        if ((rc = stage_raw_batch(c, clips, n_clips, 0, false, nf))) return rc;
        c->timing.h2d_s = now_s() - t0;
        {
            Prof p(c, WH_KG_MEL);
            wh_launch_ingest(s, c->ing_raw[0], c->ing_desc, (int)n_clips, c->ing_max_out, c->pcm);
        }
        c->ing_n = 0;
        for (size_t i = 0; i < n_clips; i++) {
            n_samples_out[i] = wh_resampled_len(clips[i].n_frames, clips[i].sample_rate);
            CTX_HIP(c, hipMemcpyAsync(pcm_out + i * cap_samples, c->pcm + i * WH_CLIP_SAMPLES, n_samples_out[i] * 4, hipMemcpyDeviceToHost, s));
        }
    }
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    c->timing.preprocess_s = c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

int wh_transcribe_batch_raw_next(wh_ctx* c, const wh_raw_clip* clips, size_t n_clips, const wh_raw_clip* next, size_t n_next,
                                 const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!clips || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    rc = prefix_check(c, p, (int)n_clips, false);
    if (rc) return rc;
    if ((rc = align_check(c, (int)n_clips)) || (rc = beam_check(c, p, (int)n_clips)) || (rc = sample_check(c, (int)n_clips, false))) return rc;
    if (next && (n_next == 0 || n_next > (size_t)c->max_batch)) return fail(c, WH_ERR_ARG, "n_next must be 1..max_batch (%d)", c->max_batch);
    if ((rc = check_raw_clips(c, clips, n_clips, WH_CLIP_SAMPLES, RAW_TOO_LONG))) return rc;
    if (next && (rc = check_raw_clips(c, next, n_next, WH_CLIP_SAMPLES, RAW_TOO_LONG))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    auto same = [](const wh_raw_clip& a, const wh_raw_clip& b) {
        return a.data == b.data && a.n_frames == b.n_frames && a.sample_rate == b.sample_rate && a.channels == b.channels && a.format == b.format;
    };
    // this batch's raw bytes: already on their way (copied beside the previous call's work), or copied now
    bool hit = c->h2d_valid && c->h2d_is_raw && c->h2d_raw_clips.size() == n_clips;
    for (size_t i = 0; hit && i < n_clips; i++) hit = same(c->h2d_raw_clips[i], clips[i]);
    if (!hit && (rc = drop_pending_h2d(c))) return rc;   // (an f32 prefetch may be on its way into c->pcm, a raw one into the buffer reused now)
    const int k = hit ? c->h2d_buf : 0;
    WhIngestPlan plan_next;
    if (next) {   // both staging buffers exist before anything is launched: a refusal for memory leaves no work behind
        wh_ingest_pack(next, n_next, WH_CLIP_SAMPLES, plan_next);
        if ((rc = ensure_copy_stream(c)) || (rc = ensure_ingest(c, k ^ 1, plan_next.total_bytes))) return rc;
    }
    if ((rc = enc_begin(c))) return rc;
    c->pre_valid = false;
    c->timing = wh_timing{};
    if (hit) CTX_HIP(c, hipStreamWaitEvent(c->s_enc, c->ev_h2d, 0));
    c->h2d_valid = false;
    std::vector<int> nf;
    if ((rc = stage_raw_batch(c, clips, n_clips, k, hit, nf))) { c->ing_n = 0; return rc; }
    c->timing.h2d_s = now_s() - t0;   // (a prefetched batch: what was left of its copy)
    std::function<int()> copy_next;
    if (next) {
        // issued once this batch's conversion, log-mel, encoder and cross-K/V step are enqueued, as wh_transcribe_batch_next does
        copy_next = [c, next, n_next, k, plan_next]() -> int {
            int rc2 = copy_raw_clips(c, next, plan_next, k ^ 1, c->s_copy);
            if (rc2) return rc2;
            CTX_HIP(c, hipEventRecord(c->ev_h2d, c->s_copy));
            c->h2d_is_raw = true;
            c->h2d_buf = k ^ 1;
            c->h2d_raw_clips.assign(next, next + n_next);
            c->h2d_n = (int)n_next;
            c->h2d_valid = true;
            return WH_OK;
        };
    }
    c->enc_nframes = nf;
    rc = transcribe_resident(c, c->pcm, (int)n_clips, false, nullptr, 0, p, tokens_out, n_tokens_out, t0, copy_next);
    c->ing_n = 0;
    return rc;
}

int wh_transcribe_batch_raw(wh_ctx* c, const wh_raw_clip* clips, size_t n_clips, const wh_decode_params* p, int64_t* tokens_out,
                            size_t* n_tokens_out) {
    return wh_transcribe_batch_raw_next(c, clips, n_clips, nullptr, 0, p, tokens_out, n_tokens_out);
}

int wh_transcribe_longform_raw(wh_ctx* c, const wh_raw_clip* file, double chunk_length_s, double overlap_s, const wh_decode_params* p,
                               int64_t* tokens_out, size_t* n_tokens_out, size_t cap_chunks, size_t* n_chunks_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!file || !tokens_out || !n_tokens_out || !n_chunks_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if ((rc = check_raw_clips(c, file, 1, 0x7fffffffu, "longer than 2^31 samples"))) return rc;
    const size_t n = wh_resampled_len(file->n_frames, file->sample_rate);
    CTX_HIP(c, hipSetDevice(c->m->device));
    if ((rc = drop_pending_h2d(c))) return rc;   // (staging buffer 0 may hold a prefetched raw batch)
    if ((rc = ensure_ingest(c, 0, file->n_frames * file->channels * wh_pcm_sample_bytes(file->format)))) return rc;
    return longform_impl(c, nullptr, file, n, chunk_length_s, overlap_s, p, tokens_out, n_tokens_out, cap_chunks, n_chunks_out);
}

}  // extern "C"
