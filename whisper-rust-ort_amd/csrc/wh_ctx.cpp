// wh_ctx.cpp — model and context lifecycle of the C ABI (include/whisper_hip.h): error reporting, the profiling hooks' bookkeeping, context
// creation and workspace placement, wh_ctx_free, and the timing / profile getters.
#include "wh_host_shared.h"

using namespace wh;

namespace wh {

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

void drop_step_graph(wh_ctx* c) {
    if (c->step_exec[0] && c->stream) hipStreamSynchronize(c->stream);  // an error path may have left replays in flight
    if (c->step_exec[0] && c->step_key.free && c->s_split) hipStreamSynchronize(c->s_split);   // (the second range's segments replay there)
    // A two-branch step: measured, an executable graph with two branches that is destroyed after a wait for c->stream alone leaves
    // the context's workspace allocated after hipFree (a 1024-clip context: 29 GB per context closed; every call returns success); with a wait
    // for the device first, nothing stays.  The cause inside the runtime is not known — presumably the branch's replay on streams the runtime
    // owns.  One-chain graphs never showed it and are destroyed as before: the device wait also stalls other contexts and the encoder stream
    // The free-running halves (§5t) have no graph with branches: four single chains, destroyed like the one chain.
    if (c->step_exec[0] && c->step_key.split && !c->step_key.free) hipDeviceSynchronize();
    for (int i = 0; i < wh_ctx::STEP_GRAPHS; i++) {
        if (c->step_exec[i]) hipGraphExecDestroy(c->step_exec[i]);
        if (c->step_graph[i]) hipGraphDestroy(c->step_graph[i]);
        c->step_exec[i] = nullptr;
        c->step_graph[i] = nullptr;
    }
    c->step_key = wh_ctx::StepKey();
}

}  // namespace wh

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
    if (dec_masked) c->dec_mask.assign(opts->dec_cu_mask, opts->dec_cu_mask + opts->dec_cu_mask_words);
    if (const char* e = getenv("WH_DEC_SPLIT")) c->split_mode = atoi(e) != 0;                     // A/B runs: the split token loop off / on
    if (const char* e = getenv("WH_DEC_SPLIT_ROWS")) c->split_rows = std::max(0, atoi(e));
    if (const char* e = getenv("WH_DEC_SPLIT_CUS")) c->split_cus = std::max(1, atoi(e));
    if (const char* e = getenv("WH_DEC_FREE")) c->free_mode = atoi(e) != 0;                       // A/B runs: the free-running halves off / on
    if (const char* e = getenv("WH_DEC_FREE_EB")) c->free_eb = atoi(e) != 0;                      // ... and without the edge that bounds the first range's lead
    c->no_graph = getenv("WH_NO_GRAPH") != nullptr;
    c->sync_every_pos = getenv("WH_SYNC_EVERY_POS") != nullptr;
    c->al.timing = getenv("WH_ALIGN_TIMING") != nullptr;
    c->bm.timing = getenv("WH_BEAM_TIMING") != nullptr;
    c->sm.timing = getenv("WH_SAMPLE_TIMING") != nullptr;
    c->sc.timing = getenv("WH_SCORE_TIMING") != nullptr;
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
    const size_t o_nout = cv.take(B * 4), o_done = cv.take(B * 4), o_forced = cv.take(TC * 4), o_pos = cv.take(2 * 4);
    const size_t o_stk = cv.take(2 * 4);   // (two each: the whole batch's, and the second range's while the halves run free)
    const size_t o_m1 = cv.take((D.vocab / 32 + 1) * 4), o_m2 = cv.take((D.vocab / 32 + 1) * 4);
    const size_t o_ns = cv.take(B * 4), o_nf = cv.take(B * 4), o_si = cv.take(B * 4), o_fs = cv.take(B * 4), o_gm = cv.take(B * 4);
    const size_t o_lsel = cv.take(B * 4);
    hipError_t he = hipMalloc(&c->ws.p, cv.off);
    if (he != hipSuccess) { delete c; return wh_fail_hip(he, "hipMalloc(workspace)", __FILE__, __LINE__); }
    c->ws.bytes = cv.off;
    he = hipMemset(c->ws, 0, c->ws.bytes);  // conv zero rows, V^T key padding, caches
    if (he != hipSuccess) { delete c; return wh_fail_hip(he, "hipMemset(workspace)", __FILE__, __LINE__); }
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
        if (he != hipSuccess) { delete c; return wh_fail_hip(he, "hipMemcpy(row offsets)", __FILE__, __LINE__); }
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
    if (he != hipSuccess) { delete c; return wh_fail_hip(he, "hipStreamCreate", __FILE__, __LINE__); }
    c->s_enc = c->stream;
    if (opts->enc_cu_mask_words || (opts->flags & WH_CTX_TWO_STREAMS)) {
        if (enc_masked) he = hipExtStreamCreateWithCUMask(&c->s_enc, (uint32_t)opts->enc_cu_mask_words, opts->enc_cu_mask);
        else he = hipStreamCreateWithFlags(&c->s_enc, hipStreamNonBlocking);
        if (he != hipSuccess) { hipStreamDestroy(c->stream); delete c; return wh_fail_hip(he, "hipStreamCreate(encoder stream)", __FILE__, __LINE__); }
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

void wh_ctx_free(wh_ctx* c) {
    if (!c) return;
    hipSetDevice(c->m->device);
    if (c->s_enc && c->s_enc != c->stream) hipStreamSynchronize(c->s_enc);   // a prefetched encoder pass may be in flight
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->s_split) hipStreamSynchronize(c->s_split);
    drop_step_graph(c);
    for (auto& e : c->split_ev) hipEventDestroy(e);
    for (auto& e : c->free_ev) hipEventDestroy(e);
    if (c->s_split) hipStreamDestroy(c->s_split);
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
    c->reset_option_results();   // (timing events of a call that failed before its read-back)
    if (c->s_copy) { hipStreamSynchronize(c->s_copy); hipStreamDestroy(c->s_copy); }
    if (c->ev_h2d) hipEventDestroy(c->ev_h2d);
    delete c;   // the owned buffers (DevBuf) go here: after the streams have drained and the step graph is gone
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

// test hooks (tests/test_step_split_gpu.py; not in the public header).  rows > 0: the generated positions of the following decode calls run rows
// [0, rows) and [rows, nb) as two branches wherever the call is eligible (choose_split, wh_decode_host.cpp); 0: the context's own rule again
extern "C" int wh_debug_set_step_split(wh_ctx* c, int rows) {
    if (!c || rows < 0) return WH_ERR_ARG;
    c->dbg_split = rows;
    return WH_OK;
}
// the first range's rows of the last decode call; 0 = it ran one chain
extern "C" int wh_debug_get_step_split(const wh_ctx* c) { return c ? c->last_split : -1; }
// test hooks (tests/test_free_halves_gpu.py; not in the public header).  on != 0: where wh_debug_set_step_split makes the following decode calls
// split, their two ranges run free (choose_free, wh_decode_host.cpp); 0: only where the context's own rule splits
extern "C" int wh_debug_set_step_free(wh_ctx* c, int on) {
    if (!c) return WH_ERR_ARG;
    c->dbg_free = on != 0;
    return WH_OK;
}
// 1: the generated positions of the last decode call ran as free halves
extern "C" int wh_debug_get_step_free(const wh_ctx* c) { return c ? c->last_free : -1; }

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

}  // extern "C"
