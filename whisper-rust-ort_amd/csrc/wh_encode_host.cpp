// wh_encode_host.cpp — the host side of log-mel and the encoder: the encoder's launches for a batch (run_encoder; reference src/main.rs:698-707),
// the batch log-mel, an encoder pass with its stage events, and the whole-file log-mel of the long-form entries (:407-509, 870-872).
#include "wh_host_shared.h"

using namespace wh;

namespace wh {

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

// mel of nb clips resident at `pcm` ([nb][480000] f32, n samples each in c->d_nsamp) → conv1 operand in c->melT
static int run_mel_batch(wh_ctx* c, const float* pcm, int nb) {
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

// grow the whole-file buffers to hold n samples / nf frames
int ensure_long(wh_ctx* c, size_t n, size_t nf) {
    const size_t mel_bytes = (size_t)c->m->dims.n_mels * align_up(nf, 16) * 4;
    int rc;   // free first: a whole file's buffers are large, and nothing is in them that the call still needs
    if ((rc = grow(c, c->pcm_long, n * 4, false, GROW_FREE_FIRST, "the whole-file PCM")) || (rc = grow(c, c->raw_long, mel_bytes, false, GROW_FREE_FIRST, "the whole-file raw log-mel")) ||
        (rc = grow(c, c->mel_out_long, mel_bytes, false, GROW_FREE_FIRST, "the whole-file log-mel")))
        return rc;
    return WH_OK;
}

// whole-file raw log-mel into c->raw_long (row stride = align16(frames)); returns frames
// `raw` (optional): the file as it was read; it is converted into c->pcm_long on the device instead of copying `pcm`
int whole_file_mel(wh_ctx* c, const float* pcm, size_t n, size_t* nf_out, size_t* ld_out, const wh_raw_clip* raw,
                   double* h2d_s_out) {
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

// ---- the resident file set (wh_files_load) ----------------------------------------------------------------------------
// Whole-file raw log-mels of n validated files (f32 `files`, or `raws` converted on the device), back to back in c->fs.mel: file f is
// [n_mels][ld_f] floats at desc[f].base, computed by its own k_mel_stft launch with the arguments whole_file_mel uses — so it is
// wh_log_mel's result bit for bit.  Every buffer exists before anything is launched or the loaded set is touched: a refusal for memory
// (WH_ERR_NOMEM) leaves the old set usable.  The files pass through c->pcm_long one at a time, in stream order.
int load_file_set(wh_ctx* c, const wh_clip* files, const wh_raw_clip* raws, size_t n) {
    const size_t C = (size_t)c->m->dims.n_mels;
    std::vector<WhFileDesc> desc(n);
    std::vector<WhIngestDesc> ing(raws ? n : 0);
    size_t total = 0, max_n = 0, max_raw = 0;
    for (size_t f = 0; f < n; f++) {
        const size_t ns = raws ? wh_resampled_len(raws[f].n_frames, raws[f].sample_rate) : files[f].n_samples;
        const size_t nf = wh_mel_frames(ns), ld = align_up(nf, 16);
        desc[f] = WhFileDesc{(long long)total, (int)ld, (int)nf, 0u, (int)ns};
        total += C * ld;
        max_n = std::max(max_n, ns);
        if (raws) {
            WhIngestPlan one;
            wh_ingest_pack(raws + f, 1, 0, one);
            ing[f] = one.desc[0];
            max_raw = std::max(max_raw, one.total_bytes);
        }
    }
    int rc;
    if ((rc = grow(c, c->pcm_long, max_n * 4, false, GROW_KEEP_OLD, "the whole-file PCM")) ||
        (rc = grow(c, c->fs.desc, (size_t)WH_MAX_FILES * sizeof(WhFileDesc), false, GROW_KEEP_OLD, "the file set's descriptors")) ||
        (rc = grow(c, c->fs.rows, (size_t)2 * c->max_batch * sizeof(int), false, GROW_KEEP_OLD, "the window rows")))
        return rc;
    if (raws && ((rc = grow(c, c->ing_raw[0], max_raw, false, GROW_KEEP_OLD, "raw audio staging")) ||
                 (rc = grow(c, c->fs.ing, (size_t)WH_MAX_FILES * sizeof(WhIngestDesc), false, GROW_KEEP_OLD, "the file set's raw descriptors"))))
        return rc;
    DevBuf<float> store;
    if (total * 4 > c->fs.mel.bytes) {
        const hipError_t e = hipMalloc(&store.p, total * 4);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, WH_ERR_NOMEM, "the file set's log-mel store (%zu bytes): hipMalloc: %s", total * 4, hipGetErrorString(e));
        }
        store.bytes = total * 4;
    }
    if ((rc = enc_begin(c))) return rc;
    hipStream_t s = c->s_enc;
    c->fs.n = 0;   // from here on the old set is gone
    c->fs.host.clear();
    if (store.p) c->fs.mel = std::move(store);
    CTX_HIP(c, hipMemcpyAsync(c->fs.desc, desc.data(), n * sizeof(WhFileDesc), hipMemcpyHostToDevice, s));
    if (raws) CTX_HIP(c, hipMemcpyAsync(c->fs.ing, ing.data(), n * sizeof(WhIngestDesc), hipMemcpyHostToDevice, s));
    for (size_t f = 0; f < n; f++) {
        char* d = (char*)c->fs.desc.p + f * sizeof(WhFileDesc);
        if (raws) {
            CTX_HIP(c, hipMemcpyAsync(c->ing_raw[0], raws[f].data, raws[f].n_frames * raws[f].channels * wh_pcm_sample_bytes(raws[f].format), hipMemcpyHostToDevice, s));
            Prof p(c, WH_KG_MEL);
            wh_launch_ingest(s, c->ing_raw[0], (WhIngestDesc*)c->fs.ing + f, 1, ing[f].n_out, c->pcm_long);
        } else {
            CTX_HIP(c, hipMemcpyAsync(c->pcm_long, files[f].pcm, files[f].n_samples * 4, hipMemcpyHostToDevice, s));
        }
        Prof p(c, WH_KG_MEL);
        wh_launch_mel_stft(s, c->pcm_long, 0, (const int*)(d + offsetof(WhFileDesc, n_samples)), 1, (long)desc[f].frames, c->m->mel_tw, c->m->mel_win,
                           c->m->mel_fbT, (int)C, (float*)c->fs.mel + desc[f].base, 0, (long)desc[f].ld, (unsigned*)(d + offsetof(WhFileDesc, gmax)));
    }
    CTX_HIP(c, hipStreamSynchronize(s));   // (the host copies of the descriptors, and the caller's files, are read until here)
    CTX_HIP(c, hipGetLastError());
    c->fs.host = std::move(desc);
    c->fs.n = n;
    return WH_OK;
}

// the conv1 operand of nb windows of the file set (rows already in c->fs.rows: [0] the files, [1] the seeks) into c->melT
void launch_window_cut(wh_ctx* c, int nb) {
    const wh_dims& D = c->m->dims;
    hipStream_t s = c->s_enc;
    c->cur = s;
    Prof p(c, WH_KG_MEL);
    const int* rf = c->fs.rows;
    const int* rs = rf + c->max_batch;
    if (c->m->esz == 4) wh_launch_mel_window<float>(s, c->fs.mel, c->fs.desc, rf, rs, D.n_mels, nb, (float*)c->melT, (long)TOK_ROWS * D.n_mels);
    else wh_launch_mel_window<bf16>(s, c->fs.mel, c->fs.desc, rf, rs, D.n_mels, nb, (bf16*)c->melT, (long)TOK_ROWS * D.n_mels);
}

}  // namespace wh

extern "C" {

size_t wh_mel_frames(size_t n) {  // src/main.rs:444-452
    size_t nf = 1 + n / 160;
    if (nf > 1) nf -= 1;
    return nf;
}

}  // extern "C"
