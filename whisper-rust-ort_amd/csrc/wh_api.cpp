// wh_api.cpp — the C ABI of include/whisper_hip.h: the entry points that run the pipeline, i.e. the orchestration of
// log-mel → encoder → cross-KV → batched greedy decode on one HIP stream.
//
// Mirrors, per entry point: whisper_log_mel_80 (reference src/main.rs:407-509), run_encoder
// (:698-707), greedy_decode_with_past (:753-829) and the per-window body of
// transcribe_longform_chunked (:870-915, 946-967).
#include "wh_host_shared.h"

using namespace wh;

namespace wh {

// stage times of the batch whose encoder pass is in event set c->enc_set and whose decode ran between ev[5] and ev[3]
static int finish_timing(wh_ctx* c, double t_start) {
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

static int check_params(wh_ctx* c, const wh_decode_params* p) {
    // (every decode entry passes here once, first: what wh_get_logprobs returns belongs to the call that starts now)
    c->reset_option_results();
    if (!p) return fail(c, WH_ERR_ARG, "decode params are NULL");
    if ((p->n_suppress && !p->suppress) || (p->n_begin_suppress && !p->begin_suppress) || (p->n_forced && !p->forced))
        return fail(c, WH_ERR_ARG, "decode params: NULL list with non-zero length");
    return WH_OK;
}

}  // namespace wh

extern "C" {

// grow raw staging buffer `k` to `bytes`.  A failed allocation leaves the ctx as it was, with no sticky HIP error (GROW_KEEP_OLD).
static int ensure_ingest(wh_ctx* c, int k, size_t bytes) {
    if (int rc = grow(c, c->ing_desc, (size_t)c->max_batch * sizeof(WhIngestDesc), false, GROW_KEEP_OLD, "raw audio descriptors")) return rc;
    return grow(c, c->ing_raw[k], bytes, false, GROW_KEEP_OLD, "raw audio staging");
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

// the common tail of the decode-only entries: the decode of the resident encoder states and its stage times (run_decode brackets the decode
// with ev[5] .. ev[3])
static int decode_resident(wh_ctx* c, int nb, const wh_decode_params* p, int64_t* tokens_out, size_t cap_tokens, size_t* n_tokens_out, float* logits_out,
                           size_t logits_rows, const int32_t* rows = nullptr, size_t n_rows = 0) {
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    if (int rc = run_decode(c, nb, p, tokens_out, cap_tokens, n_tokens_out, logits_out, logits_rows, nullptr, rows, n_rows)) return rc;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[5], c->ev[3]);
    const double d2h = c->timing.d2h_s;
    c->timing = wh_timing{};
    c->timing.decode_s = ms * 1e-3;
    c->timing.d2h_s = d2h;
    c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
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
    if (logits_out && c->bm.on && c->bm.k > 1)
        return fail(c, WH_ERR_ARG, "wh_decode_greedy: logits_out holds one row's logits, beam search has %d rows per clip; use wh_decode_greedy_rows", c->bm.k);
    if ((rc = options_check(c, p, 1, false))) return rc;
    return decode_resident(c, 1, p, tokens_out, cap_tokens, n_tokens_out, logits_out, p->max_new_tokens);
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
    if (logits_out && c->bm.on && cap_clips < (size_t)nb * c->bm.k)
        return fail(c, WH_ERR_ARG, "wh_decode_greedy_batch: with beam search logits_out holds %d clips x %d beams: cap_clips must be at least %d", nb, c->bm.k, nb * c->bm.k);
    if ((rc = options_check(c, p, nb, false))) return rc;
    return decode_resident(c, nb, p, tokens_out, cap_tokens, n_tokens_out, logits_out, logits_out ? cap_logits_rows : 0);
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
    const size_t phys = (size_t)nb * (c->bm.on ? c->bm.k : 1);   // (beam search: rows address the physical rows, clip * K + beam)
    if (!rows || n_rows == 0 || n_rows > phys || !logits_out) return fail(c, WH_ERR_ARG, "wh_decode_greedy_rows: need 1..%zu rows and a logits buffer", phys);
    if (!tokens_out || !n_tokens_out || cap_clips < (size_t)nb || cap_tokens < p->n_prompt + p->max_new_tokens)
        return fail(c, WH_ERR_ARG, "tokens_out needs %d rows of capacity n_prompt + max_new_tokens", nb);
    if (cap_logits_rows < p->max_new_tokens) return fail(c, WH_ERR_ARG, "logits_out needs max_new_tokens rows per selected clip");
    if ((rc = options_check(c, p, nb, false))) return rc;
    return decode_resident(c, nb, p, tokens_out, cap_tokens, n_tokens_out, logits_out, cap_logits_rows, rows, n_rows);
}

// log p(given tokens | audio) of n_hyp hypotheses over the resident clips, one decoder pass over all their positions (wh_score_host.cpp)
int wh_score_tokens(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, float* logprob_out, int64_t* argmax_out, size_t cap_tokens,
                    const int32_t* logit_hyps, size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    prof_reset(c);
    const double t0 = now_s();
    if ((rc = run_score(c, p, in, logprob_out, argmax_out, cap_tokens, logit_hyps, n_logit_hyps, logits_out, cap_logits_rows))) return rc;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[5], c->ev[3]);
    c->timing = wh_timing{};
    c->timing.decode_s = ms * 1e-3;
    c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

// forced alignment: the frame of every token of given transcripts over the resident clips, from the same pass (wh_score_host.cpp)
int wh_align_tokens(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, const wh_alignment_opts* heads, int32_t* frames_out, int32_t* n_frames_out,
                    float* logprob_out, size_t cap_tokens) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    prof_reset(c);
    const double t0 = now_s();
    if ((rc = run_align_tokens(c, p, in, heads, frames_out, n_frames_out, logprob_out, cap_tokens))) return rc;
    float ms = 0;
    hipEventElapsedTime(&ms, c->ev[5], c->ev[3]);
    c->timing = wh_timing{};
    c->timing.decode_s = ms * 1e-3;
    c->timing.total_s = now_s() - t0;
    prof_collect(c);
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

int wh_transcribe_batch(wh_ctx* c, const wh_clip* clips, size_t n_clips, const wh_decode_params* p, int64_t* tokens_out,
                        size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!clips || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    if ((rc = options_check(c, p, (int)n_clips, false))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    rc = drop_pending_h2d(c);   // (a prefetch of wh_transcribe_batch*_next may be on its way into c->pcm)
    if (rc) return rc;
    rc = enc_begin(c);
    if (rc) return rc;
    hipStream_t s = c->s_enc;
    std::vector<int> ns, nf;
    if ((rc = host_batch_counts(c, clips, n_clips, ns, nf))) return rc;
    for (size_t i = 0; i < n_clips; i++)
        CTX_HIP(c, hipMemcpyAsync(c->pcm + i * WH_CLIP_SAMPLES, clips[i].pcm, clips[i].n_samples * 4, hipMemcpyHostToDevice, s));
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

int wh_transcribe_batch_next(wh_ctx* c, const wh_clip* clips, size_t n_clips, const wh_clip* next_clips, size_t n_next,
                             const wh_decode_params* p, int64_t* tokens_out, size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!clips || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (n_clips == 0 || n_clips > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_clips must be 1..max_batch (%d)", c->max_batch);
    if ((rc = options_check(c, p, (int)n_clips, false))) return rc;
    if (next_clips && (n_next == 0 || n_next > (size_t)c->max_batch)) return fail(c, WH_ERR_ARG, "n_next must be 1..max_batch (%d)", c->max_batch);
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    if (!c->pcm2) {   // second PCM buffer, copy stream and its event: only contexts that use this entry pay for them
        if ((rc = grow(c, c->pcm2, (size_t)c->max_batch * WH_CLIP_SAMPLES * 4, false, GROW_FREE_FIRST, "the second PCM buffer")) || (rc = ensure_copy_stream(c))) return rc;
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
    float* d_pcm = buf ? (float*)c->pcm2 : c->pcm;
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
        float* d_next = buf ? c->pcm : (float*)c->pcm2;
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
    if ((rc = options_check(c, p, (int)n_clips, false))) return rc;
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
    {   // (alignment debug rows are rows of a device batch: they must exist in every batch of the call, so in its last, smallest one)
        size_t nw = 0;
        wh_longform_plan(n_samples, chunk_length_s, overlap_s, nullptr, 0, &nw);
        if ((rc = options_check(c, p, 1, true, nw ? (int)(nw - (nw - 1) / c->max_batch * c->max_batch) : 1))) return rc;
    }
    const size_t win_batch = (size_t)(c->bm.on ? c->max_batch / c->bm.k : c->max_batch);   // windows per device batch (beam search: K rows each)
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
        ~LangScope() { c->lang.bcast = false; c->lang.fixed = -1; c->pfx.win_base = -1; }   // (and the prefix's window scope)
    } lang_scope{c};
    c->lang.bcast = true;
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
        c->pfx.win_base = (long)base;   // per-clip prefixes: which rows of this batch are window 0
        rc = run_decode(c, nb, p, tokens_out + base * stride, stride, n_tokens_out + base, nullptr, 0);
        if (rc) return rc;
        if (c->lang.on && base == 0) c->lang.fixed = c->lang.rows[0];
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
    if ((rc = options_check(c, p, (int)n_clips, false))) return rc;
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

// ---- the resident file set and windows cut from it ----

// the common body of the two loads, after their refusals
static int files_load_impl(wh_ctx* c, const wh_clip* files, const wh_raw_clip* raws, size_t n, int64_t* n_frames_out) {
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    int rc = drop_pending_h2d(c);   // (staging buffer 0 may hold a prefetched raw batch)
    if (rc) return rc;
    if ((rc = load_file_set(c, files, raws, n))) return rc;
    for (size_t f = 0; f < n; f++) n_frames_out[f] = c->fs.host[f].frames;
    c->timing = wh_timing{};
    c->timing.preprocess_s = c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

static int files_free(wh_ctx* c) {
    CTX_HIP(c, hipSetDevice(c->m->device));
    int rc = drop_pending_h2d(c);
    if (rc) return rc;
    c->fs.n = 0;
    c->fs.host.clear();
    c->fs.mel.reset();
    return WH_OK;
}

int wh_files_load(wh_ctx* c, const wh_clip* files, size_t n_files, int64_t* n_frames_out) {
    if (!c) return WH_ERR_ARG;
    if (!files || n_files == 0) return files_free(c);
    if (n_files > WH_MAX_FILES) return fail(c, WH_ERR_ARG, "n_files must be 1..%d", WH_MAX_FILES);
    if (!n_frames_out) return fail(c, WH_ERR_ARG, "NULL argument");
    for (size_t f = 0; f < n_files; f++) {
        if (files[f].n_samples && !files[f].pcm) return fail(c, WH_ERR_ARG, "file %zu: pcm is NULL", f);
        if (files[f].n_samples > 0x7fffffffu) return fail(c, WH_ERR_ARG, "file %zu: audio longer than 2^31 samples", f);
    }
    for (size_t f = 0; f < n_files; f++)
        if (files[f].n_samples == 0) return fail(c, WH_ERR_EMPTY_AUDIO, "Empty audio");   // src/main.rs:414-416
    return files_load_impl(c, files, nullptr, n_files, n_frames_out);
}

int wh_files_load_raw(wh_ctx* c, const wh_raw_clip* files, size_t n_files, int64_t* n_frames_out) {
    if (!c) return WH_ERR_ARG;
    if (!files || n_files == 0) return files_free(c);
    if (n_files > WH_MAX_FILES) return fail(c, WH_ERR_ARG, "n_files must be 1..%d", WH_MAX_FILES);
    if (!n_frames_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (int rc = check_raw_clips(c, files, n_files, 0x7fffffffu, "longer than 2^31 samples")) return rc;
    return files_load_impl(c, nullptr, files, n_files, n_frames_out);
}

// the refusals of a window row, before anything is launched
static int check_window(wh_ctx* c, int64_t file, int64_t seek, size_t i) {
    if (file < 0 || (size_t)file >= c->fs.n) return fail(c, WH_ERR_ARG, "row %zu: file %lld outside the set of %zu files", i, (long long)file, c->fs.n);
    if (seek < 0 || seek >= c->fs.host[file].frames)
        return fail(c, WH_ERR_ARG, "row %zu: seek %lld outside file %lld's %d frames", i, (long long)seek, (long long)file, c->fs.host[file].frames);
    return WH_OK;
}

static int upload_window_rows(wh_ctx* c, const std::vector<int>& rf, const std::vector<int>& rs) {
    CTX_HIP(c, hipMemcpyAsync(c->fs.rows, rf.data(), rf.size() * 4, hipMemcpyHostToDevice, c->s_enc));
    CTX_HIP(c, hipMemcpyAsync((int*)c->fs.rows + c->max_batch, rs.data(), rs.size() * 4, hipMemcpyHostToDevice, c->s_enc));
    CTX_HIP(c, hipStreamSynchronize(c->s_enc));
    return WH_OK;
}

int wh_transcribe_windows(wh_ctx* c, const int32_t* file, const int64_t* seek_frame, size_t n_rows, const wh_decode_params* p, int64_t* tokens_out,
                          size_t* n_tokens_out) {
    if (!c) return WH_ERR_ARG;
    int rc = check_params(c, p);
    if (rc) return rc;
    if (!file || !seek_frame || !tokens_out || !n_tokens_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (c->fs.n == 0) return fail(c, WH_ERR_STATE, "wh_transcribe_windows: no file set is loaded (call wh_files_load first)");
    if (n_rows == 0 || n_rows > (size_t)c->max_batch) return fail(c, WH_ERR_ARG, "n_rows must be 1..max_batch (%d)", c->max_batch);
    for (size_t i = 0; i < n_rows; i++)
        if ((rc = check_window(c, file[i], seek_frame[i], i))) return rc;
    if ((rc = options_check(c, p, (int)n_rows, false))) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    if ((rc = drop_pending_h2d(c)) || (rc = enc_begin(c))) return rc;
    hipStream_t s = c->s_enc;
    c->pre_valid = false;   // the resident encoder states are replaced
    std::vector<int> rf(file, file + n_rows), rs(n_rows), nf(n_rows);
    for (size_t i = 0; i < n_rows; i++) {
        rs[i] = (int)seek_frame[i];
        nf[i] = std::min<int>(WH_N_FRAMES, c->fs.host[rf[i]].frames - rs[i]);   // each window's valid mel frames
    }
    if ((rc = upload_window_rows(c, rf, rs))) return rc;
    c->timing = wh_timing{};
    c->timing.h2d_s = now_s() - t0;
    CTX_HIP(c, hipEventRecord(c->enc_ev[c->enc_set][0], s));
    launch_window_cut(c, (int)n_rows);
    CTX_HIP(c, hipEventRecord(c->enc_ev[c->enc_set][1], s));
    if ((rc = run_encoder(c, (int)n_rows, false))) return rc;
    CTX_HIP(c, hipEventRecord(c->enc_ev[c->enc_set][2], s));
    c->enc_nframes = nf;
    if ((rc = run_decode(c, (int)n_rows, p, tokens_out, p->n_prompt + p->max_new_tokens, n_tokens_out, nullptr, 0))) return rc;
    return finish_timing(c, t0);
}

int wh_files_window_mel(wh_ctx* c, int32_t file, int64_t seek_frame, float* mel_out) {
    if (!c) return WH_ERR_ARG;
    if (!mel_out) return fail(c, WH_ERR_ARG, "NULL argument");
    if (c->fs.n == 0) return fail(c, WH_ERR_STATE, "wh_files_window_mel: no file set is loaded (call wh_files_load first)");
    int rc = check_window(c, file, seek_frame, 0);
    if (rc) return rc;
    CTX_HIP(c, hipSetDevice(c->m->device));
    prof_reset(c);
    const double t0 = now_s();
    if ((rc = drop_pending_h2d(c)) || (rc = enc_begin(c))) return rc;
    hipStream_t s = c->s_enc;
    if ((rc = upload_window_rows(c, std::vector<int>(1, file), std::vector<int>(1, (int)seek_frame)))) return rc;
    launch_window_cut(c, 1);
    // the conv1 operand's rows 1 .. 3000 of batch row 0, token-major in the compute dtype -> [n_mels][3000] f32
    const size_t C = (size_t)c->m->dims.n_mels, esz = c->m->esz;
    std::vector<char> tok((size_t)WH_N_FRAMES * C * esz);
    CTX_HIP(c, hipMemcpyAsync(tok.data(), (char*)c->melT + C * esz, tok.size(), hipMemcpyDeviceToHost, s));
    CTX_HIP(c, hipStreamSynchronize(s));
    CTX_HIP(c, hipGetLastError());
    for (size_t t = 0; t < WH_N_FRAMES; t++)
        for (size_t m = 0; m < C; m++) {
            float v;
            if (esz == 4) {
                memcpy(&v, tok.data() + (t * C + m) * 4, 4);
            } else {   // bf16: the upper half of the f32
                uint16_t h;
                memcpy(&h, tok.data() + (t * C + m) * 2, 2);
                const uint32_t w = (uint32_t)h << 16;
                memcpy(&v, &w, 4);
            }
            mel_out[m * WH_N_FRAMES + t] = v;
        }
    c->timing = wh_timing{};
    c->timing.preprocess_s = c->timing.total_s = now_s() - t0;
    prof_collect(c);
    return WH_OK;
}

}  // extern "C"
