// wh_internal.h — wh_model / wh_ctx definitions (internal to libwhisper_hip.so).
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/whisper_hip.h"
#include "wh_kernels.h"

struct EncLayerDev {
    void *qk_w, *v_w, *o_w, *fc1_w, *fc2_w;
    float *qk_b, *v_b, *o_b, *fc1_b, *fc2_b;
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b;
    // WH_PREC_FP8: the matrices above hold the e4m3 code VALUES (exact in bf16); these are the per-output-channel scales
    float *qk_sc = nullptr, *v_sc = nullptr, *o_sc = nullptr, *fc1_sc = nullptr, *fc2_sc = nullptr;
    // ... and these the raw e4m3 codes [N][K] (one byte each) for the fp8-MFMA GEMMs (wh_gemm8_mx.hip)
    void *qk_w8 = nullptr, *v_w8 = nullptr, *fc1_w8 = nullptr, *fc2_w8 = nullptr;
    // WH_PREC_BF16, LayerNorm folded into the consumer GEMMs (wh_gemm8.hip, run_encoder's fold path): W (.) gamma in bf16,
    // s[n] = sum_k of the stored values, c[n] = bias[n] + sum_k beta[k] W[n][k]
    void *qk_wf = nullptr, *v_wf = nullptr, *fc1_wf = nullptr;
    float *qk_s = nullptr, *qk_c = nullptr, *v_s = nullptr, *v_c = nullptr, *fc1_s = nullptr, *fc1_c = nullptr;
};
struct DecLayerDev {
    void *qkv_w, *o_w, *cq_w, *co_w, *fc1_w, *fc2_w;
    float *qkv_b, *o_b, *cq_b, *co_b, *fc1_b, *fc2_b;
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *ln3_w, *ln3_b;
    // LayerNorm folded into the consumer GEMMs: qkv_w/cq_w/fc1_w hold W ⊙ γ, *_b hold c[n], *_s hold s[n]
    float *qkv_s, *cq_s, *fc1_s;
    // WH_PREC_FP8: every matrix above is raw e4m3 codes [N][K] (one byte each) with these per-output-channel scales;
    // LayerNorm's γ is then applied on the activation side (the producers write x ⊙ γ_next into the slab) and
    // *_s hold sum_k γ[k] * W[n][k], *_b hold c[n], both of the dequantised weights
    float *qkv_sc = nullptr, *o_sc = nullptr, *cq_sc = nullptr, *co_sc = nullptr, *fc1_sc = nullptr, *fc2_sc = nullptr;
    // cross-attention on the encoder states (wh_cross_es.hip, wh_model::cross_es): cqx_w [H][d][64] = head h's rows of the cross W_k,
    // transposed (the query-side expansion); cv_w / cv_b = this layer's plain W_v rows and b_v inside the stacked cross-K/V projection
    void *cqx_w = nullptr, *cv_w = nullptr;
    float* cv_b = nullptr;
};

struct wh_model {
    wh_dims dims{};
    int prec = WH_PREC_BF16;
    int device = 0;
    size_t esz = 2;  // bytes per element of the compute dtype
    // f32 master copy in canonical order (modelspec.tensor_table) + name → (offset, count)
    std::vector<float> master;
    std::map<std::string, std::pair<size_t, size_t>> index;
    // device arena
    char* arena = nullptr;
    size_t arena_bytes = 0;
    int conv1_k = 0;  // 3*n_mels rounded up to 32
    void *conv1_w = nullptr, *conv2_w = nullptr, *tok_emb = nullptr, *cross_kv_w = nullptr;
    float *conv1_b = nullptr, *conv2_b = nullptr, *enc_pos = nullptr, *dec_pos = nullptr, *cross_kv_b = nullptr;
    float *enc_ln_w = nullptr, *enc_ln_b = nullptr, *dec_ln_w = nullptr, *dec_ln_b = nullptr;
    float* cross_kv_sc = nullptr;  // WH_PREC_FP8: scales of the cross K/V projection rows [Ld][2][d]
    void* cross_kv_w8 = nullptr;   // WH_PREC_FP8: the same rows as raw e4m3 codes
    void* cross_kv_wf = nullptr;   // WH_PREC_BF16: the same rows with the encoder's final LayerNorm folded in (+ s, c)
    float *cross_kv_s = nullptr, *cross_kv_c = nullptr;
    void* lm_w = nullptr;  // tied embedding ⊙ final-LN γ (LM head operand); WH_PREC_FP8: the embedding itself (γ on the activation side)
    float *lm_s = nullptr, *lm_c = nullptr;
    bool cross_es = false;   // the decoder layers carry cqx_w / cv_* (bf16, whisper-base geometry)
    std::vector<EncLayerDev> enc;
    std::vector<DecLayerDev> dec;
    // log-mel tables
    double* mel_tw = nullptr;
    float *mel_win = nullptr, *mel_fbT = nullptr;
};

struct wh_ctx {
    wh_model* m = nullptr;
    int max_batch = 1;
    int dec_cus = 256;              // compute units of the token-loop stream (its CU mask's population, else the device's count)
    hipStream_t stream = nullptr;   // cross-K/V projection + token loop (and everything else when s_enc == stream)
    // log-mel + encoder.  The same stream unless the context was created with wh_ctx_create_ex (CU masks / two streams):
    // then the next batch's encoder runs beside this batch's token loop, each on its own part of the chip.
    hipStream_t s_enc = nullptr;
    hipStream_t cur = nullptr;      // stream of the phase being launched (event brackets of the profiling hooks)
    // hand-offs between the two streams: encoder states ready (recorded on s_enc), encoder states consumed by the
    // cross-K/V projection (recorded on stream; the next encoder pass may overwrite them)
    hipEvent_t ev_enc_done = nullptr, ev_kv_done = nullptr;
    bool kv_done_armed = false;
    // stage events of an encoder pass {start, mel done, encoder done}: two sets, because a prefetched pass (the NEXT
    // batch's) is recorded while the resident pass's times have not been read yet
    hipEvent_t enc_ev[2][3] = {{nullptr}};
    int enc_set = 0;                // set of the resident encoder states
    // encoder states prefetched by wh_transcribe_batch_device_next for its `next` batch
    const float* pre_pcm = nullptr;
    int pre_n = 0;
    bool pre_valid = false;
    std::string err;
    wh_timing timing{};
    bool have_enc = false;  // encoder states of `enc_batch` clips are resident
    int enc_batch = 0;
    // profiling hooks
    bool prof = false;
    int prof_mask = 0;  // bit g set: kernel group g is bracketed by events
    int prof_stride = 0;     // > 1: only every stride-th generated position is launched eagerly with events
    bool capturing = false;  // a decode step is being captured into a hipGraph
    bool no_graph = false;  // WH_NO_GRAPH=1: launch every decode step eagerly
    bool sync_every_pos = false;  // WH_SYNC_EVERY_POS=1: host waits after every decoder position (profiler triage only)
    int prof_group = -1;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_events[WH_KG_COUNT];
    size_t prof_used[WH_KG_COUNT] = {0};
    double prof_ms[WH_KG_COUNT] = {0};
    int64_t prof_launches[WH_KG_COUNT] = {0};
    hipEvent_t ev[8] = {nullptr};

    // ---- device workspace (sized for max_batch clips) ----
    char* ws = nullptr;
    size_t ws_bytes = 0;
    float* pcm = nullptr;       // [B][480000]
    size_t pcm_cap = 0;         // samples allocated behind `pcm_long` for whole-file mel
    float* pcm_long = nullptr;  // staged-API / long-form whole file (grown on demand)
    float* raw_long = nullptr;  // [n_mels][frames] raw log-mel of a whole file (grown on demand)
    size_t raw_long_cap = 0;    // frames
    float* mel_out_long = nullptr;
    int* d_nsamp = nullptr;     // [B]
    int* d_nframes = nullptr;   // [B]
    int* d_src_index = nullptr; // [B]
    int* d_frame_start = nullptr;
    unsigned* d_gmax = nullptr; // [B]
    float* raw = nullptr;       // [B][n_mels][3008]
    float* mel_stage = nullptr; // [n_mels][3000] staged-API mel upload
    void* melT = nullptr;       // [B][3002][n_mels] (+slack)
    void* h1 = nullptr;         // [B][3001][d]
    float* x = nullptr;         // [B][S][d] f32 residual stream
    void* xn = nullptr;         // [B][S][d]
    void* qk = nullptr;         // [B][S][2d]
    void* vT = nullptr;         // [B][d][ldv]
    void* att = nullptr;        // [B][S][d]
    void* hbuf = nullptr;       // [B][S][ffn]
    void* enc_out = nullptr;    // [B][S][d] compute dtype (cross-KV GEMM operand)
    // WH_PREC_FP8, MX activations (e4m3 codes + E8M0 block exponents [row][4][K/128]) when the geometry allows (mx_ok)
    bool mx_ok = false;
    unsigned char *xn8 = nullptr, *xn8_sc = nullptr;   // LayerNorm outputs [B*S][d]
    unsigned char *h8 = nullptr, *h8_sc = nullptr;     // GELU(fc1) [B*S][ffn]
    float* enc_out_f32 = nullptr;  // [B][S][d] f32 (API output)
    // WH_PREC_BF16 with the encoder LayerNorms folded into their consumer GEMMs (enc_fold): the residual stream again as bf16
    // (written by the producing GEMM's epilogue; the consumers' operand), the producers' partial sums and {mean, rstd} per row
    bool enc_fold = false;
    bool enc_mlp = false;    // ... and the feed-forward block of a layer as one launch (wh_mlp.hip) where its geometry is covered
    void* xb = nullptr;            // [B][S][d] bf16
    float* enc_part = nullptr;     // [d/64][B*S][2]
    float* enc_stat = nullptr;     // [B*S][2]
    float* enc_shift = nullptr;    // [B*S] running row offsets of the folded LayerNorms (GemmArgs::row_shift)
    float* enc_shift0 = nullptr;   // [B*S] the first producer's offsets: the row means of the positional table (conv2 adds it), fixed
    int ldv = 0;
    void* cross_kv = nullptr;   // [Ld][2][B][S][d]
    // cross-attention on the encoder states (wh_cross_es.hip): decided at creation from the model and the context's capacity.
    // es_E [B][S][d] = the encoder's final LayerNorm output in the compute dtype, decode-side storage like cross_kv (which is
    // then not allocated); dqe [B][H d] f32 expanded queries; dctx = the H d context values per clip, slab layout
    bool cross_es = false;
    void* es_E = nullptr;
    int es_rows = 0;            // rows from one clip's states to the next in es_E (>= n_audio_ctx)
    // workspace placement step of wh_ctx_create_ex: workspaces timed (0: step not taken), the cross-attention launch time on the first and on the kept one
    int place_tries = 0;
    float place_us_first = 0.0f, place_us_kept = 0.0f;
    int es_rows_cap = 0;        // rows per clip the buffer was sized for
    float* dq32 = nullptr;      // [B][d] f32 cross-attention queries (pre-scaled)
    float* dqe = nullptr;
    void* dctx = nullptr;
    void* cross_kv8 = nullptr;  // WH_PREC_FP8: the same planes as e4m3 codes (cross_kv is then the bf16 staging copy)
    float* kv_amax = nullptr;   // WH_PREC_FP8: [Ld][2][B][H] max|.| of each head's block (scale = amax / 448)
    void *self_k = nullptr, *self_v = nullptr;  // [Ld][B][H][TC][64]
    // decode step buffers
    float* dx = nullptr;        // [B][d]
    void* dxn = nullptr;        // [B][d]
    void* dxs = nullptr;        // raw residual rows, compute dtype, slab layout [d/32][mpad][32]
    float* lnpart = nullptr;    // LayerNorm partial sums [d/16][mpad][2]
    float* dshift = nullptr;    // [mpad] running row offsets of the decoder's folded LayerNorms (SkinnyArgs::row_shift / shift_io)
    void* dqkv = nullptr;       // [B][3d]
    void* datt = nullptr;       // [B][d]
    void* dq = nullptr;         // [B][d]
    void* dh = nullptr;         // [B][ffn]
    float* cpart = nullptr;     // [B][splits][d]
    float* cml = nullptr;       // [B][splits][H][2]
    float* part_val = nullptr;  // [B][n_tiles]
    int* part_idx = nullptr;
    int *feed = nullptr, *out_tokens = nullptr, *n_out = nullptr, *done = nullptr, *forced = nullptr, *pos = nullptr;
    int* step_ticket = nullptr;  // zeroed at creation, re-armed by its last arriver
    unsigned *mask_first = nullptr, *mask_base = nullptr;
    float* logits = nullptr;    // optional parity buffer (grown on demand)
    size_t logits_cap = 0;
    int* logits_sel = nullptr;  // [B]: slot of a batch row in `logits` or -1 (wh_decode_greedy_rows)
    // wh_transcribe_batch_next: the next batch's PCM copied to a second device buffer on a copy stream beside this batch's work
    float* pcm2 = nullptr;      // [B][480000], allocated at the first call of that entry
    hipStream_t s_copy = nullptr;
    hipEvent_t ev_h2d = nullptr;
    int h2d_buf = 0;            // buffer (0: pcm, 1: pcm2) that holds / will hold the prefetched batch
    const float* h2d_src = nullptr;   // host address of the prefetched batch's first clip
    int h2d_n = 0;
    bool h2d_valid = false;
    std::vector<int> h2d_ns, h2d_nf;  // its per-clip sample / frame counts
    // raw audio ingest: two grow-only staging buffers for the clips' raw bytes (the batch being converted, and the next batch's
    // prefetch on the copy stream) and the descriptors' device copy; allocated by the first raw entry that needs them
    void* ing_raw[2] = {nullptr, nullptr};
    size_t ing_raw_cap[2] = {0, 0};
    struct WhIngestDesc* ing_desc = nullptr;   // [max_batch]
    // the conversion the next encoder pass runs before its log-mel (inside the pass's preprocess events); n == 0: none
    int ing_n = 0, ing_buf = 0;
    size_t ing_max_out = 0;
    int ing_last_n = 0, ing_last_buf = 0;      // the last conversion into c->pcm (measurement hook wh_debug_ingest_times)
    size_t ing_last_max_out = 0;
    bool h2d_is_raw = false;                   // the pending prefetch is a raw batch in ing_raw[h2d_buf] (else f32 PCM in pcm / pcm2)
    std::vector<wh_raw_clip> h2d_raw_clips;    // its clips, every field
    int tok_ld = 0;
    int mpad = 16;              // row pitch of the k-slab-major decode activations (multiple of 16)
    int cross_splits = 1;
    // the decode GEMMs as LDS-DMA tile GEMMs (wh_dec_tile.hip): decided at creation from the model and the context's capacity
    bool dec_tile = false;
    // The decode step's key: every call-dependent value an emitting decoder position bakes into kernel arguments.  launch_step (wh_api.cpp)
    // sees the context and this struct and nothing else of the call, so a value that is not listed here cannot reach the captured step; the
    // context supplies only fixed workspace addresses and the option buffers.  A call with the same key replays the instantiated graph as it
    // is; the graph is destroyed in wh_ctx_free (after the stream has drained) or when the key changes.
    // The rule for the option buffers: a setter that frees or reallocates a buffer the step holds calls drop_step_graph first.
    // What follows from the members needs no entry of its own: 1 / rep_p, the repetition exemption from ts_begin (and ts_ld = vocab -
    // ts_begin), the non-temporal cross-K/V loads and the cache strides from nb, the LM head's partial count from the shape.
    struct StepKey {
        int nb = 0, n_prompt = 0, eot = 0, n_forced = 0, logits_rows = 0;
        float* d_logits = nullptr;
        const int* d_sel = nullptr;
        int ts_begin = -1, ts_max_init = -1;   // timestamp rules: ts_begin -1 = off (other kernels, other arguments)
        float* lp_sum = nullptr;               // token log-probabilities: nullptr = off (other kernels, other arguments)
        bool pfx = false;                      // per-clip prefixes with a non-empty one in the batch: the prefix-aware kernels
        bool rep = false;                      // repetition penalty / no-repeat n-grams: other kernels, other arguments
        float rep_p = 1.0f;
        int rep_n = 0;
        float* al_q = nullptr;                 // word-level timestamps: nullptr = off (no launch); the side buffer the queries are copied to,
        int al_cap = 0;                        // its rows per clip (the call's max_new_tokens) and the identity of the head list (al_gen)
        unsigned al_gen = 0;
        int beam_k = 0, beam_c = 0;            // beam search: beam_k 0 = off; nb then counts rows = clips x beam_k.  beam_buf: the identity of the
        const void* beam_buf = nullptr;        // setter's buffers (logits scratch and search state: one allocation each, freed together)
        const void* sample_buf = nullptr;      // temperature sampling: nullptr = off; the identity of the setter's buffers (the per-row values are read through them)
        auto members() const { return std::tie(nb, n_prompt, eot, n_forced, logits_rows, d_logits, d_sel, ts_begin, ts_max_init, lp_sum, pfx, rep, rep_p, rep_n, al_q, al_cap, al_gen, beam_k, beam_c, beam_buf, sample_buf); }
        bool operator==(const StepKey& o) const { return members() == o.members(); }
    } step_key;
    // Whisper's timestamp rules (wh_ctx_set_timestamp_rules): off unless ts_on.  The timestamp logits and the per-row state
    // are allocated when rules are set (not part of the workspace carve; the logits again when timestamp_begin changes) and freed in wh_ctx_free.
    bool ts_on = false;
    int64_t ts_begin = 0, ts_no_ts = -1;
    int ts_max_init = 50;
    float* ts_logits = nullptr; // [mpad][ts_ld] allowed timestamp logits of the current position (-inf: not allowed)
    int ts_ld = 0;              // vocab - timestamp_begin
    int* ts_state = nullptr;    // [mpad][4] {text_lo, ts_lo, ts_hi, last timestamp}
    // Token log-probabilities and the no-speech probe (wh_ctx_set_logprobs): off unless lp_on.  One allocation made by the setter
    // (not part of the workspace carve), freed in wh_ctx_free: the (max, sum) partials' sums, the tokens' log-probabilities, an all-zero
    // suppress mask, the probe's logit and its result.
    bool lp_on = false;
    int64_t lp_no_speech = -1;
    int lp_sot_index = 0;
    char* lp_buf = nullptr;
    float* lp_part_sum = nullptr;   // [part][mpad], beside part_val / part_idx
    float* lp_tok = nullptr;        // [max_batch][tok_ld], DecodeState::logprob
    unsigned* lp_mask_zero = nullptr;
    float* lp_probe_v = nullptr;    // [mpad] logit of no_speech at the probed position
    float* lp_ns = nullptr;         // [max_batch] no-speech probability
    // what wh_get_logprobs returns: the last decode call's clips in the order their tokens were returned (a long-form call: every device batch)
    bool lp_have = false, lp_have_ns = false;
    std::vector<std::vector<float>> lp_rows;
    std::vector<float> lp_ns_rows;
    // Language detection (wh_ctx_set_language_detection): off unless lang_on.  One allocation made by the setter (not part of the
    // workspace carve), freed in wh_ctx_free: the id list, the listed ids' logits, the probabilities and the chosen ids.  Lives in the eagerly
    // launched prompt positions only (launch_step's PromptStep): the captured step and its key know nothing of it.
    bool lang_on = false;
    int lang_sot_index = 0;
    std::vector<int64_t> lang_ids;  // the caller's list, in the caller's order
    char* lang_buf = nullptr;
    int* lang_d_ids = nullptr;      // [WH_LANG_LD], padded with the first listed id
    float* lang_logits = nullptr;   // [mpad][WH_LANG_LD]
    float* lang_probs = nullptr;    // [max_batch][n_lang]
    int* lang_chosen = nullptr;     // [max_batch]
    // long-form: the first device batch detects on its row 0 for every row (lang_bcast); later batches of the same call decode with that id
    // in the prompt (lang_fixed >= 0) and report window 0's probabilities
    bool lang_bcast = false;
    int64_t lang_fixed = -1;
    // what wh_get_languages returns: the last decode call's clips in the order their tokens were returned
    bool lang_have = false;
    size_t lang_have_n = 0;         // n_lang of that call
    std::vector<int64_t> lang_rows;
    std::vector<float> lang_prob_rows;   // [clips][lang_have_n]
    // Per-clip prompt prefixes (wh_ctx_set_prefixes): off unless pfx_on.  pfx_off is allocated by the first setter call (not part
    // of the workspace carve) and freed in wh_ctx_free; upload_token_state fills it per call.  A call whose rows all have empty prefixes passes no
    // offsets to the kernels and launches what a context without prefixes launches.
    bool pfx_on = false;
    std::vector<int64_t> pfx_ids;      // the clips' prefixes back to back (the setter's copy)
    std::vector<size_t> pfx_offsets;   // [n_clips + 1]
    int pfx_scope = 0;                 // WH_PREFIX_*
    int* pfx_off = nullptr;            // [max_batch] device: first live global position of each row (Nmax - n_b)
    long pfx_win_base = -1;            // long-form: index of the device batch's first window (row b is window pfx_win_base + b); -1: rows are clips
    // Repetition penalty / no-repeat n-grams (wh_ctx_set_repetition): off unless rep_on.  The bitmap and the side buffer are
    // allocated by the setter (not part of the workspace carve) and freed when the option is cleared and in wh_ctx_free; upload_token_state clears
    // the bitmap at the start of a call.
    bool rep_on = false;
    float rep_p = 1.0f;
    int rep_n = 0;
    int rep_words = 0;                 // ceil(vocab / 32)
    unsigned* rep_bits = nullptr;      // [max_batch][rep_words] touched ids of each row's current position
    float* rep_side = nullptr;         // [max_batch][vocab] raw logits of the touched ids (only those entries are written)
    // Word-level timestamps (wh_ctx_set_alignment): off unless al_on.  The captured step copies the listed heads' queries into
    // al_q (grown on demand by a call; the step graph is dropped when its address changes); the post-pass of a call works in al_ws, a chunk of
    // clips at a time.  al_d (frames + per-clip frame counts) is allocated by the setter and freed in wh_ctx_free with the rest.
    bool al_on = false;
    unsigned al_gen = 0;                       // counts the setter's calls: the identity of the head list in the step's key
    std::vector<int> al_heads;                 // [n][2] (layer, head), the caller's order
    std::vector<int> al_debug;                 // batch rows whose P and M are kept
    std::vector<AlignLayerHeads> al_layer;     // [dec_layers] the listed heads of each layer
    float* al_q = nullptr;                     // [n_heads][nb][max_new_tokens][dk] f32
    size_t al_q_cap = 0;                       // floats
    char* al_ws = nullptr;                     // post-pass workspace: P, M, the DTW steps of one chunk of clips
    size_t al_ws_cap = 0;                      // bytes
    int* al_frames = nullptr;                  // [max_batch][n_text_ctx] frame of each generated token
    int* al_sb = nullptr;                      // [max_batch] S_b of each row
    bool al_timing = false;                    // WH_ALIGN_TIMING=1: events around the three post-pass kernels (tools/align_bench.py)
    double al_ms[3] = {0, 0, 0};               // scores, filter, DTW of the last call, milliseconds
    std::vector<int> enc_nframes;              // mel frames of each clip whose encoder states are resident (what S_b derives from)
    // what wh_get_token_frames / wh_get_alignment_debug return: the last decode call's clips in the order their tokens were returned
    bool al_have = false;
    std::vector<std::vector<int>> al_rows;
    std::vector<int> al_nframes;
    struct AlignDebug { int n_heads = 0, n_gen = 0, sb = 0; std::vector<float> probs, matrix; };
    std::vector<AlignDebug> al_dbg;
    // Beam search (wh_ctx_set_beam_search): off unless bm_on.  The logits scratch and the search state are allocated by the setter
    // (not part of the workspace carve) and freed when the option is cleared and in wh_ctx_free; the captured step is dropped before that.
    bool bm_on = false;
    int bm_k = 0, bm_c = 0;
    float bm_length_penalty = -1.0f;
    std::vector<int> bm_trace_clips;
    float* bm_logits = nullptr;       // [max_batch][vocab] raw logits of the current position
    char* bm_buf = nullptr;           // the search state, carved into:
    float* bm_scores = nullptr;       // [max_batch]
    int* bm_parent = nullptr;         // [max_batch]
    int* bm_state = nullptr;          // [max_batch][WH_BEAM_STATE]
    int* bm_pool_n = nullptr;         // [max_batch] per clip
    int* bm_n_steps = nullptr;        // [max_batch] per clip
    int* bm_pool = nullptr;           // [max_batch][WH_MAX_BEAM_CANDIDATES][4] per clip
    int *bm_tr_parent = nullptr, *bm_tr_token = nullptr, *bm_tr_pool = nullptr;   // [tok_ld][max_batch]
    float *bm_tr_score = nullptr, *bm_tr_lp = nullptr;
    // what wh_get_beams / wh_get_beam_trace return: the last decode call's clips in the order their tokens were returned
    struct BeamHyp { std::vector<int> tokens; std::vector<float> lps; float sum = 0.0f, rank = 0.0f; bool finished = false; };
    struct BeamTrace { int K = 0, n_steps = 0; std::vector<int> parents, tokens, pool; std::vector<float> scores; };
    bool bm_timing = false;                    // WH_BEAM_TIMING=1: events around the two kernels of every eagerly launched position (tools/beam_bench.py)
    std::vector<std::array<hipEvent_t, 3>> bm_events;
    double bm_ms[2] = {0, 0};                  // k_beam_select, k_beam_reorder of the last call, milliseconds, over bm_timed positions
    long bm_timed = 0;
    bool bm_have = false;
    std::vector<std::vector<BeamHyp>> bm_hyps;
    std::vector<BeamTrace> bm_traces;
    // Temperature sampling (wh_ctx_set_sampling): off unless sm_on.  The logits scratch and the per-row values are allocated by
    // the setter (not part of the workspace carve) and freed when the option is cleared and in wh_ctx_free; the captured step is dropped before
    // that.  The setter keeps the caller's lists; upload_token_state writes each call's rows to the device.
    bool sm_on = false;
    uint64_t sm_seed = 0;
    std::vector<float> sm_temp;            // [n_rows]
    std::vector<uint8_t> sm_active;        // [n_rows]
    std::vector<uint64_t> sm_ids;          // [n_rows]
    float* sm_logits = nullptr;            // [max_batch][vocab] raw logits of the current position
    char* sm_buf = nullptr;                // carved into:
    float* sm_d_temp = nullptr;            // [max_batch]
    unsigned long long* sm_d_ids = nullptr;    // [max_batch]
    unsigned long long* sm_d_seed = nullptr;   // [1]
    int* sm_state = nullptr;               // [max_batch][4] rule state of each row
    float* sm_lp = nullptr;                // [max_batch][tok_ld] DecodeState::logprob of a sampling call
    bool sm_timing = false;                // WH_SAMPLE_TIMING=1: events around k_sample_select of every eagerly launched position (tools/sample_bench.py)
    std::vector<std::array<hipEvent_t, 2>> sm_events;
    double sm_ms = 0;                      // k_sample_select of the last call, milliseconds, over sm_timed positions
    long sm_timed = 0;
    hipGraph_t step_graph = nullptr;
    hipGraphExec_t step_exec = nullptr;
};

// Linear weights that arrived already quantised (F8_E4M3 + "<name>_scale" in model.safetensors, written by
// quantize_fp8.py): keyed by the tensor's offset in the f32 master blob, which then holds dequant(code) * scale.
// WH_PREC_FP8 uses these codes and scales as they are instead of quantising the master copy again.
struct WhPreQuantEntry {
    std::vector<uint8_t> codes;  // [rows][cols]
    std::vector<float> scale;    // [rows]
};
typedef std::map<size_t, WhPreQuantEntry> WhPreQuant;

// wh_model.cpp
int wh_model_build(const wh_dims& dims, std::vector<float>&& master, int device, int precision, wh_model** out,
                   const WhPreQuant* pre = nullptr);
void wh_synth_weights(const wh_dims& dims, uint64_t seed, std::vector<float>& out);
void wh_tensor_table(const wh_dims& dims, std::vector<std::pair<std::string, std::vector<int64_t>>>& out);
bool wh_preset_dims(const std::string& name, wh_dims* out);
uint8_t wh_e4m3_from_f32(float x);
float wh_e4m3_to_f32(uint8_t c);
int wh_load_model_dir(const std::string& dir, wh_dims* dims, std::vector<float>& master, WhPreQuant* pre = nullptr);
