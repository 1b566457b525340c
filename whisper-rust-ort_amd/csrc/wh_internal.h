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

// A hipMalloc'ed block and its size in bytes: move-only, freed by reset() and by the destructor.  A context's buffers are members of wh_ctx, so
// `delete c` at the end of wh_ctx_free frees them — after the streams have drained and the step graph is gone.  Converts to its T*.
template <typename T = char>
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) hipFree(p); p = nullptr; bytes = 0; }
    operator T*() const { return (T*)p; }
};

// the events of a timing hook, N per timed position: adds the N - 1 intervals to ms (nullptr: the call failed before its read-back) and destroys them
template <size_t N>
void wh_drain_events(std::vector<std::array<hipEvent_t, N>>& events, double* ms) {
    for (auto& te : events) {
        for (size_t i = 0; ms && i + 1 < N; i++) { float t = 0; hipEventElapsedTime(&t, te[i], te[i + 1]); ms[i] += t; }
        for (auto& e : te) hipEventDestroy(e);
    }
    events.clear();
}

struct wh_ctx {
    wh_model* m = nullptr;
    int max_batch = 1;
    int dec_cus = 256;              // compute units of the token-loop stream (its CU mask's population, else the device's count)
    hipStream_t stream = nullptr;   // cross-K/V projection + token loop (and everything else when s_enc == stream)
    // log-mel + encoder.  The same stream unless the context was created with wh_ctx_create_ex (CU masks / two streams):
    // then the next batch's encoder runs beside this batch's token loop, each on its own part of the chip.
    hipStream_t s_enc = nullptr;
    hipStream_t cur = nullptr;      // stream of the phase being launched (event brackets of the profiling hooks)
    // The split token loop: a generated position runs the decoder layers of two row ranges of the batch as two branches, the
    // second on s_split (created with the token-loop stream's CU mask, at the first call that splits), forked and joined through split_ev.
    // split_mode / split_rows / split_cus: WH_DEC_SPLIT (0 off, 1 on, unset: the rule of choose_split), WH_DEC_SPLIT_ROWS (rows of the first
    // range, 0: half the batch) and WH_DEC_SPLIT_CUS (compute units of a range's cross-attention launch), read at creation for A/B runs.
    // dbg_split: wh_debug_set_step_split's forced first-range rows (0: none); last_split: what the last decode call ran with (0: one chain)
    hipStream_t s_split = nullptr;
    std::vector<hipEvent_t> split_ev;
    std::vector<uint32_t> dec_mask;
    int split_mode = -1, split_rows = 0, split_cus = 160, dbg_split = 0, last_split = 0;
    // The free-running halves: the two ranges of a split call run whole positions, LM head and finish included, each on its own
    // stream with its own device-side position (pos[1], step_ticket[1]: the second range's), ordered by two events per position (free_ev).
    // free_mode: WH_DEC_FREE (0 off, 1 on, unset: on wherever choose_split splits by its rule); free_eb: WH_DEC_FREE_EB=0 drops the edge that
    // keeps the first range at most one position ahead (A/B runs); dbg_free: wh_debug_set_step_free; last_free: the last call's loop ran free
    std::vector<hipEvent_t> free_ev;
    int free_mode = -1, dbg_free = 0, last_free = 0;
    bool free_eb = true;
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
    DevBuf<> ws;
    float* pcm = nullptr;       // [B][480000]
    DevBuf<float> pcm_long;     // staged-API / long-form whole file (grown on demand)
    DevBuf<float> raw_long;     // [n_mels][frames] raw log-mel of a whole file (grown on demand)
    DevBuf<float> mel_out_long;
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
    // pos and step_ticket are two elements each: everything that runs on the whole batch uses element 0; element 1 is the second row range's
    // own position and ticket while the halves of the token loop run free
    unsigned *mask_first = nullptr, *mask_base = nullptr;
    DevBuf<float> logits;       // optional parity buffer (grown on demand)
    int* logits_sel = nullptr;  // [B]: slot of a batch row in `logits` or -1 (wh_decode_greedy_rows)
    // wh_transcribe_batch_next: the next batch's PCM copied to a second device buffer on a copy stream beside this batch's work
    DevBuf<float> pcm2;         // [B][480000], allocated at the first call of that entry
    hipStream_t s_copy = nullptr;
    hipEvent_t ev_h2d = nullptr;
    int h2d_buf = 0;            // buffer (0: pcm, 1: pcm2) that holds / will hold the prefetched batch
    const float* h2d_src = nullptr;   // host address of the prefetched batch's first clip
    int h2d_n = 0;
    bool h2d_valid = false;
    std::vector<int> h2d_ns, h2d_nf;  // its per-clip sample / frame counts
    // raw audio ingest: two grow-only staging buffers for the clips' raw bytes (the batch being converted, and the next batch's
    // prefetch on the copy stream) and the descriptors' device copy; allocated by the first raw entry that needs them
    DevBuf<> ing_raw[2];
    DevBuf<WhIngestDesc> ing_desc;      // [max_batch]
    // the conversion the next encoder pass runs before its log-mel (inside the pass's preprocess events); n == 0: none
    int ing_n = 0, ing_buf = 0;
    size_t ing_max_out = 0;
    int ing_last_n = 0, ing_last_buf = 0;      // the last conversion into c->pcm (measurement hook wh_debug_ingest_times)
    size_t ing_last_max_out = 0;
    bool h2d_is_raw = false;                   // the pending prefetch is a raw batch in ing_raw[h2d_buf] (else f32 PCM in pcm / pcm2)
    std::vector<wh_raw_clip> h2d_raw_clips;    // its clips, every field
    // The resident file set (wh_files_load / wh_files_load_raw): the whole-file raw log-mels of many files in one ragged store,
    // which wh_transcribe_windows cuts its rows from.  Its own buffers, like an option's: no other entry reads or writes them (raw_long stays
    // the one-file entries').  Allocated by the first load, grown by a later one that needs more, freed by wh_files_load(NULL, 0) and with the context.
    struct FileSet {
        size_t n = 0;                     // files loaded; 0: no set
        DevBuf<float> mel;                // file f: [n_mels][ld_f] raw log-power at host[f].base
        DevBuf<WhFileDesc> desc;          // [WH_MAX_FILES] what k_mel_window looks up per row (gmax written by the file's k_mel_stft)
        DevBuf<WhIngestDesc> ing;         // [WH_MAX_FILES] the raw load's conversion descriptors
        DevBuf<int> rows;                 // [2][max_batch] the file and the seek of each row of a window call
        std::vector<WhFileDesc> host;     // the descriptors' host copy (gmax not filled)
    } fs;
    int tok_ld = 0;
    int mpad = 16;              // row pitch of the k-slab-major decode activations (multiple of 16)
    int cross_splits = 1;
    // the decode GEMMs as LDS-DMA tile GEMMs (wh_dec_tile.hip): decided at creation from the model and the context's capacity
    bool dec_tile = false;
    // The decode step's key: every call-dependent value an emitting decoder position bakes into kernel arguments.  launch_step (wh_decode_host.cpp)
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
        int split = 0, split_cus = 0;          // the split token loop: rows of the first range (0 = one chain) and the compute units of a range's cross-attention launch
        bool free = false;                     // ... and its ranges run whole positions on their own streams, four single-chain graphs
        auto members() const { return std::tie(split, split_cus, free, nb, n_prompt, eot, n_forced, logits_rows, d_logits, d_sel, ts_begin, ts_max_init, lp_sum, pfx, rep, rep_p, rep_n, al_q, al_cap, al_gen, beam_k, beam_c, beam_buf, sample_buf); }
        bool operator==(const StepKey& o) const { return members() == o.members(); }
    } step_key;
    // ---- the decode options: one struct each, laid out alike — `on` and the settings, the device buffers (DevBuf: freed with the context or
    // when the struct is reset), what the getter returns for the last call, and the timing hook's fields where the option has one.
    // reset_results() forgets the last call (check_params, first thing in every decode entry).  DESIGN.md §5g, "An option's state".
    // Whisper's timestamp rules (wh_ctx_set_timestamp_rules): off unless on.  The timestamp logits and the per-row state
    // are allocated when rules are set (not part of the workspace carve; the logits again when timestamp_begin changes) and freed with the context.
    struct TimestampRules {
        bool on = false;
        int64_t begin = 0, no_ts = -1;
        int max_init = 50;
        int ld = 0;                 // vocab - timestamp_begin
        DevBuf<float> logits;       // [mpad][ld] allowed timestamp logits of the current position (-inf: not allowed)
        DevBuf<int> state;          // [mpad][4] {text_lo, ts_lo, ts_hi, last timestamp}
        void reset_results() {}
    } ts;
    // Token log-probabilities and the no-speech probe (wh_ctx_set_logprobs): off unless on.  One allocation made by the setter
    // (not part of the workspace carve), freed with the context: the (max, sum) partials' sums, the tokens' log-probabilities, an all-zero
    // suppress mask, the probe's logit and its result.
    struct Logprobs {
        bool on = false;
        int64_t no_speech = -1;
        int sot_index = 0;
        DevBuf<> buf;
        float* part_sum = nullptr;   // [part][mpad], beside part_val / part_idx
        float* tok = nullptr;        // [max_batch][tok_ld], DecodeState::logprob
        unsigned* mask_zero = nullptr;
        float* probe_v = nullptr;    // [mpad] logit of no_speech at the probed position
        float* ns = nullptr;         // [max_batch] no-speech probability
        // what wh_get_logprobs returns: the last decode call's clips in the order their tokens were returned (a long-form call: every device batch)
        bool have = false, have_ns = false;
        std::vector<std::vector<float>> rows;
        std::vector<float> ns_rows;
        void reset_results() { have = have_ns = false; rows.clear(); ns_rows.clear(); }
    } lp;
    // Language detection (wh_ctx_set_language_detection): off unless on.  One allocation made by the setter (not part of the
    // workspace carve), freed with the context: the id list, the listed ids' logits, the probabilities and the chosen ids.  Lives in the eagerly
    // launched prompt positions only (launch_step's PromptStep): the captured step and its key know nothing of it.
    struct LanguageDetection {
        bool on = false;
        int sot_index = 0;
        std::vector<int64_t> ids;   // the caller's list, in the caller's order
        DevBuf<> buf;
        int* d_ids = nullptr;       // [WH_LANG_LD], padded with the first listed id
        float* logits = nullptr;    // [mpad][WH_LANG_LD]
        float* probs = nullptr;     // [max_batch][n_lang]
        int* chosen = nullptr;      // [max_batch]
        // long-form: the first device batch detects on its row 0 for every row (bcast); later batches of the same call decode with that id
        // in the prompt (fixed >= 0) and report window 0's probabilities
        bool bcast = false;
        int64_t fixed = -1;
        // what wh_get_languages returns: the last decode call's clips in the order their tokens were returned
        bool have = false;
        size_t have_n = 0;          // n_lang of that call
        std::vector<int64_t> rows;
        std::vector<float> prob_rows;   // [clips][have_n]
        void reset_results() { have = false; rows.clear(); prob_rows.clear(); }
    } lang;
    // Per-clip prompt prefixes (wh_ctx_set_prefixes): off unless on.  `off` is allocated by the first setter call (not part
    // of the workspace carve) and freed with the context; upload_token_state fills it per call.  A call whose rows all have empty prefixes passes no
    // offsets to the kernels and launches what a context without prefixes launches.
    struct Prefixes {
        bool on = false;
        std::vector<int64_t> ids;      // the clips' prefixes back to back (the setter's copy)
        std::vector<size_t> offsets;   // [n_clips + 1]
        int scope = 0;                 // WH_PREFIX_*
        long win_base = -1;            // long-form: index of the device batch's first window (row b is window win_base + b); -1: rows are clips
        DevBuf<int> off;               // [max_batch] device: first live global position of each row (Nmax - n_b)
        void reset_results() {}
    } pfx;
    // Repetition penalty / no-repeat n-grams (wh_ctx_set_repetition): off unless on.  The bitmap and the side buffer are
    // allocated by the setter (not part of the workspace carve) and freed when the option is cleared and with the context; upload_token_state
    // clears the bitmap at the start of a call.
    struct Repetition {
        bool on = false;
        float p = 1.0f;
        int n = 0;
        int words = 0;                 // ceil(vocab / 32)
        DevBuf<unsigned> bits;         // [max_batch][words] touched ids of each row's current position
        DevBuf<float> side;            // [max_batch][vocab] raw logits of the touched ids (only those entries are written)
        bool held() const { return bits || side; }   // buffers the captured step may hold
        void reset_results() {}
    } rep;
    // Word-level timestamps (wh_ctx_set_alignment): off unless on.  The captured step copies the listed heads' queries into
    // q (grown on demand by a call; the step graph is dropped when its address changes); the post-pass of a call works in ws, a chunk of
    // clips at a time.  frames and sb (per-clip frame counts) are allocated by the setter and freed with the context like the rest.
    struct AlignDebug { int n_heads = 0, n_gen = 0, sb = 0; std::vector<float> probs, matrix; };
    struct Alignment {
        bool on = false;
        unsigned gen = 0;                       // counts the setter's calls: the identity of the head list in the step's key
        std::vector<int> heads;                 // [n][2] (layer, head), the caller's order
        std::vector<int> debug;                 // batch rows whose P and M are kept
        std::vector<AlignLayerHeads> layer;     // [dec_layers] the listed heads of each layer
        DevBuf<float> q;                        // [n_heads][nb][max_new_tokens][dk] f32
        DevBuf<> ws;                            // post-pass workspace: P, M, the DTW steps of one chunk of clips
        DevBuf<int> frames;                     // [max_batch][n_text_ctx] frame of each generated token
        DevBuf<int> sb;                         // [max_batch] S_b of each row
        // what wh_get_token_frames / wh_get_alignment_debug return: the last decode call's clips in the order their tokens were returned
        bool have = false;
        std::vector<std::vector<int>> rows;
        std::vector<int> nframes;
        std::vector<AlignDebug> dbg;
        bool timing = false;                    // WH_ALIGN_TIMING=1: events around the three post-pass kernels (tools/align_bench.py)
        double ms[3] = {0, 0, 0};               // scores, filter, DTW of the last call, milliseconds
        bool have_dbg = false;                  // dbg belongs to a wh_align_tokens call: wh_get_alignment_debug serves it, wh_get_token_frames does not
        void reset_results() { have = have_dbg = false; rows.clear(); nframes.clear(); dbg.clear(); }
    } al;
    // Forced alignment of given transcripts (wh_align_tokens): no setting, its own buffers only — grown on demand by the calls,
    // freed with the context.  No captured step holds them, and the call touches none of `al`'s device buffers.
    struct ForcedAlign {
        DevBuf<float> q;                        // [n_heads][G][Lmax][dk] f32: the listed heads' queries of a pass's hypotheses (k_align_gather)
        DevBuf<> ws;                            // post-pass workspace of one chunk of hypotheses
        DevBuf<int> ints;                       // carved into frames [G][Lmax], sb [G], n_out [G] (P + n_g) of a pass: 3 x max_batch ints
        std::vector<std::array<hipEvent_t, 2>> ev_gather;   // WH_ALIGN_TIMING=1 (tools/forced_align_bench.py): events around every k_align_gather
        double ms_gather = 0;
        void reset_results() { wh_drain_events(ev_gather, nullptr); }
    } fa;
    std::vector<int> enc_nframes;              // mel frames of each clip whose encoder states are resident (what alignment's S_b derives from)
    // Beam search (wh_ctx_set_beam_search): off unless on.  The logits scratch and the search state are allocated by the setter
    // (not part of the workspace carve) and freed when the option is cleared and with the context; the captured step is dropped before that.
    struct BeamHyp { std::vector<int> tokens; std::vector<float> lps; float sum = 0.0f, rank = 0.0f; bool finished = false; };
    struct BeamTrace { int K = 0, n_steps = 0; std::vector<int> parents, tokens, pool; std::vector<float> scores; };
    struct BeamSearch {
        bool on = false;
        int k = 0, c = 0;
        float length_penalty = -1.0f;
        std::vector<int> trace_clips;
        DevBuf<float> logits;          // [max_batch][vocab] raw logits of the current position
        DevBuf<> buf;                  // the search state, carved into:
        float* scores = nullptr;       // [max_batch]
        int* parent = nullptr;         // [max_batch]
        int* state = nullptr;          // [max_batch][WH_BEAM_STATE]
        int* pool_n = nullptr;         // [max_batch] per clip
        int* n_steps = nullptr;        // [max_batch] per clip
        int* pool = nullptr;           // [max_batch][WH_MAX_BEAM_CANDIDATES][4] per clip
        int *tr_parent = nullptr, *tr_token = nullptr, *tr_pool = nullptr;   // [tok_ld][max_batch]
        float *tr_score = nullptr, *tr_lp = nullptr;
        bool held() const { return logits || buf; }   // buffers the captured step may hold
        // what wh_get_beams / wh_get_beam_trace return: the last decode call's clips in the order their tokens were returned
        bool have = false;
        std::vector<std::vector<BeamHyp>> hyps;
        std::vector<BeamTrace> traces;
        bool timing = false;                    // WH_BEAM_TIMING=1: events around the two kernels of every eagerly launched position (tools/beam_bench.py)
        std::vector<std::array<hipEvent_t, 3>> events;
        double ms[2] = {0, 0};                  // k_beam_select, k_beam_reorder of the last call, milliseconds, over `timed` positions
        long timed = 0;
        void collect_timing() { ms[0] = ms[1] = 0; timed = (long)events.size(); wh_drain_events(events, ms); }
        void reset_results() { have = false; hyps.clear(); traces.clear(); wh_drain_events(events, nullptr); }   // (events of a call that failed before its read-back)
    } bm;
    // Temperature sampling (wh_ctx_set_sampling): off unless on.  The logits scratch and the per-row values are allocated by
    // the setter (not part of the workspace carve) and freed when the option is cleared and with the context; the captured step is dropped before
    // that.  The setter keeps the caller's lists; upload_token_state writes each call's rows to the device.
    struct Sampling {
        bool on = false;
        uint64_t seed = 0;
        std::vector<float> temp;            // [n_rows]
        std::vector<uint8_t> active;        // [n_rows]
        std::vector<uint64_t> ids;          // [n_rows]
        DevBuf<float> logits;               // [max_batch][vocab] raw logits of the current position
        DevBuf<> buf;                       // carved into:
        float* d_temp = nullptr;            // [max_batch]
        unsigned long long* d_ids = nullptr;    // [max_batch]
        unsigned long long* d_seed = nullptr;   // [1]
        int* state = nullptr;               // [max_batch][4] rule state of each row
        float* lp = nullptr;                // [max_batch][tok_ld] DecodeState::logprob of a sampling call
        bool held() const { return logits || buf; }   // buffers the captured step may hold
        bool timing = false;                // WH_SAMPLE_TIMING=1: events around k_sample_select of every eagerly launched position (tools/sample_bench.py)
        std::vector<std::array<hipEvent_t, 2>> events;
        double ms = 0;                      // k_sample_select of the last call, milliseconds, over `timed` positions
        long timed = 0;
        void collect_timing() { ms = 0; timed = (long)events.size(); wh_drain_events(events, &ms); }
        void reset_results() { wh_drain_events(events, nullptr); }
    } sm;
    // Scoring given transcripts (wh_score_tokens): no setting, its own buffers only — allocated by the first scoring call, freed
    // with the context.  No captured step holds them: the pass is launched eagerly.
    struct Scoring {
        DevBuf<float> logits;               // [max_batch][vocab] raw logits of a pass's rows (the LM head's scratch)
        DevBuf<> buf;                       // carved into:
        int* tok = nullptr;                 // [n_text_ctx + max_batch] the rows' input tokens from index T - 1 on (k_dec_embed reads feed[row + *pos])
        int* off = nullptr;                 // [max_batch] T - 1 - t of each row: k_dec_embed<T, true> then embeds model position t
        int* len = nullptr;                 // [max_batch] tokens of each hypothesis of the pass
        int* target = nullptr;              // [max_batch] the given tokens, [hypothesis][Lmax]
        float* lp = nullptr;                // [max_batch] log-probabilities, [hypothesis][Lmax]
        int* am = nullptr;                  // [max_batch] argmax, [hypothesis][Lmax]
        bool timing = false;                // WH_SCORE_TIMING=1: events around the two scoring kernels (tools/score_bench.py)
        std::vector<std::array<hipEvent_t, 2>> ev_attn, ev_finish;
        double ms[2] = {0, 0};              // k_score_self_attn (all layers), k_score_finish of the last call, milliseconds
        void collect_timing() { ms[0] = ms[1] = 0; wh_drain_events(ev_attn, &ms[0]); wh_drain_events(ev_finish, &ms[1]); }
        void reset_results() { wh_drain_events(ev_attn, nullptr); wh_drain_events(ev_finish, nullptr); }
    } sc;
    void reset_option_results() { sc.reset_results(); fa.reset_results(); ts.reset_results(); lp.reset_results(); lang.reset_results(); pfx.reset_results(); rep.reset_results(); al.reset_results(); bm.reset_results(); sm.reset_results(); }
    // the captured step: one graph (element 0), or the four single-chain segments of the free-running halves (A1, A2, B1, B2)
    static constexpr int STEP_GRAPHS = 4;
    hipGraph_t step_graph[STEP_GRAPHS] = {nullptr, nullptr, nullptr, nullptr};
    hipGraphExec_t step_exec[STEP_GRAPHS] = {nullptr, nullptr, nullptr, nullptr};
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
