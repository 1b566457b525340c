// wh_host_capi.cpp — C entry points over wh_host.h so the host logic (statistics, emitters,
// resampler, stitcher, detokeniser) can be unit-tested from Python without a GPU.
#include <cstring>

#include "wh_host.h"

using namespace whhost;

static size_t put(const std::string& s, char* out, size_t cap) {
    if (out && cap) {
        size_t n = std::min(cap - 1, s.size());
        memcpy(out, s.data(), n);
        out[n] = 0;
    }
    return s.size();
}

extern "C" {

size_t whh_fmt_f64(double v, char* out, size_t cap) { return put(fmt_f64(v), out, cap); }
double whh_percentile(const double* xs, size_t n, double p) { return percentile(std::vector<double>(xs, xs + n), p); }
void whh_stat_block(const double* xs, size_t n, double* out6) {
    StatBlock s = stat_block(std::vector<double>(xs, xs + n));
    out6[0] = s.min; out6[1] = s.median; out6[2] = s.p90; out6[3] = s.p95; out6[4] = s.max; out6[5] = s.mean;
}
size_t whh_stat_json(const double* xs, size_t n, char* out, size_t cap) {
    return put(stat_json(stat_block(std::vector<double>(xs, xs + n))).pretty(), out, cap);
}
// rows: files/texts as NUL-separated lists
static std::vector<RowOut> rows_from(const char* files, const char* texts, const double* dur, const double* e2e, size_t n) {
    std::vector<RowOut> rows;
    for (size_t i = 0; i < n; i++) {
        std::string f(files), t(texts);
        files += f.size() + 1;
        texts += t.size() + 1;
        rows.push_back(make_row(f, dur[i], e2e[i], t));
    }
    return rows;
}
size_t whh_csv(const char* files, const char* texts, const double* dur, const double* e2e, size_t n, char* out, size_t cap) {
    return put(csv_text(rows_from(files, texts, dur, e2e, n)), out, cap);
}
size_t whh_per_file_json(const char* files, const char* texts, const double* dur, const double* e2e, size_t n, char* out, size_t cap) {
    return put(per_file_json(rows_from(files, texts, dur, e2e, n)), out, cap);
}
// the reference's summary object (src/main.rs:1235-1257) from per-file lists: lists = [end2end | load | preprocess | model_only | decode | rtf],
// n values each; strs = NUL-separated model_id, onnx_dir, language, task, tokenizer_json, execution_mode, graph_opt;
// ints = intra_op, inter_op, max_new_tokens; flags bit 0 timestamps, 1 cpu_mem_arena, 2 mem_pattern, 3 allow_spinning, bits 4-7 --beam-size (0: not given)
size_t whh_summary_json(const double* lists, size_t n, const char* strs, const long long* ints, unsigned flags, char* out, size_t cap) {
    SummaryIn in;
    auto take = [&](int k) { return std::vector<double>(lists + (size_t)k * n, lists + (size_t)(k + 1) * n); };
    in.end2end = take(0); in.load = take(1); in.preprocess = take(2); in.model_only = take(3); in.decode = take(4); in.rtf = take(5);
    in.n_files = n;
    std::string* dst[7] = {&in.model_id, &in.onnx_dir, &in.language, &in.task, &in.tokenizer_json, &in.cfg.execution_mode, &in.cfg.graph_opt};
    for (auto* d : dst) { *d = std::string(strs); strs += d->size() + 1; }
    in.cfg.intra_op = ints[0]; in.cfg.inter_op = ints[1]; in.max_new_tokens = ints[2];
    in.timestamps = flags & 1; in.cfg.cpu_mem_arena = flags & 2; in.cfg.mem_pattern = flags & 4; in.cfg.allow_spinning = flags & 8;
    if ((flags >> 4) & 15) in.cfg.beam_size = (flags >> 4) & 15;
    return put(reference_summary(in).pretty(), out, cap);
}
size_t whh_lower(const char* s, char* out, size_t cap) { return put(lower(s), out, cap); }
size_t whh_trim(const char* s, char* out, size_t cap) { return put(trim(s), out, cap); }
size_t whh_resample_linear(const float* x, size_t n, unsigned sr_in, unsigned sr_out, float* out, size_t cap) {
    std::vector<float> y = resample_linear(std::vector<float>(x, x + n), sr_in, sr_out);
    if (out) memcpy(out, y.data(), std::min(cap, y.size()) * sizeof(float));
    return y.size();
}
size_t whh_stitch(const char* chunks, size_t n, char* out, size_t cap) {
    std::vector<std::string> v;
    for (size_t i = 0; i < n; i++) { std::string c(chunks); chunks += c.size() + 1; v.push_back(c); }
    return put(stitch_texts(v), out, cap);
}
size_t whh_word_overlap(const char* a, const char* b, size_t max_words) { return word_overlap(a, b, max_words); }
size_t whh_decode_tokens(const long long* toks, size_t n, const char* tokenizer_json, char* out, size_t cap) {
    Tokenizer t;
    std::vector<int64_t> v(toks, toks + n);
    if (tokenizer_json && *tokenizer_json) load_tokenizer(tokenizer_json, t);
    return put(decode_tokens(v, t.loaded ? &t : nullptr), out, cap);
}
// timestamped segments as JSON [{"start": s, "end": s, "tokens": [ids]}] (wh_host.h split_segments / merge_window_segments)
static std::string segments_json(const std::vector<Segment>& segs) {
    std::string o = "[";
    char b[64];
    for (size_t i = 0; i < segs.size(); i++) {
        snprintf(b, sizeof b, "%s{\"start\": %.6f, \"end\": %.6f, \"tokens\": [", i ? ", " : "", segs[i].start, segs[i].end);
        o += b;
        for (size_t j = 0; j < segs[i].tokens.size(); j++) o += (j ? ", " : "") + std::to_string(segs[i].tokens[j]);
        o += "]";
        if (segs[i].has_conf) o += ", \"avg_logprob\": " + fmt_conf(segs[i].avg_logprob) + ", \"no_speech_prob\": " + fmt_conf(segs[i].no_speech_prob);   // only when supplied
        o += "}";
    }
    return o + "]";
}
size_t whh_segments_json(const long long* toks, size_t n, long long tb, long long eot, double duration, char* out, size_t cap) {
    return put(segments_json(split_segments(std::vector<int64_t>(toks, toks + n), tb, eot, duration)), out, cap);
}
// the same with the window's avg_logprob / no_speech_prob on each of its segments
size_t whh_segments_conf_json(const long long* toks, size_t n, long long tb, long long eot, double duration, double avg_lp, double no_speech_prob,
                              char* out, size_t cap) {
    std::vector<Segment> segs = split_segments(std::vector<int64_t>(toks, toks + n), tb, eot, duration);
    set_conf(segs, avg_lp, no_speech_prob);
    return put(segments_json(segs), out, cap);
}
double whh_avg_logprob(const float* logprobs, const long long* toks, size_t n, long long eot) {
    return avg_logprob(std::vector<float>(logprobs, logprobs + n), std::vector<int64_t>(toks, toks + n), eot);
}
// the silence rule the CLI applies (wh_host.h skip_window; a NaN threshold is off)
int whh_skip_window(double no_speech_prob, double avg_lp, double no_speech_threshold, double logprob_threshold) {
    return skip_window(no_speech_prob, avg_lp, no_speech_threshold, logprob_threshold) ? 1 : 0;
}
long long whh_no_speech_token(const char* language, const char* task, const char* tokenizer_json) {
    try {
        Tokenizer t;
        if (tokenizer_json && *tokenizer_json) load_tokenizer(tokenizer_json, t);
        return special_tokens(language, task, t.loaded ? &t : nullptr).no_speech;
    } catch (...) { return -1; }
}
// long-form: the windows' generated tokens back to back (lens[k] each), window starts and durations in seconds
size_t whh_longform_segments_json(const long long* toks, const size_t* lens, size_t n_windows, const double* starts, const double* durations,
                                  double overlap_s, long long tb, long long eot, char* out, size_t cap) {
    std::vector<std::vector<Segment>> w;
    for (size_t k = 0; k < n_windows; k++) {
        w.push_back(split_segments(std::vector<int64_t>(toks, toks + lens[k]), tb, eot, durations[k]));
        toks += lens[k];
    }
    return put(segments_json(merge_window_segments(w, std::vector<double>(starts, starts + n_windows), overlap_s)), out, cap);
}
// word-level timestamps: a window's generated tokens and their frames -> [{"word", "start", "end"}] (wh_host.h words_from_tokens)
size_t whh_words_json(const long long* toks, const int* frames, size_t n, long long tb, long long eot, double duration, double offset,
                      const char* tokenizer_json, char* out, size_t cap) {
    Tokenizer t;
    if (tokenizer_json && *tokenizer_json) load_tokenizer(tokenizer_json, t);
    return put(words_json(words_from_tokens(std::vector<int64_t>(toks, toks + n), std::vector<int32_t>(frames, frames + n), tb, eot, duration, offset,
                                            t.loaded ? &t : nullptr)), out, cap);
}
static std::vector<Cue> cues_from(const double* starts, const double* ends, const char* texts, size_t n) {
    std::vector<Cue> c;
    for (size_t i = 0; i < n; i++) {
        std::string t(texts);
        texts += t.size() + 1;
        c.push_back(Cue{starts[i], ends[i], t});
    }
    return c;
}
size_t whh_srt(const double* starts, const double* ends, const char* texts, size_t n, char* out, size_t cap) {
    return put(srt_text(cues_from(starts, ends, texts, n)), out, cap);
}
size_t whh_vtt(const double* starts, const double* ends, const char* texts, size_t n, char* out, size_t cap) {
    return put(vtt_text(cues_from(starts, ends, texts, n)), out, cap);
}
// --language auto: the language table (wh_host.h language_table) as comma-joined codes and their ids; returns the count, or -1 with the
// refusal's text in err
long long whh_language_table(const char* tokenizer_json, long long vocab, long long* ids, size_t cap_ids, char* codes, size_t cap_codes, char* err, size_t cap_err) {
    try {
        Tokenizer t;
        if (tokenizer_json && *tokenizer_json) load_tokenizer(tokenizer_json, t);
        LanguageTable lt = language_table(t.loaded ? &t : nullptr, vocab);
        std::string joined;
        for (size_t i = 0; i < lt.codes.size(); i++) {
            joined += (i ? "," : "") + lt.codes[i];
            if (ids && i < cap_ids) ids[i] = lt.ids[i];
        }
        put(joined, codes, cap_codes);
        return (long long)lt.ids.size();
    } catch (const std::exception& e) {
        put(e.what(), err, cap_err);
        return -1;
    }
}
// text context: build_prev_prefix's ids into out (cap entries at most); returns the prefix length
size_t whh_build_prefix(const long long* history, size_t n, long long sot_prev, int n_text_ctx, long long* out, size_t cap) {
    std::vector<int64_t> pre = build_prev_prefix(std::vector<int64_t>(history, history + n), sot_prev, n_text_ctx);
    for (size_t i = 0; i < pre.size() && out && i < cap; i++) out[i] = pre[i];
    return pre.size();
}
int whh_special_tokens(const char* language, const char* task, const char* tokenizer_json, long long* out5) {
    try {
        Tokenizer t;
        if (tokenizer_json && *tokenizer_json) load_tokenizer(tokenizer_json, t);
        WhisperSpecial s = special_tokens(language, task, t.loaded ? &t : nullptr);
        out5[0] = s.sot; out5[1] = s.eot; out5[2] = s.lang; out5[3] = s.task; out5[4] = s.no_timestamps;
        return 0;
    } catch (...) { return 1; }
}
// clip `seed` of the CLI's --synthetic-clips input (file i of a run is clip --seed + i): 480000 samples
size_t whh_synthetic_clip(unsigned long long seed, float* out, size_t cap) {
    std::vector<float> x = synthetic_clip(seed);
    if (out) memcpy(out, x.data(), std::min(cap, x.size()) * sizeof(float));
    return x.size();
}
int whh_load_wav(const char* path, float* out, size_t cap, size_t* n, double* dur) {
    try {
        std::vector<float> a;
        load_audio_16k_mono(path, a, dur);
        *n = a.size();
        if (out) memcpy(out, a.data(), std::min(cap, a.size()) * sizeof(float));
        return 0;
    } catch (...) { return 1; }
}
// read_wav_raw: the payload bytes (up to cap) and info = {format (WH_PCM_*), channels, sample_rate}; 0, or 1 with the refusal's text in err
int whh_read_wav_raw(const char* path, unsigned char* out, size_t cap, size_t* n_bytes, size_t* n_frames, unsigned* info3, char* err, size_t cap_err) {
    try {
        const RawWav r = read_wav_raw(path);
        *n_bytes = r.n_bytes;
        *n_frames = r.n_frames;
        info3[0] = (unsigned)r.format; info3[1] = r.channels; info3[2] = r.sample_rate;
        if (out) memcpy(out, r.payload(), std::min(cap, r.n_bytes));
        return 0;
    } catch (const std::exception& e) {
        put(e.what(), err, cap_err);
        return 1;
    }
}
// The CLI's loader / worker pipeline (run_file_pipeline) with stand-in load and process callbacks: file `bad_load` fails to
// load, the batch holding file `bad_process` fails in the worker (either may be >= nfiles: none), `pool_buffers` staging
// buffers can be allocated before the allocator runs dry (0 = no pool).  Returns 0 and the number of processed files, or 1
// and the error text; a deadlock would simply never return — the test runs it under a timeout.
int whh_pipeline_selftest(size_t nfiles, int n_loaders, size_t n_workers, size_t max_batch, size_t bad_load, size_t bad_process,
                          size_t pool_buffers, size_t long_every, size_t* n_processed, char* err, size_t cap) {
    const size_t window = 64;
    std::atomic<size_t> allocated{0}, done{0};
    std::vector<int> seen(nfiles, 0);
    std::mutex sm;
    BufferPool pool([&]() -> float* { return allocated.fetch_add(1) < pool_buffers ? (float*)malloc(window * sizeof(float)) : nullptr; },
                    [](float* p) { free(p); });
    auto load = [&](size_t i, std::vector<float>& audio, double& dur) {
        if (i == bad_load) throw std::runtime_error("cannot decode file " + std::to_string(i));
        const bool is_long = long_every && (i % long_every) == long_every - 1;
        audio.assign(is_long ? 3 * window : window - (i % 5), (float)i);
        dur = (double)audio.size();
        std::this_thread::sleep_for(std::chrono::microseconds(200 + 37 * (i % 7)));
    };
    std::atomic<size_t> with_next{0};
    std::vector<size_t> expect_first(n_workers, (size_t)-1);   // per worker: first index of the batch announced as `next`
    auto process = [&](size_t wi, std::vector<PipeItem>& batch, std::vector<PipeItem>* next) {
        if (batch.empty() || batch.size() > max_batch) throw std::runtime_error("bad batch size");
        if (expect_first[wi] != (size_t)-1 && batch[0].idx != expect_first[wi]) throw std::runtime_error("the announced next batch was not the next batch");
        expect_first[wi] = (size_t)-1;
        if (next) {
            if (next->empty() || next->size() > max_batch) throw std::runtime_error("bad next batch size");
            for (auto& it : *next)
                if (it.n() > window) throw std::runtime_error("a multi-window file was announced as a next batch");
            if ((*next)[0].data()[0] != (float)(*next)[0].idx) throw std::runtime_error("next payload mismatch");
            expect_first[wi] = (*next)[0].idx;
            with_next++;
        }
        if (batch.size() > 1)
            for (auto& it : batch)
                if (it.n() > window) throw std::runtime_error("a multi-window file must go alone");
        for (size_t k = 0; k < batch.size(); k++) {
            if (k && batch[k].idx != batch[k - 1].idx + 1) throw std::runtime_error("batch not in file order");
            if (batch[k].idx == bad_process) throw std::runtime_error("transcribe failed for file " + std::to_string(batch[k].idx));
            if (batch[k].data()[0] != (float)batch[k].idx) throw std::runtime_error("payload mismatch");
            std::lock_guard<std::mutex> lk(sm);
            seen[batch[k].idx]++;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(500));
        done += batch.size();
    };
    const std::string e = run_file_pipeline(nfiles, n_loaders, n_workers, max_batch, window, pool_buffers ? &pool : nullptr, load, process);
    if (n_processed) *n_processed = done.load();
    put(e, err, cap);
    if (!e.empty()) return 1;
    for (size_t i = 0; i < nfiles; i++)
        if (seen[i] != 1) { put("file " + std::to_string(i) + " processed " + std::to_string(seen[i]) + " times", err, cap); return 2; }
    return 0;
}

// ---- the temperature ladder (tests/test_sample_cpu.py) ----
// compression_ratio of n bytes; *compressed (optional) = the compressed length.  Returns NaN with the message in err when zlib is missing.
double whh_compression_ratio(const char* text, size_t n, size_t* compressed, char* err, size_t cap) {
    try {
        const std::string s(text, n);
        if (compressed) *compressed = zlib_compressed_size(s);
        return compression_ratio(s);
    } catch (const std::exception& e) {
        put(e.what(), err, cap);
        return std::nan("");
    }
}
size_t whh_zlib_version(char* out, size_t cap) {
    try { return put(Zlib::get().version(), out, cap); } catch (const std::exception&) { return 0; }
}
int whh_needs_fallback(double cr, double avg_lp, double no_speech_prob, double cr_thr, double lp_thr, double ns_thr) {
    return needs_fallback(cr, avg_lp, no_speech_prob, cr_thr, lp_thr, ns_thr) ? 1 : 0;
}
// run_ladder over a scripted decoder: script [n_rungs][n][3] = {compression_ratio, avg_logprob, no_speech_prob} a window would score at a rung.
// rung_of [n]; decoded [n_rungs][n]: 1 where the window was decoded at that rung.
void whh_run_ladder(size_t n, size_t n_rungs, const double* script, double cr_thr, double lp_thr, double ns_thr, int* rung_of, unsigned char* decoded) {
    std::vector<int> ro;
    std::vector<WindowScore> sc;
    memset(decoded, 0, n * n_rungs);
    run_ladder(n, n_rungs, cr_thr, lp_thr, ns_thr,
               [&](size_t r, const std::vector<unsigned char>& active, std::vector<WindowScore>& scores) {
                   for (size_t w = 0; w < n; w++) {
                       if (!active[w]) continue;
                       decoded[r * n + w] = 1;
                       const double* s = script + (r * n + w) * 3;
                       scores[w] = WindowScore{s[0], s[1], s[2]};
                   }
               },
               ro, sc);
    for (size_t w = 0; w < n; w++) rung_of[w] = ro[w];
}
// ---- sequential long-form (tests/test_sequential_cpu.py) ----
static std::string ids_json(const std::vector<int64_t>& v) {
    std::string o = "[";
    for (size_t j = 0; j < v.size(); j++) o += (j ? ", " : "") + std::to_string(v[j]);
    return o + "]";
}
static std::string f64_json(double v) {   // round-trips exactly
    char b[40];
    snprintf(b, sizeof b, "%.17g", v);
    return b;
}
static std::string seq_segments_json(const std::vector<SeqSegment>& segs) {
    std::string o = "[";
    for (size_t i = 0; i < segs.size(); i++)
        o += std::string(i ? ", " : "") + "{\"start\": " + f64_json(segs[i].start) + ", \"end\": " + f64_json(segs[i].end) + ", \"ids\": " + ids_json(segs[i].ids) + "}";
    return o + "]";
}
// seek_advance: {"advance": frames, "segments": [{"start", "end", "ids"}]}
size_t whh_seek_advance(const long long* toks, size_t n, long long tb, long long eot, long long seg_frames, char* out, size_t cap) {
    std::vector<SeqSegment> segs;
    const int64_t adv = seek_advance(std::vector<int64_t>(toks, toks + n), tb, eot, seg_frames, segs);
    return put("{\"advance\": " + std::to_string(adv) + ", \"segments\": " + seq_segments_json(segs) + "}", out, cap);
}
// run_sequential over a scripted step.  cfg_i = {tb, eot, sot_prev, n_text_ctx, n_prompt, max_new_tokens, condition_on_previous_text}; cfg_d =
// {no_speech_threshold, logprob_threshold} (NaN: off).  The script is a table of windows: file f's window k is entry first[f] + min(k, count[f] - 1)
// (the last entry repeats), entry e = lens[e] generated ids of `toks` (back to back) and scores[e] = {avg_logprob, no_speech_prob, temperature}.
// JSON out: {"steps": [[files of step 0], ...], "files": [{"windows": [...], "segments": [...]}]}.
size_t whh_run_sequential(const long long* frames, size_t n_files, const long long* cfg_i, const double* cfg_d, const long long* initial_prompt, size_t n_initial,
                          const size_t* first, const size_t* count, const long long* toks, const size_t* lens, const double* scores, size_t n_entries, char* out,
                          size_t cap) {
    SeqConfig cfg;
    cfg.tb = cfg_i[0]; cfg.eot = cfg_i[1]; cfg.sot_prev = cfg_i[2]; cfg.n_text_ctx = (int)cfg_i[3]; cfg.n_prompt = (size_t)cfg_i[4]; cfg.max_new_tokens = (size_t)cfg_i[5];
    cfg.condition_on_previous_text = cfg_i[6] != 0;
    cfg.no_speech_threshold = cfg_d[0]; cfg.logprob_threshold = cfg_d[1];
    cfg.initial_prompt.assign(initial_prompt, initial_prompt + n_initial);
    std::vector<size_t> tok_off(n_entries + 1, 0);
    for (size_t e = 0; e < n_entries; e++) tok_off[e + 1] = tok_off[e] + lens[e];
    std::string steps = "[";
    std::vector<SeqFile> files;
    run_sequential(std::vector<int64_t>(frames, frames + n_files), cfg,
                   [&](const std::vector<SeqRow>& rows, std::vector<SeqStepResult>& res) {
                       std::vector<int64_t> fs;
                       for (size_t i = 0; i < rows.size(); i++) {
                           const size_t f = rows[i].file, e = first[f] + std::min(rows[i].window, count[f] - 1);
                           fs.push_back((int64_t)f);
                           res[i].tokens.assign(toks + tok_off[e], toks + tok_off[e + 1]);
                           res[i].avg_logprob = scores[e * 3]; res[i].no_speech_prob = scores[e * 3 + 1]; res[i].temperature = scores[e * 3 + 2];
                       }
                       steps += (steps.size() > 1 ? ", " : "") + ids_json(fs);
                   },
                   files);
    std::string o = "{\"steps\": " + steps + "], \"files\": [";
    for (size_t f = 0; f < files.size(); f++) {
        o += std::string(f ? ", " : "") + "{\"windows\": [";
        for (size_t k = 0; k < files[f].windows.size(); k++) {
            const SeqWindow& w = files[f].windows[k];
            o += std::string(k ? ", " : "") + "{\"seek\": " + std::to_string(w.seek) + ", \"seg_frames\": " + std::to_string(w.seg_frames) + ", \"advance\": " + std::to_string(w.advance) +
                 ", \"skipped\": " + (w.skipped ? "true" : "false") + ", \"temperature\": " + f64_json(w.temperature) + ", \"tokens\": " + ids_json(w.tokens) +
                 ", \"prefix\": " + ids_json(w.prefix) + "}";
        }
        o += "], \"segments\": " + seq_segments_json(files[f].segments) + "}";
    }
    return put(o + "]}", out, cap);
}
// parse_temperatures: the count (out: up to cap values), or -1 with the message in err
long whh_parse_temperatures(const char* txt, float* out, size_t cap, char* err, size_t ecap) {
    try {
        const std::vector<float> t = parse_temperatures(txt);
        for (size_t i = 0; i < t.size() && i < cap; i++) out[i] = t[i];
        return (long)t.size();
    } catch (const std::exception& e) {
        put(e.what(), err, ecap);
        return -1;
    }
}
// per_file_json of one row, with (ladder != 0) or without the ladder's keys
size_t whh_ladder_row_json(const char* file, const char* text, double temperature, double cr, int ladder, char* out, size_t cap) {
    RowOut r = make_row(file, 1.0, 1.0, text);
    r.has_ladder = ladder != 0; r.temperature = temperature; r.compression_ratio = cr;
    return put(per_file_json({r}), out, cap);
}
// config_used of a ladder (n == 0: none)
size_t whh_ladder_config_json(const float* temps, size_t n, char* out, size_t cap) {
    OrtCfg c;
    c.temperature.assign(temps, temps + n);
    return put(c.json(true).pretty(), out, cap);
}
}
