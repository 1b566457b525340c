// whisper_bench.cpp — the reference CLI's surface (src/main.rs:23-86, 1065-1271) over
// libwhisper_hip.so.  Same flags and defaults, same CSV / per-file JSON / summary JSON / stdout;
// the ort::Session calls and the Rust log-mel are replaced by the C ABI.  CPU-EP tuning flags are
// accepted and echoed in `config_used`; GPU-side extras live under new keys / new flags.
#include <dirent.h>
#include <sys/stat.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <thread>

#include <hip/hip_runtime_api.h>

#include "../../include/whisper_hip.h"
#include "wh_host.h"

using namespace whhost;

struct Args {
    std::string audio_dir = "audio", model_id = "openai/whisper-base", onnx_dir = "whisper-base-with-past";
    std::string language = "en", task = "transcribe";
    size_t max_new_tokens = 128, warmup = 0, limit_files = 0;
    std::string discovery_best_json, out_csv = "results/benchmarks/inference_per_file.csv",
                                     out_json = "results/benchmarks/inference_per_file.json",
                                     out_summary_json = "results/benchmarks/inference_summary.json";
    long long intra_op = 0, inter_op = 0;
    bool write_txt = false, timestamps = false;
    // additive: Whisper's timestamp rules in the token loop, segments in the per-file JSON; SRT / VTT files (imply the rules)
    bool timestamp_rules = false, write_srt = false, write_vtt = false;
    // additive: avg_logprob / no_speech_prob in the per-file JSON (wh_ctx_set_logprobs); the thresholds of openai-whisper's silence rule (NaN: off)
    bool logprobs = false;
    double no_speech_threshold = std::nan(""), logprob_threshold = std::nan("");
    std::string tokenizer_json;
    size_t chunk_parallelism = 0;
    float chunk_length_s = 30.0f, overlap_s = 5.0f;
    // additive (GPU) flags
    int device = 0, max_batch = 16;
    std::string devices;            // "0-7", "0,2,5": one model per listed device (default: --device)
    int streams_per_gpu = 1;        // contexts (HIP streams) per device, one host thread each
    int load_threads = 0;           // host threads that decode / synthesise audio ahead of the GPU (0 = min(16, cores))
    std::string precision = "bf16";
    bool print_plan = false;   // --print-plan: print the device -> context plan of this command line and exit before any device is touched
    size_t synthetic_clips = 0;
    uint64_t seed = 1000;
    // additive: the loaders only read and parse; sample conversion, downmix and resampling run on the GPU (wh_transcribe_batch_raw_next /
    // wh_transcribe_longform_raw).  --synthetic-clips ignores it
    bool gpu_ingest = false;
    // additive: text context (wh_ctx_set_prefixes): ids for every file, or DIR/<audio stem>.txt per file; the prefix on every window of a long file
    std::string prompt_ids, prompt_ids_dir;
    bool prompt_all_windows = false;
    // additive: HF's repetition penalty and no-repeat n-grams in the token loop (wh_ctx_set_repetition); each is echoed in the summary when given
    bool have_rep_penalty = false, have_rep_ngram = false;
    float rep_penalty = 1.0f;
    int rep_ngram = 0;
    // additive: word-level timestamps (wh_ctx_set_alignment): words and token times in the per-file JSON; the alignment heads as "l:h,l:h,..."
    bool word_timestamps = false;
    std::string alignment_heads;
    std::string align_ids_dir;   // --align-ids-dir: forced alignment of given transcripts (wh_align_tokens) instead of a decode
    bool align() const { return !align_ids_dir.empty(); }
    // additive: beam search (wh_ctx_set_beam_search).  --beam-size 1 is the greedy path with the option not set
    int beam_size = 1, n_best = 1;
    float patience = 1.0f, length_penalty = -1.0f;
    // additive: the temperature ladder (wh_ctx_set_sampling; openai-whisper's decode_with_fallback).  The single rung 0 is the greedy path with the
    // option not set; --seed also seeds the sampler
    std::vector<float> temperature = {0.0f};
    double compression_ratio_threshold = std::nan("");
    // additive: sequential long-form (wh_files_load / wh_transcribe_windows; wh_host.h run_sequential): a worker's files advance in lockstep, each
    // window starting where the timestamps of the one before say; implies --timestamp-rules.  A worker loads at most this much audio into one
    // file set: n_mels * 400 bytes per second of audio = 115 MB per hour at 80 mel bins, 184 MB at 128 (4 h: 461 / 737 MB)
    bool sequential = false, condition_on_previous_text = true, overlap_given = false;
    double sequential_max_audio_s = 14400.0;
    bool ladder() const { return temperature.size() > 1 || temperature[0] != 0.0f; }
    bool beam() const { return beam_size >= 2; }
    bool prompts() const { return !prompt_ids.empty() || !prompt_ids_dir.empty(); }
};

// ids separated by commas or whitespace
static std::vector<int64_t> parse_ids(const std::string& txt, const std::string& what) {
    std::vector<int64_t> out;
    size_t i = 0;
    while (i < txt.size()) {
        if (txt[i] == ',' || isspace((unsigned char)txt[i])) { i++; continue; }
        size_t j = i;
        while (j < txt.size() && txt[j] != ',' && !isspace((unsigned char)txt[j])) j++;
        const std::string w = txt.substr(i, j - i);
        char* e = nullptr;
        const long long v = strtoll(w.c_str(), &e, 10);
        if (*e || v < 0) throw std::runtime_error(what + ": '" + w + "' is not a token id");
        out.push_back(v);
        i = j;
    }
    return out;
}

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

static void mkdir_p(const std::string& path) {
    size_t pos = 0;
    while ((pos = path.find('/', pos + 1)) != std::string::npos) mkdir(path.substr(0, pos).c_str(), 0755);
    mkdir(path.c_str(), 0755);
}
static std::string parent_dir(const std::string& p) {
    size_t s = p.rfind('/');
    return s == std::string::npos ? "" : p.substr(0, s);
}
static bool is_file(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
static bool is_dir(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode); }
static void write_file(const std::string& p, const std::string& s) {
    FILE* f = fopen(p.c_str(), "wb");
    if (!f) throw std::runtime_error("cannot write " + p);
    fwrite(s.data(), 1, s.size(), f);
    fclose(f);
}

static bool parse_args(int argc, char** argv, Args& a) {
    auto need = [&](int& i, const std::string& key, std::string& val, const std::string& inl) {
        if (!inl.empty() || key.find('=') != std::string::npos) { val = inl; return true; }
        if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", key.c_str()); return false; }
        val = argv[++i];
        return true;
    };
    for (int i = 1; i < argc; i++) {
        std::string k = argv[i], inl;
        size_t eq = k.find('=');
        if (eq != std::string::npos) { inl = k.substr(eq + 1); k = k.substr(0, eq); }
        std::string v;
        if (k == "--write-txt") a.write_txt = true;
        else if (k == "--timestamps") a.timestamps = true;
        else if (k == "--timestamp-rules") a.timestamp_rules = true;
        else if (k == "--write-srt") a.write_srt = a.timestamp_rules = true;
        else if (k == "--write-vtt") a.write_vtt = a.timestamp_rules = true;
        else if (k == "--logprobs") a.logprobs = true;
        else if (k == "--gpu-ingest") a.gpu_ingest = true;
        else if (k == "--word-timestamps") a.word_timestamps = true;
        else if (k == "--print-plan") a.print_plan = true;
        else if (k == "--prompt-all-windows") a.prompt_all_windows = true;
        else if (k == "--sequential") a.sequential = a.timestamp_rules = true;
        else if (k == "--help" || k == "-h") {
            printf("Usage: whisper_bench [--audio-dir DIR] [--model-id ID] [--onnx-dir DIR|synthetic:<preset>:<seed>] [--language en|auto] "
                   "[--task transcribe] [--max-new-tokens 128] [--warmup 0] [--limit-files 0] [--discovery-best-json F] "
                   "[--out-csv F] [--out-json F] [--out-summary-json F] [--intra-op N] [--inter-op N] [--write-txt] "
                   "[--tokenizer-json F] [--timestamps] [--chunk-parallelism N] [--chunk-length-s 30] [--overlap-s 5] "
                   "[--device 0] [--devices 0-7] [--streams-per-gpu 1] [--load-threads N] [--precision bf16|f32|fp8|f16x3] [--max-batch 16] "
                   "[--synthetic-clips N] [--seed 1000] [--print-plan] [--gpu-ingest] [--timestamp-rules] [--write-srt] [--write-vtt] "
                   "[--logprobs] [--no-speech-threshold X] [--logprob-threshold Y] [--prompt-ids a,b,c] [--prompt-ids-dir DIR] [--prompt-all-windows] "
                   "[--repetition-penalty F] [--no-repeat-ngram-size N] [--beam-size N] [--patience F] [--length-penalty F] [--n-best M] "
                   "[--temperature 0,0.2,...] [--compression-ratio-threshold X] [--sequential] [--condition-on-previous-text 0|1] [--sequential-max-audio-s S]\n"
                   "  --sequential             openai-whisper's sequential long-form instead of fixed overlapping windows: a worker takes up to --max-batch files of any\n"
                   "                           length, keeps their log-mels on the device and decodes one window of every unfinished file per step as one batch; a file's\n"
                   "                           next window starts where the last complete timestamp pair of this one ends (else a whole window on), the previous text is\n"
                   "                           its prompt, silent windows (--no-speech-threshold / --logprob-threshold) are skipped, and with a --temperature ladder a\n"
                   "                           failing window is decoded again at the next rung.  Implies --timestamp-rules; the text is the segments' text one after the\n"
                   "                           other (no stitcher); the per-file JSON gains windows.  Not with --language auto, --overlap-s or --beam-size\n"
                   "  --condition-on-previous-text 0|1   1 (the default): a window's prompt is the file's text so far (reset after a window decoded above temperature 0.5);\n"
                   "                           0: only the first window sees --prompt-ids\n"
                   "  --sequential-max-audio-s S   audio a worker loads into one file set (default 14400: n_mels x 400 bytes per second, 115 MB per hour at 80 mel bins,\n"
                   "                           184 MB at 128); a batch holding more is run as several sets, a single longer file alone\n"
                   "  --temperature a,b,c      the temperature ladder (openai-whisper's decode_with_fallback; default 0 = greedy, today's outputs byte for byte): every\n"
                   "                           window is decoded at the first rung; a window whose compression ratio exceeds --compression-ratio-threshold or whose\n"
                   "                           avg_logprob lies below --logprob-threshold — and whose no_speech_prob does not exceed --no-speech-threshold — is decoded\n"
                   "                           again at the next rung (sampled at that temperature, seeded by --seed and the file's index), the others keep their result;\n"
                   "                           after the last rung the last result stands.  The per-file JSON gains temperature and compression_ratio, config_used the\n"
                   "                           ladder.  With a ladder the batches go through the unpipelined transcribe entry (the re-decode reads the batch's resident\n"
                   "                           encoder states, which a prefetched next batch would replace), and every file must fit one 30 s window unless --sequential is given\n"
                   "  --compression-ratio-threshold X   openai-whisper's default is 2.4 (off unless given)\n"
                   "  --beam-size N            beam search with N beams per window (1 .. 8; 1 = greedy, the default); a device batch then holds max-batch / N files\n"
                   "  --patience F             round(N * F) finished hypotheses end a window's search (openai-whisper's patience; default 1)\n"
                   "  --length-penalty F       rank by score / ((5 + len) / 6)^F; below 0 (the default): by score / len\n"
                   "  --n-best M               hypotheses [{text, sum_logprob, rank_score, finished}] of the M best per file in the per-file JSON (a file of several windows:\n"
                   "                           every window's M best one after the other, each with its window index)\n"
                   "  --repetition-penalty F   HF generate's repetition_penalty on each row's generated history (F > 0; 1 = off)\n"
                   "  --no-repeat-ngram-size N no n-gram of N ids is generated twice (0 = off, at most 32); timestamps are exempt from both\n"
                   "  --language auto          the language of every file is detected from its audio (its first window's, for a file of several) among\n"
                   "                           the tokenizer's <|xx|> tokens, else the multilingual ids from 50259 on; the per-file JSON and CSV gain\n"
                   "                           language and language_probability\n"
                   "  --prompt-ids a,b,c       text context for every file: token ids of the previous text / vocabulary hints; <|startofprev|> is put in\n"
                   "                           front and only the last n_text_ctx/2 - 1 ids are kept (openai-whisper's initial_prompt rule)\n"
                   "  --prompt-ids-dir DIR     the same per file: DIR/<audio stem>.txt holds the ids, separated by commas or whitespace (no file: the\n"
                   "                           --prompt-ids list, else no context); the per-file JSON gains prompt_tokens\n"
                   "  --prompt-all-windows     a file of several windows: the context conditions every window (default: the first one only)\n"
                   "  --logprobs               avg_logprob and no_speech_prob in every row of the per-file JSON (and in its segments)\n"
                   "  --no-speech-threshold X  with --logprob-threshold Y: a window with no_speech_prob > X and avg_logprob < Y becomes empty text and\n"
                   "  --logprob-threshold Y    no segments (both off unless given, each implies --logprobs; openai-whisper's defaults are 0.6 and -1.0)\n"
                   "  --word-timestamps        words [{word, start, end}] and token_times in every row of the per-file JSON (cross-attention alignment + DTW);\n"
                   "                           a one-window file's words concatenate to its text, a longer file's are its windows' words one after the other\n"
                   "                           (the overlap of two windows is not removed from them as it is from the stitched text)\n"
                   "  --align-ids-dir DIR      forced alignment: DIR/<audio stem>.txt holds the token ids of the file's transcript (as --prompt-ids-dir's files);\n"
                   "                           every batch is encoded and then aligned instead of decoded (wh_align_tokens): text = the given ids decoded, words,\n"
                   "                           token_times, avg_logprob of the given ids and aligned: true in every row; one-window files only; heads as --word-timestamps\n"
                   "  --alignment-heads L      its heads as \"layer:head,layer:head,...\" (default: alignment_heads of the model directory's generation_config.json,\n"
                   "                           else every head of the upper half of the decoder layers, the topmost layers first, 32 heads at most)\n");
            exit(0);
        } else {
            if (!need(i, argv[i], v, inl)) return false;
            if (k == "--audio-dir") a.audio_dir = v;
            else if (k == "--model-id") a.model_id = v;
            else if (k == "--onnx-dir") a.onnx_dir = v;
            else if (k == "--language") a.language = v;
            else if (k == "--task") a.task = v;
            else if (k == "--max-new-tokens") a.max_new_tokens = strtoull(v.c_str(), nullptr, 10);
            else if (k == "--warmup") a.warmup = strtoull(v.c_str(), nullptr, 10);
            else if (k == "--limit-files") a.limit_files = strtoull(v.c_str(), nullptr, 10);
            else if (k == "--discovery-best-json") a.discovery_best_json = v;
            else if (k == "--out-csv") a.out_csv = v;
            else if (k == "--out-json") a.out_json = v;
            else if (k == "--out-summary-json") a.out_summary_json = v;
            else if (k == "--intra-op") a.intra_op = atoll(v.c_str());
            else if (k == "--inter-op") a.inter_op = atoll(v.c_str());
            else if (k == "--tokenizer-json") a.tokenizer_json = v;
            else if (k == "--chunk-parallelism") a.chunk_parallelism = strtoull(v.c_str(), nullptr, 10);
            else if (k == "--chunk-length-s") a.chunk_length_s = strtof(v.c_str(), nullptr);
            else if (k == "--overlap-s") { a.overlap_s = strtof(v.c_str(), nullptr); a.overlap_given = true; }
            else if (k == "--condition-on-previous-text") {
                if (v != "0" && v != "1") { fprintf(stderr, "error: --condition-on-previous-text '%s' is not 0 or 1\n", v.c_str()); return false; }
                a.condition_on_previous_text = v == "1";
            } else if (k == "--sequential-max-audio-s") {
                char* end = nullptr;
                a.sequential_max_audio_s = strtod(v.c_str(), &end);
                if (v.empty() || *end || !(a.sequential_max_audio_s > 0.0)) { fprintf(stderr, "error: --sequential-max-audio-s '%s' is not a value above 0\n", v.c_str()); return false; }
            }
            else if (k == "--device") a.device = atoi(v.c_str());
            else if (k == "--devices") a.devices = v;
            else if (k == "--streams-per-gpu") a.streams_per_gpu = std::max(1, atoi(v.c_str()));
            else if (k == "--load-threads") a.load_threads = atoi(v.c_str());
            else if (k == "--precision") a.precision = v;
            else if (k == "--max-batch") a.max_batch = atoi(v.c_str());
            else if (k == "--synthetic-clips") a.synthetic_clips = strtoull(v.c_str(), nullptr, 10);
            else if (k == "--no-speech-threshold") { a.no_speech_threshold = strtod(v.c_str(), nullptr); a.logprobs = true; }
            else if (k == "--logprob-threshold") { a.logprob_threshold = strtod(v.c_str(), nullptr); a.logprobs = true; }
            else if (k == "--seed") a.seed = strtoull(v.c_str(), nullptr, 10);
            else if (k == "--temperature") {   // what wh_ctx_set_sampling refuses is refused here, before any device is touched
                try { a.temperature = parse_temperatures(v); } catch (const std::exception& e) { fprintf(stderr, "error: %s\n", e.what()); return false; }
            } else if (k == "--compression-ratio-threshold") {
                char* end = nullptr;
                a.compression_ratio_threshold = strtod(v.c_str(), &end);
                if (v.empty() || *end || std::isnan(a.compression_ratio_threshold)) { fprintf(stderr, "error: --compression-ratio-threshold '%s' is not a number\n", v.c_str()); return false; }
            }
            else if (k == "--prompt-ids") a.prompt_ids = v;
            else if (k == "--alignment-heads") a.alignment_heads = v;
            else if (k == "--prompt-ids-dir") a.prompt_ids_dir = v;
            else if (k == "--align-ids-dir") a.align_ids_dir = v;
            else if (k == "--repetition-penalty") {   // what wh_ctx_set_repetition refuses is refused here, before any device is touched
                char* end = nullptr;
                a.rep_penalty = strtof(v.c_str(), &end);
                if (v.empty() || *end || !std::isfinite(a.rep_penalty) || !(a.rep_penalty > 0.0f)) {
                    fprintf(stderr, "error: --repetition-penalty '%s' is not a finite value above 0\n", v.c_str());
                    return false;
                }
                a.have_rep_penalty = true;
            } else if (k == "--no-repeat-ngram-size") {
                char* end = nullptr;
                const long n = strtol(v.c_str(), &end, 10);
                if (v.empty() || *end || n < 0 || n > WH_MAX_NGRAM) {
                    fprintf(stderr, "error: --no-repeat-ngram-size '%s' is outside 0 .. %d\n", v.c_str(), WH_MAX_NGRAM);
                    return false;
                }
                a.rep_ngram = (int)n;
                a.have_rep_ngram = true;
            }
            else if (k == "--beam-size" || k == "--n-best") {   // what wh_ctx_set_beam_search refuses is refused here, before any device is touched
                char* end = nullptr;
                const long n = strtol(v.c_str(), &end, 10);
                const long hi = k == "--beam-size" ? WH_MAX_BEAMS : WH_MAX_BEAMS + WH_MAX_BEAM_CANDIDATES;
                if (v.empty() || *end || n < 1 || n > hi) {
                    fprintf(stderr, "error: %s '%s' is outside 1 .. %ld\n", k.c_str(), v.c_str(), hi);
                    return false;
                }
                (k == "--beam-size" ? a.beam_size : a.n_best) = (int)n;
            } else if (k == "--patience" || k == "--length-penalty") {
                char* end = nullptr;
                const float f = strtof(v.c_str(), &end);
                const bool pat = k == "--patience";
                if (v.empty() || *end || std::isnan(f) || (pat && (!std::isfinite(f) || !(f > 0.0f)))) {
                    fprintf(stderr, "error: %s '%s' is not %s\n", k.c_str(), v.c_str(), pat ? "a finite value above 0" : "a number");
                    return false;
                }
                (pat ? a.patience : a.length_penalty) = f;
            }
            else { fprintf(stderr, "error: unexpected argument '%s'\n", k.c_str()); return false; }
        }
    }
    if (a.beam()) {   // the combinations every decode call would refuse, and a candidate count outside the library's range
        const long cand = lroundf((float)a.beam_size * a.patience);
        if (cand < 1 || cand > WH_MAX_BEAM_CANDIDATES) {
            fprintf(stderr, "error: round(--beam-size * --patience) = %ld is outside 1 .. %d\n", cand, WH_MAX_BEAM_CANDIDATES);
            return false;
        }
        if (a.max_batch < a.beam_size) { fprintf(stderr, "error: --max-batch %d holds no file of --beam-size %d\n", a.max_batch, a.beam_size); return false; }
        const char* clash = a.have_rep_penalty || a.have_rep_ngram ? "--repetition-penalty / --no-repeat-ngram-size" : a.word_timestamps ? "--word-timestamps"
                            : a.prompts() ? "--prompt-ids / --prompt-ids-dir" : a.precision == "fp8" || a.precision == "f16x3" ? "--precision fp8 / f16x3" : nullptr;
        if (clash) { fprintf(stderr, "error: --beam-size %d cannot be combined with %s\n", a.beam_size, clash); return false; }
    } else if (a.n_best > 1) {
        fprintf(stderr, "error: --n-best %d needs --beam-size 2 or more\n", a.n_best);
        return false;
    }
    if (a.align()) {   // forced alignment takes the transcript as given: nothing that chooses tokens, no per-row text context, no long-form walk
        const char* clash = a.sequential ? "--sequential" : a.beam() ? "--beam-size" : a.ladder() ? "--temperature" : a.prompts() ? "--prompt-ids / --prompt-ids-dir"
                            : a.language == "auto" ? "--language auto" : a.precision == "fp8" || a.precision == "f16x3" ? "--precision fp8 / f16x3"
                            : a.timestamp_rules ? "--timestamp-rules" : a.have_rep_penalty || a.have_rep_ngram ? "--repetition-penalty / --no-repeat-ngram-size" : nullptr;
        if (clash) { fprintf(stderr, "error: --align-ids-dir cannot be combined with %s\n", clash); return false; }
    }
    if (a.sequential) {
        if (a.language == "auto") {
            fprintf(stderr, "error: --sequential cannot be combined with --language auto: one prompt serves all rows of a device batch and its files may differ in "
                            "language; detect the languages with a run without --sequential first\n");
            return false;
        }
        if (a.overlap_given) { fprintf(stderr, "error: --sequential cannot be combined with --overlap-s: its windows start where the timestamps say, they do not overlap\n"); return false; }
        if (a.beam()) { fprintf(stderr, "error: --sequential cannot be combined with --beam-size: beam search refuses the per-row text context\n"); return false; }
    }
    if (a.ladder()) {   // the combinations every sampling call would refuse; the fallback decision reads avg_logprob and no_speech_prob
        const char* clash = a.beam() ? "--beam-size" : a.have_rep_penalty || a.have_rep_ngram ? "--repetition-penalty / --no-repeat-ngram-size"
                            : a.word_timestamps ? "--word-timestamps" : nullptr;
        if (clash) { fprintf(stderr, "error: --temperature %s cannot be combined with %s\n", "above 0 or with several rungs", clash); return false; }
        a.logprobs = true;
    } else if (!std::isnan(a.compression_ratio_threshold)) {
        fprintf(stderr, "error: --compression-ratio-threshold needs a --temperature ladder\n");
        return false;
    }
    return true;
}

static OrtCfg suggested_optimum_cfg() {  // src/main.rs:108-122
    unsigned cpu = std::thread::hardware_concurrency();
    if (!cpu) cpu = 8;
    OrtCfg c;
    c.intra_op = std::min<unsigned>(cpu, 16);
    return c;
}

static OrtCfg load_best_cfg_from_discovery(const std::string& path) {  // src/main.rs:124-167
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("cannot read " + path);
    std::string txt; char b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) txt.append(b, n);
    fclose(f);
    std::string err;
    auto j = whjson::parse(txt, &err);
    if (!j) throw std::runtime_error(path + ": " + err);
    const whjson::Value* best = j->get("best");
    OrtCfg c = suggested_optimum_cfg();
    c.inter_op = 1;
    auto get = [&](const char* k) -> const whjson::Value* { return best && best->is(whjson::Value::Obj) ? best->get(k) : nullptr; };
    auto as_bool = [&](const char* k, bool d) {
        auto v = get(k);
        if (!v) return d;
        if (v->is(whjson::Value::Bool)) return v->b;
        if (v->is(whjson::Value::Num)) return v->as_i64() != 0;
        if (v->is(whjson::Value::Str)) { std::string s = lower(trim(v->str)); return s == "1" || s == "true" || s == "yes" || s == "y" || s == "on"; }
        return d;
    };
    auto as_usize = [&](const char* k, long long d) {
        auto v = get(k);
        if (!v) return d;
        if (v->is(whjson::Value::Num)) return (long long)v->as_i64();
        if (v->is(whjson::Value::Str)) { char* e; long long r = strtoll(v->str.c_str(), &e, 10); return (*e || v->str.empty()) ? d : r; }
        return d;
    };
    auto as_str = [&](const char* k, const std::string& d) { auto v = get(k); return (v && v->is(whjson::Value::Str)) ? v->str : d; };
    c.intra_op = as_usize("intra_op", c.intra_op);
    c.inter_op = as_usize("inter_op", 1);
    c.execution_mode = as_str("execution_mode", "SEQUENTIAL");
    c.graph_opt = as_str("graph_opt", "ENABLE_ALL");
    c.cpu_mem_arena = as_bool("cpu_mem_arena", true);
    c.mem_pattern = as_bool("mem_pattern", true);
    c.allow_spinning = as_bool("allow_spinning", true);
    return c;
}

struct GenCfg { std::vector<int64_t> suppress, begin_suppress; std::vector<int32_t> alignment_heads; /* (layer, head) pairs */ };
static GenCfg load_generation_cfg(const std::string& path) {  // src/main.rs:650-657
    GenCfg g;
    if (!is_file(path)) return g;
    FILE* f = fopen(path.c_str(), "rb");
    std::string txt; char b[4096]; size_t n;
    while ((n = fread(b, 1, sizeof b, f)) > 0) txt.append(b, n);
    fclose(f);
    std::string err;
    auto j = whjson::parse(txt, &err);
    if (!j) throw std::runtime_error(path + ": " + err);
    if (auto v = j->get("suppress_tokens")) for (auto& e : v->arr) g.suppress.push_back(e->as_i64());
    if (auto v = j->get("begin_suppress_tokens")) for (auto& e : v->arr) g.begin_suppress.push_back(e->as_i64());
    if (auto v = j->get("alignment_heads"))
        for (auto& e : v->arr)
            if (e->arr.size() == 2) { g.alignment_heads.push_back((int32_t)e->arr[0]->as_i64()); g.alignment_heads.push_back((int32_t)e->arr[1]->as_i64()); }
    return g;
}

// A model id of the form org/name that was downloaded earlier has its files under
// $HF_HOME/hub/models--org--name/snapshots/<revision>/ ($HF_HOME defaults to $HOME/.cache/huggingface): the tokenizer.json of
// the most recently modified snapshot directory that holds one (reference src/main.rs:597-633).  "" when there is none.
static std::string hf_cache_tokenizer(const std::string& model_id) {
    const size_t slash = model_id.find('/');
    if (slash == std::string::npos || slash == 0 || slash + 1 >= model_id.size()) return "";
    const std::string org = model_id.substr(0, slash), name = model_id.substr(slash + 1);
    std::string base;
    if (const char* h = getenv("HF_HOME")) base = h;
    else { const char* home = getenv("HOME"); base = std::string(home ? home : ".") + "/.cache/huggingface"; }
    const std::string snaps = base + "/hub/models--" + org + "--" + name + "/snapshots";
    DIR* d = opendir(snaps.c_str());
    if (!d) return "";
    std::string best;
    bool have = false;
    struct timespec best_m = {0, 0};
    while (struct dirent* e = readdir(d)) {
        const std::string rev = e->d_name;
        if (rev == "." || rev == "..") continue;
        const std::string dir = snaps + "/" + rev, cand = dir + "/tokenizer.json";
        struct stat st_dir, st_tok;
        if (stat(cand.c_str(), &st_tok) != 0 || !S_ISREG(st_tok.st_mode) || stat(dir.c_str(), &st_dir) != 0) continue;
        const bool newer = st_dir.st_mtim.tv_sec > best_m.tv_sec || (st_dir.st_mtim.tv_sec == best_m.tv_sec && st_dir.st_mtim.tv_nsec > best_m.tv_nsec);
        if (!have || newer) { have = true; best_m = st_dir.st_mtim; best = cand; }
    }
    closedir(d);
    return best;
}

static std::vector<int> parse_devices(const std::string& spec, int fallback) {   // "0-7", "0,2,5", "" -> {fallback}
    std::vector<int> out;
    if (trim(spec).empty()) { out.push_back(fallback); return out; }
    size_t pos = 0;
    while (pos <= spec.size()) {
        size_t c = spec.find(',', pos);
        std::string part = trim(spec.substr(pos, c == std::string::npos ? std::string::npos : c - pos));
        if (!part.empty()) {
            size_t dash = part.find('-');
            int lo = atoi(part.c_str()), hi = dash == std::string::npos ? lo : atoi(part.c_str() + dash + 1);
            if (hi < lo) throw std::runtime_error("bad --devices range: " + part);
            for (int d = lo; d <= hi; d++) out.push_back(d);
        }
        if (c == std::string::npos) break;
        pos = c + 1;
    }
    if (out.empty()) throw std::runtime_error("--devices names no device");
    return out;
}

struct Timing { double preprocess_s = 0, model_only_s = 0, decode_s = 0, end_to_end_s = 0; };

// transcribe_longform_chunked (src/main.rs:834-1008) over the C ABI
// --timestamp-rules: the segments of one window's generated tokens (wh_host.h split_segments) and their cues
static std::vector<Segment> window_segments(const std::vector<int64_t>& g, const WhisperSpecial& sp, double duration) {
    return split_segments(g, sp.timestamp_begin, sp.eot, duration);
}
static std::vector<Cue> to_cues(const std::vector<Segment>& segs, const Tokenizer* tok) {
    std::vector<Cue> c;
    for (const Segment& s : segs) {
        std::string text = trim(decode_tokens(s.tokens, tok));
        if (!text.empty()) c.push_back(Cue{s.start, s.end, text, s.has_conf, s.avg_logprob, s.no_speech_prob});   // (a slice between two timestamp pairs may hold no text)
    }
    return c;
}
// the text ids of a generated sequence (timestamp tokens left out)
static std::vector<int64_t> text_ids(const std::vector<int64_t>& g, int64_t tb) {
    std::vector<int64_t> o;
    for (int64_t x : g)
        if (x < tb) o.push_back(x);
    return o;
}

// --logprobs: what a file's row carries.  One window: its avg_logprob and no_speech_prob.  Several windows (long-form): the windows' summed
// log-probabilities over their summed lengths + 1 each, and the mean of their no-speech probabilities.
struct Conf {
    bool has = false;
    double sum_lp = 0, len = 0, sum_ns = 0;
    size_t windows = 0;
    void add(double avg_lp, size_t n_tokens, double ns) { has = true; sum_lp += avg_lp * (double)(n_tokens + 1); len += (double)(n_tokens + 1); sum_ns += ns; windows++; }
    double avg_logprob() const { return len > 0 ? sum_lp / len : 0.0; }
    double no_speech_prob() const { return windows ? sum_ns / (double)windows : 0.0; }
};
// the last decode call's log-probabilities ([n][max_new_tokens], 0 past a window's end) and no-speech probabilities
// --word-timestamps: the alignment heads as (layer, head) pairs — --alignment-heads, else the model directory's generation_config.json, else
// every head of the upper half of the decoder layers (openai-whisper's default), the topmost layers first, while they fit WH_MAX_ALIGN_HEADS
static std::vector<int32_t> alignment_heads(const Args& a, const GenCfg& gen, const wh_dims& dims) {
    std::vector<int32_t> h;
    if (!a.alignment_heads.empty()) {
        const char* p = a.alignment_heads.c_str();
        while (*p) {
            char* e = nullptr;
            const long l = strtol(p, &e, 10);
            if (e == p || *e != ':') throw std::runtime_error("--alignment-heads: expected layer:head,layer:head,... in '" + a.alignment_heads + "'");
            p = e + 1;
            const long hd = strtol(p, &e, 10);
            if (e == p || (*e && *e != ',')) throw std::runtime_error("--alignment-heads: expected layer:head,layer:head,... in '" + a.alignment_heads + "'");
            h.push_back((int32_t)l); h.push_back((int32_t)hd);
            p = *e ? e + 1 : e;
        }
        if (h.empty()) throw std::runtime_error("--alignment-heads names no head");
        return h;
    }
    if (!gen.alignment_heads.empty()) return gen.alignment_heads;
    for (int l = dims.dec_layers - 1; l >= dims.dec_layers / 2 && (int)h.size() / 2 + dims.n_heads <= WH_MAX_ALIGN_HEADS; l--)
        for (int hd = 0; hd < dims.n_heads; hd++) { h.push_back(l); h.push_back(hd); }
    if (h.empty())   // (a model whose layers are wider than the limit: the first heads of the top layer)
        for (int hd = 0; hd < std::min<int>(dims.n_heads, WH_MAX_ALIGN_HEADS); hd++) { h.push_back(dims.dec_layers - 1); h.push_back(hd); }
    return h;
}
// the last decode call's token frames: frames [n][max_new], 0 past a window's end
static void fetch_frames(wh_ctx* ctx, size_t n, size_t max_new, std::vector<int32_t>& frames) {
    frames.assign(std::max<size_t>(1, n) * max_new, 0);
    size_t got = 0;
    if (int rc = wh_get_token_frames(ctx, frames.data(), max_new, nullptr, n, &got)) throw std::runtime_error(std::string("wh_get_token_frames: ") + std::to_string(rc));
    if (got != n) throw std::runtime_error("wh_get_token_frames: " + std::to_string(got) + " windows, expected " + std::to_string(n));
}
// one window's words and token times (seconds from the start of the file) appended to the file's
struct WordOut { std::vector<Word> words; std::vector<double> token_times; };
static void window_words(const Args& a, const std::vector<int64_t>& g, const int32_t* frames, const WhisperSpecial& sp, double duration, double offset,
                         const Tokenizer* tok, WordOut& out) {
    const std::vector<int32_t> fr(frames, frames + g.size());
    // (what the row's text keeps is a word: without --timestamp-rules the text keeps ids at and above timestamp_begin too)
    std::vector<Word> w = words_from_tokens(g, fr, a.timestamp_rules ? sp.timestamp_begin : -1, sp.eot, duration, offset, tok);
    out.words.insert(out.words.end(), w.begin(), w.end());
    for (size_t i = 0; i < g.size(); i++) out.token_times.push_back(std::min(duration, fr[i] * 0.02) + offset);
}
static std::string times_json(const std::vector<double>& t) {
    std::string o = "[";
    char b[32];
    for (size_t i = 0; i < t.size(); i++) { snprintf(b, sizeof b, "%s%.2f", i ? ", " : "", t[i]); o += b; }
    return o + "]";
}

static void fetch_logprobs(wh_ctx* ctx, size_t n, size_t max_new, std::vector<float>& lp, std::vector<float>& ns) {
    lp.assign(std::max<size_t>(1, n) * max_new, 0.0f);
    ns.assign(std::max<size_t>(1, n), 0.0f);
    size_t got = 0;
    if (int rc = wh_get_logprobs(ctx, lp.data(), max_new, ns.data(), n, &got))
        throw std::runtime_error(std::string("wh_get_logprobs: ") + std::to_string(rc));
    if (got != n) throw std::runtime_error("wh_get_logprobs: " + std::to_string(got) + " windows, expected " + std::to_string(n));
}
// --language auto: the last decode call's languages as (code, probability of the chosen language) per window
struct Lang { bool has = false; std::string code; double prob = 0; };
static std::vector<Lang> fetch_languages(wh_ctx* ctx, size_t n, const LanguageTable& lt) {
    std::vector<int64_t> ids(std::max<size_t>(1, n));
    std::vector<float> probs(std::max<size_t>(1, n) * lt.ids.size());
    size_t got = 0;
    if (int rc = wh_get_languages(ctx, ids.data(), probs.data(), n, &got))
        throw std::runtime_error(std::string("wh_get_languages: ") + std::to_string(rc));
    if (got != n) throw std::runtime_error("wh_get_languages: " + std::to_string(got) + " windows, expected " + std::to_string(n));
    std::vector<Lang> out(n);
    for (size_t k = 0; k < n; k++) {
        const size_t j = (size_t)(std::find(lt.ids.begin(), lt.ids.end(), ids[k]) - lt.ids.begin());
        if (j >= lt.ids.size()) throw std::runtime_error("wh_get_languages: id " + std::to_string(ids[k]) + " is not in the language table");
        out[k] = Lang{true, lt.codes[j], (double)probs[k * lt.ids.size() + j]};
    }
    return out;
}
// one window under --logprobs: its avg_logprob (over the generated tokens `g`, EOT still on them), the silence rule; returns true if the window is
// to be skipped
static bool window_conf(const Args& a, const std::vector<int64_t>& g, const float* lp, double ns, int64_t eot, Conf& conf, double& avg_lp) {
    avg_lp = avg_logprob(std::vector<float>(lp, lp + g.size()), g, eot);
    size_t n = 0;
    while (n < g.size() && g[n] != eot) n++;
    conf.add(avg_lp, n, ns);
    return skip_window(ns, avg_lp, a.no_speech_threshold, a.logprob_threshold);
}
static void cues_conf(std::vector<Cue>& cues, double avg_lp, double ns) {
    for (Cue& c : cues) { c.has_conf = true; c.avg_logprob = avg_lp; c.no_speech_prob = ns; }
}

// --beam-size N >= 2: the n best hypotheses of each of the n clips / windows of the last decode call as the comma-separated members of a JSON
// array, {text, sum_logprob, rank_score, finished}, best first; with_window: a leading "window" key (the windows of a long file)
static std::vector<std::string> fetch_hypotheses(wh_ctx* ctx, size_t n, const Args& a, const WhisperSpecial& sp, const Tokenizer* tok, bool with_window) {
    const size_t nh = (size_t)a.n_best, cap = a.max_new_tokens;
    std::vector<int64_t> ht(n * nh * cap);
    std::vector<size_t> hn(n * nh), hcount(n);
    std::vector<float> hs(n * nh), hr(n * nh);
    std::vector<int32_t> hf(n * nh);
    size_t got = 0;
    if (int rc = wh_get_beams(ctx, ht.data(), cap, hn.data(), hs.data(), hr.data(), hf.data(), nh, hcount.data(), n, &got))
        throw std::runtime_error(std::string("wh_get_beams: ") + std::to_string(rc));
    std::vector<std::string> out(n);
    for (size_t k = 0; k < n; k++)
        for (size_t h = 0; h < hcount[k]; h++) {
            const size_t at = k * nh + h;
            std::vector<int64_t> g(ht.begin() + at * cap, ht.begin() + at * cap + hn[at]);
            if (!g.empty() && g.back() == sp.eot) g.pop_back();
            if (a.timestamp_rules) g = text_ids(g, sp.timestamp_begin);
            JVal j = JVal::obj(false);
            JVal s1, s2;
            s1.raw = fmt_conf(hs[at]); s2.raw = fmt_conf(hr[at]);
            if (with_window) j.set("window", JVal::integer((long long)k));
            j.set("text", JVal::str(trim(decode_tokens(g, tok)))).set("sum_logprob", s1).set("rank_score", s2).set("finished", JVal::boolean(hf[at] != 0));
            out[k] += (h ? ", " : "");
            j.write(out[k], 4);
        }
    return out;
}

// a pipeline item's raw payload as the C ABI takes it
static wh_raw_clip raw_clip_of(const PipeItem& it) {
    wh_raw_clip r{};
    r.data = it.raw_data();
    r.n_frames = it.raw.n_frames;
    r.sample_rate = it.raw.sample_rate;
    r.channels = (uint16_t)std::min<uint32_t>(it.raw.channels, 0xFFFF);   // (more than WH_MAX_CHANNELS: the library refuses the clip)
    r.format = (uint16_t)it.raw.format;
    return r;
}

static std::string transcribe(wh_ctx* ctx, const std::vector<float>& audio, const Args& a, const Tokenizer* tok,
                              const GenCfg& gen, Timing& t, std::vector<Cue>* cues = nullptr, Conf* conf = nullptr,
                              const LanguageTable* lt = nullptr, Lang* lang = nullptr, const std::vector<int64_t>* prefix = nullptr, WordOut* words = nullptr,
                              std::string* hyps = nullptr, const wh_raw_clip* raw = nullptr) {
    const double t0 = now_s();
    const size_t n_audio = raw ? wh_resampled_samples(raw->n_frames, raw->sample_rate) : audio.size();   // (raw: the file is converted on the device)
    if (a.prompts()) {   // the file's text context, on its first window or on every one (no context: an empty prefix)
        const size_t offs[2] = {0, prefix ? prefix->size() : 0};
        wh_prefix_opts po{sizeof(wh_prefix_opts), prefix ? prefix->data() : nullptr, offs, 1, a.prompt_all_windows ? WH_PREFIX_ALL_WINDOWS : WH_PREFIX_FIRST_WINDOW};
        if (int rc = wh_ctx_set_prefixes(ctx, &po)) throw std::runtime_error(std::string("wh_ctx_set_prefixes: ") + std::to_string(rc) + ": " + wh_last_error(ctx));
    }
    WhisperSpecial sp = special_tokens(a.language, a.task, tok);
    std::vector<int64_t> prompt = {sp.sot, sp.lang, sp.task};
    if (!a.timestamps && !a.timestamp_rules) prompt.push_back(sp.no_timestamps);
    wh_decode_params p{};
    p.prompt = prompt.data(); p.n_prompt = prompt.size(); p.max_new_tokens = a.max_new_tokens; p.eot = sp.eot;
    p.suppress = gen.suppress.data(); p.n_suppress = gen.suppress.size();
    p.begin_suppress = gen.begin_suppress.data(); p.n_begin_suppress = gen.begin_suppress.size();
    size_t nch = 0;
    wh_longform_plan(n_audio, a.chunk_length_s, a.overlap_s, nullptr, 0, &nch);
    const size_t stride = prompt.size() + a.max_new_tokens;
    std::vector<int64_t> toks(std::max<size_t>(1, nch) * stride);
    std::vector<size_t> ntok(std::max<size_t>(1, nch));
    size_t got = 0;
    int rc = raw ? wh_transcribe_longform_raw(ctx, raw, a.chunk_length_s, a.overlap_s, &p, toks.data(), ntok.data(), ntok.size(), &got)
                 : wh_transcribe_longform(ctx, audio.data(), audio.size(), a.chunk_length_s, a.overlap_s, &p, toks.data(),
                                          ntok.data(), ntok.size(), &got);
    if (rc) throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc) + ": " + wh_last_error(ctx));
    wh_timing wt{};
    wh_get_timings(ctx, &wt);
    t.preprocess_s = wt.preprocess_s;
    t.model_only_s = wt.encode_s + wt.decode_s;
    std::vector<float> lps, nss;
    if (a.logprobs) fetch_logprobs(ctx, got, a.max_new_tokens, lps, nss);
    if (lt && lang && got) *lang = fetch_languages(ctx, got, *lt)[0];   // the file's language: its first window's
    std::vector<int32_t> frames;
    if (a.word_timestamps) fetch_frames(ctx, got, a.max_new_tokens, frames);
    if (a.beam() && hyps) {   // a long file: every window's n best, one after the other, each naming its window
        std::string o;
        for (const std::string& w : fetch_hypotheses(ctx, got, a, sp, tok, true))
            if (!w.empty()) o += (o.empty() ? "" : ", ") + w;
        *hyps = "[" + o + "]";
    }
    const double td0 = now_s();
    std::vector<std::string> texts;
    std::vector<size_t> offs(std::max<size_t>(1, got));
    if (a.timestamp_rules || a.word_timestamps) wh_longform_plan(n_audio, a.chunk_length_s, a.overlap_s, offs.data(), offs.size(), &nch);
    std::vector<std::vector<Segment>> wsegs;
    std::vector<double> wstart;
    for (size_t c = 0; c < got; c++) {  // :926-943
        std::vector<int64_t> g;
        if (ntok[c] > prompt.size()) g.assign(toks.begin() + c * stride + prompt.size(), toks.begin() + c * stride + ntok[c]);
        double avg_lp = 0;
        Conf unused;
        const bool skip = a.logprobs && window_conf(a, g, lps.data() + c * a.max_new_tokens, nss[c], sp.eot, conf ? *conf : unused, avg_lp);
        if (skip) g.clear();   // the silence rule: empty text, no segments
        if (a.word_timestamps && words) {
            const size_t wlen = std::min<size_t>(n_audio - offs[c], (size_t)std::llround(a.chunk_length_s * 16000.0));
            window_words(a, g, frames.data() + c * a.max_new_tokens, sp, (double)wlen / 16000.0, (double)offs[c] / 16000.0, tok, *words);
        }
        if (!g.empty() && g.back() == sp.eot) g.pop_back();
        if (a.timestamp_rules) {
            const size_t len = std::min<size_t>(n_audio - offs[c], (size_t)std::llround(a.chunk_length_s * 16000.0));
            wsegs.push_back(skip ? std::vector<Segment>() : window_segments(g, sp, (double)len / 16000.0));
            if (a.logprobs) set_conf(wsegs.back(), avg_lp, nss[c]);
            wstart.push_back((double)offs[c] / 16000.0);
            g = text_ids(g, sp.timestamp_begin);
        }
        std::string text = skip ? std::string() : decode_tokens(g, tok);
        if (text.empty()) text = "[EMPTY]";
        if (text != "[EMPTY]") texts.push_back(text);
    }
    if (cues) *cues = to_cues(merge_window_segments(wsegs, wstart, a.overlap_s), tok);
    t.decode_s = now_s() - td0;
    std::string full = stitch_texts(texts);
    t.end_to_end_s = now_s() - t0;
    return full;
}

int main(int argc, char** argv) {
    Args a;
    if (!parse_args(argc, argv, a)) return 2;
    if (a.language == "auto" && a.prompts()) {   // (the library would refuse each call: reported here, before any device is touched)
        fprintf(stderr, "Error: --language auto cannot be combined with --prompt-ids / --prompt-ids-dir: the language is detected from the logits at "
                        "<|startoftranscript|>, which a text context changes; detect the language with a run without the prompt flags first\n");
        return 2;
    }
    try {
        for (auto* p : {&a.out_csv, &a.out_json, &a.out_summary_json})
            if (!parent_dir(*p).empty()) mkdir_p(parent_dir(*p));
        OrtCfg cfg = a.discovery_best_json.empty() ? suggested_optimum_cfg() : load_best_cfg_from_discovery(a.discovery_best_json);
        if (a.intra_op > 0) cfg.intra_op = a.intra_op;
        if (a.inter_op > 0) cfg.inter_op = a.inter_op;
        if (a.beam()) cfg.beam_size = a.beam_size;   // (config_used gains beam_size only then: the greedy summaries keep their bytes)
        if (a.ladder()) cfg.temperature = a.temperature;   // (the same for the ladder)

        Tokenizer tok;  // resolve_tokenizer, src/main.rs:574-635: explicit path, model directories, then the Hugging Face cache
        if (!trim(a.tokenizer_json).empty()) {
            if (!is_file(trim(a.tokenizer_json))) throw std::runtime_error("tokenizer_json not found: " + trim(a.tokenizer_json));
            load_tokenizer(trim(a.tokenizer_json), tok);
        } else {
            std::string found;
            for (const std::string& cand : {a.onnx_dir + "/tokenizer.json", a.model_id + "/tokenizer.json"})
                if (is_file(cand)) { found = cand; break; }
            if (found.empty()) found = hf_cache_tokenizer(a.model_id);
            if (!found.empty()) load_tokenizer(found, tok);
        }
        const bool synthetic_model = a.onnx_dir.rfind("synthetic:", 0) == 0;
        GenCfg gen = load_generation_cfg(a.onnx_dir + "/generation_config.json");
        if (!synthetic_model && !is_dir(a.onnx_dir)) throw std::runtime_error("onnx_dir does not exist or is not a directory: " + a.onnx_dir);

        const int prec = a.precision == "f32" ? WH_PREC_F32 : a.precision == "fp8" ? WH_PREC_FP8 : a.precision == "f16x3" ? WH_PREC_F16X3 : WH_PREC_BF16;
        // One model per device (the reference shares its three `&Session`s across the rayon pool, src/main.rs:890-919),
        // `--streams-per-gpu` contexts per model, one host thread per context; files are independent units
        // (src/main.rs:1164 loops over them serially) and are dealt to whichever context is free.
        const std::vector<int> devices = parse_devices(a.devices, a.device);
        if (a.print_plan) {   // what the command line asks for, before wh_model_load touches a device (CPU test of the --devices surface)
            JVal plan = JVal::obj(false);
            std::string devs = "[", ctxl = "[";
            for (size_t i = 0; i < devices.size(); i++) {
                devs += (i ? ", " : "") + std::to_string(devices[i]);
                for (int st = 0; st < a.streams_per_gpu; st++)
                    ctxl += std::string(ctxl.size() > 1 ? ", " : "") + "{\"context\": " + std::to_string(i * a.streams_per_gpu + st) + ", \"device\": " + std::to_string(devices[i]) +
                            ", \"stream\": " + std::to_string(st) + "}";
            }
            JVal jd; jd.raw = devs + "]";
            JVal jc; jc.raw = ctxl + "]";
            plan.set("devices", jd).set("models", JVal::integer((long long)devices.size())).set("contexts", jc)
                .set("host_threads", JVal::integer((long long)(devices.size() * a.streams_per_gpu))).set("max_batch", JVal::integer(a.max_batch))
                .set("precision", JVal::str(a.precision));
            if (a.beam())
                plan.set("beam_size", JVal::integer(a.beam_size)).set("patience", JVal::num(a.patience)).set("length_penalty", JVal::num(a.length_penalty))
                    .set("n_best", JVal::integer(a.n_best)).set("files_per_batch", JVal::integer(a.max_batch / a.beam_size));
            if (a.ladder()) {
                JVal t, thr;
                t.raw = "[";
                for (size_t i = 0; i < a.temperature.size(); i++) t.raw += (i ? ", " : "") + fmt_f32(a.temperature[i]);
                t.raw += "]";
                thr.raw = fmt_conf(a.compression_ratio_threshold);
                plan.set("temperature", t).set("compression_ratio_threshold", thr).set("seed", JVal::integer((long long)a.seed)).set("pipelined", JVal::boolean(false));
            }
            printf("%s\n", plan.pretty().c_str());
            return 0;
        }
        std::vector<wh_model*> models;
        std::vector<wh_ctx*> ctxs;
        const bool lang_auto = a.language == "auto";
        LanguageTable lang_table;
        for (int dev : devices) {
            wh_model* m = nullptr;
            if (int rc = wh_model_load(a.onnx_dir.c_str(), dev, prec, &m))
                throw std::runtime_error("Failed to load " + a.onnx_dir + " on device " + std::to_string(dev) + ": libwhisper_hip error " +
                                         std::to_string(rc) + ": " + wh_last_error(nullptr));
            models.push_back(m);
            if (lang_auto && lang_table.ids.empty()) {
                wh_dims dims{};
                wh_model_get_dims(m, &dims);
                lang_table = language_table(tok.loaded ? &tok : nullptr, dims.vocab);
            }
            for (int st = 0; st < a.streams_per_gpu; st++) {
                wh_ctx* c = nullptr;
                int rows = a.max_batch;
                if (a.align()) {   // a pass holds whole files of prompt + transcript - 1 rows each: room for one of any length at least
                    wh_dims dims{};
                    wh_model_get_dims(m, &dims);
                    rows = std::max(rows, dims.n_text_ctx);
                }
                if (int rc = wh_ctx_create(m, rows, &c))
                    throw std::runtime_error(std::string("wh_ctx_create: ") + std::to_string(rc) + ": " + wh_last_error(nullptr));
                if (a.timestamp_rules) {   // Whisper's timestamp rules on every context (no reference counterpart)
                    WhisperSpecial sp = special_tokens(a.language, a.task, &tok);
                    wh_timestamp_rules tr{sizeof(wh_timestamp_rules), sp.timestamp_begin, sp.no_timestamps, 50};
                    if (int rc = wh_ctx_set_timestamp_rules(c, &tr))
                        throw std::runtime_error(std::string("wh_ctx_set_timestamp_rules: ") + std::to_string(rc) + ": " + wh_last_error(c));
                }
                if (a.logprobs) {   // token log-probabilities and the no-speech probe at <|startoftranscript|> (prompt position 0)
                    WhisperSpecial sp = special_tokens(a.language, a.task, &tok);
                    wh_logprob_opts lo{sizeof(wh_logprob_opts), sp.no_speech, 0};
                    if (int rc = wh_ctx_set_logprobs(c, &lo))
                        throw std::runtime_error(std::string("wh_ctx_set_logprobs: ") + std::to_string(rc) + ": " + wh_last_error(c));
                }
                if (a.have_rep_penalty || a.have_rep_ngram) {   // repetition penalty / no-repeat n-grams on every context (no reference counterpart)
                    wh_repetition_opts ro{sizeof(wh_repetition_opts), a.rep_penalty, a.rep_ngram};
                    if (int rc = wh_ctx_set_repetition(c, &ro))
                        throw std::runtime_error(std::string("wh_ctx_set_repetition: ") + std::to_string(rc) + ": " + wh_last_error(c));
                }
                if (a.beam()) {   // beam search on every context (no reference counterpart)
                    wh_beam_opts bo{sizeof(wh_beam_opts), a.beam_size, a.patience, a.length_penalty, nullptr, 0};
                    if (int rc = wh_ctx_set_beam_search(c, &bo))
                        throw std::runtime_error(std::string("wh_ctx_set_beam_search: ") + std::to_string(rc) + ": " + wh_last_error(c));
                }
                if (a.word_timestamps) {   // word-level timestamps on every context (no reference counterpart)
                    wh_dims dims{};
                    wh_model_get_dims(m, &dims);
                    const std::vector<int32_t> heads = alignment_heads(a, gen, dims);
                    wh_alignment_opts ao{sizeof(wh_alignment_opts), heads.data(), heads.size() / 2, nullptr, 0};
                    if (int rc = wh_ctx_set_alignment(c, &ao))
                        throw std::runtime_error(std::string("wh_ctx_set_alignment: ") + std::to_string(rc) + ": " + wh_last_error(c));
                }
                if (lang_auto) {   // each clip's language from the logits at <|startoftranscript|> (prompt position 0), decoded into position 1
                    wh_language_opts lo{sizeof(wh_language_opts), lang_table.ids.data(), lang_table.ids.size(), 0};
                    if (int rc = wh_ctx_set_language_detection(c, &lo))
                        throw std::runtime_error(std::string("wh_ctx_set_language_detection: ") + std::to_string(rc) + ": " + wh_last_error(c));
                }
                ctxs.push_back(c);
            }
        }

        std::vector<std::string> files;
        if (a.synthetic_clips) {
            for (size_t i = 0; i < a.synthetic_clips; i++) { char b[64]; snprintf(b, sizeof b, "clip_%04zu.wav", i); files.push_back(b); }
        } else {
            DIR* d = opendir(a.audio_dir.c_str());
            if (!d) throw std::runtime_error("cannot read audio dir " + a.audio_dir);
            while (dirent* e = readdir(d)) {
                std::string n = e->d_name;
                size_t dot = n.rfind('.');
                if (dot == std::string::npos) continue;
                std::string ext = lower(n.substr(dot + 1));
                if (ext == "wav" || ext == "flac" || ext == "mp3") files.push_back(n);
            }
            closedir(d);
        }
        std::sort(files.begin(), files.end());
        if (a.limit_files > 0 && files.size() > a.limit_files) files.resize(a.limit_files);
        if (files.empty()) throw std::runtime_error("No audio files found in " + a.audio_dir);

        // text context: each file's prefix = <|startofprev|> ++ the tail of its ids (wh_host.h build_prev_prefix)
        std::vector<std::vector<int64_t>> file_prefix(files.size()), file_hist(files.size());   // (file_hist: the ids themselves, the head of --sequential's history)
        if (a.prompts()) {
            wh_dims dims{};
            wh_model_get_dims(models[0], &dims);
            const WhisperSpecial spp = special_tokens(a.language, a.task, &tok);
            const std::vector<int64_t> every = parse_ids(a.prompt_ids, "--prompt-ids");
            for (size_t i = 0; i < files.size(); i++) {
                std::vector<int64_t> hist = every;
                const std::string path = a.prompt_ids_dir + "/" + files[i].substr(0, files[i].rfind('.')) + ".txt";
                if (!a.prompt_ids_dir.empty() && is_file(path)) {
                    FILE* f = fopen(path.c_str(), "rb");
                    if (!f) throw std::runtime_error("cannot read " + path);
                    std::string txt; char b[4096]; size_t n;
                    while ((n = fread(b, 1, sizeof b, f)) > 0) txt.append(b, n);
                    fclose(f);
                    hist = parse_ids(txt, path);
                }
                for (int64_t t : hist)
                    if (t >= dims.vocab) throw std::runtime_error("prompt id " + std::to_string(t) + " of " + files[i] + " is outside the vocabulary (" + std::to_string(dims.vocab) + ")");
                file_prefix[i] = build_prev_prefix(hist, spp.sot_prev, dims.n_text_ctx);
                file_hist[i] = hist;
            }
        }

        // forced alignment: each file's transcript ids
        std::vector<std::vector<int64_t>> file_align(files.size());
        std::vector<int32_t> align_heads;
        if (a.align()) {
            wh_dims dims{};
            wh_model_get_dims(models[0], &dims);
            align_heads = alignment_heads(a, gen, dims);
            for (size_t i = 0; i < files.size(); i++) {
                const std::string path = a.align_ids_dir + "/" + files[i].substr(0, files[i].rfind('.')) + ".txt";
                FILE* f = is_file(path) ? fopen(path.c_str(), "rb") : nullptr;
                if (!f) throw std::runtime_error("--align-ids-dir: no transcript ids for " + files[i] + ": cannot read " + path);
                std::string txt; char b[4096]; size_t n;
                while ((n = fread(b, 1, sizeof b, f)) > 0) txt.append(b, n);
                fclose(f);
                file_align[i] = parse_ids(txt, path);
                if (file_align[i].empty()) throw std::runtime_error("--align-ids-dir: " + path + " holds no id");
                for (int64_t t : file_align[i])
                    if (t >= dims.vocab) throw std::runtime_error("id " + std::to_string(t) + " of " + path + " is outside the vocabulary (" + std::to_string(dims.vocab) + ")");
            }
        }

        auto load = [&](size_t idx, std::vector<float>& audio, double& dur) {
            if (a.synthetic_clips) { audio = synthetic_clip(a.seed + idx); dur = (double)audio.size() / 16000.0; }
            else load_audio_16k_mono(a.audio_dir + "/" + files[idx], audio, &dur);
        };
        // --gpu-ingest: the loader reads and parses only (wh_host.h read_wav_raw); duration_s is the resampled length over 16000, as above
        auto load_raw = [&](size_t idx, PipeItem& it) {
            it.raw = read_wav_raw(a.audio_dir + "/" + files[idx]);
            it.is_raw = true;
            it.n_16k = wh_resampled_samples(it.raw.n_frames, it.raw.sample_rate);
            it.dur = (double)it.n_16k / 16000.0;
        };
        const bool gpu_ingest = a.gpu_ingest && !a.synthetic_clips;
        if (a.warmup > 0) {  // :1131-1152
            std::vector<float> a0; double d0;
            load(0, a0, d0);
            for (wh_ctx* c : ctxs)
                for (size_t i = 0; i < a.warmup; i++) { Timing t; transcribe(c, a0, a, &tok, gen, t); }
        }

        // ---- the file loop (:1164-1213) as a pipeline (wh_host.h run_file_pipeline): loader threads -> bounded queue -> one
        // worker per context; one-window files are staged in page-locked buffers ----
        typedef PipeItem Item;
        BufferPool pool([]() -> float* {
                            float* p = nullptr;
                            return hipHostMalloc((void**)&p, (size_t)WH_CLIP_SAMPLES * sizeof(float), hipHostMallocDefault) == hipSuccess ? p : nullptr;
                        },
                        [](float* p) { (void)hipHostFree(p); });
        struct Result { std::string text; double dur = 0, load_s = 0; Timing t; bool ok = false; std::vector<Cue> cues; Conf conf; Lang lang; WordOut words; std::string hyps;
                        bool has_ladder = false; double temperature = 0, compression_ratio = 0; std::string windows;
                        bool aligned = false; double aligned_avg_lp = 0; };
        const size_t nfiles = files.size();
        std::vector<Result> results(nfiles);
        const unsigned hc = std::thread::hardware_concurrency();
        const int n_loaders = a.load_threads > 0 ? a.load_threads : (int)std::min<unsigned>(8, std::max<unsigned>(1, hc / 2));
        WhisperSpecial sp = special_tokens(a.language, a.task, &tok);
        std::vector<int64_t> prompt = {sp.sot, sp.lang, sp.task};
        if (!a.timestamps && !a.timestamp_rules) prompt.push_back(sp.no_timestamps);
        std::vector<double> busy_s(ctxs.size(), 0.0);
        // ---- --sequential: a worker's files as resident file sets, advanced in lockstep (wh_host.h run_sequential).  A step's rows go
        // through wh_transcribe_windows with each row's text so far as its prefix; with a ladder, a step is run_ladder over its rows — rung 0 that call,
        // later rungs wh_decode_greedy_batch on the resident states — and a row's random stream is (file index << 32 | window ordinal), so a result
        // does not depend on --max-batch ----
        wh_dims model_dims{};
        wh_model_get_dims(models[0], &model_dims);
        auto process_sequential = [&](wh_ctx* ctx, std::vector<Item>& batch) {
            const size_t stride = prompt.size() + a.max_new_tokens, max_new = a.max_new_tokens;
            wh_decode_params p{};
            p.prompt = prompt.data(); p.n_prompt = prompt.size(); p.max_new_tokens = max_new; p.eot = sp.eot;
            p.suppress = gen.suppress.data(); p.n_suppress = gen.suppress.size();
            p.begin_suppress = gen.begin_suppress.data(); p.n_begin_suppress = gen.begin_suppress.size();
            SeqConfig cfg;
            cfg.tb = sp.timestamp_begin; cfg.eot = sp.eot; cfg.sot_prev = sp.sot_prev; cfg.n_text_ctx = model_dims.n_text_ctx;
            cfg.n_prompt = prompt.size(); cfg.max_new_tokens = max_new; cfg.condition_on_previous_text = a.condition_on_previous_text;
            cfg.no_speech_threshold = a.no_speech_threshold; cfg.logprob_threshold = a.logprob_threshold;
            struct WinExtra { double avg_lp = 0, ns = 0; size_t n_tok = 0; std::vector<int32_t> frames; };
            for (size_t at = 0; at < batch.size();) {
                size_t end = at;   // the files of one set: as many as --sequential-max-audio-s holds, one at least
                double audio_s = 0;
                while (end < batch.size() && (end == at || audio_s + batch[end].dur <= a.sequential_max_audio_s)) audio_s += batch[end++].dur;
                const size_t n = end - at;
                const double t0 = now_s();
                std::vector<int64_t> frames(n);
                int rc;
                if (batch[at].is_raw) {
                    std::vector<wh_raw_clip> rcl(n);
                    for (size_t k = 0; k < n; k++) rcl[k] = raw_clip_of(batch[at + k]);
                    rc = wh_files_load_raw(ctx, rcl.data(), n, frames.data());
                } else {
                    std::vector<wh_clip> cl(n);
                    for (size_t k = 0; k < n; k++) { cl[k].pcm = batch[at + k].data(); cl[k].n_samples = batch[at + k].n(); }
                    rc = wh_files_load(ctx, cl.data(), n, frames.data());
                }
                if (rc) throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                wh_timing wt{};
                wh_get_timings(ctx, &wt);
                const double mel_s = wt.preprocess_s;
                double cut_s = 0, model_s = 0;
                cfg.file_prompts.assign(n, std::vector<int64_t>());
                for (size_t k = 0; k < n; k++) cfg.file_prompts[k] = file_hist[batch[at + k].idx];
                std::vector<std::vector<WinExtra>> extra(n);
                std::vector<double> done_s(n, 0.0);
                std::vector<SeqFile> out;
                run_sequential(frames, cfg, [&](const std::vector<SeqRow>& rows, std::vector<SeqStepResult>& res) {
                    const size_t nr = rows.size();
                    std::vector<int32_t> fi(nr);
                    std::vector<int64_t> sk(nr), ids;
                    std::vector<size_t> offs(1, 0);
                    for (size_t i = 0; i < nr; i++) {
                        fi[i] = (int32_t)rows[i].file; sk[i] = rows[i].seek;
                        ids.insert(ids.end(), rows[i].prefix.begin(), rows[i].prefix.end());
                        offs.push_back(ids.size());
                    }
                    wh_prefix_opts po{sizeof(wh_prefix_opts), ids.data(), offs.data(), nr, WH_PREFIX_FIRST_WINDOW};
                    if (int rc2 = wh_ctx_set_prefixes(ctx, &po)) throw std::runtime_error(std::string("wh_ctx_set_prefixes: ") + std::to_string(rc2) + ": " + wh_last_error(ctx));
                    std::vector<int64_t> toks(nr * stride);
                    std::vector<size_t> ntok(nr);
                    std::vector<float> lps(nr * max_new, 0.0f), nss(nr, 0.0f);
                    std::vector<int> rung_of(nr, 0);
                    std::vector<WindowScore> scores;
                    auto timings = [&] { wh_timing w{}; wh_get_timings(ctx, &w); cut_s += w.preprocess_s; model_s += w.encode_s + w.decode_s; };
                    if (!a.ladder()) {
                        if (int rc2 = wh_transcribe_windows(ctx, fi.data(), sk.data(), nr, &p, toks.data(), ntok.data()))
                            throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc2) + ": " + wh_last_error(ctx));
                        timings();
                        if (a.logprobs) fetch_logprobs(ctx, nr, max_new, lps, nss);
                    } else {
                        run_ladder(nr, a.temperature.size(), a.compression_ratio_threshold, a.logprob_threshold, a.no_speech_threshold,
                                   [&](size_t rung, const std::vector<unsigned char>& active, std::vector<WindowScore>& sc) {
                                       std::vector<float> temps(nr);
                                       std::vector<uint8_t> act(active.begin(), active.end());
                                       std::vector<uint64_t> rid(nr);
                                       for (size_t i = 0; i < nr; i++) {
                                           temps[i] = active[i] ? a.temperature[rung] : 0.0f;
                                           rid[i] = ((uint64_t)batch[at + rows[i].file].idx << 32) | (uint64_t)rows[i].window;
                                       }
                                       wh_sampling_opts so{sizeof(wh_sampling_opts), a.seed, temps.data(), act.data(), rid.data(), nr};
                                       if (int rc2 = wh_ctx_set_sampling(ctx, &so)) throw std::runtime_error(std::string("wh_ctx_set_sampling: ") + std::to_string(rc2) + ": " + wh_last_error(ctx));
                                       std::vector<int64_t> toks2(nr * stride);
                                       std::vector<size_t> ntok2(nr);
                                       size_t got = 0;
                                       const int rc2 = rung == 0 ? wh_transcribe_windows(ctx, fi.data(), sk.data(), nr, &p, toks2.data(), ntok2.data())
                                                                 : wh_decode_greedy_batch(ctx, &p, toks2.data(), stride, ntok2.data(), nr, &got, nullptr, 0);
                                       if (rc2) throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc2) + ": " + wh_last_error(ctx));
                                       timings();
                                       std::vector<float> lps2, nss2;
                                       fetch_logprobs(ctx, nr, max_new, lps2, nss2);
                                       for (size_t i = 0; i < nr; i++) {
                                           if (!active[i]) continue;
                                           std::copy_n(toks2.begin() + i * stride, stride, toks.begin() + i * stride);
                                           ntok[i] = ntok2[i];
                                           std::copy_n(lps2.begin() + i * max_new, max_new, lps.begin() + i * max_new);
                                           nss[i] = nss2[i];
                                           std::vector<int64_t> g;
                                           if (ntok[i] > prompt.size()) g.assign(toks.begin() + i * stride + prompt.size(), toks.begin() + i * stride + ntok[i]);
                                           sc[i].avg_logprob = avg_logprob(std::vector<float>(lps.begin() + i * max_new, lps.begin() + i * max_new + g.size()), g, sp.eot);
                                           sc[i].no_speech_prob = nss[i];
                                           if (!g.empty() && g.back() == sp.eot) g.pop_back();
                                           sc[i].compression_ratio = compression_ratio(trim(decode_tokens(text_ids(g, sp.timestamp_begin), &tok)));
                                       }
                                   },
                                   rung_of, scores);
                    }
                    std::vector<int32_t> fr;
                    if (a.word_timestamps) fetch_frames(ctx, nr, max_new, fr);
                    for (size_t i = 0; i < nr; i++) {
                        std::vector<int64_t> g;
                        if (ntok[i] > prompt.size()) g.assign(toks.begin() + i * stride + prompt.size(), toks.begin() + i * stride + ntok[i]);
                        WinExtra x;
                        if (a.logprobs) {
                            x.avg_lp = avg_logprob(std::vector<float>(lps.begin() + i * max_new, lps.begin() + i * max_new + g.size()), g, sp.eot);
                            x.ns = nss[i];
                        }
                        while (x.n_tok < g.size() && g[x.n_tok] != sp.eot) x.n_tok++;
                        if (a.word_timestamps) x.frames.assign(fr.begin() + i * max_new, fr.begin() + i * max_new + g.size());
                        res[i].tokens = g;
                        res[i].avg_logprob = x.avg_lp;
                        res[i].no_speech_prob = x.ns;
                        res[i].temperature = a.ladder() ? (double)a.temperature[rung_of[i]] : 0.0;
                        extra[rows[i].file].push_back(std::move(x));
                        done_s[rows[i].file] = now_s() - t0;
                    }
                }, out);
                for (size_t k = 0; k < n; k++) {
                    Result& r = results[batch[at + k].idx];
                    const double td0 = now_s();
                    std::string text, wj = "[";
                    for (const SeqSegment& s : out[k].segments) {
                        const std::string piece = decode_tokens(text_ids(s.ids, sp.timestamp_begin), &tok);
                        text += piece;
                        const WinExtra& x = extra[k][s.window];
                        if (!trim(piece).empty()) r.cues.push_back(Cue{s.start, s.end, trim(piece), a.logprobs, x.avg_lp, x.ns});
                    }
                    r.text = trim(text);
                    double t_max = 0;
                    for (size_t w = 0; w < out[k].windows.size(); w++) {
                        const SeqWindow& sw = out[k].windows[w];
                        const WinExtra& x = extra[k][w];
                        if (a.logprobs) r.conf.add(x.avg_lp, x.n_tok, x.ns);
                        t_max = std::max(t_max, sw.temperature);
                        if (a.word_timestamps && !sw.skipped) {   // the words of what the window's segments cover, its frames offset by its seek
                            const std::vector<int64_t> g(sw.tokens.begin(), sw.tokens.begin() + (long)std::min(sw.consumed, sw.tokens.size()));
                            window_words(a, g, x.frames.data(), sp, sw.seg_frames * 0.01, (double)sw.seek * 0.01, &tok, r.words);
                        }
                        wj += std::string(w ? ", " : "") + "{\"seek_s\": " + fmt_f64((double)sw.seek * 0.01) + ", \"frames\": " + std::to_string(sw.seg_frames) + ", \"advance_s\": " +
                              fmt_f64((double)sw.advance * 0.01) + ", \"skipped\": " + (sw.skipped ? "true" : "false") + ", \"temperature\": " + fmt_f32((float)sw.temperature) + ", \"tokens\": [";
                        for (size_t j = 0; j < sw.tokens.size(); j++) wj += (j ? ", " : "") + std::to_string(sw.tokens[j]);
                        wj += "]}";
                    }
                    r.windows = wj + "]";
                    if (a.ladder()) { r.has_ladder = true; r.temperature = t_max; r.compression_ratio = r.text.empty() ? 0.0 : compression_ratio(r.text); }
                    r.t.preprocess_s = mel_s + cut_s;
                    r.t.model_only_s = model_s;
                    r.t.decode_s = now_s() - td0;
                    r.t.end_to_end_s = done_s[k] + r.t.decode_s;   // a file completes with the step that decodes its last window
                    r.dur = batch[at + k].dur; r.load_s = batch[at + k].load_s; r.ok = true;
                }
                at = end;
            }
        };
        auto process = [&](size_t wi, std::vector<Item>& batch, std::vector<Item>* next) {
            wh_ctx* ctx = ctxs[wi];
            const size_t stride = prompt.size() + a.max_new_tokens;
            const double tb0 = now_s();
            if (a.sequential) {
                process_sequential(ctx, batch);
                busy_s[wi] += now_s() - tb0;
                return;
            }
            if (a.align())
                for (const PipeItem& it : batch)
                    if (it.n() > (size_t)WH_CLIP_SAMPLES)
                        throw std::runtime_error("--align-ids-dir: " + files[it.idx] + " is longer than one 30 s window; forced alignment is built for one-window files");
            if (batch.size() == 1 && batch[0].n() > (size_t)WH_CLIP_SAMPLES) {
                // a file longer than one window goes alone through the long-form entry (which batches its windows)
                Result& r = results[batch[0].idx];
                if (a.ladder())   // (the re-decode needs the windows' encoder states resident: the long-form entry keeps its last device batch's only)
                    throw std::runtime_error("--temperature: " + files[batch[0].idx] + " is longer than one 30 s window; the ladder is built for one-window files (--sequential runs it on files of any length)");
                wh_raw_clip rc0{};
                if (batch[0].is_raw) rc0 = raw_clip_of(batch[0]);
                r.text = transcribe(ctx, batch[0].audio, a, &tok, gen, r.t, &r.cues, &r.conf, lang_auto ? &lang_table : nullptr, &r.lang, &file_prefix[batch[0].idx], &r.words, &r.hyps,
                                    batch[0].is_raw ? &rc0 : nullptr);
                r.dur = batch[0].dur; r.load_s = batch[0].load_s; r.ok = true;
            } else {
                // the per-window body of transcribe_longform_chunked (:870-915) for a batch of one-window files
                std::vector<int64_t> toks(batch.size() * stride);
                std::vector<size_t> ntok(batch.size());
                wh_decode_params p{};
                p.prompt = prompt.data(); p.n_prompt = prompt.size(); p.max_new_tokens = a.max_new_tokens; p.eot = sp.eot;
                p.suppress = gen.suppress.data(); p.n_suppress = gen.suppress.size();
                p.begin_suppress = gen.begin_suppress.data(); p.n_begin_suppress = gen.begin_suppress.size();
                std::vector<wh_clip> clips(batch.size()), nclips(next ? next->size() : 0);
                const bool raw = batch[0].is_raw;   // --gpu-ingest: every item of the run carries the file's own samples
                std::vector<wh_raw_clip> rclips(raw ? batch.size() : 0), rnext(raw && next ? next->size() : 0);
                if (raw) {
                    for (size_t k = 0; k < batch.size(); k++) rclips[k] = raw_clip_of(batch[k]);
                    for (size_t k = 0; k < rnext.size(); k++) rnext[k] = raw_clip_of((*next)[k]);
                } else {
                    for (size_t k = 0; k < batch.size(); k++) { clips[k].pcm = batch[k].data(); clips[k].n_samples = batch[k].n(); }
                    for (size_t k = 0; k < nclips.size(); k++) { nclips[k].pcm = (*next)[k].data(); nclips[k].n_samples = (*next)[k].n(); }
                }
                if (a.prompts()) {   // every file of the batch with its own text context
                    std::vector<int64_t> ids;
                    std::vector<size_t> offs(1, 0);
                    for (size_t k = 0; k < batch.size(); k++) {
                        ids.insert(ids.end(), file_prefix[batch[k].idx].begin(), file_prefix[batch[k].idx].end());
                        offs.push_back(ids.size());
                    }
                    wh_prefix_opts po{sizeof(wh_prefix_opts), ids.data(), offs.data(), batch.size(), WH_PREFIX_FIRST_WINDOW};
                    if (int rc = wh_ctx_set_prefixes(ctx, &po)) throw std::runtime_error(std::string("wh_ctx_set_prefixes: ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                }
                const double t0 = now_s();
                wh_timing wt{};
                std::vector<float> lps, nss;
                std::vector<int> rung_of;
                std::vector<WindowScore> scores;
                std::vector<int32_t> frames;
                size_t row_cap = a.max_new_tokens;   // entries per file of lps and frames
                if (a.align()) {
                    // the batch is encoded as usual (one position decoded: the entry that leaves the encoder states resident), then aligned: the
                    // given ids take the place of the generated ones below
                    p.max_new_tokens = 1;
                    int rc = raw ? wh_transcribe_batch_raw_next(ctx, rclips.data(), rclips.size(), rnext.empty() ? nullptr : rnext.data(), rnext.size(), &p, toks.data(), ntok.data())
                                 : wh_transcribe_batch_next(ctx, clips.data(), clips.size(), nclips.empty() ? nullptr : nclips.data(), nclips.size(), &p, toks.data(), ntok.data());
                    if (rc) throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                    wh_get_timings(ctx, &wt);
                    std::vector<int64_t> ids;
                    std::vector<size_t> offs(1, 0);
                    row_cap = 1;
                    for (size_t k = 0; k < batch.size(); k++) {
                        const std::vector<int64_t>& t = file_align[batch[k].idx];
                        ids.insert(ids.end(), t.begin(), t.end());
                        offs.push_back(ids.size());
                        row_cap = std::max(row_cap, t.size());
                    }
                    wh_score_input in{sizeof(wh_score_input), ids.data(), offs.data(), batch.size(), 1};
                    wh_alignment_opts ao{sizeof(wh_alignment_opts), align_heads.data(), align_heads.size() / 2, nullptr, 0};
                    frames.assign(batch.size() * row_cap, 0);
                    lps.assign(batch.size() * row_cap, 0.0f);
                    if ((rc = wh_align_tokens(ctx, &p, &in, &ao, frames.data(), nullptr, lps.data(), row_cap)))
                        throw std::runtime_error(std::string("wh_align_tokens: ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                    wh_timing wa{};
                    wh_get_timings(ctx, &wa);
                    wt.decode_s += wa.decode_s;
                } else if (!a.ladder()) {
                    // the next batch of this worker, if it is loaded already, is copied to the device beside this batch's work
                    int rc = raw ? wh_transcribe_batch_raw_next(ctx, rclips.data(), rclips.size(), rnext.empty() ? nullptr : rnext.data(), rnext.size(), &p, toks.data(), ntok.data())
                                 : wh_transcribe_batch_next(ctx, clips.data(), clips.size(), nclips.empty() ? nullptr : nclips.data(), nclips.size(), &p, toks.data(), ntok.data());
                    if (rc) throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                    wh_get_timings(ctx, &wt);
                    if (a.logprobs) fetch_logprobs(ctx, batch.size(), a.max_new_tokens, lps, nss);
                } else {
                    // The temperature ladder over this device batch (wh_host.h run_ladder).  Rung 0 is the ordinary, unpipelined transcribe call
                    // (every temperature 0: the plain kernels); a later rung decodes the resident encoder states again with the failing rows
                    // sampled at its temperature and the others inactive, and replaces the failing rows' results only.  A row's random stream
                    // is named by its file's index, so a result does not depend on --max-batch.
                    const size_t n = batch.size();
                    lps.assign(n * a.max_new_tokens, 0.0f);
                    nss.assign(n, 0.0f);
                    run_ladder(n, a.temperature.size(), a.compression_ratio_threshold, a.logprob_threshold, a.no_speech_threshold,
                               [&](size_t rung, const std::vector<unsigned char>& active, std::vector<WindowScore>& sc) {
                                   std::vector<float> temps(n);
                                   std::vector<uint8_t> act(active.begin(), active.end());
                                   std::vector<uint64_t> ids(n);
                                   for (size_t k = 0; k < n; k++) { temps[k] = active[k] ? a.temperature[rung] : 0.0f; ids[k] = (uint64_t)batch[k].idx; }
                                   wh_sampling_opts so{sizeof(wh_sampling_opts), a.seed, temps.data(), act.data(), ids.data(), n};
                                   if (int rc = wh_ctx_set_sampling(ctx, &so)) throw std::runtime_error(std::string("wh_ctx_set_sampling: ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                                   std::vector<int64_t> toks2(n * stride);
                                   std::vector<size_t> ntok2(n);
                                   size_t got = 0;
                                   const int rc = rung == 0 ? (raw ? wh_transcribe_batch_raw(ctx, rclips.data(), n, &p, toks2.data(), ntok2.data())
                                                                   : wh_transcribe_batch(ctx, clips.data(), n, &p, toks2.data(), ntok2.data()))
                                                            : wh_decode_greedy_batch(ctx, &p, toks2.data(), stride, ntok2.data(), n, &got, nullptr, 0);
                                   if (rc) throw std::runtime_error(std::string("libwhisper_hip error ") + std::to_string(rc) + ": " + wh_last_error(ctx));
                                   if (rung == 0) wh_get_timings(ctx, &wt);
                                   std::vector<float> lps2, nss2;
                                   fetch_logprobs(ctx, n, a.max_new_tokens, lps2, nss2);
                                   for (size_t k = 0; k < n; k++) {
                                       if (!active[k]) continue;
                                       std::copy_n(toks2.begin() + k * stride, stride, toks.begin() + k * stride);
                                       ntok[k] = ntok2[k];
                                       std::copy_n(lps2.begin() + k * a.max_new_tokens, a.max_new_tokens, lps.begin() + k * a.max_new_tokens);
                                       nss[k] = nss2[k];
                                       std::vector<int64_t> g;
                                       if (ntok[k] > prompt.size()) g.assign(toks.begin() + k * stride + prompt.size(), toks.begin() + k * stride + ntok[k]);
                                       sc[k].avg_logprob = avg_logprob(std::vector<float>(lps.begin() + k * a.max_new_tokens, lps.begin() + k * a.max_new_tokens + g.size()), g, sp.eot);
                                       sc[k].no_speech_prob = nss[k];
                                       if (!g.empty() && g.back() == sp.eot) g.pop_back();
                                       if (a.timestamp_rules) g = text_ids(g, sp.timestamp_begin);
                                       sc[k].compression_ratio = compression_ratio(trim(decode_tokens(g, &tok)));
                                   }
                               },
                               rung_of, scores);
                    for (size_t k = 0; k < n; k++) {
                        Result& r = results[batch[k].idx];
                        r.has_ladder = true; r.temperature = a.temperature[rung_of[k]]; r.compression_ratio = scores[k].compression_ratio;
                    }
                }
                const double batch_s = now_s() - t0;
                std::vector<Lang> langs;
                if (lang_auto) langs = fetch_languages(ctx, batch.size(), lang_table);
                if (a.word_timestamps && !a.align()) fetch_frames(ctx, batch.size(), a.max_new_tokens, frames);
                if (a.beam()) {   // the n best hypotheses of every file of the batch
                    const std::vector<std::string> hy = fetch_hypotheses(ctx, batch.size(), a, sp, &tok, false);
                    for (size_t k = 0; k < batch.size(); k++) results[batch[k].idx].hyps = "[" + hy[k] + "]";
                }
                for (size_t k = 0; k < batch.size(); k++) {   // :926-943
                    Result& r = results[batch[k].idx];
                    if (lang_auto) r.lang = langs[k];
                    const double td0 = now_s();
                    std::vector<int64_t> g;
                    if (a.align()) {
                        g = file_align[batch[k].idx];
                        r.aligned = true;
                        r.aligned_avg_lp = avg_logprob(std::vector<float>(lps.begin() + k * row_cap, lps.begin() + k * row_cap + g.size()), g, sp.eot);
                    } else if (ntok[k] > prompt.size()) g.assign(toks.begin() + k * stride + prompt.size(), toks.begin() + k * stride + ntok[k]);
                    double avg_lp = 0;
                    const bool skip = !a.align() && a.logprobs && window_conf(a, g, lps.data() + k * a.max_new_tokens, nss[k], sp.eot, r.conf, avg_lp);
                    if (skip) g.clear();   // the silence rule: empty text, no segments
                    if (a.word_timestamps || a.align()) {
                        window_words(a, g, frames.data() + k * row_cap, sp, batch[k].dur, 0.0, &tok, r.words);
                        // a one-window file's text is trimmed: so are the ends of its words, which then concatenate to the text
                        if (!r.words.words.empty()) {
                            r.words.words.front().word = ltrim(r.words.words.front().word);
                            r.words.words.back().word = rtrim(r.words.words.back().word);
                        }
                    }
                    if (!g.empty() && g.back() == sp.eot) g.pop_back();
                    if (a.timestamp_rules) {
                        if (!skip) r.cues = to_cues(window_segments(g, sp, batch[k].dur), &tok);
                        if (a.logprobs) cues_conf(r.cues, avg_lp, nss[k]);
                        g = text_ids(g, sp.timestamp_begin);
                    }
                    std::string text = skip ? std::string() : decode_tokens(g, &tok);
                    if (text.empty()) text = "[EMPTY]";
                    std::vector<std::string> texts;
                    if (text != "[EMPTY]") texts.push_back(text);
                    r.text = stitch_texts(texts);
                    r.t.preprocess_s = wt.preprocess_s;
                    r.t.model_only_s = wt.encode_s + wt.decode_s;
                    r.t.decode_s = now_s() - td0;
                    r.t.end_to_end_s = batch_s + r.t.decode_s;   // every clip of a batch completes with its batch
                    r.dur = batch[k].dur; r.load_s = batch[k].load_s; r.ok = true;
                }
            }
            busy_s[wi] += now_s() - tb0;
        };
        // synthetic clips are one-window files by construction: allocate the page-locked staging pool now, outside the timed loop
        // (5.9 GB at --max-batch 1024; a directory of audio files allocates it when the first one-window file shows up)
        const size_t files_per_batch = (size_t)(a.max_batch / std::max(1, a.beam() ? a.beam_size : 1));   // beam search: a file takes beam_size rows
        if (a.synthetic_clips && !a.sequential) pool.ensure(file_pipeline_pool_size(files_per_batch, ctxs.size(), n_loaders));
        const double loop0 = now_s();
        // (--sequential: files of any length share a batch — to the pipeline every file is a "one-window" file — and stay in pageable memory: the
        // pool's buffers hold one 30 s window)
        const std::string first_error = run_file_pipeline(nfiles, n_loaders, ctxs.size(), files_per_batch, a.sequential ? (size_t)-1 : (size_t)WH_CLIP_SAMPLES,
                                                          a.sequential ? nullptr : &pool, load, process,
                                                          gpu_ingest ? std::function<void(size_t, PipeItem&)>(load_raw) : nullptr);
        const double loop_s = now_s() - loop0;
        if (!first_error.empty()) throw std::runtime_error(first_error);

        std::vector<RowOut> rows;
        std::vector<double> e2e, loadl, pre, model_only, dec, rtfl;
        const std::string txt_dir = parent_dir(a.out_csv);
        double audio_total = 0;
        for (size_t i = 0; i < nfiles; i++) {
            const Result& r = results[i];
            if (!r.ok) throw std::runtime_error("file " + files[i] + " was not processed");
            const double end_to_end = r.load_s + r.t.end_to_end_s;   // :1190
            rows.push_back(make_row(files[i], r.dur, end_to_end, r.text));
            if (a.timestamp_rules) rows.back().segments = cues_json(r.cues);
            if (a.word_timestamps || a.align()) { rows.back().words = words_json(r.words.words); rows.back().token_times = times_json(r.words.token_times); }
            if (r.aligned) { rows.back().aligned = true; rows.back().avg_logprob = r.aligned_avg_lp; }
            if (!r.hyps.empty()) rows.back().hypotheses = r.hyps;
            if (a.sequential) rows.back().windows = r.windows;
            if (a.prompts()) { rows.back().has_prompt = true; rows.back().prompt_tokens = (long long)file_prefix[i].size(); }
            if (r.lang.has) { rows.back().has_lang = true; rows.back().language = r.lang.code; rows.back().language_probability = r.lang.prob; }
            if (r.conf.has) { rows.back().has_conf = true; rows.back().avg_logprob = r.conf.avg_logprob(); rows.back().no_speech_prob = r.conf.no_speech_prob(); }
            if (r.has_ladder) { rows.back().has_ladder = true; rows.back().temperature = r.temperature; rows.back().compression_ratio = r.compression_ratio; }
            loadl.push_back(r.load_s); pre.push_back(r.t.preprocess_s); model_only.push_back(r.t.model_only_s);
            dec.push_back(r.t.decode_s); e2e.push_back(end_to_end); rtfl.push_back(end_to_end / std::max(r.dur, 1e-9));
            audio_total += r.dur;
            if (a.write_txt) {
                std::string base = files[i].substr(0, files[i].rfind('.'));
                write_file((txt_dir.empty() ? "." : txt_dir) + "/" + base + ".transcript.txt", trim(r.text) + "\n");
            }
            if (a.write_srt || a.write_vtt) {   // subtitle files into the directory --write-txt uses
                const std::string base = (txt_dir.empty() ? "." : txt_dir) + "/" + files[i].substr(0, files[i].rfind('.'));
                if (!parent_dir(base).empty()) mkdir_p(parent_dir(base));
                if (a.write_srt) write_file(base + ".srt", srt_text(r.cues));
                if (a.write_vtt) write_file(base + ".vtt", vtt_text(r.cues));
            }
        }
        const double busy_max = *std::max_element(busy_s.begin(), busy_s.end());
        write_file(a.out_csv, csv_text(rows));
        write_file(a.out_json, per_file_json(rows));
        std::vector<double> rtfx;
        for (double r : rtfl) rtfx.push_back(1.0 / std::max(r, 1e-12));
        SummaryIn si;   // :1235-1257: the reference's keys from wh_host.h reference_summary (pinned to the reference's archived summary)
        si.cfg = cfg; si.end2end = e2e; si.load = loadl; si.preprocess = pre; si.model_only = model_only; si.decode = dec; si.rtf = rtfl;
        si.n_files = rows.size(); si.model_id = a.model_id; si.onnx_dir = a.onnx_dir; si.language = a.language; si.task = a.task;
        si.tokenizer_json = tok.loaded ? tok.path : ""; si.max_new_tokens = (long long)a.max_new_tokens; si.timestamps = a.timestamps;
        JVal summary = reference_summary(si);   // + additive keys gpu, rtfx_end_to_end
        summary
            .set("rtfx_end_to_end", stat_json(stat_block(rtfx)))
            .set("gpu", JVal::obj().set("backend", JVal::str("libwhisper_hip (gfx950)")).set("device", JVal::integer(devices[0]))
                            .set("devices", JVal::integer((long long)devices.size())).set("streams_per_gpu", JVal::integer(a.streams_per_gpu))
                            .set("precision", JVal::str(a.precision)).set("max_batch", JVal::integer(a.max_batch))
                            .set("load_threads", JVal::integer(n_loaders)).set("audio_s", JVal::num(audio_total))
                            // whole-job throughput: audio seconds per wall second of the file loop (loading overlapped), and per
                            // second the busiest context spent inside the library (what bench.py measures with PCM resident)
                            .set("wall_s", JVal::num(loop_s)).set("throughput_rtfx", JVal::num(audio_total / std::max(loop_s, 1e-12)))
                            .set("gpu_busy_s", JVal::num(busy_max)).set("gpu_throughput_rtfx", JVal::num(audio_total / std::max(busy_max, 1e-12))));
        if (gpu_ingest) summary.set("gpu_ingest", JVal::boolean(true));
        if (a.sequential) summary.set("sequential", JVal::boolean(true)).set("condition_on_previous_text", JVal::boolean(a.condition_on_previous_text));
        if (a.timestamp_rules) summary.set("timestamp_rules", JVal::boolean(true));
        if (a.logprobs) summary.set("logprobs", JVal::boolean(true));
        if (a.have_rep_penalty) summary.set("repetition_penalty", JVal::num(a.rep_penalty));
        if (a.have_rep_ngram) summary.set("no_repeat_ngram_size", JVal::integer(a.rep_ngram));
        if (a.ladder()) {
            summary.set("seed", JVal::integer((long long)a.seed));
            if (!std::isnan(a.compression_ratio_threshold)) summary.set("compression_ratio_threshold", JVal::num(a.compression_ratio_threshold));
        }
        if (a.beam()) summary.set("patience", JVal::num(a.patience)).set("length_penalty", JVal::num(a.length_penalty)).set("n_best", JVal::integer(a.n_best));
        write_file(a.out_summary_json, summary.pretty());
        printf("DONE\n");  // :1261-1268
        printf("Config used:\n%s\n", cfg.json(false).pretty().c_str());
        printf("Per-file CSV: %s\n", a.out_csv.c_str());
        printf("Per-file JSON: %s\n", a.out_json.c_str());
        printf("Summary JSON: %s\n", a.out_summary_json.c_str());
        double p95 = stat_block(e2e).p95;
        if (std::isfinite(p95)) printf("End-to-end p95(s): %.6f\n", p95);
        for (wh_ctx* c : ctxs) wh_ctx_free(c);
        for (wh_model* m : models) wh_model_free(m);
    } catch (const std::exception& e) {
        fprintf(stderr, "Error: %s\n", e.what());
        return 1;
    }
    return 0;
}
