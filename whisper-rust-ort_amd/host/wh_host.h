// wh_host.h — host-side pieces of the reference's binary that sit either side of the hot path,
// restated in C++ (Rust is not available in this image): statistics + emitters byte-compatible with
// serde_json / the csv crate, WAV reader + linear resampler, prompt ids, token → text fallback and
// byte-level BPE decode, long-form stitcher.  Citations: /root/reference/src/main.rs.
#pragma once
#include <dlfcn.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../csrc/wh_json.h"
#include "wh_unicode_lower.h"

namespace whhost {

// ---------------------------------------------------------------------------------------------
// f64 → text exactly as serde_json (ryu `format_finite`): shortest round-trip digits, decimal
// notation while -5 < kk <= 16 else d.ddde±x; integers keep a trailing ".0"; NaN/inf → null.
// ---------------------------------------------------------------------------------------------
inline std::string fmt_f64(double v) {
    if (!std::isfinite(v)) return "null";
    if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
    char buf[64];
    int prec = 1;
    for (; prec <= 17; prec++) {
        snprintf(buf, sizeof buf, "%.*e", prec - 1, v);
        if (strtod(buf, nullptr) == v) break;
    }
    // buf = [-]d[.ddd]e±XX
    std::string s(buf);
    bool neg = s[0] == '-';
    if (neg) s.erase(0, 1);
    size_t epos = s.find('e');
    int exp10 = atoi(s.c_str() + epos + 1);
    std::string digits = s.substr(0, epos);
    digits.erase(std::remove(digits.begin(), digits.end(), '.'), digits.end());
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const int len = (int)digits.size();
    const int kk = exp10 + 1;  // 10^(kk-1) <= v < 10^kk
    const int k = kk - len;
    std::string out;
    if (0 <= k && kk <= 16) {  // 1234e7 -> 12340000000.0
        out = digits + std::string((size_t)k, '0') + ".0";
    } else if (0 < kk && kk <= 16) {  // 1234e-2 -> 12.34
        out = digits.substr(0, (size_t)kk) + "." + digits.substr((size_t)kk);
    } else if (-5 < kk && kk <= 0) {  // 1234e-6 -> 0.001234
        out = "0." + std::string((size_t)(-kk), '0') + digits;
    } else if (len == 1) {  // 1e30
        out = digits + "e" + std::to_string(kk - 1);
    } else {  // 1234e30 -> 1.234e33
        out = digits.substr(0, 1) + "." + digits.substr(1) + "e" + std::to_string(kk - 1);
    }
    return neg ? "-" + out : out;
}

inline std::string json_escape(const std::string& s) {  // serde_json string escaping
    std::string o = "\"";
    for (unsigned char c : s) {
        switch (c) {
            case '"': o += "\\\""; break;
            case '\\': o += "\\\\"; break;
            case '\n': o += "\\n"; break;
            case '\r': o += "\\r"; break;
            case '\t': o += "\\t"; break;
            case '\b': o += "\\b"; break;
            case '\f': o += "\\f"; break;
            default:
                if (c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
                else o += (char)c;
        }
    }
    return o + "\"";
}

// ---------------------------------------------------------------------------------------------
// statistics — src/main.rs:1021-1048
// ---------------------------------------------------------------------------------------------
inline double percentile(std::vector<double> xs, double p) {  // :1021-1031
    if (xs.empty()) return NAN;
    std::sort(xs.begin(), xs.end());
    double k = ((double)xs.size() - 1.0) * (p / 100.0);
    size_t f = (size_t)std::floor(k), c = (size_t)std::ceil(k);
    if (f == c) return xs[f];
    return xs[f] + (xs[c] - xs[f]) * (k - (double)f);
}

struct StatBlock { double min, median, p90, p95, max, mean; };

inline StatBlock stat_block(const std::vector<double>& xs) {  // :1033-1048 (median = v[len/2])
    std::vector<double> v = xs;
    std::sort(v.begin(), v.end());
    StatBlock s;
    s.min = v.empty() ? NAN : v.front();
    s.max = v.empty() ? NAN : v.back();
    double sum = 0;
    for (double x : v) sum += x;
    s.mean = v.empty() ? NAN : sum / (double)v.size();
    s.median = v.empty() ? NAN : v[v.size() / 2];
    s.p90 = percentile(xs, 90.0);
    s.p95 = percentile(xs, 95.0);
    return s;
}

// A tiny ordered-or-sorted JSON writer: serde_json::json! maps serialise with keys in ALPHABETICAL
// order (no preserve_order feature), derived structs in declaration order.
struct JVal {
    enum Kind { Raw, Obj } kind = Raw;
    std::string raw;                                   // already-encoded scalar
    std::vector<std::pair<std::string, JVal>> fields;  // object
    bool sorted = true;
    static JVal num(double v) { JVal j; j.raw = fmt_f64(v); return j; }
    static JVal integer(long long v) { JVal j; j.raw = std::to_string(v); return j; }
    static JVal boolean(bool b) { JVal j; j.raw = b ? "true" : "false"; return j; }
    static JVal str(const std::string& s) { JVal j; j.raw = json_escape(s); return j; }
    static JVal obj(bool sorted_keys = true) { JVal j; j.kind = Obj; j.sorted = sorted_keys; return j; }
    JVal& set(const std::string& k, JVal v) { fields.emplace_back(k, std::move(v)); return *this; }
    void write(std::string& out, int indent) const {  // serde_json PrettyFormatter, 2 spaces
        if (kind == Raw) { out += raw; return; }
        if (fields.empty()) { out += "{}"; return; }
        std::vector<const std::pair<std::string, JVal>*> order;
        for (auto& f : fields) order.push_back(&f);
        if (sorted) std::stable_sort(order.begin(), order.end(), [](auto a, auto b) { return a->first < b->first; });
        out += "{\n";
        for (size_t i = 0; i < order.size(); i++) {
            out += std::string((size_t)(indent + 2), ' ') + json_escape(order[i]->first) + ": ";
            order[i]->second.write(out, indent + 2);
            out += (i + 1 < order.size()) ? ",\n" : "\n";
        }
        out += std::string((size_t)indent, ' ') + "}";
    }
    std::string pretty() const { std::string o; write(o, 0); return o; }
};

inline JVal stat_json(const StatBlock& s) {
    return JVal::obj().set("min", JVal::num(s.min)).set("median", JVal::num(s.median)).set("p90", JVal::num(s.p90))
        .set("p95", JVal::num(s.p95)).set("max", JVal::num(s.max)).set("mean", JVal::num(s.mean));
}

// ---------------------------------------------------------------------------------------------
// rows + emitters — src/main.rs:1053-1060, 1193-1199, 1215-1232
// ---------------------------------------------------------------------------------------------
struct RowOut {
    std::string file; double duration_s, end_to_end_s, rtf; std::string text;
    std::string segments;   // JSON array of {start, end, text} (--timestamp-rules), empty: no key
    std::string words, token_times;   // --word-timestamps: JSON arrays of {word, start, end} and of the generated tokens' times; empty: no key
    bool has_conf = false;  // --logprobs: avg_logprob and no_speech_prob keys
    double avg_logprob = 0, no_speech_prob = 0;
    bool has_lang = false;  // --language auto: the detected language code and its probability
    std::string language;
    double language_probability = 0;
    std::string hypotheses;   // --beam-size N >= 2: JSON array of the n best {text, sum_logprob, rank_score, finished}; empty: no key
    bool has_ladder = false;  // --temperature with a ladder other than the single rung 0: the rung that produced the row and its compression ratio
    double temperature = 0, compression_ratio = 0;
    bool has_prompt = false;  // --prompt-ids / --prompt-ids-dir: the length of the file's text context (<|startofprev|> included; 0: none)
    long long prompt_tokens = 0;
    bool aligned = false;     // --align-ids-dir: the row's text is the given transcript, aligned; avg_logprob (above) is the transcript's own
    std::string windows;      // --sequential: JSON array of the file's windows {seek_s, frames, advance_s, skipped, temperature, tokens}; empty: no key
};

// avg_logprob / no_speech_prob in JSON: shortest text that reads back as the same float (the library's values are floats); a window in which
// nothing was allowed has avg_logprob -inf, which JSON cannot hold: null
inline std::string fmt_conf(double v) {
    if (!std::isfinite(v)) return "null";
    char b[48];
    snprintf(b, sizeof b, "%.9g", v);
    return b;
}

// a float as the shortest decimal text that reads back as the same float (0.2f -> "0.2")
inline std::string fmt_f32(float v) {
    if (!std::isfinite(v)) return "null";
    char b[48];
    for (int p = 1; p <= 9; p++) {
        snprintf(b, sizeof b, "%.*g", p, (double)v);
        if (strtof(b, nullptr) == v) break;
    }
    return b;
}

inline double round_to(double v, double scale) { return std::round(v * scale) / scale; }  // f64::round: half away from zero

inline RowOut make_row(const std::string& file, double dur, double e2e, const std::string& text) {  // :1190-1199
    RowOut r;
    r.file = file;
    double rtf = e2e / std::max(dur, 1e-9);
    r.duration_s = round_to(dur, 1000.0);
    r.end_to_end_s = round_to(e2e, 10000.0);
    r.rtf = round_to(rtf, 1000000.0);
    r.text = text;
    return r;
}

inline std::string csv_field(const std::string& f) {  // csv crate, QuoteStyle::Necessary
    bool q = f.empty() ? false : false;
    for (char c : f)
        if (c == '"' || c == ',' || c == '\n' || c == '\r') { q = true; break; }
    if (!q) return f;
    std::string o = "\"";
    for (char c : f) { if (c == '"') o += '"'; o += c; }
    return o + "\"";
}

inline std::string csv_text(const std::vector<RowOut>& rows) {  // :1215-1229
    bool lang = false;   // --language auto: two more columns (any other run: the reference's five)
    for (auto& r : rows) lang = lang || r.has_lang;
    std::string o = lang ? "file,duration_s,end_to_end_s,rtf,text,language,language_probability\n" : "file,duration_s,end_to_end_s,rtf,text\n";
    char b[64];
    for (auto& r : rows) {
        o += csv_field(r.file) + ",";
        snprintf(b, sizeof b, "%.3f", r.duration_s); o += b; o += ",";
        snprintf(b, sizeof b, "%.4f", r.end_to_end_s); o += b; o += ",";
        snprintf(b, sizeof b, "%.6f", r.rtf); o += b; o += ",";
        o += csv_field(r.text);
        if (lang) { o += "," + csv_field(r.language) + "," + fmt_conf(r.language_probability); }
        o += "\n";
    }
    return o;
}

inline std::string per_file_json(const std::vector<RowOut>& rows) {  // :1232 to_string_pretty(&rows)
    if (rows.empty()) return "[]";
    std::string o = "[\n";
    for (size_t i = 0; i < rows.size(); i++) {
        JVal r = JVal::obj(false);  // derived struct: declaration order
        r.set("file", JVal::str(rows[i].file)).set("duration_s", JVal::num(rows[i].duration_s))
            .set("end_to_end_s", JVal::num(rows[i].end_to_end_s)).set("rtf", JVal::num(rows[i].rtf))
            .set("text", JVal::str(rows[i].text));
        if (rows[i].has_lang) { JVal v; v.raw = fmt_conf(rows[i].language_probability); r.set("language", JVal::str(rows[i].language)).set("language_probability", v); }
        if (rows[i].has_prompt) r.set("prompt_tokens", JVal::integer(rows[i].prompt_tokens));
        if (rows[i].has_conf) { JVal v; v.raw = fmt_conf(rows[i].avg_logprob); r.set("avg_logprob", v); v.raw = fmt_conf(rows[i].no_speech_prob); r.set("no_speech_prob", v); }
        if (rows[i].aligned) { JVal v; v.raw = fmt_conf(rows[i].avg_logprob); r.set("avg_logprob", v).set("aligned", JVal::boolean(true)); }
        if (rows[i].has_ladder) { JVal v; v.raw = fmt_f32((float)rows[i].temperature); r.set("temperature", v); v.raw = fmt_conf(rows[i].compression_ratio); r.set("compression_ratio", v); }
        if (!rows[i].windows.empty()) { JVal w; w.raw = rows[i].windows; r.set("windows", w); }
        if (!rows[i].segments.empty()) { JVal sg; sg.raw = rows[i].segments; r.set("segments", sg); }
        if (!rows[i].hypotheses.empty()) { JVal h; h.raw = rows[i].hypotheses; r.set("hypotheses", h); }
        if (!rows[i].words.empty()) { JVal w; w.raw = rows[i].words; r.set("words", w); w.raw = rows[i].token_times; r.set("token_times", w); }
        o += "  ";
        r.write(o, 2);
        o += (i + 1 < rows.size()) ? ",\n" : "\n";
    }
    return o + "]";
}

struct OrtCfg {  // :91-100 — CPU-EP knobs: accepted and echoed only, they have no GPU analogue
    long long intra_op = 1, inter_op = 1;
    std::string execution_mode = "SEQUENTIAL", graph_opt = "ENABLE_ALL";
    bool cpu_mem_arena = true, mem_pattern = true, allow_spinning = true;
    long long beam_size = 1;   // additive (no reference counterpart: the reference is greedy): echoed only when >= 2, so a greedy run's config_used keeps the reference's keys
    std::vector<float> temperature;   // additive: the temperature ladder, echoed only when it is not the single rung 0 (left empty then)
    JVal json(bool sorted) const {
        JVal j = JVal::obj(sorted);
        j.set("intra_op", JVal::integer(intra_op)).set("inter_op", JVal::integer(inter_op))
            .set("execution_mode", JVal::str(execution_mode)).set("graph_opt", JVal::str(graph_opt))
            .set("cpu_mem_arena", JVal::boolean(cpu_mem_arena)).set("mem_pattern", JVal::boolean(mem_pattern))
            .set("allow_spinning", JVal::boolean(allow_spinning));
        if (beam_size >= 2) j.set("beam_size", JVal::integer(beam_size));
        if (!temperature.empty()) {
            JVal t;
            t.raw = "[";
            for (size_t i = 0; i < temperature.size(); i++) t.raw += (i ? ", " : "") + fmt_f32(temperature[i]);
            t.raw += "]";
            j.set("temperature", t);
        }
        return j;
    }
};

// The summary object of src/main.rs:1235-1257, from the per-file lists of :1200-1205 — exactly the reference's keys (the
// CLI appends its additive gpu{} / rtfx_end_to_end{} keys afterwards).  tests/test_host_cpu.py rebuilds the reference's own
// archived inference_summary.json from its values through this function and requires the bytes to match.
struct SummaryIn {
    OrtCfg cfg;
    std::vector<double> end2end, load, preprocess, model_only, decode, rtf;
    size_t n_files = 0;
    std::string model_id, onnx_dir, language, task, tokenizer_json;   // tokenizer_json: "" when none was loaded (:1250)
    long long max_new_tokens = 128;
    bool timestamps = false;
};
inline JVal reference_summary(const SummaryIn& in) {
    JVal summary = JVal::obj();
    summary.set("config_used", in.cfg.json(true)).set("n_files", JVal::integer((long long)in.n_files))
        .set("latency_end_to_end_s", stat_json(stat_block(in.end2end)))
        .set("breakdown_s", JVal::obj().set("load_s", stat_json(stat_block(in.load))).set("preprocess_s", stat_json(stat_block(in.preprocess)))
                                .set("model_only_s", stat_json(stat_block(in.model_only))).set("decode_s", stat_json(stat_block(in.decode))))
        .set("rtf_end_to_end", stat_json(stat_block(in.rtf))).set("model_id", JVal::str(in.model_id)).set("onnx_dir", JVal::str(in.onnx_dir))
        .set("language", JVal::str(in.language)).set("task", JVal::str(in.task)).set("max_new_tokens", JVal::integer(in.max_new_tokens))
        .set("tokenizer_json", JVal::str(in.tokenizer_json)).set("timestamps", JVal::boolean(in.timestamps))
        .set("notes", JVal::obj().set("longform", JVal::str("Rust approximation: chunked 30s windows with overlap; greedy decode via decoder_with_past"))
                          .set("token_decode", JVal::str(!in.tokenizer_json.empty() ? "Tokenizer decode (skip_special_tokens=true)" : "Prints token IDs unless you provide tokenizer.json.")));
    return summary;
}

// ---------------------------------------------------------------------------------------------
// audio — src/main.rs:207-316 (WAV container only; FLAC/MP3 are out of scope here)
// ---------------------------------------------------------------------------------------------
inline std::vector<float> resample_linear(const std::vector<float>& x, uint32_t sr_in, uint32_t sr_out) {  // :207-226
    if (sr_in == sr_out) return x;
    double ratio = (double)sr_out / (double)sr_in;
    size_t n_out = (size_t)std::llround((double)x.size() * ratio);
    std::vector<float> y;
    y.reserve(n_out);
    for (size_t i = 0; i < n_out; i++) {
        double t = (double)i / ratio;
        long long i0 = (long long)std::floor(t), i1 = i0 + 1;
        double a = t - (double)i0;
        float s0 = (i0 < 0 || (size_t)i0 >= x.size()) ? 0.0f : x[(size_t)i0];
        float s1 = (i1 < 0 || (size_t)i1 >= x.size()) ? 0.0f : x[(size_t)i1];
        y.push_back((float)(1.0 - a) * s0 + (float)a * s1);
    }
    return y;
}

// The RIFF walk of the loader: the whole file in `d`, the fmt chunk's fields and the data chunk's place in it.
struct WavLayout {
    uint32_t fmt = 0, ch = 0, sr = 0, bits = 0;
    size_t data_off = 0, data_len = 0;
};
inline WavLayout read_wav_layout(const std::string& path, std::vector<unsigned char>& d) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) throw std::runtime_error("Failed to open audio: " + path);
    unsigned char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    auto u16 = [&](size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); };
    auto u32 = [&](size_t o) { return u16(o) | (u16(o + 2) << 16); };
    if (d.size() < 12 || memcmp(d.data(), "RIFF", 4) || memcmp(d.data() + 8, "WAVE", 4))
        throw std::runtime_error("Unsupported container (only RIFF/WAVE is decoded here): " + path);
    WavLayout w;
    size_t p = 12;
    while (p + 8 <= d.size()) {
        uint32_t len = u32(p + 4);
        if (!memcmp(d.data() + p, "fmt ", 4) && p + 8 + 16 <= d.size()) {
            w.fmt = u16(p + 8); w.ch = u16(p + 10); w.sr = u32(p + 12); w.bits = u16(p + 22);
            if (w.fmt == 0xFFFE && len >= 26) w.fmt = u16(p + 8 + 24);  // WAVE_FORMAT_EXTENSIBLE sub-format
        } else if (!memcmp(d.data() + p, "data", 4)) {
            w.data_off = p + 8;
            w.data_len = std::min<size_t>(len, d.size() - w.data_off);
            break;
        }
        p += 8 + len + (len & 1);
    }
    if (!w.sr) throw std::runtime_error("Unknown sample rate");
    if (!w.ch) throw std::runtime_error("Unknown channels");
    return w;
}

// The file's samples as it holds them (whisper_bench --gpu-ingest, wh_transcribe_batch_raw*): the same walk, the same refusals with the same
// texts as load_audio_16k_mono, and no conversion.  `format` is the C ABI's WH_PCM_* (S16 0, U8 1, F32 2).
struct RawWav {
    std::vector<unsigned char> file;   // the whole file; the payload is file[data_off .. data_off + n_bytes)
    size_t data_off = 0, n_bytes = 0, n_frames = 0;
    uint32_t sample_rate = 0, channels = 0;
    int format = -1;
    const unsigned char* payload() const { return file.data() + data_off; }
};
inline RawWav read_wav_raw(const std::string& path) {
    RawWav r;
    const WavLayout w = read_wav_layout(path, r.file);
    const size_t bps = w.bits / 8;
    r.n_frames = bps ? w.data_len / (bps * w.ch) : 0;
    if (w.fmt == 1 && w.bits == 8) r.format = 1;
    else if (w.fmt == 1 && w.bits == 16) r.format = 0;
    else if (w.fmt == 3 && w.bits == 32) r.format = 2;
    else if (r.n_frames) throw std::runtime_error("Unsupported decoded sample format");  // :303 (the loader meets it at the first sample)
    r.data_off = w.data_off;
    r.n_bytes = r.n_frames * bps * w.ch;
    r.sample_rate = w.sr;
    r.channels = w.ch;
    return r;
}

// Decodes PCM WAV (U8 / S16 / IEEE F32), channel-mean downmix (:266-302), resample to 16 kHz.
inline void load_audio_16k_mono(const std::string& path, std::vector<float>& out, double* dur_s) {
    std::vector<unsigned char> d;
    const WavLayout w = read_wav_layout(path, d);
    auto u16 = [&](size_t o) { return (uint32_t)d[o] | ((uint32_t)d[o + 1] << 8); };
    auto u32 = [&](size_t o) { return u16(o) | (u16(o + 2) << 16); };
    const uint32_t fmt = w.fmt, ch = w.ch, sr = w.sr, bits = w.bits;
    const size_t data_off = w.data_off, data_len = w.data_len;
    std::vector<float> s;
    const size_t bps = bits / 8, frames = (bps && ch) ? data_len / (bps * ch) : 0;
    s.reserve(frames);
    for (size_t i = 0; i < frames; i++) {
        float acc = 0.0f;
        for (uint32_t c = 0; c < ch; c++) {
            size_t o = data_off + (i * ch + c) * bps;
            if (fmt == 1 && bits == 8) acc += ((float)d[o] - 128.0f) / 128.0f;
            else if (fmt == 1 && bits == 16) acc += (float)(int16_t)u16(o) / 32768.0f;
            else if (fmt == 3 && bits == 32) { uint32_t u = u32(o); float v; memcpy(&v, &u, 4); acc += v; }
            else throw std::runtime_error("Unsupported decoded sample format");  // :303
        }
        s.push_back(acc / (float)ch);
    }
    if (sr != 16000) s = resample_linear(s, sr, 16000);
    *dur_s = (double)s.size() / 16000.0;
    out.swap(s);
}

// ---------------------------------------------------------------------------------------------
// tokens — src/main.rs:518-569, 637-657
// ---------------------------------------------------------------------------------------------
struct Tokenizer {
    std::map<std::string, int64_t> special;        // added token content → id
    std::vector<std::string> id_to_tok;            // vocab
    std::vector<bool> is_special;
    bool loaded = false;
    std::string path;
};

inline bool load_tokenizer(const std::string& path, Tokenizer& t) {
    FILE* f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string txt;
    char buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) txt.append(buf, n);
    fclose(f);
    std::string err;
    auto j = whjson::parse(txt, &err);
    if (!j) throw std::runtime_error("Failed to load tokenizer " + path + ": " + err);
    auto grow = [&](size_t id) { if (t.id_to_tok.size() <= id) { t.id_to_tok.resize(id + 1); t.is_special.resize(id + 1, false); } };
    if (auto m = j->get("model"))
        if (auto v = m->get("vocab"))
            for (auto& kv : v->obj) { size_t id = (size_t)kv.second->as_i64(); grow(id); t.id_to_tok[id] = kv.first; }
    if (auto a = j->get("added_tokens"))
        for (auto& e : a->arr) {
            auto c = e->get("content"); auto i = e->get("id"); auto sp = e->get("special");
            if (!c || !i) continue;
            size_t id = (size_t)i->as_i64();
            grow(id);
            t.id_to_tok[id] = c->str;
            t.is_special[id] = sp ? sp->b : true;
            t.special[c->str] = (int64_t)id;
        }
    t.loaded = true;
    t.path = path;
    return true;
}

struct WhisperSpecial { int64_t sot, eot, lang, task, no_timestamps, timestamp_begin, no_speech, sot_prev; };

inline WhisperSpecial special_tokens(const std::string& language, const std::string& task, const Tokenizer* tok) {
    if (tok && tok->loaded) {  // :529-541
        auto get = [&](const std::string& s) {
            auto it = tok->special.find(s);
            if (it == tok->special.end()) throw std::runtime_error("Tokenizer missing token: " + s);
            return it->second;
        };
        // (--language auto: the language slot of the prompt is a placeholder the library overwrites per clip)
        WhisperSpecial s{get("<|startoftranscript|>"), get("<|endoftext|>"), get("<|" + (language == "auto" ? std::string("en") : language) + "|>"), get("<|" + task + "|>"),
                         get("<|notimestamps|>"), 0, 0};
        auto ts = tok->special.find("<|0.00|>");   // <|0.00|> if the tokenizer lists it, else the id after <|notimestamps|>
        s.timestamp_begin = ts != tok->special.end() ? ts->second : s.no_timestamps + 1;
        s.no_speech = s.no_timestamps - 1;   // <|nospeech|> (<|nocaptions|> in the older vocabularies) if the tokenizer lists it, else the id before <|notimestamps|>
        for (const char* name : {"<|nospeech|>", "<|nocaptions|>"}) {
            auto ns = tok->special.find(name);
            if (ns != tok->special.end()) { s.no_speech = ns->second; break; }
        }
        auto sp = tok->special.find("<|startofprev|>");   // text context (--prompt-ids): <|startofprev|> if the tokenizer lists it, else the multilingual id
        s.sot_prev = sp != tok->special.end() ? sp->second : 50361;
        return s;
    }
    WhisperSpecial s;  // :549-566 hard-coded multilingual ids
    s.sot = 50258; s.eot = 50257;
    s.lang = language == "en" ? 50259 : language == "hi" ? 50276 : 50259;
    s.task = task == "transcribe" ? 50359 : task == "translate" ? 50358 : 50359;
    s.no_timestamps = 50363;
    s.timestamp_begin = 50364;
    s.no_speech = s.no_timestamps - 1;   // 50362
    s.sot_prev = 50361;
    return s;
}

// ---- text context (--prompt-ids; wh_ctx_set_prefixes) ----------------------------------------------------------------------------------
// openai-whisper's rule (decoding.py _get_initial_tokens): [<|startofprev|>] ++ the last n_text_ctx / 2 - 1 ids of the history; no history,
// no prefix.
inline std::vector<int64_t> build_prev_prefix(const std::vector<int64_t>& history, int64_t sot_prev, int n_text_ctx) {
    std::vector<int64_t> out;
    if (history.empty()) return out;
    const size_t keep = std::min(history.size(), (size_t)std::max(n_text_ctx / 2 - 1, 0));
    out.push_back(sot_prev);
    out.insert(out.end(), history.end() - (long)keep, history.end());
    return out;
}

// ---- --language auto: the ids language detection chooses among (wh_ctx_set_language_detection) ----------------------------------------
// Whisper's language codes in the order of their tokens (openai-whisper tokenizer.py LANGUAGES): <|en|> is the id after
// <|startoftranscript|>, the others follow; the 100th (yue) exists in the 51866-id vocabulary of large-v3 only.
inline const std::vector<std::string>& whisper_language_codes() {
    static const std::vector<std::string> codes = {
        "en", "zh", "de", "es", "ru", "ko", "fr", "ja", "pt", "tr", "pl", "ca", "nl", "ar", "sv", "it", "id", "hi", "fi", "vi",
        "he", "uk", "el", "ms", "cs", "ro", "da", "hu", "ta", "no", "th", "ur", "hr", "bg", "lt", "la", "mi", "ml", "cy", "sk",
        "te", "fa", "lv", "bn", "sr", "az", "sl", "kn", "et", "mk", "br", "eu", "is", "hy", "ne", "mn", "bs", "kk", "sq", "sw",
        "gl", "mr", "pa", "si", "km", "sn", "yo", "so", "af", "oc", "ka", "be", "tg", "sd", "gu", "am", "yi", "lo", "uz", "fo",
        "ht", "ps", "tk", "nn", "mt", "sa", "lb", "my", "bo", "tl", "mg", "as", "tt", "haw", "ln", "ha", "ba", "jw", "su", "yue"};
    return codes;
}
struct LanguageTable {
    std::vector<std::string> codes;
    std::vector<int64_t> ids;
};
// With a tokenizer: its <|xx|> tokens of the codes above, in that order.  Without: the multilingual block starting at 50259 — 99 codes, 100
// when the vocabulary has 51866 ids; a vocabulary too small to hold that block is refused.
inline LanguageTable language_table(const Tokenizer* tok, long long vocab) {
    LanguageTable t;
    const std::vector<std::string>& all = whisper_language_codes();
    if (tok && tok->loaded) {
        for (const std::string& c : all) {
            auto it = tok->special.find("<|" + c + "|>");
            if (it != tok->special.end() && it->second < vocab) { t.codes.push_back(c); t.ids.push_back(it->second); }
        }
        if (t.ids.empty()) throw std::runtime_error("--language auto: the tokenizer lists no <|xx|> language token");
        return t;
    }
    const size_t n = vocab == 51866 ? 100 : 99;
    if (vocab < 50259 + (long long)n)
        throw std::runtime_error("--language auto needs a tokenizer.json or a multilingual vocabulary: the language tokens are ids 50259.." + std::to_string(50259 + n - 1) +
                                 ", this model's vocabulary has " + std::to_string(vocab) + " ids");
    for (size_t i = 0; i < n; i++) { t.codes.push_back(all[i]); t.ids.push_back(50259 + (int64_t)i); }
    return t;
}

// ---- the CLI's --synthetic-clips input ------------------------------------------------------------------------------------------------
// deterministic in-memory clip (SURVEY §8d config 3 shape): three enveloped sinusoids (80-4000 Hz) + noise of standard
// deviation 0.02, clipped to [-1, 1].  Built for speed, because the loader threads have to keep a GPU fed that transcribes
// ~900 clips per second: oscillators and the 4 Hz raised-cosine envelope advance by complex rotation in float (re-seeded
// from sin/cos every 1024 samples so the recurrence cannot drift), the noise is a 4-term Irwin-Hall sum (four 16-bit
// uniforms from one splitmix64 draw, variance-matched to N(0,1)): ~3 ms per 30 s clip on one host core.
inline std::vector<float> synthetic_clip(uint64_t seed) {
    uint64_t st = seed * 0x9E3779B97F4A7C15ull + 1;
    auto next64 = [&]() { st += 0x9E3779B97F4A7C15ull; uint64_t z = st; z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 27; z *= 0x94D049BB133111EBull; z ^= z >> 31; return z; };
    auto u01 = [&]() { return (double)(next64() >> 11) / 9007199254740992.0; };
    double fr[4], ph[4];
    for (int j = 0; j < 3; j++) { fr[j] = 80.0 + 3920.0 * u01(); ph[j] = 2 * M_PI * u01(); }
    fr[3] = 4.0; ph[3] = 0.0;   // envelope 0.5 - 0.5 cos(2 pi 4 t)
    std::vector<float> x(480000);   // one 30 s window
    float re[4], im[4], cr[4], ci[4];
    for (int j = 0; j < 4; j++) { const double w = 2 * M_PI * fr[j] / 16000.0; cr[j] = (float)cos(w); ci[j] = (float)sin(w); }
    const float nscale = 0.02f * 1.7320508f / 32768.0f;   // sum of 4 U(-1/2,1/2) has variance 1/3
    for (size_t i = 0; i < x.size(); i++) {
        if ((i & 1023) == 0)
            for (int j = 0; j < 4; j++) { const double a = 2 * M_PI * fr[j] * ((double)i / 16000.0) + ph[j]; re[j] = (float)cos(a); im[j] = (float)sin(a); }
        const float s = im[0] + im[1] + im[2], env = 0.5f - 0.5f * re[3];
        const uint64_t r = next64();
        const int sum4 = (int)(r & 0xFFFF) + (int)((r >> 16) & 0xFFFF) + (int)((r >> 32) & 0xFFFF) + (int)(r >> 48) - 2 * 65535;
        const float v = 0.25f * s * env + nscale * (float)sum4 * 0.5f;
        x[i] = std::max(-1.0f, std::min(1.0f, v));
        for (int j = 0; j < 4; j++) { const float nr = re[j] * cr[j] - im[j] * ci[j]; im[j] = re[j] * ci[j] + im[j] * cr[j]; re[j] = nr; }
    }
    return x;
}

// ---- timestamped segments (Whisper's timestamp tokens, openai-whisper's slicing rule) ---------------------------------------------------
struct Segment {
    double start = 0, end = 0;
    std::vector<int64_t> tokens;   // the text ids (no timestamp) of the segment
    bool has_conf = false;         // avg_logprob / no_speech_prob supplied: its window's values (openai-whisper puts them on every segment of a window)
    double avg_logprob = 0, no_speech_prob = 0;
};
// openai-whisper's sum_logprobs / (len(tokens) + 1) of one window: the sum runs over the generated tokens' log-probabilities up to and
// including the first EOT, the length counts the tokens before it (a window cut at max_new_tokens has no EOT: every token counts)
inline double avg_logprob(const std::vector<float>& logprobs, const std::vector<int64_t>& tokens, int64_t eot) {
    double s = 0;
    size_t n = 0;
    for (size_t i = 0; i < logprobs.size() && i < tokens.size(); i++) {
        s += (double)logprobs[i];
        if (tokens[i] == eot) break;
        n++;
    }
    return s / (double)(n + 1);
}
// openai-whisper's silence rule for one window: skipped (empty text, no segments) when no_speech_prob > no_speech_threshold and avg_logprob <
// logprob_threshold.  A NaN threshold is off: without a no-speech threshold nothing is skipped, without a log-probability threshold the
// no-speech test decides alone.  openai's defaults are 0.6 and -1.0.
inline bool skip_window(double no_speech_prob, double avg_lp, double no_speech_threshold, double logprob_threshold) {
    if (std::isnan(no_speech_threshold) || !(no_speech_prob > no_speech_threshold)) return false;
    return std::isnan(logprob_threshold) || avg_lp < logprob_threshold;
}
// ---- the temperature ladder (openai-whisper's decode_with_fallback; --temperature) ----------------------------------------------------------
// zlib, loaded by its soname at the first use (the development symlink libz.so is not needed): compress2, compressBound, zlibVersion
struct Zlib {
    typedef int (*compress2_t)(unsigned char*, unsigned long*, const unsigned char*, unsigned long, int);
    typedef unsigned long (*bound_t)(unsigned long);
    typedef const char* (*version_t)();
    compress2_t compress2 = nullptr;
    bound_t bound = nullptr;
    version_t version = nullptr;
    static const Zlib& get() {
        static const Zlib z = [] {
            Zlib r;
            void* h = dlopen("libz.so.1", RTLD_NOW | RTLD_GLOBAL);
            if (!h) throw std::runtime_error(std::string("compression_ratio needs zlib: dlopen(\"libz.so.1\") failed: ") + dlerror());
            r.compress2 = (compress2_t)dlsym(h, "compress2");
            r.bound = (bound_t)dlsym(h, "compressBound");
            r.version = (version_t)dlsym(h, "zlibVersion");
            if (!r.compress2 || !r.bound || !r.version) throw std::runtime_error("compression_ratio needs zlib: libz.so.1 lacks compress2 / compressBound / zlibVersion");
            return r;
        }();
        return z;
    }
};
// bytes of zlib's compress2 of `text` at the default level (Python's zlib.compress(text))
inline size_t zlib_compressed_size(const std::string& text) {
    const Zlib& z = Zlib::get();
    unsigned long n = z.bound((unsigned long)text.size());
    std::vector<unsigned char> out(n);
    const int rc = z.compress2(out.data(), &n, (const unsigned char*)text.data(), (unsigned long)text.size(), -1);   // Z_DEFAULT_COMPRESSION
    if (rc != 0) throw std::runtime_error("zlib compress2 failed: " + std::to_string(rc));
    return (size_t)n;
}
// openai-whisper's compression_ratio: byte length / compressed byte length
inline double compression_ratio(const std::string& text) { return (double)text.size() / (double)zlib_compressed_size(text); }
// openai-whisper's fallback decision for one window: too repetitive (compression ratio above its threshold) or too unlikely (avg_logprob
// below its threshold) — unless the window counts as silence (no_speech_prob above its threshold).  A NaN threshold is off, as in skip_window.
inline bool needs_fallback(double cr, double avg_lp, double no_speech_prob, double cr_thr, double lp_thr, double ns_thr) {
    bool need = (!std::isnan(cr_thr) && cr > cr_thr) || (!std::isnan(lp_thr) && avg_lp < lp_thr);
    if (!std::isnan(ns_thr) && no_speech_prob > ns_thr) need = false;
    return need;
}
// The ladder over the n windows of one device batch.  decode(rung, active, scores) decodes the windows with active[w] != 0 at temperatures[rung]
// (rung 0: every window) and fills their scores; a window that needs a fallback is decoded again at the next rung, the others keep their
// result; after the last rung the last result stands.  rung_of[w] = the rung that produced window w's result.
struct WindowScore { double compression_ratio = 0, avg_logprob = 0, no_speech_prob = 0; };
template <typename Decode>
inline void run_ladder(size_t n, size_t n_rungs, double cr_thr, double lp_thr, double ns_thr, Decode&& decode, std::vector<int>& rung_of, std::vector<WindowScore>& scores) {
    rung_of.assign(n, 0);
    scores.assign(n, WindowScore());
    std::vector<unsigned char> active(n, 1);
    for (size_t r = 0; r < n_rungs; r++) {
        bool any = false;
        for (size_t w = 0; w < n; w++) any = any || active[w];
        if (!any) break;
        decode(r, active, scores);
        for (size_t w = 0; w < n; w++) {
            if (!active[w]) continue;
            rung_of[w] = (int)r;
            active[w] = needs_fallback(scores[w].compression_ratio, scores[w].avg_logprob, scores[w].no_speech_prob, cr_thr, lp_thr, ns_thr) ? 1 : 0;
        }
    }
}
inline std::string trim_ascii(const std::string& s) {
    size_t a = 0, b = s.size();
    while (a < b && isspace((unsigned char)s[a])) a++;
    while (b > a && isspace((unsigned char)s[b - 1])) b--;
    return s.substr(a, b - a);
}
// "0,0.2,0.4": the rungs of --temperature; each finite and >= 0, at least one
inline std::vector<float> parse_temperatures(const std::string& txt) {
    std::vector<float> out;
    size_t i = 0;
    while (i <= txt.size()) {
        const size_t j = std::min(txt.find(',', i), txt.size());
        const std::string w = trim_ascii(txt.substr(i, j - i));
        char* e = nullptr;
        const float f = strtof(w.c_str(), &e);
        if (w.empty() || *e || !std::isfinite(f) || f < 0.0f) throw std::runtime_error("--temperature: '" + w + "' is not a finite value >= 0");
        out.push_back(f);
        i = j + 1;
    }
    return out;
}

inline void set_conf(std::vector<Segment>& segs, double avg_lp, double no_speech_prob) {
    for (Segment& s : segs) { s.has_conf = true; s.avg_logprob = avg_lp; s.no_speech_prob = no_speech_prob; }
}
constexpr double kTimePrecision = 0.02;   // seconds per timestamp step

// Generated tokens of one 30 s window (the prompt left out; everything from the first EOT on is dropped) -> segments:
//   - split at every pair of adjacent timestamps; a slice runs from its first token's time (0 if that is text) to its last token's;
//   - tokens that end in a single timestamp: it closes the last slice;
//   - text after the last pair with no closing timestamp: a final segment from the pair's second timestamp to `duration`;
//   - no pair at all: one segment from 0 to the last timestamp (if one above <|0.00|> exists), else to `duration`.
inline std::vector<Segment> split_segments(const std::vector<int64_t>& generated, int64_t tb, int64_t eot, double duration) {
    std::vector<int64_t> t;
    for (int64_t x : generated) {
        if (x == eot) break;
        t.push_back(x);
    }
    auto is_ts = [&](size_t i) { return t[i] >= tb; };
    auto text_of = [&](size_t a, size_t b) {
        std::vector<int64_t> o;
        for (size_t i = a; i < b; i++)
            if (!is_ts(i)) o.push_back(t[i]);
        return o;
    };
    std::vector<size_t> cuts;
    for (size_t i = 1; i < t.size(); i++)
        if (is_ts(i - 1) && is_ts(i)) cuts.push_back(i);
    std::vector<Segment> out;
    if (cuts.empty()) {
        Segment s;
        s.end = duration;
        for (size_t i = t.size(); i-- > 0;)
            if (is_ts(i)) { if (t[i] > tb) s.end = (double)(t[i] - tb) * kTimePrecision; break; }
        s.tokens = text_of(0, t.size());
        out.push_back(s);
        return out;
    }
    const bool single_end = t.size() >= 2 && is_ts(t.size() - 1) && !is_ts(t.size() - 2);
    if (single_end) cuts.push_back(t.size());
    size_t last = 0;
    for (size_t c : cuts) {
        Segment s;
        s.start = is_ts(last) ? (double)(t[last] - tb) * kTimePrecision : 0.0;   // (only the first slice can open with text: from 0)
        s.end = (double)(t[c - 1] - tb) * kTimePrecision;
        s.tokens = text_of(last, c);
        out.push_back(s);
        last = c;
    }
    if (last < t.size()) {
        std::vector<int64_t> rest = text_of(last, t.size());
        if (!rest.empty()) {
            Segment s;
            s.start = is_ts(last) ? (double)(t[last] - tb) * kTimePrecision : out.back().end;
            s.end = duration;
            s.tokens = rest;
            out.push_back(s);
        }
    }
    return out;
}

// Long-form: window k's segments shifted by its start; where windows k and k+1 overlap, a segment belongs to k if it starts before
// start(k+1) + overlap / 2, else to k + 1.
inline std::vector<Segment> merge_window_segments(const std::vector<std::vector<Segment>>& windows, const std::vector<double>& starts, double overlap_s) {
    std::vector<Segment> out;
    for (size_t k = 0; k < windows.size(); k++) {
        const double lo = k == 0 ? -1e300 : starts[k] + overlap_s / 2;
        const double hi = k + 1 < windows.size() ? starts[k + 1] + overlap_s / 2 : 1e300;
        for (Segment s : windows[k]) {
            s.start += starts[k];
            s.end += starts[k];
            if (s.start >= lo && s.start < hi) out.push_back(s);
        }
    }
    return out;
}

// ---- sequential long-form (whisper_bench --sequential) --------------------------------------------------------------------
// openai-whisper's transcribe() without word_timestamps, stated on tokens: where a window's segments end and how far the file advances.
// `generated` are one window's generated ids (the prompt left out); g = those before the first EOT, ts(i) = g[i] >= tb;
// cuts = { i >= 1 : ts(i-1) && ts(i) }; single_end = len >= 2 && !ts(len-2) && ts(len-1).
//   - cuts non-empty: with single_end, len joins the cuts.  One segment per slice [last, c): from (g[last] - tb) * 0.02 s (0 if the slice opens
//     with text, which the timestamp rules never produce) to (g[c-1] - tb) * 0.02 s.  Text after the last cut is NOT a segment: the next window
//     decodes it again.  advance = seg_frames if single_end, else (g[c_last - 1] - tb) * 2 frames, c_last the last pair's cut;
//   - no cuts: one segment from 0 to seg_frames * 0.01 s, or to (t - tb) * 0.02 s where t, the last timestamp among g, lies above tb;
//     advance = seg_frames;
//   - a segment with start == end, or without a text id, is dropped.  A kept segment's ids are its slice, timestamps included.
// Deviation from openai-whisper: an advance of 0 (a closing pair at <|0.00|>) becomes seg_frames — openai-whisper would decode the same
// window for ever there, and flat synthetic logits do produce it.  The advance may exceed seg_frames at a file's end; the loop ends there.
struct SeqSegment {
    double start = 0, end = 0;
    std::vector<int64_t> ids;   // the slice: text ids and timestamps
    size_t window = 0;          // run_sequential: the ordinal of its window in the file
};
// *consumed (optional): how many of the generated ids the slices cover — what --word-timestamps takes its words from.
inline int64_t seek_advance(const std::vector<int64_t>& generated, int64_t tb, int64_t eot, int64_t seg_frames, std::vector<SeqSegment>& segs, size_t* consumed = nullptr) {
    segs.clear();
    std::vector<int64_t> g;
    for (int64_t x : generated) {
        if (x == eot) break;
        g.push_back(x);
    }
    const size_t len = g.size();
    auto ts = [&](size_t i) { return g[i] >= tb; };
    auto keep = [&](SeqSegment&& s) {
        bool text = false;
        for (int64_t x : s.ids) text = text || x < tb;
        if (text && s.start != s.end) segs.push_back(std::move(s));
    };
    std::vector<size_t> cuts;
    for (size_t i = 1; i < len; i++)
        if (ts(i - 1) && ts(i)) cuts.push_back(i);
    int64_t advance = seg_frames;
    if (!cuts.empty()) {
        const bool single_end = len >= 2 && !ts(len - 2) && ts(len - 1);
        if (!single_end) advance = (g[cuts.back() - 1] - tb) * 2;
        if (single_end) cuts.push_back(len);
        size_t last = 0;
        for (size_t c : cuts) {
            SeqSegment s;
            s.start = ts(last) ? (double)(g[last] - tb) * kTimePrecision : 0.0;
            s.end = (double)(g[c - 1] - tb) * kTimePrecision;
            s.ids.assign(g.begin() + (long)last, g.begin() + (long)c);
            keep(std::move(s));
            last = c;
        }
    } else {
        SeqSegment s;
        s.end = (double)seg_frames * 0.01;
        for (size_t i = len; i-- > 0;)
            if (ts(i)) { if (g[i] > tb) s.end = (double)(g[i] - tb) * kTimePrecision; break; }
        s.ids = g;
        keep(std::move(s));
    }
    if (consumed) *consumed = cuts.empty() ? len : cuts.back();
    return advance == 0 ? seg_frames : advance;
}

// The loop over many files in lockstep: step t decodes, as ONE device batch, the current window of every file that is not finished.
struct SeqConfig {
    int64_t tb = 0, eot = 0, sot_prev = 0;
    int n_text_ctx = 448;
    size_t n_prompt = 0, max_new_tokens = 0;
    bool condition_on_previous_text = true;
    double no_speech_threshold = std::nan(""), logprob_threshold = std::nan("");   // skip_window's; NaN: off
    std::vector<int64_t> initial_prompt;   // every file's history starts with these ids ...
    std::vector<std::vector<int64_t>> file_prompts;   // ... or, where this holds an entry for the file, with its own
};
struct SeqRow {          // one row of a step
    size_t file = 0, window = 0;   // the file, and the ordinal of this window in it
    int64_t seek = 0;
    int seg_frames = 0;            // min(3000, frames - seek)
    std::vector<int64_t> prefix;   // [sot_prev] ++ history, or empty
};
struct SeqStepResult {   // what step() returns per row
    std::vector<int64_t> tokens;   // the generated ids
    double avg_logprob = 0, no_speech_prob = 0, temperature = 0;
};
struct SeqWindow {
    int64_t seek = 0, advance = 0;
    int seg_frames = 0;
    bool skipped = false;
    size_t consumed = 0;           // generated ids its segments cover (seek_advance)
    std::vector<int64_t> tokens, prefix;
    double temperature = 0, avg_logprob = 0, no_speech_prob = 0;
};
struct SeqFile {
    std::vector<SeqWindow> windows;
    std::vector<SeqSegment> segments;   // times in the file
};
constexpr int kSeqWindowFrames = 3000;
constexpr double kSeqPromptResetTemperature = 0.5;   // openai-whisper's constant: a window decoded above it does not condition the next one
// the row's prefix: build_prev_prefix of the live history, trimmed from the front (the oldest ids go; <|startofprev|> stays) so that
// prefix + n_prompt + max_new_tokens <= n_text_ctx; no room for a single id: no prefix
inline std::vector<int64_t> seq_prefix(const std::vector<int64_t>& history, size_t reset_since, const SeqConfig& cfg) {
    std::vector<int64_t> pre = build_prev_prefix(std::vector<int64_t>(history.begin() + (long)std::min(reset_since, history.size()), history.end()), cfg.sot_prev, cfg.n_text_ctx);
    const long room = (long)cfg.n_text_ctx - (long)cfg.n_prompt - (long)cfg.max_new_tokens;
    if ((long)pre.size() <= room) return pre;
    if (room < 2) return {};
    std::vector<int64_t> out(1, cfg.sot_prev);
    out.insert(out.end(), pre.end() - (room - 1), pre.end());
    return out;
}
// frames[f]: mel frames of file f.  step(rows, results) decodes the rows (in file order) and fills one SeqStepResult per row.  Per file:
// seek = 0, history = the initial prompt, reset_since = 0; per window: a skipped one (skip_window) yields no segments, advances the whole
// window and leaves the history and reset_since alone (openai-whisper `continue`s there); any other goes through seek_advance, its segments
// shifted by seek * 0.01 s, their ids appended to the history; then, without conditioning or above the reset temperature, reset_since = the
// history's length.
template <typename Step>
inline void run_sequential(const std::vector<int64_t>& frames, const SeqConfig& cfg, Step&& step, std::vector<SeqFile>& out) {
    const size_t n = frames.size();
    out.assign(n, SeqFile());
    std::vector<int64_t> seek(n, 0);
    std::vector<std::vector<int64_t>> history(n, cfg.initial_prompt);
    for (size_t f = 0; f < n && f < cfg.file_prompts.size(); f++) history[f] = cfg.file_prompts[f];
    std::vector<size_t> reset_since(n, 0);
    for (;;) {
        std::vector<SeqRow> rows;
        for (size_t f = 0; f < n; f++) {
            if (seek[f] >= frames[f]) continue;
            SeqRow r;
            r.file = f;
            r.window = out[f].windows.size();
            r.seek = seek[f];
            r.seg_frames = (int)std::min<int64_t>(kSeqWindowFrames, frames[f] - seek[f]);
            r.prefix = seq_prefix(history[f], reset_since[f], cfg);
            rows.push_back(std::move(r));
        }
        if (rows.empty()) break;
        std::vector<SeqStepResult> res(rows.size());
        step(rows, res);
        for (size_t i = 0; i < rows.size(); i++) {
            const size_t f = rows[i].file;
            SeqWindow w;
            w.seek = rows[i].seek;
            w.seg_frames = rows[i].seg_frames;
            w.prefix = rows[i].prefix;
            w.tokens = res[i].tokens;
            w.temperature = res[i].temperature;
            w.avg_logprob = res[i].avg_logprob;
            w.no_speech_prob = res[i].no_speech_prob;
            if (skip_window(res[i].no_speech_prob, res[i].avg_logprob, cfg.no_speech_threshold, cfg.logprob_threshold)) {
                w.skipped = true;
                w.advance = w.seg_frames;
            } else {
                std::vector<SeqSegment> segs;
                w.advance = seek_advance(res[i].tokens, cfg.tb, cfg.eot, w.seg_frames, segs, &w.consumed);
                for (SeqSegment& s : segs) {
                    s.start += (double)w.seek * 0.01;
                    s.end += (double)w.seek * 0.01;
                    s.window = rows[i].window;
                    history[f].insert(history[f].end(), s.ids.begin(), s.ids.end());
                    out[f].segments.push_back(std::move(s));
                }
                if (!cfg.condition_on_previous_text || res[i].temperature > kSeqPromptResetTemperature) reset_since[f] = history[f].size();
            }
            seek[f] += w.advance;
            out[f].windows.push_back(std::move(w));
        }
    }
}

// "HH:MM:SS,mmm" (SRT) / "HH:MM:SS.mmm" (VTT), rounded to the millisecond
inline std::string fmt_cue_time(double t, char sep) {
    long long ms = std::llround(std::max(t, 0.0) * 1000.0);
    char b[48];
    snprintf(b, sizeof b, "%02lld:%02lld:%02lld%c%03lld", ms / 3600000, (ms / 60000) % 60, (ms / 1000) % 60, sep, ms % 1000);
    return b;
}
struct Cue {
    double start, end; std::string text;
    bool has_conf = false; double avg_logprob = 0, no_speech_prob = 0;   // its segment's (--logprobs)
};
inline std::string srt_text(const std::vector<Cue>& cues) {
    std::string o;
    for (size_t i = 0; i < cues.size(); i++)
        o += std::to_string(i + 1) + "\n" + fmt_cue_time(cues[i].start, ',') + " --> " + fmt_cue_time(cues[i].end, ',') + "\n" + cues[i].text + "\n\n";
    return o;
}
inline std::string cues_json(const std::vector<Cue>& cues) {   // [{"start": s, "end": s, "text": "..."}] on one line
    std::string o = "[";
    for (size_t i = 0; i < cues.size(); i++)
        o += (i ? ", " : "") + std::string("{\"start\": ") + fmt_f64(cues[i].start) + ", \"end\": " + fmt_f64(cues[i].end) + ", \"text\": " +
             json_escape(cues[i].text) +
             (cues[i].has_conf ? ", \"avg_logprob\": " + fmt_conf(cues[i].avg_logprob) + ", \"no_speech_prob\": " + fmt_conf(cues[i].no_speech_prob) : std::string()) + "}";
    return o + "]";
}
inline std::string vtt_text(const std::vector<Cue>& cues) {
    std::string o = "WEBVTT\n\n";
    for (size_t i = 0; i < cues.size(); i++)
        o += std::to_string(i + 1) + "\n" + fmt_cue_time(cues[i].start, '.') + " --> " + fmt_cue_time(cues[i].end, '.') + "\n" + cues[i].text + "\n\n";
    return o;
}

// GPT-2 byte-level alphabet: unicode code point → byte
inline const std::map<uint32_t, unsigned char>& byte_decoder() {
    static std::map<uint32_t, unsigned char> m;
    if (m.empty()) {
        std::vector<int> bs;
        for (int b = '!'; b <= '~'; b++) bs.push_back(b);
        for (int b = 0xA1; b <= 0xAC; b++) bs.push_back(b);
        for (int b = 0xAE; b <= 0xFF; b++) bs.push_back(b);
        std::vector<int> cs = bs;
        int n = 0;
        for (int b = 0; b < 256; b++)
            if (std::find(bs.begin(), bs.end(), b) == bs.end()) { bs.push_back(b); cs.push_back(256 + n++); }
        for (size_t i = 0; i < bs.size(); i++) m[(uint32_t)cs[i]] = (unsigned char)bs[i];
    }
    return m;
}

inline std::string decode_tokens(const std::vector<int64_t>& tokens, const Tokenizer* tok) {  // :637-648
    if (tok && tok->loaded) {  // byte-level BPE decode, skip_special_tokens = true
        std::string joined;
        for (int64_t t : tokens) {
            if (t < 0 || (size_t)t >= tok->id_to_tok.size() || tok->is_special[(size_t)t]) continue;
            joined += tok->id_to_tok[(size_t)t];
        }
        std::string bytes;
        const auto& bd = byte_decoder();
        for (size_t i = 0; i < joined.size();) {
            unsigned char c = (unsigned char)joined[i];
            uint32_t cp; int len;
            if (c < 0x80) { cp = c; len = 1; }
            else if ((c >> 5) == 6) { cp = c & 31; len = 2; }
            else if ((c >> 4) == 14) { cp = c & 15; len = 3; }
            else { cp = c & 7; len = 4; }
            for (int k = 1; k < len && i + k < joined.size(); k++) cp = (cp << 6) | ((unsigned char)joined[i + k] & 63);
            i += (size_t)len;
            auto it = bd.find(cp);
            if (it != bd.end()) bytes += (char)it->second;
        }
        return bytes;
    }
    std::string o = "[TOKENS:";  // :644-647, first 200 ids
    for (size_t i = 0; i < tokens.size() && i < 200; i++) { if (i) o += " "; o += std::to_string(tokens[i]); }
    return o + "]";
}

// ---------------------------------------------------------------------------------------------
// word-level timestamps (wh_ctx_set_alignment / wh_get_token_frames; no reference counterpart): a window's generated tokens and their
// frames -> words, as openai-whisper's split_tokens_on_spaces does.  Timestamp tokens (ids >= tb, tb < 0: none), EOT and the tokenizer's
// special tokens are dropped; of the kept tokens a new word begins where the decoded piece begins with a space (and at the first piece); a
// piece that ends inside a UTF-8 sequence stays with the next one.  A word starts at its first token's frame x 0.02 s and ends where the
// next kept token starts (the last word: at the window's duration); both are offset by the window's start.  Punctuation is not merged into
// its neighbours.  Without a tokenizer the pieces are those of decode_tokens' "[TOKENS:a b c]" form (its first 200 ids), so that the words
// of a window always concatenate to its text.
// ---------------------------------------------------------------------------------------------
struct Word {
    std::string word;
    double start = 0, end = 0;
};

inline bool utf8_complete(const std::string& s) {   // false when s ends inside a multi-byte sequence
    size_t i = 0;
    while (i < s.size()) {
        const unsigned char c = (unsigned char)s[i];
        const size_t len = c < 0x80 ? 1 : (c >> 5) == 6 ? 2 : (c >> 4) == 14 ? 3 : (c >> 3) == 30 ? 4 : 1;
        if (i + len > s.size()) return false;
        i += len;
    }
    return true;
}

inline std::vector<Word> words_from_tokens(const std::vector<int64_t>& tokens, const std::vector<int32_t>& frames, int64_t tb, int64_t eot,
                                           double duration, double offset, const Tokenizer* tok) {
    const bool have_tok = tok && tok->loaded;
    std::vector<size_t> kept;   // rows that carry text
    for (size_t i = 0; i < tokens.size() && i < frames.size(); i++) {
        const int64_t t = tokens[i];
        if (t == eot || (tb >= 0 && t >= tb) || t < 0) continue;
        if (have_tok && ((size_t)t >= tok->id_to_tok.size() || tok->is_special[(size_t)t])) continue;
        if (!have_tok && kept.size() == 200) break;
        kept.push_back(i);
    }
    auto t_of = [&](size_t k) { return std::min(duration, std::max(0.0, frames[kept[k]] * 0.02)) + offset; };
    std::vector<Word> words;
    std::string pending;       // bytes of pieces that did not end on a character boundary yet
    size_t pending_first = 0;  // kept index of the first token in `pending`
    for (size_t k = 0; k < kept.size(); k++) {
        std::string piece;
        if (have_tok) piece = decode_tokens({tokens[kept[k]]}, tok);
        else piece = (k == 0 ? "[TOKENS:" : " ") + std::to_string(tokens[kept[k]]) + (k + 1 == kept.size() ? "]" : "");
        if (pending.empty()) pending_first = k;
        pending += piece;
        if (!utf8_complete(pending) && k + 1 < kept.size()) continue;
        if (words.empty() || pending[0] == ' ') {
            Word w;
            w.word = pending;
            w.start = t_of(pending_first);
            words.push_back(w);
        } else {
            words.back().word += pending;
        }
        // the word ends where the next kept token starts
        words.back().end = k + 1 < kept.size() ? t_of(k + 1) : duration + offset;
        pending.clear();
    }
    for (Word& w : words) w.end = std::max(w.end, w.start);
    return words;
}

inline std::string words_json(const std::vector<Word>& words) {   // [{"word": "...", "start": s, "end": s}] on one line
    std::string o = "[";
    char b[96];
    for (size_t i = 0; i < words.size(); i++) {
        snprintf(b, sizeof b, ", \"start\": %.2f, \"end\": %.2f}", words[i].start, words[i].end);
        o += std::string(i ? ", " : "") + "{\"word\": " + json_escape(words[i].word) + b;
    }
    return o + "]";
}

// ---------------------------------------------------------------------------------------------
// long-form stitcher — src/main.rs:659-696
// ---------------------------------------------------------------------------------------------
// Rust's str::split_whitespace / trim split on the Unicode White_Space property and str::to_lowercase maps every cased
// letter (src/main.rs:663, 671, 686-688 use all three): the helpers below decode UTF-8 and do the same — the White_Space set
// in full, lowercase through the complete table of simple case mappings (wh_unicode_lower.h, generated from the Unicode
// Character Database by tools/gen_unicode_lower.py), the one multi-character mapping (U+0130 -> "i" + U+0307) and the
// contextual final sigma.
inline size_t utf8_next(const std::string& s, size_t i, uint32_t* cp) {   // decodes one scalar value, returns its byte length (malformed: 1 byte, U+FFFD)
    const unsigned char c = (unsigned char)s[i];
    auto cont = [&](size_t k) { return i + k < s.size() && ((unsigned char)s[i + k] & 0xC0) == 0x80; };
    if (c < 0x80) { *cp = c; return 1; }
    if ((c & 0xE0) == 0xC0 && cont(1)) { *cp = ((c & 0x1Fu) << 6) | ((unsigned char)s[i + 1] & 0x3Fu); return 2; }
    if ((c & 0xF0) == 0xE0 && cont(1) && cont(2)) { *cp = ((c & 0x0Fu) << 12) | (((unsigned char)s[i + 1] & 0x3Fu) << 6) | ((unsigned char)s[i + 2] & 0x3Fu); return 3; }
    if ((c & 0xF8) == 0xF0 && cont(1) && cont(2) && cont(3)) {
        *cp = ((c & 0x07u) << 18) | (((unsigned char)s[i + 1] & 0x3Fu) << 12) | (((unsigned char)s[i + 2] & 0x3Fu) << 6) | ((unsigned char)s[i + 3] & 0x3Fu);
        return 4;
    }
    *cp = 0xFFFD;
    return 1;
}
inline void utf8_put(std::string& o, uint32_t cp) {
    if (cp < 0x80) o += (char)cp;
    else if (cp < 0x800) { o += (char)(0xC0 | (cp >> 6)); o += (char)(0x80 | (cp & 0x3F)); }
    else if (cp < 0x10000) { o += (char)(0xE0 | (cp >> 12)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
    else { o += (char)(0xF0 | (cp >> 18)); o += (char)(0x80 | ((cp >> 12) & 0x3F)); o += (char)(0x80 | ((cp >> 6) & 0x3F)); o += (char)(0x80 | (cp & 0x3F)); }
}
inline bool is_unicode_ws(uint32_t c) {   // the White_Space property (char::is_whitespace)
    return (c >= 0x09 && c <= 0x0D) || c == 0x20 || c == 0x85 || c == 0xA0 || c == 0x1680 || (c >= 0x2000 && c <= 0x200A) || c == 0x2028 ||
           c == 0x2029 || c == 0x202F || c == 0x205F || c == 0x3000;
}
inline uint32_t lower_cp(uint32_t c) {   // simple lowercase mapping: the generated table (wh_unicode_lower.h), binary search over its runs
    if (c < 0x80) return (c >= 'A' && c <= 'Z') ? c + 32 : c;
    int lo = 0, hi = kLowerRunCount - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) / 2;
        const LowerRun& r = kLowerRuns[mid];
        if (c < r.first) hi = mid - 1;
        else if (c > r.last) lo = mid + 1;
        else return ((c - r.first) % r.stride) == 0 ? (uint32_t)((int32_t)c + r.delta) : c;
    }
    return c;
}
// cased / case-ignorable, as far as the final-sigma rule of str::to_lowercase needs them: a letter with a case mapping in either
// direction is cased; apostrophes, full stop, colon, soft hyphen, combining marks (U+0300-036F) and modifier letters are ignorable
inline bool is_cased(uint32_t c) {
    if (lower_cp(c) != c) return true;
    if ((c >= 'a' && c <= 'z') || (c >= 0xDF && c <= 0xFF && c != 0xF7) || c == 0xB5 || c == 0xAA || c == 0xBA) return true;
    if ((c >= 0x100 && c <= 0x24F) || (c >= 0x3AC && c <= 0x3CE) || (c >= 0x430 && c <= 0x52F) || (c >= 0x561 && c <= 0x587) ||
        (c >= 0x1E00 && c <= 0x1FFF) || (c >= 0xFF41 && c <= 0xFF5A)) return true;
    return false;
}
inline bool is_case_ignorable(uint32_t c) {
    return c == '\'' || c == '.' || c == ':' || c == '^' || c == '`' || c == 0xA8 || c == 0xAD || c == 0xAF || c == 0xB4 || c == 0xB7 || c == 0xB8 ||
           c == 0x2019 || c == 0x2018 || (c >= 0x2B0 && c <= 0x36F) || (c >= 0x483 && c <= 0x489) || (c >= 0x200B && c <= 0x200F);
}
inline std::vector<std::string> split_ws(const std::string& s) {   // str::split_whitespace
    std::vector<std::string> w;
    std::string cur;
    for (size_t i = 0; i < s.size();) {
        uint32_t cp;
        const size_t n = utf8_next(s, i, &cp);
        if (is_unicode_ws(cp)) { if (!cur.empty()) { w.push_back(cur); cur.clear(); } }
        else cur.append(s, i, n);
        i += n;
    }
    if (!cur.empty()) w.push_back(cur);
    return w;
}
inline std::string lower(const std::string& s) {   // str::to_lowercase
    std::string o;
    for (size_t i = 0; i < s.size();) {
        uint32_t cp;
        const size_t n = utf8_next(s, i, &cp);
        if (cp == 0xFFFD && n == 1 && (unsigned char)s[i] >= 0x80) o += s[i];        // malformed byte: passed through
        else if (cp == 0x130) { o += 'i'; utf8_put(o, 0x307); }
        else if (cp == 0x3A3) {
            // final sigma (the one contextual rule of str::to_lowercase): preceded by a cased letter and not followed by one,
            // case-ignorable characters skipped on both sides -> U+03C2, else U+03C3
            bool before = false, after = false;
            for (size_t q = i; q > 0;) {
                size_t b = q - 1;
                while (b > 0 && ((unsigned char)s[b] & 0xC0) == 0x80) b--;
                uint32_t pc;
                utf8_next(s, b, &pc);
                q = b;
                if (is_case_ignorable(pc)) continue;
                before = is_cased(pc);
                break;
            }
            for (size_t q = i + n; q < s.size();) {
                uint32_t nc;
                const size_t m = utf8_next(s, q, &nc);
                q += m;
                if (is_case_ignorable(nc)) continue;
                after = is_cased(nc);
                break;
            }
            utf8_put(o, (before && !after) ? 0x3C2 : 0x3C3);
        }
        else utf8_put(o, lower_cp(cp));
        i += n;
    }
    return o;
}
inline std::string trim(const std::string& s) {   // str::trim
    size_t a = 0, b = s.size();
    while (a < b) {
        uint32_t cp;
        const size_t n = utf8_next(s, a, &cp);
        if (!is_unicode_ws(cp)) break;
        a += n;
    }
    while (b > a) {   // step back one scalar value
        size_t q = b - 1;
        while (q > a && ((unsigned char)s[q] & 0xC0) == 0x80) q--;
        uint32_t cp;
        utf8_next(s, q, &cp);
        if (!is_unicode_ws(cp)) break;
        b = q;
    }
    return s.substr(a, b - a);
}
inline std::string ltrim(const std::string& s) { return s.substr(s.size() - trim(s + "x").size() + 1); }   // leading white space only
inline std::string rtrim(const std::string& s) { return s.substr(0, trim("x" + s).size() - 1); }            // trailing white space only
inline size_t word_overlap(const std::string& a, const std::string& b, size_t max_words) {  // :686-696
    auto aw = split_ws(a), bw = split_ws(b);
    for (auto& w : aw) w = lower(w);
    for (auto& w : bw) w = lower(w);
    size_t mx = std::min(max_words, std::min(aw.size(), bw.size()));
    for (size_t k = mx; k >= 1; k--) {
        if (std::equal(aw.end() - (long)k, aw.end(), bw.begin())) return k;
        if (k == 1) break;
    }
    return 0;
}
inline std::string stitch_texts(const std::vector<std::string>& chunks) {  // :659-684
    std::string out;
    for (auto& chunk : chunks) {
        std::string t = trim(chunk);
        if (t.empty()) continue;
        if (out.empty()) { out = t; continue; }
        size_t ov = word_overlap(out, t, 16);
        if (ov > 0) {
            auto words = split_ws(t);
            std::string rem;
            for (size_t i = ov; i < words.size(); i++) { if (!rem.empty()) rem += " "; rem += words[i]; }
            if (!rem.empty()) { out += " "; out += rem; }
        } else {
            out += " ";
            out += t;
        }
    }
    return out;
}


// ---------------------------------------------------------------------------------------------
// the file loop (src/main.rs:1164-1213) as a pipeline: loader threads -> bounded, index-ordered queue -> one worker
// per context.  The reference loads and transcribes one file after the other and fails fast with the first error;
// here loading runs ahead of the GPUs, rows stay in file order, and the first error — from a loader or a worker — ends
// every thread: each path that sets the error or makes a thread leave wakes all three wait points (items, space, pool).
// ---------------------------------------------------------------------------------------------
struct PipeItem {
    size_t idx = 0;
    std::vector<float> audio;
    double dur = 0, load_s = 0;
    float* pin = nullptr;   // samples in a pool buffer instead of `audio`
    size_t n_pin = 0;
    // a raw payload beside `audio` (whisper_bench --gpu-ingest): the file's samples as it holds them, in `raw.file` or, when they fit, in the
    // pool buffer `pin`; n_16k = their length once resampled, which is what decides between a batch of one-window files and the long-form entry
    RawWav raw;
    bool is_raw = false;
    size_t n_16k = 0;
    size_t n() const { return is_raw ? n_16k : pin ? n_pin : audio.size(); }
    const float* data() const { return pin ? pin : audio.data(); }
    const void* raw_data() const { return pin ? (const void*)pin : (const void*)raw.payload(); }
};

// Fixed-size staging buffers from caller-supplied alloc / free (page-locked memory in the CLI).  Allocated on first use
// (only runs that meet a one-window file pay for it) and all or nothing: with a partial pool the loader of the next index
// in line could wait for a buffer while later, parked indices hold every one of them.
class BufferPool {
  public:
    BufferPool(std::function<float*()> alloc, std::function<void(float*)> dealloc) : alloc_(std::move(alloc)), free_(std::move(dealloc)) {}
    ~BufferPool() { for (float* p : all_) free_(p); }   // every buffer the pool allocated, wherever an aborted run left it
    // true if the pool holds `n` buffers (allocating them now if this is the first call); false = use pageable memory
    bool ensure(size_t n) {
        std::lock_guard<std::mutex> lk(m_);
        if (tried_) return total_ > 0;
        tried_ = true;
        for (size_t i = 0; i < n; i++) {
            float* p = alloc_();
            if (!p) {   // not enough page-locked memory: give back what was taken, run without the pool — and say so: throughput changes
                for (float* q : free_list_) free_(q);
                free_list_.clear();
                all_.clear();
                fprintf(stderr, "[wh_host] staging pool: %zu of %zu buffers could be allocated; continuing with pageable memory (slower host-to-device copies)\n", i, n);
                return false;
            }
            free_list_.push_back(p);
            all_.push_back(p);
        }
        total_ = n;
        return total_ > 0;
    }
    float* acquire() {   // nullptr once aborted
        std::unique_lock<std::mutex> lk(m_);
        cv_.wait(lk, [&] { return aborted_ || !free_list_.empty(); });
        if (aborted_) return nullptr;
        float* p = free_list_.back();
        free_list_.pop_back();
        return p;
    }
    void release(float* p) {
        { std::lock_guard<std::mutex> lk(m_); free_list_.push_back(p); }
        cv_.notify_one();
    }
    void abort() {
        { std::lock_guard<std::mutex> lk(m_); aborted_ = true; }
        cv_.notify_all();
    }
    size_t total() const { return total_; }

  private:
    std::function<float*()> alloc_;
    std::function<void(float*)> free_;
    std::vector<float*> free_list_, all_;
    size_t total_ = 0;
    bool tried_ = false, aborted_ = false;
    std::mutex m_;
    std::condition_variable cv_;
};

// look-ahead of the loaders (files loaded but not yet handed to a worker: one batch per worker — a worker waits for a FULL batch, so
// anything less would stall it) / buffers a staging pool needs: the look-ahead + the two batches a worker holds (the one it
// transcribes and the one whose host-to-device copy runs beside it) + one per loader
inline size_t file_pipeline_lookahead(size_t max_batch, size_t n_workers) { return max_batch * n_workers + 4; }
inline size_t file_pipeline_pool_size(size_t max_batch, size_t n_workers, int n_loaders) {
    return file_pipeline_lookahead(max_batch, n_workers) + 2 * max_batch * n_workers + (size_t)n_loaders;
}

// load(idx, audio, dur) fills one file; process(worker, batch, next) transcribes a batch of one-window files (<= max_batch of
// them, only what is already loaded) or ONE multi-window file; `next` (may be null) is the batch of one-window files this worker
// will be given next, already loaded — the place to start its host-to-device copy (wh_transcribe_batch_next); both may throw.
// Returns the first error ("" = none).  `pool` (optional) stages one-window files; a batch's buffers go back to the pool after
// the process() call that transcribed it returns.  `load_raw` (optional) replaces `load`: it fills the item's raw payload, n_16k and dur
// (it.raw, it.is_raw); a payload of a one-window file that fits a pool buffer (window_samples floats) is staged there like converted samples.
inline std::string run_file_pipeline(size_t nfiles, int n_loaders, size_t n_workers, size_t max_batch, size_t window_samples, BufferPool* pool,
                                     const std::function<void(size_t, std::vector<float>&, double&)>& load,
                                     const std::function<void(size_t, std::vector<PipeItem>&, std::vector<PipeItem>*)>& process,
                                     const std::function<void(size_t, PipeItem&)>& load_raw = nullptr) {
    std::mutex mu;
    std::condition_variable cv_items, cv_space;
    std::deque<PipeItem> ready;               // loaded files, in index order
    std::map<size_t, PipeItem> parked;        // loaded out of order, waiting for their turn
    size_t next_ready = 0;                    // index the queue is waiting for
    size_t handed = 0;                        // files handed to workers so far (under mu)
    std::atomic<size_t> next_load{0};
    std::string first_error;
    const size_t cap = file_pipeline_lookahead(max_batch, n_workers);
    const size_t pool_size = file_pipeline_pool_size(max_batch, n_workers, n_loaders);
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    auto fail = [&](const std::string& what) {   // call WITHOUT mu held
        {
            std::lock_guard<std::mutex> lk(mu);
            if (first_error.empty()) first_error = what.empty() ? "unknown error" : what;
        }
        cv_items.notify_all();
        cv_space.notify_all();
        if (pool) pool->abort();
    };
    auto loader = [&]() {
        for (;;) {
            const size_t i = next_load.fetch_add(1);
            if (i >= nfiles) return;
            { std::lock_guard<std::mutex> lk(mu); if (!first_error.empty()) return; }
            PipeItem it;
            it.idx = i;
            try {
                const double tl0 = now();
                if (load_raw) load_raw(i, it);
                else load(i, it.audio, it.dur);
                it.load_s = now() - tl0;
                if (it.is_raw) {
                    if (pool && it.n_16k <= window_samples && it.raw.n_bytes <= window_samples * sizeof(float) && pool->ensure(pool_size)) {
                        it.pin = pool->acquire();
                        if (!it.pin) return;   // aborted: another thread has failed
                        memcpy(it.pin, it.raw.payload(), it.raw.n_bytes);
                        std::vector<unsigned char>().swap(it.raw.file);
                    }
                } else
                // one-window files move into a staging buffer of the pool (page-locked in the CLI: the library's host-to-device
                // copy is then one DMA at link speed; a pageable source goes through the runtime's staging buffers)
                if (pool && it.audio.size() <= window_samples && pool->ensure(pool_size)) {
                    it.pin = pool->acquire();
                    if (!it.pin) return;   // aborted: another thread has failed
                    memcpy(it.pin, it.audio.data(), it.audio.size() * sizeof(float));
                    it.n_pin = it.audio.size();
                    std::vector<float>().swap(it.audio);
                }
            } catch (const std::exception& e) {
                fail(e.what());
                return;
            }
            std::unique_lock<std::mutex> lk(mu);
            cv_space.wait(lk, [&] { return !first_error.empty() || i < handed + cap; });   // bounded look-ahead of the consumers
            if (!first_error.empty()) {
                if (it.pin) pool->release(it.pin);
                return;
            }
            parked.emplace(i, std::move(it));
            while (!parked.empty() && parked.begin()->first == next_ready) {
                ready.push_back(std::move(parked.begin()->second));
                parked.erase(parked.begin());
                next_ready++;
            }
            cv_items.notify_all();
        }
    };
    // take the next batch off the queue (under mu): a full batch, the tail of the input, or a multi-window file alone.
    // `block`: wait for one; else only what is available right now.  Returns false when there is none (end of input, error, or not yet).
    auto take = [&](std::unique_lock<std::mutex>& lk, bool block, bool one_window_only, std::vector<PipeItem>& batch) -> bool {
        auto avail = [&] {
            return !first_error.empty() || handed == nfiles || ready.size() >= max_batch || handed + ready.size() == nfiles ||
                   (!ready.empty() && ready.front().n() > window_samples);
        };
        for (;;) {
            if (block) cv_items.wait(lk, avail);
            else if (!avail()) return false;
            if (!first_error.empty()) return false;
            if (ready.empty()) {
                if (handed == nfiles || !block) return false;
                continue;
            }
            break;
        }
        if (ready.front().n() > window_samples) {
            if (one_window_only) return false;   // a multi-window file is never a "next" batch: it goes alone through the long-form entry
            batch.push_back(std::move(ready.front()));
            ready.pop_front();
        } else {
            while (!ready.empty() && batch.size() < max_batch && ready.front().n() <= window_samples) {
                batch.push_back(std::move(ready.front()));
                ready.pop_front();
            }
        }
        handed += batch.size();
        return true;
    };
    auto give_back = [&](std::vector<PipeItem>& batch) {
        for (PipeItem& it : batch)
            if (it.pin) { pool->release(it.pin); it.pin = nullptr; }
        batch.clear();
    };
    auto worker = [&](size_t wi) {
        std::vector<PipeItem> cur, nxt;
        bool have_next = false;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu);
                if (have_next) { cur = std::move(nxt); nxt.clear(); have_next = false; }
                else if (!take(lk, true, false, cur)) { give_back(cur); return; }
                // one batch of look-ahead for this worker, if it is loaded already (never waited for)
                const bool cur_one_window = cur.size() > 1 || cur[0].n() <= window_samples;
                if (cur_one_window) have_next = take(lk, false, true, nxt);
            }
            cv_space.notify_all();
            cv_items.notify_all();
            try {
                process(wi, cur, have_next ? &nxt : nullptr);
                give_back(cur);
            } catch (const std::exception& e) {
                give_back(cur);
                give_back(nxt);
                fail(e.what());
                return;
            }
        }
    };
    std::vector<std::thread> threads;
    for (int i = 0; i < n_loaders; i++) threads.emplace_back(loader);
    for (size_t wi = 0; wi < n_workers; wi++) threads.emplace_back(worker, wi);
    for (auto& t : threads) t.join();
    return first_error;
}

}  // namespace whhost
