// wh_host_shared.h — what the host files of libwhisper_hip.so share (wh_ctx.cpp, wh_options.cpp, wh_encode_host.cpp, wh_decode_host.cpp,
// wh_score_host.cpp, wh_api.cpp): error reporting, the profiling scope, the carve and growth helpers, and the functions one file defines for another.
#pragma once
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

namespace wh {

constexpr int RAW_LD = 3008;   // raw log-mel row stride (frames), multiple of 16
constexpr int TOK_ROWS = 3002; // conv1 operand rows per clip: zero row, 3000 frames, zero row
constexpr int H1_ROWS = 3001;  // conv2 operand rows per clip: zero row, 3000 positions

inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// records the message as the context's (and the library's) last error; returns `code` (wh_ctx.cpp)
int fail(wh_ctx* c, int code, const char* fmt, ...);

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

void prof_reset(wh_ctx* c);     // wh_ctx.cpp
void prof_collect(wh_ctx* c);

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) {
        size_t o = off;
        off = align_up(off + bytes, 256);
        return o;
    }
};
template <typename T> T* at(void* base, size_t off) { return (T*)((char*)base + off); }

// destroys the captured decode step (wh_ctx.cpp): before a buffer it holds is freed, when its key changes, and in wh_ctx_free
void drop_step_graph(wh_ctx* c);

// A grow-on-demand buffer of the context (`what`, for the error text) grows to at least `bytes`.  step_holds: the captured decode step holds the buffer's address, so the
// step graph is dropped before the buffer is freed (the rule above wh_ctx::StepKey).  Two policies, named at every call site:
//   GROW_FREE_FIRST  free, then allocate: the large buffers, where holding both copies would double the peak.  A failed allocation leaves the
//                    buffer empty and the call fails with WH_ERR_HIP.
//   GROW_KEEP_OLD    allocate first: a failed allocation keeps the old, smaller buffer, leaves no sticky HIP error behind and fails the call with
//                    WH_ERR_NOMEM, "<what> (<bytes> bytes): hipMalloc: ..." (the raw staging buffers, ensure_ingest).
enum GrowPolicy { GROW_FREE_FIRST, GROW_KEEP_OLD };
template <typename T>
int grow(wh_ctx* c, DevBuf<T>& b, size_t bytes, bool step_holds, GrowPolicy policy, const char* what) {
    if (bytes <= b.bytes) return WH_OK;
    DevBuf<T> nb;
    if (policy == GROW_KEEP_OLD) {
        const hipError_t e = hipMalloc(&nb.p, bytes);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return fail(c, WH_ERR_NOMEM, "%s (%zu bytes): hipMalloc: %s", what, bytes, hipGetErrorString(e));
        }
    }
    if (step_holds) drop_step_graph(c);
    b.reset();
    if (policy == GROW_FREE_FIRST) {
        const hipError_t e = hipMalloc(&nb.p, bytes);
        if (e != hipSuccess) return fail(c, WH_ERR_HIP, "HIP error %d (%s): hipMalloc of %s (%zu bytes)", (int)e, hipGetErrorString(e), what, bytes);
    }
    nb.bytes = bytes;
    b = std::move(nb);
    return WH_OK;
}

// ---- wh_options.cpp ----
// the prefix of batch row b (first_row: index of the batch's first window in a long-form call, -1: the rows are the call's clips)
const int64_t* prefix_of(const wh_ctx* c, long first_row, int b, int* len);
int options_check(wh_ctx* c, const wh_decode_params* p, int n_clips, bool longform, int al_rows = -1);
bool sample_trivial(const wh_ctx* c);
int alignment_opts_check(wh_ctx* c, const wh_alignment_opts* o, const char* who);
void alignment_layers(const wh_dims& D, const wh_alignment_opts* o, std::vector<AlignLayerHeads>& layer);

// ---- wh_encode_host.cpp ----
int enc_begin(wh_ctx* c);
int run_encoder(wh_ctx* c, int nb, bool want_f32);
int run_encoder_pass(wh_ctx* c, const float* pcm, int nb, int set);
int ensure_long(wh_ctx* c, size_t n, size_t nf);
int whole_file_mel(wh_ctx* c, const float* pcm, size_t n, size_t* nf_out, size_t* ld_out, const wh_raw_clip* raw = nullptr, double* h2d_s_out = nullptr);
int load_file_set(wh_ctx* c, const wh_clip* files, const wh_raw_clip* raws, size_t n);
void launch_window_cut(wh_ctx* c, int nb);

// ---- wh_decode_host.cpp ----
int run_decode(wh_ctx* c, int nb, const wh_decode_params* p, int64_t* tokens_out, size_t tok_stride, size_t* n_tokens_out, float* logits_out,
               size_t logits_rows, const std::function<int()>& after_kv = nullptr, const int32_t* sel = nullptr, size_t n_sel = 0);


// ---- wh_score_host.cpp ----
int run_score(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, float* logprob_out, int64_t* argmax_out, size_t cap_tokens,
              const int32_t* logit_hyps, size_t n_logit_hyps, float* logits_out, size_t cap_logits_rows);
// wh_align_tokens: the same pass with the listed heads' queries gathered, and the alignment post-pass over its hypotheses
int run_align_tokens(wh_ctx* c, const wh_decode_params* p, const wh_score_input* in, const wh_alignment_opts* heads, int32_t* frames_out, int32_t* n_frames_out,
                     float* logprob_out, size_t cap_tokens);

}  // namespace wh
