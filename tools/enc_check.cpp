// enc_check.cpp — the encoder-side kernels, each alone against a double-precision host restatement of its contract, with an FNV-1a hash of every
// raw output buffer:  k_gemm8 and k_ln_stats (wh_gemm8.hip), k_gemm8x (wh_gemm8x.hip), k_gemm, k_layernorm and k_layernorm_w8 (wh_gemm.hip),
// k_enc_attn (wh_attn.hip).
//
//   GEMM       C = act( LN-fold( sum_k A W ) wscale + bias ) (+ R);  producers also write xb_out = bf16(C - row_shift) and, per (64-column group,
//              row), {sum, sum of squares} of C - row_shift;  k_ln_stats turns those partials into {mean, rstd} and advances the running offset.
//   attention  out[q] = sum_j softmax_j(q . k_j) v_j  per (clip, head), head width 64, keys 0 .. S - 1.
//   LayerNorm  y = (x - mean) rstd w + b, biased variance, eps 1e-5, contiguous or in blocks of in_blk rows placed out_blk rows apart.
//
// The program links libwhisper_hip.so and calls only wh_launch_gemm, wh_launch_gemm8, wh_launch_gemm8x, wh_launch_ln_stats,
// wh_launch_layernorm_blocks and wh_launch_enc_attn: the same source builds against any revision of the library, and two builds that print the same
// hashes computed the same bits.  Through the C ABI the program cannot see which kernel a launch selected; the kernel name it prints is the one the
// launchers' rules give for the case (wh_launch_gemm8: BN = 256 for act == 0 and N >= 256, else BN = 128; wh_launch_gemm with small_ctx: k_gemm on
// 64 x 64 tiles, on 128 x 128 tiles from 192 blocks up; wh_launch_enc_attn: 8 waves in bf16 unless WH_ENC_ATTN_W4=1, read once per process).
//
// Inputs are random (one LCG seed per case) and exact in the mode under test: bf16 rounded on the host, fp16 limb pairs (h2) packed on the host, f32;
// the restatement works in double on those exact values.  Every output buffer is filled with a byte pattern first and everything outside the
// contracted region must come back unchanged: rows >= M, columns in [N, ldc), the rows between blocks (c_bs / out_blk), attention rows >= S, the
// 256 bytes behind each buffer.  A case prints its worst |got - want| / bound (the condition is <= 1) and the hashes; a failing one prints MISMATCH.
//
// Bounds, per output element, from the operands alone (U = 2^-24); nothing in them is fitted to what the kernels give:
//   GEMM accumulator  ((c K + 8) U) sum|a w|, c = 1, or 3 for limb pairs (three MFMA passes per k-step), + 4 U sum|a w| for their dropped lo.lo
//                     term, + 4 U sum|a w| more where the limbs are split from f32 rows at the fragment load (f32_operands);
//   wscale            the bound times |wscale|, + U |s| + U |v| for the scale and the bias add;
//   LN fold           rstd (acc - mean s) + c with {mean, rstd} as given: one U of each intermediate result (p = mean s, t, u = rstd t, v);
//   k_ln_stats        mean and rstd carry the f32 error of their sums (groups + 2 additions), of the E[x^2] - mean^2 difference and of one rsqrt;
//                     the offset one more U;
//   GELU              1.13 (the largest slope) times the bound, + 0.5 |v| (1.5e-7 + 8 U): erf_as's stated error and its f32 evaluation, + 4 U |gelu|;
//   + R, - shift      one U of the result each;
//   output            half an ulp of the stored type: 2^-8 |v| bf16 (2^-9 relative to the binade's top), U |v| f32, 2^-22 |v| + 2^-24 for a limb pair;
//   statistics        the sums of the elements' bounds (2 |u| e + e^2 for the squares) + 12 U of the sums of magnitudes (8 terms per lane, three
//                     cross-lane levels, the square).
//   attention         with w_j = p_j / sum p:  the score error d = (c 64 + 8) U sum|q k| (+ 4 U sum|q k| for limb pairs), the largest over a query's
//                     keys, moves every weight by at most exp(2 d) - 1 relatively;  exp2 and its argument 4 U + 2 U (|s_j| + |max|) per key;  the
//                     rounding of P to the operand type 2^-9 (bf16: half an ulp relative to a binade's top; a single weight at a binade's bottom
//                     can be off by 2^-8, the sum over a row's keys is held to 2^-9 — its largest weight, 1 at the maximum, is exact), 2^-22 (limb pairs), none (f32);  (S + 12) U for the sums, the rescales and the
//                     final division — all applied to sum_j w_j |v_j|; then half an ulp of the output type.
//   LayerNorm         mean: (d / 64 + 8) U sum|x| / d (a lane's terms, six cross-lane levels, the division);  t = x - mean: that + U |t|;  variance:
//                     2 sum|t| e_t / d + (d / 64 + 8) U var;  rstd: rstd (0.5 e_var / (var + eps) + 4 U);  y: |w| (rstd e_t + |t| e_rstd) + 3 U |t rstd w|
//                     + U |y|, + half an ulp of the output type.
//
//   enc_check [gemm8 | gemm8x | gemm | attn | ln]   one group, or all of them
//   enc_check --selftest   host only (no HIP call): for one case of each family the restatement carried out in the kernel's working precision (float
//                          accumulation in natural order, operand roundings in the kernel's places, output rounded to the stored type) must stay
//                          within the bound, and the same with one defect at a time must exceed it on at least one element.
//   enc_check --time       launch times on the whisper-base encoder shapes (bf16), median of 25 windows of 20 launches.
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/enc_check.cpp -o tools/enc_check -Lwhisper-rust-ort_amd -lwhisper_hip -Wl,-rpath,'$ORIGIN/../whisper-rust-ort_amd'
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>
#include "../whisper-rust-ort_amd/csrc/wh_kernels.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(3); } } while (0)

static const double U = 5.9604644775390625e-8;   // 2^-24
static const size_t TAIL = 256;                   // guard bytes behind every buffer
enum Fmt { F_BF16, F_F32, F_H2 };
enum Mode { BF16, F32, H2, X3F };                 // X3F: f32 rows split into fp16 limbs at the fragment load (GemmArgs::f32_operands)
static const char* mode_name[] = {"bf16", "f32 ", "h2  ", "x3f "};
static const char* fmt_name[] = {"bf16", "f32 ", "h2  "};
static bool g_host = false;                       // --selftest: no device, the outputs come from the host emulation

static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }   // RNE (finite inputs)
static unsigned rs = 1;
static unsigned rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static float frand(float a) { return ((int)(rnd() & 0xffff) - 32768) / 32768.0f * a; }
static unsigned long long fnv1a(const void* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}
static size_t esz(Fmt f) { return f == F_BF16 ? 2 : 4; }
// h2 (wh_common.h): 32 consecutive elements take 128 bytes, [32 x fp16 hi | 32 x fp16 lo]
static size_t h2_hi(size_t i) { return (i >> 5) * 128 + (i & 31) * 2; }
static double put(unsigned char* b, Fmt f, size_t i, float v) {   // stores v in format f, returns the value the kernel will see
    if (f == F_BF16) { const unsigned short h = f2bf(v); memcpy(b + 2 * i, &h, 2); return bf2f(h); }
    if (f == F_F32) { memcpy(b + 4 * i, &v, 4); return v; }
    const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi);
    memcpy(b + h2_hi(i), &hi, 2); memcpy(b + h2_hi(i) + 64, &lo, 2);
    return (double)(float)hi + (double)(float)lo;
}
static double get(const unsigned char* b, Fmt f, size_t i) {
    if (f == F_BF16) { unsigned short h; memcpy(&h, b + 2 * i, 2); return bf2f(h); }
    if (f == F_F32) { float v; memcpy(&v, b + 4 * i, 4); return v; }
    _Float16 hi, lo; memcpy(&hi, b + h2_hi(i), 2); memcpy(&lo, b + h2_hi(i) + 64, 2);
    return (double)(float)hi + (double)(float)lo;
}
static float limbs(float v) { const _Float16 hi = (_Float16)v, lo = (_Float16)(v - (float)hi); return (float)hi + (float)lo; }   // the value of v's limb pair
static double half_ulp(Fmt f, double v) { return f == F_BF16 ? ldexp(fabs(v), -8) : f == F_F32 ? U * fabs(v) : ldexp(fabs(v), -22) + ldexp(1.0, -24); }
static Fmt op_fmt(Mode m) { return m == BF16 ? F_BF16 : m == H2 ? F_H2 : F_F32; }
static Fmt out_fmt(Mode m, bool out_f32) { return (out_f32 || m == F32) ? F_F32 : m == BF16 ? F_BF16 : F_H2; }
static int prec_of(Mode m) { return m == BF16 ? WH_PREC_BF16 : m == F32 ? WH_PREC_F32 : WH_PREC_F16X3; }

struct Worst { double ratio = 0; void see(double got, double want, double bound) { const double r = fabs(got - want) <= 1e300 ? fabs(got - want) / bound : 1e30; if (r > ratio) ratio = r; } };

// rows 0 .. n - 1 over at most 16 host threads; f(i) returns the row's worst ratio
template <typename F> static double par_rows(long n, F f) {
    int nt = (int)std::min<long>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), std::max<long>(1, n / 8));
    std::vector<double> worst(nt, 0.0);
    std::atomic<long> next{0};
    auto body = [&](int t) { for (;;) { const long i = next.fetch_add(1); if (i >= n) break; worst[t] = std::max(worst[t], f(i)); } };
    if (nt == 1) body(0);
    else { std::vector<std::thread> th; for (int t = 0; t < nt; t++) th.emplace_back(body, t); for (auto& t : th) t.join(); }
    return *std::max_element(worst.begin(), worst.end());
}

template <typename V> static void* to_dev(const V& v) {   // an input: its bytes, then a zeroed guard tail
    if (g_host) return nullptr;
    void* p; const size_t n = v.size() * sizeof(v[0]);
    CK(hipMalloc(&p, n + TAIL)); CK(hipMemset(p, 0, n + TAIL)); if (n) CK(hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice));
    return p;
}
static void dev_free(std::initializer_list<void*> ps) { for (void* p : ps) if (p) CK(hipFree(p)); }

// an output buffer: filled with a byte pattern, every element the contract writes marked live, everything else (tail included) must come back unchanged
struct Out {
    Fmt f = F_F32; size_t n = 0; std::vector<unsigned char> h0, h, live; void* d = nullptr;
    void make(Fmt f_, size_t n_) {
        f = f_; n = (n_ + 31) / 32 * 32;
        h0.resize(n * esz(f) + TAIL);
        for (size_t i = 0; i < h0.size(); i++) h0[i] = (unsigned char)(0x5a ^ (i * 29u) ^ (i >> 7));
        live.assign(n, 0);
    }
    size_t bytes() const { return n * esz(f); }
    void up() { h = h0; if (!g_host) { CK(hipMalloc(&d, h0.size())); CK(hipMemcpy(d, h0.data(), h0.size(), hipMemcpyHostToDevice)); } }
    void down() { if (!g_host) { CK(hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost)); CK(hipFree(d)); d = nullptr; } }
    double at(size_t i) const { return get(h.data(), f, i); }
    void set(size_t i, float v) { put(h.data(), f, i, v); }
    long guard() const {   // elements outside the contract, or tail bytes, that changed
        long bad = 0;
        for (size_t i = 0; i < n; i++) {
            if (live[i]) continue;
            if (f == F_H2) bad += memcmp(&h[h2_hi(i)], &h0[h2_hi(i)], 2) != 0 || memcmp(&h[h2_hi(i) + 64], &h0[h2_hi(i) + 64], 2) != 0;
            else bad += memcmp(&h[i * esz(f)], &h0[i * esz(f)], esz(f)) != 0;
        }
        return bad + (memcmp(&h[bytes()], &h0[bytes()], TAIL) != 0);
    }
    unsigned long long hash() const { return fnv1a(h.data(), bytes()); }
};

// ===== GEMM ================================================================================================================================
enum Via { V8, V8X, VG, VDISP };   // wh_launch_gemm8, wh_launch_gemm8x, wh_launch_gemm with small_ctx (k_gemm), wh_launch_gemm without (dispatch)
enum GDefect { GD_NONE, GD_KSTEP, GD_BIASROW, GD_LAST4, GD_MPER, GD_STATROW, GD_STATCOL };
struct GC {
    const char* what = ""; Via via = V8; Mode mode = BF16; bool out_f32 = false;
    int M = 256, N = 256, K = 64, act = 0, bias_mode = 1, batch = 1;
    bool wscale = false, a_shared = false;
    int m_per = 1 << 30; long lda = 0, a_bs = 0, ldc = 0, c_bs = 0;   // 0: chosen below
    int n_per = 1 << 30;
    int resid = 0;        // 0 none, 1 a table of its own, 2 in place (R == C), 3 one table shared by the blocks (r_bs == 0)
    int ln_mode = 0; bool producer = false; int shift = 0;   // shift: 0 none, 1 random, 2 rows of mean 25 and spread 1 with the shift equal to the mean
    int st_pad = 5;       // rows of the statistics' pitch behind M
    int defect = GD_NONE;
};
struct GRes { double ratio = 0; long guard = 0; bool launched = true; unsigned long long h[3] = {0, 0, 0}; bool ok() const { return launched && ratio <= 1.0 && guard == 0; } };

static const char* gemm_kernel(const GC& c) {
    if (c.via == V8X) return "k_gemm8x     ";
    if (c.via == V8 || c.via == VDISP) return (c.act == 0 && c.N >= 256) ? "k_gemm8<256> " : "k_gemm8<128> ";
    return (long)((c.M + 127) / 128) * ((c.N + 127) / 128) * c.batch >= 192 ? "k_gemm<128>  " : "k_gemm<64>   ";
}

// the operands of one case, laid out as the kernel addresses them
struct GData {
    GC c; Fmt TA, TC;
    int nblk, mrows; long lda, a_bs, a_zs, ldw, w_zs, ldc, c_bs, c_zs, c_ns, ldr, r_bs, r_zs, st_rows, stat_zs;
    std::vector<double> A, W; std::vector<unsigned char> hA, hW;
    std::vector<float> bias, wsc, R, lns, stat, rsh;
    Out C, XB, ST;
    size_t aidx(int z, int m, int k, bool flat = false) const { return (size_t)z * a_zs + (flat ? (size_t)m * lda : (size_t)(m / c.m_per) * a_bs + (size_t)(m % c.m_per) * lda) + k; }
    size_t widx(int z, int n, int k) const { return (size_t)z * w_zs + (size_t)n * ldw + k; }
    size_t cidx(int z, int m, int n) const { return (size_t)z * c_zs + (size_t)(m / c.m_per) * c_bs + (size_t)(m % c.m_per) * ldc + (size_t)(n / c.n_per) * c_ns + n % c.n_per; }
    size_t ridx(int z, int m, int n) const { return c.resid == 2 ? cidx(z, m, n) : (size_t)z * r_zs + (size_t)(m / c.m_per) * r_bs + (size_t)(m % c.m_per) * ldr + n; }
};

static void gemm_prepare(GData& d, const GC& c, const std::vector<unsigned char>* a_bytes = nullptr, long a_ld = 0, const std::vector<float>* stat_in = nullptr) {
    d.c = c; d.TA = op_fmt(c.mode); d.TC = out_fmt(c.mode, c.out_f32);
    const int M = c.M, N = c.N, K = c.K;
    const bool blocks = c.m_per < M;
    d.nblk = blocks ? (M + c.m_per - 1) / c.m_per : 1; d.mrows = blocks ? c.m_per : M;
    d.lda = a_bytes ? a_ld : c.lda ? c.lda : K + 32;
    d.a_bs = c.a_bs ? c.a_bs : (long)(d.mrows + 1) * d.lda;
    const long a_one = blocks ? d.nblk * d.a_bs : (long)(M - 1) * d.lda + K + 32;
    d.a_zs = c.a_shared ? 0 : (a_one + 31) / 32 * 32;
    d.ldw = K + 32; d.w_zs = (long)N * d.ldw;
    const bool planes = c.n_per < N;
    d.ldc = c.ldc ? c.ldc : planes ? c.n_per : (N / 32 + 1) * 32;
    d.c_bs = c.c_bs ? c.c_bs : (c.producer ? (long)d.mrows : (long)d.mrows + 2) * d.ldc;   // (producers: contiguous rows)
    const long c_rows = blocks ? d.nblk * d.c_bs : (long)(M + 3) * d.ldc;
    d.c_ns = planes ? c_rows + 64 : 0;
    d.c_zs = planes ? (N + c.n_per - 1) / c.n_per * d.c_ns : c_rows;
    rs = 2654435761u * (unsigned)(c.via + 1) + 1000003u * c.mode + 7919u * M + 131u * N + 17u * K + 29u * c.ln_mode + 5u * c.resid + 3u * c.act + c.batch + 64u * c.out_f32 + 977u * c.producer +
         331u * c.shift + 11u * c.bias_mode + 13u * c.wscale + (blocks ? 101u : 0u) + (planes ? 211u : 0u);
    // ---- A, W ----
    const size_t a_el = (size_t)(c.a_shared ? 1 : c.batch) * ((a_one + 31) / 32 * 32), w_el = (size_t)c.batch * d.w_zs;
    d.A.assign(a_el, 0.0); d.W.assign(w_el, 0.0); d.hA.assign(a_el * esz(d.TA), 0); d.hW.assign(w_el * esz(d.TA), 0);
    if (a_bytes) {   // the previous stage's bf16 rows, as they came back
        d.hA = *a_bytes; d.hA.resize(a_el * esz(d.TA), 0); d.A.assign(a_el, 0.0);
        for (int m = 0; m < M; m++) for (int k = 0; k < K; k++) d.A[d.aidx(0, m, k)] = get(d.hA.data(), d.TA, d.aidx(0, m, k));
    } else {
        for (size_t i = 0; i < a_el; i++) { const float v = frand(1.0f); d.A[i] = put(d.hA.data(), d.TA, i, c.mode == X3F ? limbs(v) : v); }
    }
    for (size_t i = 0; i < w_el; i++) { const float v = frand(0.5f); d.W[i] = put(d.hW.data(), d.TA, i, c.mode == X3F ? limbs(v) : v); }
    // ---- epilogue operands ----
    const int nb = c.bias_mode == 2 ? M : N;
    d.bias.resize(nb); d.wsc.resize(nb); d.lns.resize(c.ln_mode == 2 ? M : N); d.rsh.resize(M);
    for (auto& v : d.bias) v = frand(0.5f);
    for (auto& v : d.wsc) v = 0.25f + fabsf(frand(1.0f));
    for (auto& v : d.lns) v = frand(1.0f);
    for (auto& v : d.rsh) v = c.shift == 2 ? 25.0f : frand(0.3f);
    d.stat_zs = 2 * (long)N;
    if (stat_in) d.stat = *stat_in;
    else if (c.ln_mode) {
        d.stat.resize(c.ln_mode == 1 ? 2 * (size_t)M : (size_t)c.batch * d.stat_zs);
        for (size_t i = 0; i < d.stat.size(); i += 2) { d.stat[i] = frand(0.5f); d.stat[i + 1] = 0.5f + fabsf(frand(2.0f)); }
    }
    // ---- outputs ----
    d.C.make(d.TC, (size_t)c.batch * d.c_zs);
    d.XB.make(F_BF16, c.producer ? (size_t)d.c_zs : 0);
    d.st_rows = M + c.st_pad;
    d.ST.make(F_F32, c.producer ? (size_t)(N / 64) * d.st_rows * 2 : 0);
    for (int z = 0; z < c.batch; z++) for (int m = 0; m < M; m++) for (int n = 0; n < N; n++) d.C.live[d.cidx(z, m, n)] = 1;
    if (c.producer) {
        for (int m = 0; m < M; m++) for (int n = 0; n < N; n++) d.XB.live[d.cidx(0, m, n)] = 1;
        for (int g = 0; g < N / 64; g++) for (int m = 0; m < M; m++) d.ST.live[((size_t)g * d.st_rows + m) * 2] = d.ST.live[((size_t)g * d.st_rows + m) * 2 + 1] = 1;
    }
    // ---- residual ----
    d.ldr = c.resid == 2 ? d.ldc : N + 4; d.r_bs = c.resid == 2 ? d.c_bs : c.resid == 3 ? 0 : (long)(d.mrows + 1) * d.ldr;
    d.r_zs = c.resid == 2 ? d.c_zs : c.resid == 3 ? 0 : (blocks ? d.nblk * d.r_bs : (long)M * d.ldr);
    if (c.resid == 2) {   // in place: the residual rows are C's own contents
        d.R.assign(d.C.n, 0.0f);
        for (int z = 0; z < c.batch; z++) for (int m = 0; m < M; m++) for (int n = 0; n < N; n++) {
            const float v = (c.shift == 2 ? 25.0f : 0.0f) + frand(1.0f);
            d.R[d.cidx(z, m, n)] = v; put(d.C.h0.data(), F_F32, d.cidx(z, m, n), v);
        }
    } else if (c.resid) {
        d.R.resize(c.resid == 3 ? (size_t)d.mrows * d.ldr : (size_t)c.batch * d.r_zs);
        for (auto& v : d.R) v = (c.shift == 2 ? 25.0f : 0.0f) + frand(1.0f);
    }
}

// the device's answer
static bool gemm_launch(GData& d) {
    const GC& c = d.c;
    void *dA = to_dev(d.hA), *dW = to_dev(d.hW), *db = to_dev(d.bias), *dws = to_dev(d.wsc), *dR = c.resid && c.resid != 2 ? to_dev(d.R) : nullptr, *dls = to_dev(d.lns),
         *dst = to_dev(d.stat), *dsh = to_dev(d.rsh);
    d.C.up(); d.XB.up(); d.ST.up();
    GemmArgs g;
    g.A = dA; g.lda = d.lda; g.a_bs = d.a_bs; g.a_zs = d.a_zs; g.W = dW; g.ldw = d.ldw; g.w_zs = d.w_zs;
    g.C = d.C.d; g.ldc = d.ldc; g.c_bs = d.c_bs; g.c_zs = d.c_zs;
    g.bias = (const float*)db; g.bias_mode = c.bias_mode;
    if (c.wscale) g.wscale = (const float*)dws;
    if (c.resid) { g.R = c.resid == 2 ? (const float*)d.C.d : (const float*)dR; g.ldr = d.ldr; g.r_bs = d.r_bs; g.r_zs = d.r_zs; }
    g.act = c.act; g.M = c.M; g.N = c.N; g.K = c.K; g.m_per = c.m_per; g.n_per = c.n_per; g.c_ns = d.c_ns; g.batch = c.batch;
    g.small_ctx = c.via == VG; g.f32_operands = c.mode == X3F;
    if (c.ln_mode) { g.ln_mode = c.ln_mode; g.ln_stat = (const float*)dst; g.ln_stat_zs = d.stat_zs; g.ln_s = (const float*)dls; }
    if (c.producer) { g.xb_out = d.XB.d; g.stats_out = (float*)d.ST.d; g.stats_rows = d.st_rows; if (c.shift) g.row_shift = (const float*)dsh; }
    const bool f32o = d.TC == F_F32;
    const int rc = c.via == V8 ? wh_launch_gemm8(0, f32o, g) : c.via == V8X ? wh_launch_gemm8x(0, !f32o, g) : wh_launch_gemm(0, prec_of(c.mode), f32o, g);
    if (rc == WH_OK) { CK(hipGetLastError()); CK(hipDeviceSynchronize()); }
    d.C.down(); d.XB.down(); d.ST.down();
    dev_free({dA, dW, db, dws, dR, dls, dst, dsh});
    return rc == WH_OK;
}

// the same contract carried out in the kernel's working precision on the host (float accumulation over k in natural order, f32 epilogue, outputs
// rounded to the stored type), with one defect if asked
static void gemm_emulate(GData& d) {
    const GC& c = d.c;
    d.C.up(); d.XB.up(); d.ST.up();
    const int Kuse = c.defect == GD_KSTEP ? c.K - 32 : c.K;
    for (int z = 0; z < c.batch; z++) for (int m = 0; m < c.M; m++) {
        std::vector<float> s1(c.N / 64 + 1, 0.0f), s2(c.N / 64 + 1, 0.0f);
        for (int n = 0; n < c.N; n++) {
            if (c.defect == GD_LAST4 && n >= c.N - 4) continue;
            float acc = 0.0f;
            for (int k = 0; k < Kuse; k++) acc += (float)d.A[d.aidx(z, m, k, c.defect == GD_MPER) % d.A.size()] * (float)d.W[d.widx(z, n, k)];
            float v;
            if (c.ln_mode == 1) { const int ms = c.defect == GD_STATROW ? (m + 1) % c.M : m; v = d.stat[2 * ms + 1] * (acc - d.stat[2 * ms] * d.lns[n]) + d.bias[n]; }
            else if (c.ln_mode == 2) v = d.stat[z * d.stat_zs + 2 * n + 1] * (acc - d.stat[z * d.stat_zs + 2 * n] * d.lns[m]) + d.bias[m];
            else {
                const int bi = c.bias_mode == 2 ? m : c.defect == GD_BIASROW ? m % c.N : n;
                v = acc * (c.wscale ? d.wsc[c.bias_mode == 2 ? m : n] : 1.0f) + d.bias[bi];
            }
            if (c.act == 1) v = 0.5f * v * (1.0f + erff(v * 0.70710678f));
            if (c.resid) v += d.R[d.ridx(z, m, n)];
            d.C.set(d.cidx(z, m, n), v);
            if (c.producer) {
                const float u = v - (c.shift ? d.rsh[m] : 0.0f);
                d.XB.set(d.cidx(0, m, n), u);
                if (!(c.defect == GD_STATCOL && n % 64 == 63)) { s1[n / 64] += u; s2[n / 64] += u * u; }
            }
        }
        if (c.producer) for (int g = 0; g < c.N / 64; g++) { d.ST.set(((size_t)g * d.st_rows + m) * 2, s1[g]); d.ST.set(((size_t)g * d.st_rows + m) * 2 + 1, s2[g]); }
    }
}

// the restatement in double and the bound, element by element
static GRes gemm_verify(const GData& d) {
    const GC& c = d.c;
    const int M = c.M, N = c.N, K = c.K;
    const bool limb = c.mode == H2 || c.mode == X3F;
    GRes r;
    r.ratio = par_rows((long)c.batch * M, [&](long zm) {
        const int z = (int)(zm / M), m = (int)(zm % M);
        Worst w;
        std::vector<double> s1w(N / 64 + 1, 0.0), s1b(N / 64 + 1, 0.0), s2w(N / 64 + 1, 0.0), s2b(N / 64 + 1, 0.0), m1(N / 64 + 1, 0.0), m2(N / 64 + 1, 0.0);
        const double* a = &d.A[d.aidx(z, m, 0)];
        for (int n = 0; n < N; n++) {
            const double* wr = &d.W[d.widx(z, n, 0)];
            double acc = 0, S = 0;
            for (int k = 0; k < K; k++) { acc += a[k] * wr[k]; S += fabs(a[k] * wr[k]); }
            double e = ((limb ? 3.0 : 1.0) * K + 8) * U * S + (limb ? 4 * U * S : 0.0) + (c.mode == X3F ? 4 * U * S : 0.0), v;
            if (c.ln_mode) {
                const double mean = c.ln_mode == 1 ? d.stat[2 * m] : d.stat[z * d.stat_zs + 2 * n], rstd = c.ln_mode == 1 ? d.stat[2 * m + 1] : d.stat[z * d.stat_zs + 2 * n + 1];
                const double s = c.ln_mode == 1 ? d.lns[n] : d.lns[m], b = c.ln_mode == 1 ? d.bias[n] : d.bias[m];
                const double p = mean * s, t = acc - p, u = rstd * t;
                v = u + b;
                e = fabs(rstd) * (e + U * fabs(p) + U * fabs(t)) + U * fabs(u) + U * fabs(v);
            } else {
                const double ws = c.wscale ? d.wsc[c.bias_mode == 2 ? m : n] : 1.0, s = acc * ws;
                v = s + d.bias[c.bias_mode == 2 ? m : n];
                e = e * fabs(ws) + (c.wscale ? U * fabs(s) : 0.0) + U * fabs(v);
            }
            if (c.act == 1) { const double g = 0.5 * v * (1.0 + erf(v * 0.70710678118654752440)); e = 1.13 * e + 0.5 * fabs(v) * (1.5e-7 + 8 * U) + 4 * U * fabs(g); v = g; }
            if (c.resid) { v += d.R[d.ridx(z, m, n)]; e += U * fabs(v); }
            w.see(d.C.at(d.cidx(z, m, n)), v, e + half_ulp(d.TC, fabs(v) + e));
            if (c.producer) {
                const double u = v - (c.shift ? d.rsh[m] : 0.0), eu = e + U * fabs(v) + (c.shift ? U * fabs(u) : 0.0);   // (the kernel starts from the stored f32 value of C)
                w.see(d.XB.at(d.cidx(0, m, n)), u, eu + half_ulp(F_BF16, fabs(u) + eu));
                const int g = n / 64;
                s1w[g] += u; s1b[g] += eu; m1[g] += fabs(u); s2w[g] += u * u; s2b[g] += 2 * fabs(u) * eu + eu * eu; m2[g] += u * u;
            }
        }
        if (c.producer) for (int g = 0; g < N / 64; g++) {
            w.see(d.ST.at(((size_t)g * d.st_rows + m) * 2), s1w[g], s1b[g] + 12 * U * m1[g]);
            w.see(d.ST.at(((size_t)g * d.st_rows + m) * 2 + 1), s2w[g], s2b[g] + 12 * U * m2[g]);
        }
        return w.ratio;
    });
    r.guard = d.C.guard() + d.XB.guard() + d.ST.guard();
    r.h[0] = d.C.hash(); r.h[1] = d.XB.hash(); r.h[2] = d.ST.hash();
    return r;
}

static double worst_gemm = 0;
static int gemm_report(const GData& d, const GRes& r, const char* tag = "") {
    const GC& c = d.c;
    printf("%s %s->%s %-26s M %4d N %4d K %3d z %d act %d bias %d ln %d%s%s%s%s: err/bound %.3f guard %ld  C %016llx xb %016llx stats %016llx  %s%s\n", gemm_kernel(c), mode_name[c.mode],
           fmt_name[d.TC], c.what, c.M, c.N, c.K, c.batch, c.act, c.bias_mode, c.ln_mode, c.wscale ? " wscale" : "", c.resid ? (c.resid == 2 ? " R=C" : c.resid == 3 ? " R shared" : " R") : "",
           c.producer ? " producer" : "", c.shift == 2 ? " mean25" : c.shift ? " shift" : "", r.ratio, r.guard, r.h[0], r.h[1], r.h[2],
           !r.launched ? "launcher refused: MISMATCH" : r.ok() ? "ok" : "MISMATCH", tag);
    worst_gemm = std::max(worst_gemm, r.ratio);
    return r.ok() ? 0 : 1;
}
static int gemm_case(const GC& c) {
    GData d; gemm_prepare(d, c);
    const bool launched = gemm_launch(d);
    GRes r = gemm_verify(d); r.launched = launched;
    return gemm_report(d, r);
}

// k_ln_stats: stat[r] = {mean, rstd} from partials [groups][rows][2], shift[r] += mean (in place)
static int ln_stats_check(const std::vector<unsigned char>& part_bytes, int groups, long rows, long st_rows, std::vector<float>& stat, std::vector<float>& shift, const char* what) {
    // the producer wrote its partials with a pitch of st_rows; k_ln_stats takes `rows` as the pitch, so it runs over all st_rows rows' slots and the
    // check looks at the first `rows` of them (the others hold the fill pattern)
    const int d = 64 * groups;
    std::vector<float> part(part_bytes.size() / 4); memcpy(part.data(), part_bytes.data(), part.size() * 4);
    for (long r = rows; r < st_rows; r++) for (int g = 0; g < groups; g++) part[((size_t)g * st_rows + r) * 2] = part[((size_t)g * st_rows + r) * 2 + 1] = 0.0f;
    part.resize((size_t)groups * st_rows * 2);
    Out ST, SH; ST.make(F_F32, (size_t)(st_rows + 3) * 2); SH.make(F_F32, (size_t)st_rows + 3);
    for (long r = 0; r < st_rows; r++) { ST.live[2 * r] = ST.live[2 * r + 1] = SH.live[r] = 1; put(SH.h0.data(), F_F32, r, r < rows ? shift[r] : 0.0f); }
    void* dp = to_dev(part);
    ST.up(); SH.up();
    wh_launch_ln_stats(0, (const float*)dp, groups, st_rows, d, (float*)ST.d, (float*)SH.d, (const float*)SH.d);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    ST.down(); SH.down(); dev_free({dp});
    Worst w;
    for (long r = 0; r < rows; r++) {
        double s1 = 0, s2 = 0, a1 = 0;
        for (int g = 0; g < groups; g++) { s1 += part[((size_t)g * st_rows + r) * 2]; a1 += fabs(part[((size_t)g * st_rows + r) * 2]); s2 += part[((size_t)g * st_rows + r) * 2 + 1]; }
        const double mean = s1 / d, ex2 = s2 / d, var = ex2 - mean * mean, tl = (groups + 2) * U;
        const double emean = tl * a1 / d + U * fabs(mean), evar = tl * ex2 + 2 * fabs(mean) * emean + 3 * U * (ex2 + mean * mean);
        const double rstd = 1.0 / sqrt(fmax(var, 0.0) + 1e-5), erstd = rstd * (0.5 * evar / (fmax(var, 0.0) + 1e-5) + 4 * U);
        w.see(ST.at(2 * r), mean, emean);
        w.see(ST.at(2 * r + 1), rstd, erstd);
        w.see(SH.at(r), shift[r] + mean, emean + U * fabs(shift[r] + mean));
    }
    const long guard = ST.guard() + SH.guard();
    const bool ok = w.ratio <= 1.0 && guard == 0;
    printf("k_ln_stats    f32  %-26s rows %4ld groups %d d %4d: err/bound %.3f guard %ld  stat %016llx shift %016llx  %s\n", what, rows, groups, d, w.ratio, guard, ST.hash(), SH.hash(),
           ok ? "ok" : "MISMATCH");
    worst_gemm = std::max(worst_gemm, w.ratio);
    stat.resize(2 * rows); shift.resize(rows);
    for (long r = 0; r < rows; r++) { stat[2 * r] = (float)ST.at(2 * r); stat[2 * r + 1] = (float)ST.at(2 * r + 1); shift[r] = (float)SH.at(r); }
    return ok ? 0 : 1;
}

// producer -> k_ln_stats -> consumer, every stage checked on the bits the stage before it wrote
static int chain_case(int groups) {
    int bad = 0;
    GC p; p.what = "chain: producer"; p.out_f32 = true; p.M = 300; p.N = 64 * groups; p.K = 64; p.resid = 2; p.producer = true; p.shift = 1; p.st_pad = 0;
    GData dp; gemm_prepare(dp, p);
    const bool launched = gemm_launch(dp);
    GRes r = gemm_verify(dp); r.launched = launched;
    bad |= gemm_report(dp, r);
    std::vector<float> stat, shift = dp.rsh;
    bad |= ln_stats_check(dp.ST.h, groups, p.M, dp.st_rows, stat, shift, "chain: statistics");
    GC q; q.what = "chain: consumer"; q.M = 300; q.N = 140; q.K = 64 * groups; q.act = 1; q.ln_mode = 1;
    GData dq; gemm_prepare(dq, q, &dp.XB.h, dp.ldc, &stat);
    const bool l2 = gemm_launch(dq);
    GRes r2 = gemm_verify(dq); r2.launched = l2;
    bad |= gemm_report(dq, r2);
    return bad;
}

static GC conv_case(Via via, Mode mode, bool out_f32, int N, int act) {
    GC c; c.what = "conv rows, R shared"; c.via = via; c.mode = mode; c.out_f32 = out_f32; c.M = 296; c.N = N; c.K = 192; c.act = act; c.m_per = 148; c.lda = 64; c.a_bs = 151 * 64;
    c.resid = 3;
    return c;
}

static int group_gemm8() {
    int bad = 0;
    for (bool f : {false, true}) {
        GC c; c.out_f32 = f;
        { GC t = c; t.what = "one tile, one k-step"; t.N = 128; t.K = 32; bad |= gemm_case(t); }
        for (int K : {64, 96, 128, 160}) {
            { GC t = c; t.what = "ring, 4 slots"; t.K = K; bad |= gemm_case(t); }
            { GC t = c; t.what = "ring, 3 slots"; t.K = K; t.N = 128; t.act = 1; bad |= gemm_case(t); }
        }
        { GC t = c; t.what = "cut row tile"; t.M = 300; bad |= gemm_case(t); }
        { GC t = c; t.what = "cut row tile"; t.M = 300; t.N = 128; t.act = 1; bad |= gemm_case(t); }
        { GC t = c; t.what = "cut column tile 8 + 4"; t.N = 268; bad |= gemm_case(t); }
        { GC t = c; t.what = "cut column tile 8 + 4"; t.N = 140; t.act = 1; bad |= gemm_case(t); }
        { GC t = c; t.what = "V^T tail 220"; t.N = 1500; t.batch = 2; t.bias_mode = 2; t.a_shared = true; t.ldc = 1536; bad |= gemm_case(t); }
        bad |= gemm_case(conv_case(V8, BF16, f, 140, 1));
        bad |= gemm_case(conv_case(V8, BF16, f, 268, 0));
        { GC t = c; t.what = "column planes of 64"; t.n_per = 64; bad |= gemm_case(t); }
        for (int bm : {1, 2}) { GC t = c; t.what = "channel scale"; t.M = 300; t.N = 268; t.bias_mode = bm; t.wscale = true; bad |= gemm_case(t); }
        { GC t = c; t.what = "channel scale"; t.N = 140; t.act = 1; t.wscale = true; bad |= gemm_case(t); }
    }
    { GC t; t.what = "in-place residual"; t.out_f32 = true; t.M = 300; t.resid = 2; bad |= gemm_case(t); }
    { GC t; t.what = "in-place residual"; t.out_f32 = true; t.M = 300; t.N = 140; t.act = 1; t.resid = 2; bad |= gemm_case(t); }
    const int tiles[5][2] = {{256, 256}, {256, 768}, {512, 1024}, {768, 768}, {1280, 1024}};   // 1, 3, 8, 9, 20 tiles of 256 x 256
    for (auto& t2 : tiles) { GC t; t.what = "tile order"; t.M = t2[0]; t.N = t2[1]; t.K = 32; bad |= gemm_case(t); }
    { GC t; t.what = "tile order, 6 of 128"; t.M = 512; t.N = 384; t.K = 32; t.act = 1; bad |= gemm_case(t); }
    for (int N : {128, 140, 256, 268}) { GC t; t.what = "LN consumer, row stats"; t.M = 300; t.N = N; t.act = N < 256; t.ln_mode = 1; bad |= gemm_case(t); }
    for (int N : {140, 268}) { GC t; t.what = "LN consumer, column stats"; t.N = N; t.batch = 2; t.bias_mode = 2; t.a_shared = true; t.ln_mode = 2; bad |= gemm_case(t); }
    for (int N : {128, 320}) for (int sh : {0, 1}) { GC t; t.what = "LN producer"; t.out_f32 = true; t.M = 300; t.N = N; t.resid = 2; t.producer = true; t.shift = sh; bad |= gemm_case(t); }
    { GC t; t.what = "LN producer"; t.out_f32 = true; t.M = 300; t.N = 320; t.resid = 2; t.producer = true; t.shift = 2; bad |= gemm_case(t); }
    { GC t; t.what = "LN producer, blocks"; t.out_f32 = true; t.M = 296; t.m_per = 148; t.N = 128; t.resid = 1; t.producer = true; t.shift = 1; bad |= gemm_case(t); }
    for (int g : {2, 5, 9}) bad |= chain_case(g);
    { GC t; t.what = "through wh_launch_gemm"; t.via = VDISP; t.M = 300; t.N = 268; bad |= gemm_case(t); }
    printf("worst err/bound gemm8 %.3f\n", worst_gemm);
    return bad;
}

static int group_gemm8x() {
    int bad = 0;
    worst_gemm = 0;
    for (bool f : {false, true}) {
        GC c; c.via = V8X; c.mode = H2; c.out_f32 = f;
        { GC t = c; t.what = "one tile, one k-step"; t.K = 32; bad |= gemm_case(t); }
        for (int K : {64, 96}) { GC t = c; t.what = "ring, 2 slots"; t.K = K; bad |= gemm_case(t); }   // the ring of wh_gemm8x.hip has two slots: both in use from K = 64, reused from 96
        { GC t = c; t.what = "cut row tile"; t.M = 300; bad |= gemm_case(t); }
        { GC t = c; t.what = "cut column tile 8 + 4"; t.N = 268; bad |= gemm_case(t); }
        { GC t = c; t.what = "cut column tile 8 + 4"; t.N = 140; t.act = 1; bad |= gemm_case(t); }
        { GC t = c; t.what = "V^T tail 220"; t.N = 1500; t.batch = 2; t.bias_mode = 2; t.a_shared = true; t.ldc = 1536; bad |= gemm_case(t); }
        bad |= gemm_case(conv_case(V8X, H2, f, 140, 1));
        bad |= gemm_case(conv_case(V8X, H2, f, 268, 0));
        { GC t = c; t.what = "column planes of 64"; t.n_per = 64; bad |= gemm_case(t); }
    }
    { GC t; t.via = V8X; t.mode = H2; t.what = "in-place residual"; t.out_f32 = true; t.M = 300; t.resid = 2; bad |= gemm_case(t); }
    const int tiles[5][2] = {{256, 256}, {256, 768}, {512, 1024}, {768, 768}, {1280, 1024}};
    for (auto& t2 : tiles) { GC t; t.via = V8X; t.mode = H2; t.what = "tile order"; t.M = t2[0]; t.N = t2[1]; t.K = 32; bad |= gemm_case(t); }
    printf("worst err/bound gemm8x %.3f\n", worst_gemm);
    return bad;
}

static int group_gemm() {
    int bad = 0;
    worst_gemm = 0;
    const struct { Mode m; bool f32; } types[] = {{BF16, false}, {BF16, true}, {F32, true}, {H2, false}, {H2, true}, {X3F, true}, {X3F, false}};
    for (auto& ty : types) {
        const int bk = ty.m == BF16 ? 64 : 32;
        GC c; c.via = VG; c.mode = ty.m; c.out_f32 = ty.f32;
        for (int ks : {1, 3}) { GC t = c; t.what = "cut tiles"; t.M = 70; t.N = 72; t.K = ks * bk; bad |= gemm_case(t); }
        { GC t = c; t.what = "cut tiles, GELU, R"; t.M = 300; t.N = 140; t.act = 1; t.resid = 1; bad |= gemm_case(t); }
        { GC t = c; t.what = "per-row bias, batch"; t.M = 70; t.N = 140; t.batch = 2; t.bias_mode = 2; t.a_shared = true; bad |= gemm_case(t); }
        bad |= gemm_case(conv_case(VG, ty.m, ty.f32, 140, 1));
        { GC t = c; t.what = "128 x 128 tiles"; t.M = 2048; t.N = 1536; bad |= gemm_case(t); }
        { GC t = c; t.what = "128 x 128 tiles, cut"; t.M = 2000; t.N = 1540; t.K = bk; t.resid = ty.f32 ? 2 : 1; bad |= gemm_case(t); }
    }
    printf("worst err/bound gemm %.3f\n", worst_gemm);
    return bad;
}

// ===== attention ===========================================================================================================================
enum ADefect { AD_NONE, AD_UNMASK, AD_NORESCALE, AD_VSWAP, AD_LANESUM };
struct AC { Mode mode = BF16; int S = 64, heads = 1, clips = 1; int peaked = 0, extra_ld = 0, defect = AD_NONE; };
struct AData {
    AC c; Fmt T; int d, ldv; std::vector<double> qk, vT; std::vector<unsigned char> hqk, hvT; Out O;
    size_t qi(int clip, int s, int col) const { return ((size_t)clip * c.S + s) * 2 * d + col; }
    size_t vi(int clip, int row, int key) const { return ((size_t)clip * d + row) * ldv + key; }
    size_t oi(int clip, int s, int col) const { return ((size_t)clip * c.S + s) * d + col; }
};
static void attn_prepare(AData& a, const AC& c) {
    a.c = c; a.T = op_fmt(c.mode); a.d = 64 * c.heads; a.ldv = (c.S + 63) / 64 * 64 + c.extra_ld;
    const int S = c.S, d = a.d;
    rs = 40503u * S + 977u * c.heads + 131u * c.clips + 7u * c.mode + 3u * c.peaked + c.extra_ld;
    a.qk.assign((size_t)c.clips * S * 2 * d, 0.0); a.hqk.assign(a.qk.size() * esz(a.T), 0);
    a.vT.assign((size_t)c.clips * d * a.ldv, 0.0); a.hvT.assign(a.vT.size() * esz(a.T), 0);
    for (int cl = 0; cl < c.clips; cl++) {
        for (int s = 0; s < S; s++) for (int j = 0; j < d; j++) a.qk[a.qi(cl, s, d + j)] = put(a.hqk.data(), a.T, a.qi(cl, s, d + j), frand(1.0f));      // keys
        for (int r = 0; r < d; r++) for (int s = 0; s < a.ldv; s++) a.vT[a.vi(cl, r, s)] = put(a.hvT.data(), a.T, a.vi(cl, r, s), s < S ? frand(1.0f) : 0.0f);   // zero beyond S
        const int last0 = (S - 1) / 64 * 64;
        for (int h = 0; h < c.heads; h++) for (int s = 0; s < S; s++) {
            // peaked: the query is its winning key scaled so that their score is 30; a third of the winners in the first key tile, a third in the
            // last one (every other of those is key S - 1), a third anywhere
            const int win = s % 3 == 0 ? (int)(rnd() % std::min(64, S)) : s % 3 == 1 ? ((s / 3) % 2 ? S - 1 : last0 + (int)(rnd() % (S - last0))) : (int)(rnd() % S);
            double n2 = 0;
            for (int e = 0; e < 64; e++) n2 += a.qk[a.qi(cl, win, d + 64 * h + e)] * a.qk[a.qi(cl, win, d + 64 * h + e)];
            for (int e = 0; e < 64; e++) {
                const float v = c.peaked ? (float)(a.qk[a.qi(cl, win, d + 64 * h + e)] * 30.0 / n2) : frand(0.25f);
                a.qk[a.qi(cl, s, 64 * h + e)] = put(a.hqk.data(), a.T, a.qi(cl, s, 64 * h + e), v);
            }
        }
    }
    a.O.make(a.T, ((size_t)c.clips * S + 4) * d);   // four rows behind the last clip's S
    for (size_t i = 0; i < (size_t)c.clips * S * d; i++) a.O.live[i] = 1;
}
static void attn_launch(AData& a) {
    void *dq = to_dev(a.hqk), *dv = to_dev(a.hvT);
    a.O.up();
    wh_launch_enc_attn(0, prec_of(a.c.mode), dq, dv, a.O.d, a.c.clips, a.c.S, a.d, a.c.heads, a.ldv);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    a.O.down(); dev_free({dq, dv});
}
static float round_p(Mode m, float p) { return m == BF16 ? bf2f(f2bf(p)) : m == H2 ? limbs(p) : p; }
// the kernel's tile walk in float on the host: 64-key tiles, the last one masked, online maximum, the row sum kept per lane group (key % 16 / 4)
static void attn_emulate(AData& a) {
    const AC& c = a.c;
    const int S = c.S, d = a.d, nt = (S + 63) / 64;
    const float L = 1.44269504088896341f;
    a.O.up();
    for (int cl = 0; cl < c.clips; cl++) for (int h = 0; h < c.heads; h++) for (int q = 0; q < S; q++) {
        float mrow = -INFINITY, l[4] = {0, 0, 0, 0}, o[64] = {0};
        for (int it = 0; it < nt; it++) {
            const int k0 = it * 64;
            float sc[64], mx = -INFINITY;
            for (int kk = 0; kk < 64; kk++) {
                const int key = std::min(k0 + kk, S - 1);
                float s = 0.0f;
                for (int e = 0; e < 64; e++) s += (float)a.qk[a.qi(cl, q, 64 * h + e)] * (float)a.qk[a.qi(cl, key, d + 64 * h + e)];
                if (k0 + kk >= S && c.defect != AD_UNMASK) s = -INFINITY;
                sc[kk] = s; mx = fmaxf(mx, s);
            }
            const float mn = fmaxf(mrow, mx);
            float alpha = exp2f((mrow - mn) * L);
            if (c.defect == AD_NORESCALE && it > 0 && mx > mrow) alpha = 1.0f;
            float gs[4] = {0, 0, 0, 0}, p[64];
            for (int kk = 0; kk < 64; kk++) { p[kk] = exp2f(sc[kk] * L - mn * L); gs[(kk % 16) / 4] += p[kk]; }
            for (int g = 0; g < 4; g++) l[g] = l[g] * alpha + gs[g];
            for (int e = 0; e < 64; e++) {
                float acc = o[e] * alpha;
                for (int kk = 0; kk < 64; kk++) {
                    int kv = kk;
                    if (c.defect == AD_VSWAP) { const int r = kk % 32; kv = r >= 4 && r < 8 ? kk + 12 : r >= 16 && r < 20 ? kk - 12 : kk; }
                    acc += round_p(c.mode, p[kk]) * (float)a.vT[a.vi(cl, 64 * h + e, k0 + kv)];
                }
                o[e] = acc;
            }
            mrow = mn;
        }
        const float lt = (l[0] + (c.defect == AD_LANESUM ? 0.0f : l[1])) + (l[2] + l[3]), inv = 1.0f / lt;
        for (int e = 0; e < 64; e++) a.O.set(a.oi(cl, q, 64 * h + e), o[e] * inv);
    }
}
struct ARes { double ratio = 0; long guard = 0; unsigned long long h = 0; bool ok() const { return ratio <= 1.0 && guard == 0; } };
static ARes attn_verify(const AData& a) {
    const AC& c = a.c;
    const int S = c.S, d = a.d;
    const bool limb = c.mode == H2;
    const double rp = c.mode == BF16 ? ldexp(1.0, -9) : limb ? ldexp(1.0, -22) : 0.0;
    ARes r;
    r.ratio = par_rows((long)c.clips * c.heads * S, [&](long i) {
        const int q = (int)(i % S), h = (int)(i / S % c.heads), cl = (int)(i / S / c.heads);
        std::vector<double> s(S), p(S);
        double mx = -1e300, dmax = 0;
        const double* qp = &a.qk[a.qi(cl, q, 64 * h)];
        for (int j = 0; j < S; j++) {
            const double* kp = &a.qk[a.qi(cl, j, d + 64 * h)];
            double acc = 0, mag = 0;
            for (int e = 0; e < 64; e++) { acc += qp[e] * kp[e]; mag += fabs(qp[e] * kp[e]); }
            s[j] = acc; mx = std::max(mx, acc);
            dmax = std::max(dmax, ((limb ? 3.0 : 1.0) * 64 + 8) * U * mag + (limb ? 4 * U * mag : 0.0));
        }
        double den = 0;
        for (int j = 0; j < S; j++) { p[j] = exp(s[j] - mx); den += p[j]; }
        const double rel = expm1(2 * dmax) + rp + (S + 12) * U;
        Worst w;
        for (int e = 0; e < 64; e++) {
            const double* vp = &a.vT[a.vi(cl, 64 * h + e, 0)];
            double num = 0, mag = 0, ex = 0;
            for (int j = 0; j < S; j++) { num += p[j] * vp[j]; mag += p[j] * fabs(vp[j]); ex += p[j] * fabs(vp[j]) * (4 * U + 2 * U * (fabs(s[j]) + fabs(mx))); }
            const double v = num / den, eb = (rel * mag + ex) / den;
            w.see(a.O.at(a.oi(cl, q, 64 * h + e)), v, eb + half_ulp(a.T, fabs(v) + eb));
        }
        return w.ratio;
    });
    r.guard = a.O.guard(); r.h = a.O.hash();
    return r;
}
static double worst_attn = 0;
static int attn_report(const AData& a, const ARes& r, const char* kern) {
    printf("%s %s S %4d heads %d clips %d ldv %4d %s: err/bound %.3f guard %ld  out %016llx  %s\n", kern, mode_name[a.c.mode], a.c.S, a.c.heads, a.c.clips, a.ldv,
           a.c.peaked ? "peaked" : "small ", r.ratio, r.guard, r.h, r.ok() ? "ok" : "MISMATCH");
    worst_attn = std::max(worst_attn, r.ratio);
    return r.ok() ? 0 : 1;
}
static int group_attn() {
    int bad = 0;
    const bool w4 = getenv("WH_ENC_ATTN_W4") != nullptr && atoi(getenv("WH_ENC_ATTN_W4")) != 0;
    const int shapes[6][3] = {{64, 1, 1}, {100, 3, 1}, {128, 1, 1}, {192, 1, 1}, {257, 2, 4}, {1500, 2, 1}};
    for (Mode md : {BF16, F32, H2}) {
        if (w4 && md != BF16) continue;   // the switch only changes the bf16 launch
        const char* kern = md == BF16 ? (w4 ? "k_enc_attn<bf16, 4>" : "k_enc_attn<bf16, 8>") : md == F32 ? "k_enc_attn<f32, 4> " : "k_enc_attn<h2, 4>  ";
        for (auto& sh : shapes) for (int pk : {0, 1}) {
            AC c; c.mode = md; c.S = sh[0]; c.heads = sh[1]; c.clips = sh[2]; c.peaked = pk;
            AData a; attn_prepare(a, c); attn_launch(a);
            bad |= attn_report(a, attn_verify(a), kern);
        }
        AC c; c.mode = md; c.S = 100; c.heads = 3; c.peaked = 1; c.extra_ld = 64;   // 64 more columns of V^T pitch
        AData a; attn_prepare(a, c); attn_launch(a);
        bad |= attn_report(a, attn_verify(a), kern);
    }
    printf("worst err/bound attn %.3f\n", worst_attn);
    return bad;
}

// ===== LayerNorm ===========================================================================================================================
enum LDefect { LD_NONE, LD_EX2, LD_PAIR };
struct LC { Mode mode = BF16; long rows = 1; int d = 512, in_blk = 0, out_blk = 0; bool mean25 = false; int defect = LD_NONE; };
struct LData {
    LC c; Fmt T; std::vector<float> x, w, b; Out Y;
    size_t orow(long r) const { return c.in_blk > 0 ? (size_t)(r / c.in_blk) * c.out_blk + r % c.in_blk : (size_t)r; }
};
static void ln_prepare(LData& l, const LC& c) {
    l.c = c; l.T = op_fmt(c.mode);
    rs = 69069u * (unsigned)c.rows + 31u * c.d + 7u * c.mode + 3u * c.in_blk + c.mean25;
    l.x.resize((size_t)c.rows * c.d); l.w.resize(c.d); l.b.resize(c.d);
    for (auto& v : l.x) v = c.mean25 ? 25.0f + frand(1.0f) : frand(2.0f);
    for (auto& v : l.w) v = 0.5f + frand(0.5f);
    for (auto& v : l.b) v = frand(0.5f);
    const size_t out_rows = (c.in_blk > 0 ? (size_t)((c.rows + c.in_blk - 1) / c.in_blk) * c.out_blk : (size_t)c.rows) + 2;
    l.Y.make(l.T, out_rows * c.d);
    for (long r = 0; r < c.rows; r++) for (int j = 0; j < c.d; j++) l.Y.live[l.orow(r) * c.d + j] = 1;
}
static void ln_launch(LData& l) {
    void *dx = to_dev(l.x), *dw = to_dev(l.w), *db = to_dev(l.b);
    l.Y.up();
    wh_launch_layernorm_blocks(0, prec_of(l.c.mode), (const float*)dx, (const float*)dw, (const float*)db, l.Y.d, l.c.rows, l.c.d, l.c.in_blk, l.c.out_blk);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    l.Y.down(); dev_free({dx, dw, db});
}
// a wave's sum: lane l adds its own elements (groups of four, 64 lanes across a sweep) in order, then the lanes are added pairwise
template <typename F> static float wave_sum_of(int d, F term) {
    float lane[64] = {0};
    for (int j = 0; j < d; j++) lane[(j / 4) % 64] += term(j);
    for (int o = 1; o < 64; o *= 2) for (int l = 0; l < 64; l += 2 * o) lane[l] += lane[l + o];
    return lane[0];
}
static void ln_emulate(LData& l) {   // float, the sums in a wave's shape (a row's d terms in one chain would carry d roundings, the kernels' lanes d / 64 + 6)
    const LC& c = l.c;
    l.Y.up();
    for (long r = 0; r < c.rows; r++) {
        const float* x = &l.x[(size_t)r * c.d];
        const float mean = wave_sum_of(c.d, [&](int j) { return x[j]; }) / (float)c.d;
        float var;
        if (c.defect == LD_EX2) var = fmaxf(wave_sum_of(c.d, [&](int j) { return x[j] * x[j]; }) / (float)c.d - mean * mean, 0.0f);
        else var = wave_sum_of(c.d, [&](int j) { return (x[j] - mean) * (x[j] - mean); }) / (float)c.d;
        const float rstd = 1.0f / sqrtf(var + 1e-5f);
        const long ro = c.defect == LD_PAIR && r == 1 ? r - 1 : r;
        for (int j = 0; j < c.d; j++) l.Y.set(l.orow(ro) * c.d + j, (x[j] - mean) * rstd * l.w[j] + l.b[j]);
    }
}
static ARes ln_verify(const LData& l) {
    const LC& c = l.c;
    const int d = c.d;
    ARes res;
    res.ratio = par_rows(c.rows, [&](long r) {
        const float* x = &l.x[(size_t)r * d];
        double s = 0, a1 = 0, q = 0, at = 0;
        for (int j = 0; j < d; j++) { s += x[j]; a1 += fabs(x[j]); }
        const double mean = s / d, dep = (d / 64 + 8) * U, emean = dep * a1 / d;
        for (int j = 0; j < d; j++) { const double t = x[j] - mean; q += t * t; at += fabs(t) * (emean + U * fabs(t)); }
        const double var = q / d, evar = 2 * at / d + dep * var, rstd = 1.0 / sqrt(var + 1e-5), erstd = rstd * (0.5 * evar / (var + 1e-5) + 4 * U);
        Worst w;
        for (int j = 0; j < d; j++) {
            const double t = x[j] - mean, et = emean + U * fabs(t), y = t * rstd * l.w[j] + l.b[j];
            const double e = fabs(l.w[j]) * (rstd * et + fabs(t) * erstd) + 3 * U * fabs(t * rstd * l.w[j]) + U * fabs(y);
            w.see(l.Y.at(l.orow(r) * d + j), y, e + half_ulp(l.T, fabs(y) + e));
        }
        return w.ratio;
    });
    res.guard = l.Y.guard(); res.h = l.Y.hash();
    return res;
}
static double worst_ln = 0;
static int ln_report(const LData& l, const ARes& r) {
    const LC& c = l.c;
    const char* kern = c.mode == BF16 && c.d == 512 ? "k_layernorm_w8<1>" : c.mode == BF16 && c.d == 1024 ? "k_layernorm_w8<2>" : "k_layernorm      ";
    printf("%s %s rows %3ld d %4d blocks %3d -> %3d%s: err/bound %.3f guard %ld  y %016llx  %s\n", kern, mode_name[c.mode], c.rows, c.d, c.in_blk, c.out_blk, c.mean25 ? " mean25" : "", r.ratio,
           r.guard, r.h, r.ok() ? "ok" : "MISMATCH");
    worst_ln = std::max(worst_ln, r.ratio);
    return r.ok() ? 0 : 1;
}
static int group_ln() {
    int bad = 0;
    auto one = [&](const LC& c) { LData l; ln_prepare(l, c); ln_launch(l); bad |= ln_report(l, ln_verify(l)); };
    for (Mode md : {BF16, F32, H2}) for (int d : {128, 384, 512, 1024, 1280}) {
        for (long rows : {1, 7, 8, 9, 301}) { LC c; c.mode = md; c.rows = rows; c.d = d; one(c); }
        { LC c; c.mode = md; c.rows = 301; c.d = d; c.in_blk = 100; c.out_blk = 104; one(c); }
        { LC c; c.mode = md; c.rows = 9; c.d = d; c.mean25 = true; one(c); }
    }
    printf("worst err/bound ln %.3f\n", worst_ln);
    return bad;
}

// ===== --selftest: host only ===============================================================================================================
static int self_line(const char* family, const char* what, bool defect, double ratio, long guard) {
    const bool caught = ratio > 1.0 || guard != 0;
    if (!defect) { printf("selftest %-9s clean: %-58s err/bound %.3f guard %ld  %s\n", family, what, ratio, guard, caught ? "MISMATCH" : "ok"); return caught ? 1 : 0; }
    printf("selftest %-9s defect: %-57s err/bound %.3g guard %ld  %s\n", family, what, ratio, guard, caught ? "caught" : "NOT CAUGHT");
    return caught ? 0 : 1;
}
static int selftest() {
    g_host = true;
    int bad = 0;
    auto gemm = [&](GC c, int defect, const char* what) {
        c.defect = defect;
        GData d; gemm_prepare(d, c); gemm_emulate(d);
        const GRes r = gemm_verify(d);
        bad |= self_line("gemm", what, defect != GD_NONE, r.ratio, r.guard);
    };
    for (Mode md : {BF16, H2}) for (bool f : {false, true}) {
        const GC conv = conv_case(md == BF16 ? V8 : V8X, md, f, 140, 1);
        const std::string what = std::string("conv rows, GELU, shared R, N 140, ") + mode_name[md] + " -> " + fmt_name[out_fmt(md, f)];
        gemm(conv, GD_NONE, what.c_str());
    }
    const GC conv = conv_case(V8, BF16, false, 140, 1);
    gemm(conv, GD_KSTEP, "the last k-step dropped");
    gemm(conv, GD_BIASROW, "bias indexed by row instead of column");
    gemm(conv, GD_LAST4, "the last 4-column group not written");
    gemm(conv, GD_MPER, "m_per ignored in the row addressing");
    GC cons; cons.M = 300; cons.N = 140; cons.act = 1; cons.ln_mode = 1;
    gemm(cons, GD_NONE, "LN consumer, row stats");
    gemm(cons, GD_STATROW, "the consumer using the neighbouring row's {mean, rstd}");
    GC cons2; cons2.N = 140; cons2.batch = 2; cons2.bias_mode = 2; cons2.a_shared = true; cons2.ln_mode = 2;
    gemm(cons2, GD_NONE, "LN consumer, column stats");
    GC prod; prod.out_f32 = true; prod.M = 300; prod.N = 128; prod.resid = 2; prod.producer = true; prod.shift = 2;
    gemm(prod, GD_NONE, "LN producer, mean 25");
    gemm(prod, GD_STATCOL, "a stats partial missing its last column");
    GC ws; ws.M = 300; ws.N = 268; ws.wscale = true;
    gemm(ws, GD_NONE, "channel scale");

    auto attn = [&](Mode md, int S, int heads, int peaked, int defect, const char* what) {
        AC c; c.mode = md; c.S = S; c.heads = heads; c.peaked = peaked; c.defect = defect;
        AData a; attn_prepare(a, c); attn_emulate(a);
        const ARes r = attn_verify(a);
        bad |= self_line("attention", what, defect != AD_NONE, r.ratio, r.guard);
    };
    for (Mode md : {BF16, F32, H2}) for (int pk : {0, 1}) attn(md, 100, 1, pk, AD_NONE, (std::string(pk ? "S 100, peaked, " : "S 100, small, ") + mode_name[md]).c_str());
    attn(BF16, 220, 1, 1, AD_NONE, "S 220, peaked");
    attn(BF16, 100, 1, 1, AD_UNMASK, "the padded keys of the last tile unmasked");
    attn(BF16, 220, 1, 1, AD_NORESCALE, "the rescale factor omitted where the maximum rises");
    attn(BF16, 100, 1, 1, AD_VSWAP, "keys 4..7 and 16..19 exchanged in V^T only");
    attn(BF16, 100, 1, 0, AD_LANESUM, "one lane group's share of the row sum left out");

    auto ln = [&](Mode md, bool mean25, int defect, const char* what) {
        LC c; c.mode = md; c.rows = 65; c.d = 512; c.mean25 = mean25; c.in_blk = 4; c.out_blk = 6; c.defect = defect;
        LData l; ln_prepare(l, c); ln_emulate(l);
        const ARes r = ln_verify(l);
        bad |= self_line("layernorm", what, defect != LD_NONE, r.ratio, r.guard);
    };
    for (Mode md : {BF16, F32, H2}) { ln(md, false, LD_NONE, (std::string("d 512, blocks, ") + mode_name[md]).c_str()); ln(md, true, LD_NONE, (std::string("d 512, blocks, mean 25, ") + mode_name[md]).c_str()); }
    ln(F32, true, LD_EX2, "variance as E[x^2] - mean^2 in f32 on the mean-25 rows");
    ln(BF16, false, LD_PAIR, "the second row of a pair written to the first row's place");
    printf("selftest %s\n", bad ? "FAILED" : "passed");
    return bad;
}

// ===== --time: whisper-base encoder shapes, 64 clips, bf16 =================================================================================
static int timing() {
    const int clips = 64, S = 1500, dm = 512;
    const long rows = (long)clips * S;
    void *A, *W, *C, *O; float* bias;
    CK(hipMalloc(&A, rows * 2048 * 2)); CK(hipMalloc(&W, (size_t)2048 * 2048 * 2)); CK(hipMalloc(&C, rows * 2048 * 4)); CK(hipMalloc(&O, rows * dm * 2)); CK(hipMalloc((void**)&bias, 2048 * 4));
    CK(hipMemset(A, 0, rows * 2048 * 2)); CK(hipMemset(W, 0, (size_t)2048 * 2048 * 2)); CK(hipMemset(C, 0, rows * 2048 * 4)); CK(hipMemset(bias, 0, 2048 * 4));
    auto timed = [&](const char* name, auto once) {
        for (int i = 0; i < 3; i++) once();
        CK(hipDeviceSynchronize());
        std::vector<double> us;
        for (int r = 0; r < 25; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < 20; i++) once();
            CK(hipDeviceSynchronize());
            us.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / 20 * 1e6);
        }
        std::sort(us.begin(), us.end());
        printf("time %-34s median %9.1f us  min %9.1f  max %9.1f\n", name, us[12], us.front(), us.back());
    };
    const int NK[4][3] = {{1024, 512, 0}, {512, 512, 0}, {2048, 512, 1}, {512, 2048, 0}};   // QK, out, fc1 (GELU), fc2
    for (auto& nk : NK) {
        GemmArgs g; g.A = A; g.lda = nk[1]; g.W = W; g.ldw = nk[1]; g.C = C; g.ldc = nk[0]; g.bias = bias; g.bias_mode = 1; g.act = nk[2]; g.M = (int)rows; g.N = nk[0]; g.K = nk[1];
        char name[64]; snprintf(name, sizeof name, "k_gemm8 M %ld N %d K %d act %d", rows, nk[0], nk[1], nk[2]);
        timed(name, [&]() { wh_launch_gemm8(0, false, g); });
    }
    timed("k_enc_attn bf16 64 clips x 8 heads", [&]() { wh_launch_enc_attn(0, WH_PREC_BF16, A, C, O, clips, S, dm, 8, 1536); });
    timed("k_layernorm_w8<1> 96000 rows", [&]() { wh_launch_layernorm_blocks(0, WH_PREC_BF16, (const float*)C, bias, bias, O, rows, dm, 0, 0); });
    CK(hipGetLastError());
    dev_free({A, W, C, O, bias});
    return 0;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::string arg = argc > 1 ? argv[1] : "";
    if (arg == "--selftest") return selftest() ? 1 : 0;
    if (arg == "--time") return timing();
    if (!arg.empty() && arg != "gemm8" && arg != "gemm8x" && arg != "gemm" && arg != "attn" && arg != "ln") { fprintf(stderr, "usage: enc_check [gemm8 | gemm8x | gemm | attn | ln | --selftest | --time]\n"); return 2; }
    int bad = 0;
    if (arg.empty() || arg == "gemm8") bad |= group_gemm8();
    if (arg.empty() || arg == "gemm8x") bad |= group_gemm8x();
    if (arg.empty() || arg == "gemm") bad |= group_gemm();
    if (arg.empty() || arg == "attn") bad |= group_attn();
    if (arg.empty() || arg == "ln") bad |= group_ln();
    return bad ? 1 : 0;
}
