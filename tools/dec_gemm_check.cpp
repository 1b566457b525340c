// dec_gemm_check.cpp — the decode GEMM family (k_dec_gemm, k_dec_gemm_wide: wh_dec_gemm.hip; k_dec_tile: wh_dec_tile.hip), each kernel alone
// against a double-precision host restatement of the SkinnyArgs contract, with an FNV-1a hash of every raw output.
//
//   C = act( LN-fold( sum_k X W ) wscale + bias ) (+ R);  producers also write xslab_out = (C - row_shift) xgamma and the per-16-column
//   {sum, sum of squares} of C - row_shift; the consumer of a LayerNorm adds the mean it measured to shift_io; the last workgroup advances *pos_w.
//
// The program links libwhisper_hip.so and calls only wh_launch_dec_gemm / wh_launch_dec_tile, steered by wh_dbg_mt / wh_dbg_nw / wh_dbg_wide, so the
// same source builds against any revision of the library: two builds that print the same hashes computed the same bits.  Every wide case runs a
// second time with wh_dbg_wide = 0 (k_dec_gemm) and the two sets of hashes must be equal.
// Through the C ABI the program cannot see which kernel a launch selected; the kernel name it prints is the one the launcher's rules give for
// the case.  The wide shapes are chosen to meet those rules (launch_dec_gemm_mt): M > 64, no merged X, K a multiple of NW * 4 * KW (128 for the
// 4-way split of bf16 / limb pairs and 8 codes per lane, 256 for the 8-way split and 16 codes per lane), and a column-tile count (N / 16 = 4 or 6)
// divisible by wh_dbg_wide.  If the launcher ever stops choosing k_dec_gemm_wide for them, the wide = narrow comparison still passes, but trivially:
// whoever changes those rules has to move these shapes with them.
//
// Inputs are random and exact in the mode under test (bf16 rounded on the host, fp16 limb pairs packed on the host and decoded exactly, e4m3 codes,
// f32); the restatement works in double on those exact values.  Per output element the bound is built from the operands (U = 2^-24):
//   accumulator   ((c K + 8) U) sum|x w|, c = 1, or 3 for limb pairs (three MFMA passes per k-step), + 2^-22 sum|x w| for their dropped lo.lo term,
//                 + sum|w| dx where X is merged from attention partials (dx: the merged value's rounding to the operand type and (S + 12) 2^-23
//                 of sum w|p| / den for exp2 / rcp / the S-term sums);
//   wscale        the bound times |wscale|, + U |s|;
//   LN fold       mean and rstd carry the f32 error of their own sums (tiles + 2 additions, the E[x^2] - mean^2 difference, one rsqrt), each
//                 operation of rstd (s - mean ln_s) + bias one U of its result;
//   GELU          1.13 (the largest slope) times the bound, + 0.5 |v| (1.5e-7 + 8 U): erf_as's stated error and its f32 evaluation, + 4 U |gelu|;
//   + R, - shift  one U of the result each; xgamma one more;
//   output        half an ulp of the stored type: 2^-8 |v| bf16, U |v| f32, 2^-22 |v| + 2^-24 for a limb pair;
//   statistics    the sums of the elements' bounds (2 |u| each for the squares) + 20 U of the sums of magnitudes.
// Nothing in it is fitted to what the kernels give.
//
//   --time: whisper-base decode shapes, graph-replayed launches, median / min / max of 25 windows per shape.
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/dec_gemm_check.cpp -o tools/dec_gemm_check -Lwhisper-rust-ort_amd -lwhisper_hip -Wl,-rpath,'$ORIGIN/../whisper-rust-ort_amd'
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../whisper-rust-ort_amd/csrc/wh_kernels.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(3); } } while (0)

static const double U = 5.9604644775390625e-8;   // 2^-24
enum Fmt { F_BF16, F_F32, F_H2, F_E4M3 };
enum Mode { BF16, F32, H2, FP8 };
enum Kern { GEMM, WIDE, TILE };
enum Role { PLAIN, CONSUMER, PRODUCER, GROUPED };
static const char* mode_name[] = {"bf16", "f32 ", "h2  ", "fp8 "};
static const char* kern_name[] = {"k_dec_gemm     ", "k_dec_gemm_wide", "k_dec_tile     "};
static const char* role_name[] = {"plain   ", "consumer", "producer", "grouped "};

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
static size_t esz(Fmt f) { return f == F_BF16 ? 2 : f == F_E4M3 ? 1 : 4; }
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
static double e4m3(unsigned c) {   // OCP e4m3fn
    const int e = (c >> 3) & 15, m = c & 7;
    const double v = e ? ldexp(1.0 + m / 8.0, e - 7) : ldexp(m / 8.0, -6);
    return (c & 0x80) ? -v : v;
}
static double half_ulp(Fmt f, double v) { return f == F_BF16 ? ldexp(fabs(v), -8) : f == F_F32 ? U * fabs(v) : ldexp(fabs(v), -22) + ldexp(1.0, -24); }
static size_t slab(int m, int k, int mpad) { return ((size_t)(k >> 5) * mpad + m) * 32 + (k & 31); }

template <typename V> static void* to_dev(const V& v) {
    void* p; const size_t n = v.size() * sizeof(v[0]);
    CK(hipMalloc(&p, n + 256)); CK(hipMemset(p, 0, n + 256)); CK(hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice));
    return p;
}

struct Case { Kern kern; Mode mode; int M, N, K, nw, mt, wide; Role role; int splits; bool ticket; };
struct Result { unsigned long long h[4] = {0, 0, 0, 0}; double ratio = 0; bool ok = true; };
struct Worst { double ratio = 0; void see(double got, double want, double bound) { const double r = fabs(got - want) <= 1e300 ? fabs(got - want) / bound : 1e30; if (r > ratio) ratio = r; } };

static Result run(const Case& c, int wide) {
    const Fmt T = c.mode == F32 ? F_F32 : c.mode == H2 ? F_H2 : F_BF16, TW = c.mode == FP8 ? F_E4M3 : T;
    const int prec = c.mode == F32 ? WH_PREC_F32 : c.mode == H2 ? WH_PREC_F16X3 : c.mode == FP8 ? WH_PREC_FP8 : WH_PREC_BF16;
    const bool consumer = c.role == CONSUMER, producer = c.role == PRODUCER, out_f32 = producer;
    const Fmt TC = consumer ? T : (T == F_BF16 && !out_f32) ? F_BF16 : F_F32;
    const int M = c.M, N = c.N, K = c.K, zn = c.role == GROUPED ? 2 : 1, mpad = (M + 63) / 64 * 64, S = c.splits, H = K / 64;
    rs = 1000003u * c.kern + 7919u * c.mode + 131u * M + 17u * N + K + 29u * c.role + 5u * S;
    const size_t x_el = (size_t)(K / 32) * mpad * 32, nslab = (N + 31) / 32;
    const size_t c_el = consumer ? nslab * mpad * 32 : (size_t)M * N, xs_el = nslab * mpad * 32, st_el = (size_t)(N / 16) * mpad * 2;

    // ---- inputs ----
    std::vector<double> Xv((size_t)zn * M * K), Xe(S ? (size_t)M * K : 0), Wv((size_t)zn * N * K);
    std::vector<unsigned char> hX(zn * x_el * esz(T)), hW((size_t)zn * N * K * esz(TW));
    std::vector<float> xpart, xml;
    if (!S) {
        for (int z = 0; z < zn; z++) for (int m = 0; m < M; m++) for (int k = 0; k < K; k++) Xv[((size_t)z * M + m) * K + k] = put(hX.data(), T, z * x_el + slab(m, k, mpad), frand(1.0f));
    } else {   // X merged from S key ranges' partials (SkinnyArgs::xpart / xml); the second range of every third row is empty
        xpart.resize((size_t)M * S * K); xml.resize((size_t)M * S * 2 * H);
        for (int m = 0; m < M; m++) {
            for (int s = 0; s < S; s++) {
                const bool empty = s == 1 && m % 3 == 0;
                for (int h = 0; h < H; h++) {
                    xml[((size_t)m * S + s) * 2 * H + h] = empty ? -INFINITY : frand(3.0f);
                    xml[((size_t)m * S + s) * 2 * H + H + h] = empty ? 0.0f : 0.5f + fabsf(frand(4.0f));
                }
                for (int k = 0; k < K; k++) xpart[((size_t)m * S + s) * K + k] = empty ? 0.0f : frand(2.0f);
            }
            for (int k = 0; k < K; k++) {
                const int h = k / 64;
                double mx = -INFINITY, num = 0, den = 0, mag = 0;
                for (int s = 0; s < S; s++) mx = fmax(mx, (double)xml[((size_t)m * S + s) * 2 * H + h]);
                for (int s = 0; s < S; s++) {
                    const double w = exp((double)xml[((size_t)m * S + s) * 2 * H + h] - mx), p = xpart[((size_t)m * S + s) * K + k];
                    num += w * p; mag += w * fabs(p); den += w * xml[((size_t)m * S + s) * 2 * H + H + h];
                }
                Xv[(size_t)m * K + k] = num / den;
                Xe[(size_t)m * K + k] = (T == F_F32 ? 0.0 : half_ulp(T, num / den)) + (S + 12) * 2 * U * mag / den;
            }
        }
    }
    for (size_t i = 0; i < Wv.size(); i++) {
        if (TW == F_E4M3) { const unsigned code = ((rnd() & 1) << 7) | ((rnd() % 9) << 3) | (rnd() & 7); hW[i] = (unsigned char)code; Wv[i] = e4m3(code); }
        else Wv[i] = put(hW.data(), TW, i, frand(0.5f));
    }
    std::vector<float> bias((size_t)zn * N), wsc(N), xg(N), R((size_t)M * N), rsh(mpad), sh0(mpad), lnp((size_t)(K / 16) * mpad * 2, 0.0f), lns(N);
    for (auto& v : bias) v = frand(0.5f);
    for (auto& v : wsc) v = 0.25f + fabsf(frand(1.0f));
    for (auto& v : xg) v = 0.5f + fabsf(frand(1.0f));
    for (auto& v : R) v = frand(1.0f);
    for (auto& v : rsh) v = frand(0.3f);
    for (auto& v : sh0) v = frand(0.3f);
    for (auto& v : lns) v = frand(1.0f);
    if (consumer)   // the producer's partial sums of these very rows
        for (int t = 0; t < K / 16; t++) for (int m = 0; m < M; m++) {
            double s1 = 0, s2 = 0;
            for (int k = 16 * t; k < 16 * t + 16; k++) { s1 += Xv[(size_t)m * K + k]; s2 += Xv[(size_t)m * K + k] * Xv[(size_t)m * K + k]; }
            lnp[((size_t)t * mpad + m) * 2] = (float)s1; lnp[((size_t)t * mpad + m) * 2 + 1] = (float)s2;
        }

    // ---- device ----
    std::vector<unsigned char> hC(zn * c_el * esz(TC)), hXS(xs_el * esz(T)), hST(st_el * 4), hSH(mpad * 4);
    void *dX = S ? nullptr : to_dev(hX), *dW = to_dev(hW), *dbias = to_dev(bias), *dws = to_dev(wsc), *dxg = to_dev(xg), *dR = to_dev(R), *drsh = to_dev(rsh),
         *dsh = to_dev(sh0), *dlnp = to_dev(lnp), *dlns = to_dev(lns), *dC = to_dev(hC), *dXS = to_dev(hXS), *dST = to_dev(hST),
         *dxp = S ? to_dev(xpart) : nullptr, *dxml = S ? to_dev(xml) : nullptr;
    std::vector<int> tk = {0, 41};   // {ticket, position}
    int* dtk = (int*)to_dev(tk);
    SkinnyArgs a;
    a.X = dX; a.x_mpad = mpad; a.W = dW; a.bias = (const float*)dbias; a.M = M; a.N = N; a.K = K; a.C = dC;
    if (c.mode == FP8) a.wscale = (const float*)dws;
    if (consumer) { a.c_mpad = mpad; a.act = 1; a.ln_part = (const float*)dlnp; a.ln_tiles = K / 16; a.ln_s = (const float*)dlns; a.shift_io = (float*)dsh; }
    else a.ldc = N;
    if (producer) {
        a.R = (const float*)dR; a.ldr = N; a.row_shift = (const float*)drsh; a.xslab_out = dXS; a.stats_out = (float*)dST;
        if (c.mode == FP8) a.xgamma = (const float*)dxg;
    }
    if (S) { a.xpart = (const float*)dxp; a.xml = (const float*)dxml; a.x_splits = S; a.x_heads = H; }
    if (zn > 1) { a.zn = zn; a.x_zs = (long)x_el; a.w_zs = (long)N * K; a.c_zs = (long)c_el; a.bias_zs = N; }
    if (c.ticket) { a.ticket = dtk; a.pos_w = dtk + 1; }
    wh_dbg_mt = c.mt; wh_dbg_nw = c.nw; wh_dbg_wide = wide;
    if (c.kern == TILE) wh_launch_dec_tile(0, prec, out_f32, a);
    else wh_launch_dec_gemm(0, prec, out_f32, a);
    wh_dbg_mt = 0; wh_dbg_nw = 0; wh_dbg_wide = -1;
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(hC.data(), dC, hC.size(), hipMemcpyDeviceToHost)); CK(hipMemcpy(hXS.data(), dXS, hXS.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hST.data(), dST, hST.size(), hipMemcpyDeviceToHost)); CK(hipMemcpy(hSH.data(), dsh, hSH.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(tk.data(), dtk, 8, hipMemcpyDeviceToHost));
    for (void* p : {dX, dW, dbias, dws, dxg, dR, drsh, dsh, dlnp, dlns, dC, dXS, dST, dxp, dxml, (void*)dtk}) if (p) CK(hipFree(p));

    // ---- restatement ----
    Worst w;
    std::vector<double> s1w(st_el / 2, 0.0), s1b(st_el / 2, 0.0), s2w(st_el / 2, 0.0), s2b(st_el / 2, 0.0), m1(st_el / 2, 0.0), m2(st_el / 2, 0.0);
    for (int m = 0; m < M; m++) {
        double mean = 0, rstd = 1, emean = 0, erstd = 0;
        if (consumer) {
            double s1 = 0, s2 = 0, a1 = 0;
            for (int t = 0; t < K / 16; t++) { s1 += lnp[((size_t)t * mpad + m) * 2]; a1 += fabs(lnp[((size_t)t * mpad + m) * 2]); s2 += lnp[((size_t)t * mpad + m) * 2 + 1]; }
            mean = s1 / K;
            const double ex2 = s2 / K, var = ex2 - mean * mean, tl = (K / 16 + 2) * U;
            emean = tl * a1 / K + U * fabs(mean);
            const double evar = tl * ex2 + 2 * fabs(mean) * emean + 3 * U * (ex2 + mean * mean);
            rstd = 1.0 / sqrt(fmax(var, 0.0) + 1e-5);
            erstd = rstd * (0.5 * evar / (fmax(var, 0.0) + 1e-5) + 4 * U);
            float got; memcpy(&got, &hSH[4 * m], 4);
            w.see(got, sh0[m] + mean, emean + U * fabs(sh0[m] + mean));
        }
        for (int z = 0; z < zn; z++) for (int n = 0; n < N; n++) {
            const double* x = &Xv[((size_t)z * M + m) * K];
            const double* wr = &Wv[((size_t)z * N + n) * K];
            double acc = 0, A = 0, XE = 0;
            for (int k = 0; k < K; k++) { acc += x[k] * wr[k]; A += fabs(x[k] * wr[k]); }
            if (S) for (int k = 0; k < K; k++) XE += Xe[(size_t)m * K + k] * fabs(wr[k]);
            double e = ((c.mode == H2 ? 3.0 : 1.0) * K + 8) * U * A + (c.mode == H2 ? 4 * U * A : 0.0) + XE;
            const double ws = a.wscale ? wsc[n] : 1.0, s = acc * ws, b = bias[(size_t)z * N + n];
            e = e * fabs(ws) + U * fabs(s);
            double v;
            if (consumer) {
                const double p = mean * lns[n], ep = fabs(p) * U + fabs(lns[n]) * emean, t = s - p, et = e + ep + U * fabs(t), u = rstd * t;
                v = u + b;
                e = rstd * et + fabs(t) * erstd + U * fabs(u) + U * fabs(v);
            } else { v = s + b; e += U * fabs(v); }
            if (a.act == 1) { const double g = 0.5 * v * (1.0 + erf(v * 0.70710678118654752440)); e = 1.13 * e + 0.5 * fabs(v) * (1.5e-7 + 8 * U) + 4 * U * fabs(g); v = g; }
            if (producer) { v += R[(size_t)m * N + n]; e += U * fabs(v); }
            w.see(get(hC.data(), TC, z * c_el + (consumer ? slab(m, n, mpad) : (size_t)m * N + n)), v, e + half_ulp(TC, fabs(v) + e));
            if (producer) {
                const double u = v - rsh[m], eu = e + U * fabs(u), g = a.xgamma ? xg[n] : 1.0, y = u * g, ey = eu * fabs(g) + U * fabs(y);
                w.see(get(hXS.data(), T, slab(m, n, mpad)), y, ey + half_ulp(T, fabs(y) + ey));
                const size_t si = (size_t)(n >> 4) * mpad + m;
                s1w[si] += u; s1b[si] += eu; m1[si] += fabs(u); s2w[si] += u * u; s2b[si] += 2 * fabs(u) * eu + eu * eu; m2[si] += u * u;
            }
        }
        if (producer) for (int t = 0; t < N / 16; t++) {
            const size_t si = (size_t)t * mpad + m;
            float g1, g2; memcpy(&g1, &hST[8 * si], 4); memcpy(&g2, &hST[8 * si + 4], 4);
            w.see(g1, s1w[si], s1b[si] + 20 * U * m1[si]);
            w.see(g2, s2w[si], s2b[si] + 20 * U * m2[si]);
        }
    }
    Result r;
    r.ratio = w.ratio;
    r.ok = w.ratio <= 1.0 && (c.ticket ? (tk[0] == 0 && tk[1] == 42) : (tk[0] == 0 && tk[1] == 41));
    r.h[0] = fnv1a(hC.data(), hC.size()); r.h[1] = fnv1a(hXS.data(), hXS.size()); r.h[2] = fnv1a(hST.data(), hST.size()); r.h[3] = fnv1a(hSH.data(), hSH.size());
    return r;
}

static double worst_of[3] = {0, 0, 0};
static int report(const Case& c, int wide, const Result& r, const char* note) {
    printf("%s %s %s M %4d N %4d K %4d split %d mt %d wide %2d xsplits %2d%s: err/bound %.3f  C %016llx xslab %016llx stats %016llx shift %016llx  %s%s\n", kern_name[c.kern],
           mode_name[c.mode], role_name[c.role], c.M, c.N, c.K, c.nw, c.mt, wide, c.splits, c.ticket ? " ticket" : "", r.ratio, r.h[0], r.h[1], r.h[2], r.h[3], r.ok ? "ok" : "MISMATCH", note);
    worst_of[c.kern] = std::max(worst_of[c.kern], r.ratio);
    return r.ok ? 0 : 1;
}
static int check(const Case& c) {
    const Result r = run(c, c.kern == WIDE ? c.wide : -1);
    int bad = report(c, c.kern == WIDE ? c.wide : -1, r, "");
    if (c.kern == WIDE) {   // the same case through k_dec_gemm: bit for bit the same outputs
        Case n = c; n.kern = GEMM;
        const Result q = run(c, 0);
        const bool same = !memcmp(q.h, r.h, sizeof(q.h));
        bad |= report(n, 0, q, same ? "  (= wide)" : "  wide and narrow differ: MISMATCH");
        bad |= same ? 0 : 1;
    }
    return bad;
}

static int checks() {
    int bad = 0;
    const Role roles[] = {PLAIN, CONSUMER, PRODUCER};
    // k_dec_gemm: one k-step per wave; a cut last row tile at both K splits; a K tail past the prefetch depth; grouped; ticket
    for (Mode md : {BF16, F32, H2}) {
        for (Role r : roles) {
            bad |= check({GEMM, md, 5, 48, 128, 4, 1, -1, r, 0, false});
            bad |= check({GEMM, md, 37, 48, 256, 4, 3, -1, r, 0, false});
            bad |= check({GEMM, md, 37, 48, 256, 8, 3, -1, r, 0, false});
            bad |= check({GEMM, md, 64, 80, 1280, 4, 4, -1, r, 0, false});
        }
        bad |= check({GEMM, md, 37, 48, 256, 4, 3, -1, GROUPED, 0, false});
        for (int sp : {3, 6, 12}) bad |= check({GEMM, md, 19, 48, 256, 0, 0, -1, PRODUCER, sp, false});   // merged X: bounds 4, 8, 16
    }
    bad |= check({GEMM, BF16, 37, 48, 256, 4, 3, -1, PLAIN, 0, true});
    for (Role r : roles) for (int K : {128, 256}) bad |= check({GEMM, FP8, 37, 48, K, 0, 3, -1, r, 0, false});   // 8 / 16 codes per lane
    // k_dec_gemm_wide, and each case again through k_dec_gemm (fp8 takes 16 codes per lane at K = 256, whose 8-way split has no k-step: its
    // 8-way case runs at K = 512)
    for (Mode md : {BF16, H2, FP8})
        for (Role r : {CONSUMER, PRODUCER}) {
            bad |= check({WIDE, md, 70, 64, 128, 4, 0, 2, r, 0, false});
            bad |= check({WIDE, md, 70, 64, 128, 4, 0, 4, r, 0, false});
            if (md == FP8) { bad |= check({WIDE, md, 70, 96, 256, 0, 0, 2, r, 0, false}); bad |= check({WIDE, md, 70, 96, 512, 8, 0, 2, r, 0, false}); }
            else bad |= check({WIDE, md, 70, 96, 256, 8, 0, 2, r, 0, false});
        }
    bad |= check({WIDE, BF16, 70, 64, 128, 4, 0, 2, PLAIN, 0, true});
    // k_dec_tile: two row tiles (the second with 2 live rows) and a cut column tile at the minimum of four k-steps; the ring wrapping; the wide tiles
    for (Mode md : {BF16, H2}) {
        for (Role r : {CONSUMER, PRODUCER, GROUPED}) {
            bad |= check({TILE, md, 130, 80, 128, 0, 0, -1, r, 0, false});
            bad |= check({TILE, md, 130, 80, 160, 0, 0, -1, r, 0, false});
        }
        for (Role r : {CONSUMER, PRODUCER}) bad |= check({TILE, md, 1024, 2048, 128, 0, 0, -1, r, 0, false});
    }
    bad |= check({TILE, BF16, 130, 80, 128, 0, 0, -1, PLAIN, 0, true});
    for (int k = 0; k < 3; k++) printf("worst err/bound %s %.3f\n", kern_name[k], worst_of[k]);
    return bad;
}

// ---- launch times: whisper-base decode shapes, plain bf16 calls, graphs of 100 launches, 25 windows ----
static int timing() {
    const int NK[4][2] = {{1536, 512}, {512, 512}, {2048, 512}, {512, 2048}};
    const int rows[4] = {64, 256, 1024, 2048};
    hipStream_t s; CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    void *X, *W, *C; float* bias;
    CK(hipMalloc(&X, (size_t)2048 * 2048 * 2)); CK(hipMalloc(&W, (size_t)2048 * 2048 * 2)); CK(hipMalloc(&C, (size_t)2048 * 2048 * 2)); CK(hipMalloc(&bias, 2048 * 4));
    CK(hipMemset(X, 0, (size_t)2048 * 2048 * 2)); CK(hipMemset(W, 0, (size_t)2048 * 2048 * 2)); CK(hipMemset(bias, 0, 2048 * 4));
    for (int ri = 0; ri < 4; ri++) for (auto& nk : NK) {
        SkinnyArgs a; a.X = X; a.x_mpad = rows[ri]; a.W = W; a.bias = bias; a.M = rows[ri]; a.N = nk[0]; a.K = nk[1]; a.C = C; a.ldc = nk[0];
        wh_dbg_wide = ri < 2 ? 0 : -1;
        auto once = [&]() { if (ri == 3) wh_launch_dec_tile(s, WH_PREC_BF16, false, a); else wh_launch_dec_gemm(s, WH_PREC_BF16, false, a); };
        const int reps = 100, windows = 25;
        for (int i = 0; i < 3; i++) once();
        CK(hipStreamSynchronize(s));
        hipGraph_t g; hipGraphExec_t ge;
        CK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        for (int i = 0; i < reps; i++) once();
        CK(hipStreamEndCapture(s, &g)); CK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
        for (int i = 0; i < 3; i++) CK(hipGraphLaunch(ge, s));
        CK(hipStreamSynchronize(s));
        std::vector<double> us;
        for (int r = 0; r < windows; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            CK(hipGraphLaunch(ge, s)); CK(hipStreamSynchronize(s));
            us.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / reps * 1e6);
        }
        std::sort(us.begin(), us.end());
        printf("time %s rows %4d N %4d K %4d: median %.3f us  min %.3f  max %.3f\n", ri < 2 ? "k_dec_gemm" : ri == 2 ? "k_dec_gemm_wide" : "k_dec_tile", rows[ri], nk[0], nk[1],
               us[windows / 2], us.front(), us.back());
        CK(hipGraphExecDestroy(ge)); CK(hipGraphDestroy(g));
        wh_dbg_wide = -1;
    }
    return 0;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    if (argc > 1 && !strcmp(argv[1], "--time")) return timing();
    return checks() ? 1 : 0;
}
