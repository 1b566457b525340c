// dec_attn_check.cpp — the decoder's attention kernels, each alone against a double-precision host restatement of its contract, with an FNV-1a hash of
// every raw output buffer:  k_dec_self_attn (cache append and the per-clip prefix form PFX included), k_dec_cross_attn in all its instantiations,
// k_dec_cross_attn_cg (wh_dec_attn.hip), k_kv_absmax, k_kv_quant and k_dec_cross_attn8 (wh_fp8.hip).  Built on tools/enc_check.cpp, whose idioms it copies.
//
//   self-attention   one position g = *pos_p.  prec bf16 (bf16 caches, bf16 slab out), f32 (f32 everything), f16x3 (f32 q/k/v and caches, h2 slab out).
//              qkv [B][3d] (q pre-scaled | k | v), caches [B][H][tc][64].  With adv = off ? min(max(off[b], 0), g) : 0 the row attends over cache rows
//              adv .. g - 1 of its own (clip, head) plane plus the current k / v taken from qkv; it writes k and v of qkv bit for bit into cache row g of
//              that plane and out[slab_idx(b, 64 h + e, mpad)], slab_idx(m, k, mpad) = ((k >> 5) mpad + m) 32 + (k & 31).  Checked: the output within
//              the bound; cache row g of every plane equal to the words of qkv; every other cache byte unchanged; the slab unchanged outside rows < B.
//              Rows the contract reads hold valid data, every other cache row (rows >= g, rows < adv) a NaN pattern: the kernel's V prefetch loads
//              rows again for its masked lanes (the last live row, never a row >= g), a select must keep them out.
//   cross-attention  q [B][d] pre-scaled, ck / cv [B / rows_per_clip][S][d], row b reads clip b / rows_per_clip.  Key range sp is
//              [sp per, min(S, sp per + per)), per = ceil(S / splits).  splits == 1: out[slab_idx(b, n, mpad)] = softmax(q_h . K) V, part and ml untouched.
//              Otherwise, with m the range's maximum score of head h:  part[b][sp][n] = sum_j exp(s_j - m) v_j,  ml[b][sp][h] = m,
//              ml[b][sp][H + h] = sum_j exp(s_j - m),  out untouched;  an empty range (sp per >= S) writes exactly {0, -inf, 0}.  The partials are
//              compared after normalising (part / den against the range's own softmax: a maximum that is off by the score error scales part and den
//              alike), m and den against the restatement with bounds of their own.  In bf16 the kernels round each weight p — taken against the
//              stream's running maximum at that key — to bf16 before the P.V product, while the denominator sums the unrounded p: the restatement
//              keeps the exact p in both and the bound carries the rounding on the numerator alone.
//   fp8        after a caller-zeroed amax, wh_launch_kv_quant leaves amax[plane][head] = the f32 bits of max|.| over the head's S x 64 block (exact) and
//              codes = the host e4m3 (OCP, round to nearest even, saturating at 448) quantiser of float(v) / sc, sc = amax / 448, or 1 for an all-zero
//              head, the quotient in f32.  The codes must be equal; where the device's division makes one differ the case prints how many do and accepts
//              one code step, only where the exact quotient lies within one f32 ulp of a rounding tie.  k_dec_cross_attn8 is then held to the
//              cross-attention contract on the dequantised values code sc, K's scale riding on q and V's on the output (p is not rounded there).
//
//   reorder    wh_launch_beam_reorder (k_beam_reorder, wh_beam.hip) at position g - 1 on 2 clips x 3 beams (two rows sharing a parent; one clip done),
//              then the self-attention at g: out, kc and vc must hash equal to the same launch on caches permuted on the host.  bf16 and f32, g 1, 64, 65, 130.
//
// The program links libwhisper_hip.so and calls only wh_launch_dec_self_attn, wh_launch_beam_reorder, wh_launch_dec_cross_attn, wh_launch_kv_quant and wh_launch_dec_cross_attn8
// (and sets the exported wh_dbg_cross_unroll): the same source checks any revision of the library, and two builds that print the same hashes computed
// the same bits.  Variants are chosen with the stream_nt argument and wh_dbg_cross_unroll, never with the WH_CROSS_NT / WH_CROSS_UNROLL environment
// variables (read once per process).  The kernel name a case prints is the one the launchers' rules give for it (bf16: ceil(d / 8 / 64) == 1 ->
// k_dec_cross_attn<bf16, 1, unroll>, else d % 256 == 0 -> k_dec_cross_attn_cg<4>, else <bf16, 3, 2>;  f32 / f16x3: ceil(d / 4 / 64) = 1, 2, more ->
// <float, 1, 4>, <float, 2, 2>, <float, 5, 1>;  fp8: d / 16 = 32, 16, 8 -> KPI 2, 4, 8, up to 64 -> <1, 1, 4>, else <1, 2, 2>).
// Every case stays inside the launchers' preconditions, which they do not check: head width 64, d a multiple of 64, tc <= 512 (sc[512]), g < tc,
// 0 <= off[b], n_heads <= 32 on the fp8 path (hm[32]), mpad >= B, d % 16 == 0 for cross8.
//
// Inputs are random (one LCG seed per case) and exact in the mode under test: bf16 rounded on the host, f32 as is.  Every output buffer is filled with
// a byte pattern first; what the contract does not write must come back unchanged, the 256 bytes behind each buffer included.  A case prints, per
// output, the worst |got - want| / bound (the condition is <= 1), the guard result and the hash; a failing one prints MISMATCH, and the exit status is
// non-zero.
//
// Bounds, per output element, from the operands alone (U = 2^-24); nothing in them is fitted to what the kernels give.  With w_j = p_j / sum p:
//   score      d = c U sum|q k|, c = an upper count of the roundings a product passes through on its way into the score:
//                self    72 = 64 + 8, enc_check's term for an f32 dot of 64 products: a lane's chain of 64 multiply-adds (the current key: one product
//                        per lane and six cross-lane levels);
//                cross   12: bf16 — v_dot2c_f32_bf16 adds two exact bf16 products to the accumulator with at most two roundings, 4 instructions per
//                        lane, then three DPP levels (8 + 3);  f32 — 4 products per lane, their chain, four DPP levels (1 + 4 + 4);
//                cross8  24: 16 products per lane in two chains of 8 multiply-adds, their sum, two DPP levels (1 + 16 + 1 + 2), and the two scale
//                        multiplications (sk on q; the f32 quotient amax / 448 itself), 2.
//              The largest d over a range's keys moves every weight by at most exp(2 d) - 1 relatively, the maximum m by d, the denominator by
//              exp(2 d) - 1.
//   __expf     v_exp_f32(x log2 e): one ulp of the result (2 U; the accuracy AMD's CDNA ISA reference states for V_EXP_F32) and as much again for the
//              products with it, 4 U; the argument carries the subtraction, the product with log2 e and that constant's own rounding, 3 U |x|.  Along a
//              stream the rescales exp(m_old - m_new) and the merge's exp(m_w - M) have arguments of one sign that add up to m_first - M, so per key the
//              arguments cost 3 U (|s_j| + |m|) in all; each rescale's own ulp and product are counted with the sums below.
//   p to bf16  2^-8 of each weight (half an ulp at a binade's bottom) on the numerator, where the contract has it (bf16 cross kernels); none elsewhere.
//   sums       numerator: 2 roundings per key of the longest stream and 3 per register set (the rescale: exp, product), one per merged stream, + 16
//              for the final division and slack;  denominator: 1 per key, the rest alike.  The key count per stream follows the kernel's dealing:
//              self — row r to slot r % RPI (RPI 8 bf16, 4 f32) for P.V, key j to lane j % 64 for the sum;  cross — groups of UNROLL keys round-robin
//              to the 4 waves;  _cg — pairs, even key to parity 0, UNROLL pairs per group, 4 waves;  cross8 — KPI keys per instruction to the KPI
//              slots, UNROLL instructions per group, 4 waves.
//   all of these multiply sum_j w_j |v_j|;  then half an ulp of the stored type (2^-8 |v| bf16, U |v| f32, 2^-22 |v| + 2^-24 for a limb pair).
//   m: d + U |m|.   den: den (exp(2 d) - 1 + sums) + sum_j p_j (4 U + 3 U (|s_j| + |m|)).
//
//   dec_attn_check [self | reorder | cross | cross8]   one group, or all of them
//   dec_attn_check --selftest   host only (no HIP call): for one case of each family the restatement carried out in the kernel's working precision (float
//                          accumulation in the kernel's order of streams and merges, p rounded where the kernel rounds it, the output rounded to the
//                          stored type) must stay within the bound, and the same with one defect at a time must exceed it, or fail an exact
//                          condition, on at least one element.  The defects:
//                           1 self: the current key left out                        9 cross: an empty wave's -inf not skipped
//                           2 self: one cache row too many read (j <= pos)         10 _cg: the odd-parity stream dropped
//                           3 self with prefixes: adv ignored                      11 beam: kvb = b
//                           4 self: a masked V row multiplied in (NaN fill)        12 the slab indexed with pitch B instead of mpad
//                           5 self: the append at the local row                    13 fp8: K's scale not applied
//                           6 cross: the clamped tail key counted                  14 fp8: V's scale from head 0
//                           7 cross: waves / ranges merged without exp(m - M)      15 fp8: amax off by one row at a workgroup boundary
//                           8 cross: the denominator from the neighbouring head
//   dec_attn_check --time       launch times on the whisper-base decode shapes (bf16, 64 clips): the self-attention at positions 4, 64 and 447, the
//                          cross-attention with the context's split count (256 / 64 = 4); median of 25 windows of 20 launches.
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/dec_attn_check.cpp -o tools/dec_attn_check -Lwhisper-rust-ort_amd -lwhisper_hip -Wl,-rpath,'$ORIGIN/../whisper-rust-ort_amd'
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
enum Fmt { F_BF16, F_F32, F_H2, F_U8 };
enum Mode { BF16, F32, X3, FP8 };                 // X3: WH_PREC_F16X3 (f32 operands, h2 slab)
static const char* mode_name[] = {"bf16 ", "f32  ", "f16x3", "fp8  "};
static bool g_host = false;                       // --selftest: no device, the outputs come from the host emulation

static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }   // RNE (finite inputs)
static unsigned rs = 1;
static unsigned rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static float frand(float a) { return ((int)(rnd() & 0xffff) - 32768) / 32768.0f * a; }
static unsigned long long fnv1a(const void* p, size_t n, unsigned long long h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}
static size_t esz(Fmt f) { return f == F_BF16 ? 2 : f == F_U8 ? 1 : 4; }
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
static void put_nan(unsigned char* b, Fmt f, size_t i) {   // (caches: bf16 or f32)
    if (f == F_BF16) { const unsigned short h = 0x7fc0; memcpy(b + 2 * i, &h, 2); } else { const unsigned u = 0x7fc00000u; memcpy(b + 4 * i, &u, 4); }
}
static double half_ulp(Fmt f, double v) { return f == F_BF16 ? ldexp(fabs(v), -8) : f == F_F32 ? U * fabs(v) : ldexp(fabs(v), -22) + ldexp(1.0, -24); }
static int prec_of(Mode m) { return m == BF16 ? WH_PREC_BF16 : m == F32 ? WH_PREC_F32 : m == X3 ? WH_PREC_F16X3 : WH_PREC_FP8; }
static size_t slab(int m, int k, int mpad) { return ((size_t)(k >> 5) * mpad + m) * 32 + (k & 31); }

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
    unsigned long long el_hash(size_t i, unsigned long long s) const {   // one element's bytes into a running hash
        if (f == F_H2) return fnv1a(&h[h2_hi(i) + 64], 2, fnv1a(&h[h2_hi(i)], 2, s));
        return fnv1a(&h[i * esz(f)], esz(f), s);
    }
};
static unsigned long long slab_row_hash(const Out& o, int b, int d, int mpad) {
    unsigned long long s = 1469598103934665603ull;
    for (int n = 0; n < d; n++) s = o.el_hash(slab(b, n, mpad), s);
    return s;
}

// The softmax part of both contracts and its bound, for one (row, head, key range): scores s and their magnitudes sum|q k| are given for n keys, val(j, e)
// is v_j[e].  want[e] = sum p v / den and eb[e], its bound before the stored type's half ulp; m, den, their bounds.
struct Soft { double m = 0, den = 0, e_m = 0, e_den = 0, want[64], eb[64]; };
template <typename VF>
static void soft_ref(int n, const double* s, const double* mag, VF val, double dot_u, double p_round, double ch_num, double ch_den, Soft& r) {
    double mx = -1e300, dmax = 0;
    for (int j = 0; j < n; j++) { mx = std::max(mx, s[j]); dmax = std::max(dmax, dot_u * U * mag[j]); }
    std::vector<double> p(n), ee(n);
    double den = 0, exs = 0;
    for (int j = 0; j < n; j++) { p[j] = exp(s[j] - mx); ee[j] = 4 * U + 3 * U * (fabs(s[j]) + fabs(mx)); den += p[j]; exs += p[j] * ee[j]; }
    const double rel = expm1(2 * dmax) + p_round + (ch_num + ch_den) * U;
    for (int e = 0; e < 64; e++) {
        double num = 0, mg = 0, ex = 0;
        for (int j = 0; j < n; j++) { const double v = val(j, e); num += p[j] * v; mg += p[j] * fabs(v); ex += p[j] * fabs(v) * ee[j]; }
        r.want[e] = num / den; r.eb[e] = (rel * mg + 2 * ex) / den;   // (2 ex: the key's own exp, and the denominator's share of the same keys)
    }
    r.m = mx; r.den = den; r.e_m = dmax + U * fabs(mx); r.e_den = den * (expm1(2 * dmax) + ch_den * U) + exs;
}

// ===== self-attention ======================================================================================================================
enum SDefect { SD_NONE, SD_NOCUR, SD_ONEMORE, SD_NOADV, SD_MASKMUL, SD_LOCALROW };
struct SC { const char* what = ""; Mode mode = BF16; int d = 128, H = 2, tc = 448, B = 3, mpad = 64, g = 0, peaked = 0; bool pfx = false; int off[8] = {0}; int defect = SD_NONE; };
struct SData {
    SC c; Fmt T, TO;
    std::vector<double> cur, K, V;   // qkv [B][3d]; the reference's own K / V history [B][H][tc][64] (NaN where the contract reads nothing)
    std::vector<unsigned char> hqkv; Out KC, VC, O;
    size_t ci(int b, int h, int r, int e) const { return (((size_t)b * c.H + h) * c.tc + r) * 64 + e; }
    int adv(int b) const { return c.pfx ? std::min(std::max(c.off[b], 0), c.g) : 0; }
};
struct SRes { double ratio = 0; long guard = 0, append = 0; unsigned long long h[3] = {0, 0, 0}; bool ok() const { return ratio <= 1.0 && guard == 0 && append == 0; } };

// prev: the position before this one of a chain — its caches as the kernel left them, its history plus the row it appended
static void self_prepare(SData& s, const SC& c, const SData* prev = nullptr) {
    s.c = c; s.T = c.mode == BF16 ? F_BF16 : F_F32; s.TO = c.mode == BF16 ? F_BF16 : c.mode == F32 ? F_F32 : F_H2;
    const int B = c.B, H = c.H, d = c.d, tc = c.tc, g = c.g;
    rs = 2246822519u * (unsigned)(g + 1) + 7919u * d + 131u * c.mode + 17u * c.mpad + 3u * c.peaked + 977u * c.pfx + 29u * c.off[1] + 31u * c.off[2];
    const size_t nc = (size_t)B * H * tc * 64;
    s.KC.make(s.T, nc); s.VC.make(s.T, nc);
    if (prev) {
        s.K = prev->K; s.V = prev->V; s.KC.h0 = prev->KC.h; s.VC.h0 = prev->VC.h;
        for (int b = 0; b < B; b++) for (int n = 0; n < d; n++) {
            s.K[s.ci(b, n / 64, g - 1, n % 64)] = prev->cur[(size_t)b * 3 * d + d + n];
            s.V[s.ci(b, n / 64, g - 1, n % 64)] = prev->cur[(size_t)b * 3 * d + 2 * d + n];
        }
    } else {
        s.K.assign(nc, NAN); s.V.assign(nc, NAN);
        for (size_t i = 0; i < s.KC.n; i++) { put_nan(s.KC.h0.data(), s.T, i); put_nan(s.VC.h0.data(), s.T, i); }
        for (int b = 0; b < B; b++) for (int h = 0; h < H; h++) for (int r = s.adv(b); r < g; r++) for (int e = 0; e < 64; e++) {
            s.K[s.ci(b, h, r, e)] = put(s.KC.h0.data(), s.T, s.ci(b, h, r, e), frand(1.0f));
            s.V[s.ci(b, h, r, e)] = put(s.VC.h0.data(), s.T, s.ci(b, h, r, e), frand(1.0f));
        }
    }
    s.cur.assign((size_t)B * 3 * d, 0.0); s.hqkv.assign(s.cur.size() * esz(s.T), 0);
    for (int b = 0; b < B; b++) for (int n = d; n < 3 * d; n++) s.cur[(size_t)b * 3 * d + n] = put(s.hqkv.data(), s.T, (size_t)b * 3 * d + n, frand(1.0f));
    for (int b = 0; b < B; b++) for (int h = 0; h < H; h++) {
        // peaked: the query is its winning key scaled so that their score is 30; the winner is any live row, the current key included
        const int a = s.adv(b), win = a + (int)(rnd() % (unsigned)(g - a + 1));
        double kw[64], n2 = 0;
        for (int e = 0; e < 64; e++) { kw[e] = win == g ? s.cur[(size_t)b * 3 * d + d + 64 * h + e] : s.K[s.ci(b, h, win, e)]; n2 += kw[e] * kw[e]; }
        for (int e = 0; e < 64; e++) {
            const float v = c.peaked ? (float)(kw[e] * 30.0 / n2) : frand(0.25f);
            s.cur[(size_t)b * 3 * d + 64 * h + e] = put(s.hqkv.data(), s.T, (size_t)b * 3 * d + 64 * h + e, v);
        }
    }
    for (int b = 0; b < B; b++) for (int h = 0; h < H; h++) for (int e = 0; e < 64; e++) s.KC.live[s.ci(b, h, g, e)] = s.VC.live[s.ci(b, h, g, e)] = 1;
    s.O.make(s.TO, (size_t)d * c.mpad);
    for (int b = 0; b < B; b++) for (int n = 0; n < d; n++) s.O.live[slab(b, n, c.mpad)] = 1;
}
static void self_launch(SData& s) {
    const SC& c = s.c;
    std::vector<int> pos(1, c.g), off(c.off, c.off + c.B);
    void *dq = to_dev(s.hqkv), *dp = to_dev(pos), *dof = to_dev(off);
    s.KC.up(); s.VC.up(); s.O.up();
    wh_launch_dec_self_attn(0, prec_of(c.mode), dq, s.KC.d, s.VC.d, s.O.d, (const int*)dp, c.d, c.H, c.tc, c.B, c.mpad, c.pfx ? (const int*)dof : nullptr);
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    s.KC.down(); s.VC.down(); s.O.down(); dev_free({dq, dp, dof});
}
static float tree64(float* l) { for (int o = 1; o < 64; o *= 2) for (int i = 0; i < 64; i += 2 * o) l[i] += l[i + o]; return l[0]; }
// the kernel's walk in float on the host: key j scored by lane j % 64, the current key by a product per lane and a cross-lane sum, row r of P.V by slot
// r % RPI, the slots added at the end; the V prefetch of the masked rows of the last group of NPRE * RPI selected out
static void self_emulate(SData& s) {
    const SC& c = s.c;
    const int d = c.d, g = c.g, RPI = s.T == F_BF16 ? 8 : 4, GRP = 8 * RPI;
    s.KC.up(); s.VC.up(); s.O.up();
    for (int b = 0; b < c.B; b++) for (int h = 0; h < c.H; h++) {
        const int adv = c.defect == SD_NOADV ? 0 : s.adv(b), pos = g - adv, tcl = c.tc - adv;
        auto kc = [&](int r, int e) { return (float)get(s.KC.h0.data(), s.T, s.ci(b, h, adv + r, e)); };
        auto vc = [&](int r, int e) { return (float)get(s.VC.h0.data(), s.T, s.ci(b, h, adv + r, e)); };
        const size_t q0 = (size_t)b * 3 * d + 64 * h;
        float q[64], pr[64];
        for (int e = 0; e < 64; e++) { q[e] = (float)s.cur[q0 + e]; pr[e] = q[e] * (float)s.cur[q0 + d + e]; }
        const int nk = c.defect == SD_ONEMORE ? pos + 1 : pos;
        std::vector<float> sc(nk);
        float mx = -INFINITY;
        for (int j = 0; j < nk; j++) { float t = 0.0f; for (int e = 0; e < 64; e++) t += q[e] * kc(j, e); sc[j] = t; mx = fmaxf(mx, t); }
        const float scur = tree64(pr);
        if (c.defect != SD_NOCUR) mx = fmaxf(mx, scur);
        float lane[64] = {0};
        for (int j = 0; j < nk; j++) { sc[j] = expf(sc[j] - mx); lane[j % 64] += sc[j]; }
        const float pcur = c.defect == SD_NOCUR ? 0.0f : expf(scur - mx), sum = tree64(lane) + pcur;
        std::vector<float> o((size_t)RPI * 64, 0.0f);
        for (int e = 0; e < 64; e++) o[e] = pcur * (float)s.cur[q0 + 2 * d + e];
        const int rows = std::max(GRP, (nk + GRP - 1) / GRP * GRP);   // the first group is loaded whatever the position
        for (int r = 0; r < rows; r++) for (int e = 0; e < 64; e++) {
            if (r < nk) o[(size_t)(r % RPI) * 64 + e] += sc[r] * vc(r, e);
            else if (c.defect == SD_MASKMUL) o[(size_t)(r % RPI) * 64 + e] += 0.0f * vc(std::min(r, tcl - 1), e);
        }
        const float inv = 1.0f / sum;
        for (int e = 0; e < 64; e++) {
            float t = 0.0f;
            for (int sl = 0; sl < RPI; sl++) t += o[(size_t)sl * 64 + e];
            s.O.set(slab(b, 64 * h + e, c.mpad), t * inv);
        }
        const int arow = c.defect == SD_LOCALROW ? s.c.g - s.adv(b) : g;
        for (int e = 0; e < 64; e++) {
            memcpy(&s.KC.h[s.ci(b, h, arow, e) * esz(s.T)], &s.hqkv[(q0 + d + e) * esz(s.T)], esz(s.T));
            memcpy(&s.VC.h[s.ci(b, h, arow, e) * esz(s.T)], &s.hqkv[(q0 + 2 * d + e) * esz(s.T)], esz(s.T));
        }
    }
}
static SRes self_verify(const SData& s) {
    const SC& c = s.c;
    const int d = c.d, g = c.g, RPI = s.T == F_BF16 ? 8 : 4;
    SRes r;
    std::atomic<long> append{0};
    r.ratio = par_rows((long)c.B * c.H, [&](long i) {
        const int b = (int)(i / c.H), h = (int)(i % c.H), adv = s.adv(b), n = g - adv + 1;   // the past keys, then the current one
        const size_t q0 = (size_t)b * 3 * d + 64 * h;
        std::vector<double> sc(n), mag(n);
        for (int j = 0; j < n; j++) {
            double a = 0, m = 0;
            for (int e = 0; e < 64; e++) { const double k = j == n - 1 ? s.cur[q0 + d + e] : s.K[s.ci(b, h, adv + j, e)]; a += s.cur[q0 + e] * k; m += fabs(s.cur[q0 + e] * k); }
            sc[j] = a; mag[j] = m;
        }
        Soft f;
        soft_ref(n, sc.data(), mag.data(), [&](int j, int e) { return j == n - 1 ? s.cur[q0 + 2 * d + e] : s.V[s.ci(b, h, adv + j, e)]; }, 72, 0.0,
                 2.0 * ((n + RPI - 1) / RPI + 1) + RPI + 16, (n + 63) / 64 + 8 + 16, f);
        Worst w;
        for (int e = 0; e < 64; e++) w.see(s.O.at(slab(b, 64 * h + e, c.mpad)), f.want[e], f.eb[e] + half_ulp(s.TO, fabs(f.want[e]) + f.eb[e]));
        long bad = 0;
        for (int e = 0; e < 64; e++) {
            bad += memcmp(&s.KC.h[s.ci(b, h, g, e) * esz(s.T)], &s.hqkv[(q0 + d + e) * esz(s.T)], esz(s.T)) != 0;
            bad += memcmp(&s.VC.h[s.ci(b, h, g, e) * esz(s.T)], &s.hqkv[(q0 + 2 * d + e) * esz(s.T)], esz(s.T)) != 0;
        }
        append += bad;
        return w.ratio;
    });
    r.append = append; r.guard = s.KC.guard() + s.VC.guard() + s.O.guard();
    r.h[0] = s.O.hash(); r.h[1] = s.KC.hash(); r.h[2] = s.VC.hash();
    return r;
}
static double worst_self = 0;
static const char* self_kernel(const SC& c) {
    return c.mode == BF16 ? (c.pfx ? "k_dec_self_attn<bf16, bf16, PFX>" : "k_dec_self_attn<bf16, bf16>     ") : c.mode == F32 ? (c.pfx ? "k_dec_self_attn<float, float, PFX>" : "k_dec_self_attn<float, float>   ")
                                                                                                              : (c.pfx ? "k_dec_self_attn<float, h2, PFX> " : "k_dec_self_attn<float, h2>      ");
}
static int self_report(const SData& s, const SRes& r, const char* tag = "") {
    const SC& c = s.c;
    printf("%s %s %-22s g %3d d %4d H %2d B %d mpad %2d: err/bound %.3f guard %ld append %ld  out %016llx kc %016llx vc %016llx  %s%s\n", self_kernel(c), mode_name[c.mode], c.what, c.g, c.d, c.H,
           c.B, c.mpad, r.ratio, r.guard, r.append, r.h[0], r.h[1], r.h[2], r.ok() ? "ok" : "MISMATCH", tag);
    worst_self = std::max(worst_self, r.ratio);
    return r.ok() ? 0 : 1;
}
static int self_case(const SC& c) { SData s; self_prepare(s, c); self_launch(s); return self_report(s, self_verify(s)); }

// the un-prefixed launch a prefixed row must equal bit for bit: every row of it is row b of p at its local position, on the same keys
static void self_unprefixed(SData& u, const SData& p, int b) {
    SC c = p.c; c.pfx = false; c.g = p.c.g - p.adv(b); c.what = "the same, un-prefixed";
    self_prepare(u, c);
    const int d = c.d, a = p.adv(b);
    for (int b2 = 0; b2 < c.B; b2++) {
        for (int n = 0; n < 3 * d; n++) { u.cur[(size_t)b2 * 3 * d + n] = p.cur[(size_t)b * 3 * d + n]; memcpy(&u.hqkv[((size_t)b2 * 3 * d + n) * esz(u.T)], &p.hqkv[((size_t)b * 3 * d + n) * esz(u.T)], esz(u.T)); }
        for (int h = 0; h < c.H; h++) for (int r = 0; r < c.g; r++) for (int e = 0; e < 64; e++) {
            u.K[u.ci(b2, h, r, e)] = p.K[p.ci(b, h, a + r, e)]; u.V[u.ci(b2, h, r, e)] = p.V[p.ci(b, h, a + r, e)];
            memcpy(&u.KC.h0[u.ci(b2, h, r, e) * esz(u.T)], &p.KC.h0[p.ci(b, h, a + r, e) * esz(u.T)], esz(u.T));
            memcpy(&u.VC.h0[u.ci(b2, h, r, e) * esz(u.T)], &p.VC.h0[p.ci(b, h, a + r, e) * esz(u.T)], esz(u.T));
        }
    }
}
static int self_pfx_case(Mode md, int g, const int (&off)[3], bool host = false) {
    SC c; c.what = "prefixes mixed"; c.mode = md; c.g = g; c.pfx = true;
    for (int b = 0; b < 3; b++) c.off[b] = off[b];
    SData p; self_prepare(p, c);
    if (host) self_emulate(p); else self_launch(p);
    int bad = self_report(p, self_verify(p));
    for (int b = 0; b < 3; b++) {
        SData u; self_unprefixed(u, p, b);
        if (host) self_emulate(u); else self_launch(u);
        const bool same = slab_row_hash(u.O, b, c.d, c.mpad) == slab_row_hash(p.O, b, c.d, c.mpad);
        char tag[96]; snprintf(tag, sizeof tag, "  row %d off %3d local %3d: row hash %s", b, c.off[b], u.c.g, same ? "equal" : "DIFFERENT: MISMATCH");
        bad |= self_report(u, self_verify(u), tag) | !same;
    }
    return bad;
}
static int self_chain(Mode md, int n) {
    int bad = 0;
    std::vector<SData> st(2);
    for (int g = 0; g < n; g++) {
        SC c; c.what = "chain"; c.mode = md; c.g = g;
        SData& s = st[g & 1];
        self_prepare(s, c, g ? &st[(g - 1) & 1] : nullptr);
        self_launch(s);
        bad |= self_report(s, self_verify(s));
    }
    return bad;
}
static int group_self() {
    int bad = 0;
    const int positions[] = {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 447};
    for (Mode md : {BF16, F32, X3}) {
        for (int g : positions) { SC c; c.what = "small scores"; c.mode = md; c.g = g; bad |= self_case(c); }
        { SC c; c.what = "peaked scores"; c.mode = md; c.g = 191; c.peaked = 1; bad |= self_case(c); }
        { SC c; c.what = "mpad 16"; c.mode = md; c.g = 65; c.mpad = 16; bad |= self_case(c); }
        { SC c; c.what = "head and clip indexing"; c.mode = md; c.g = 130; c.d = 1280; c.H = 20; bad |= self_case(c); }
        const int g = 200, offa[3] = {0, 5, g}, offb[3] = {g + 7, g - 64, g - 128};   // no prefix, a small one, local position 0; an idle row, local positions 64 and 128
        bad |= self_pfx_case(md, g, offa);
        bad |= self_pfx_case(md, g, offb);
    }
    bad |= self_chain(BF16, 70);
    bad |= self_chain(F32, 36);
    printf("worst err/bound self %.3f\n", worst_self);
    return bad;
}

// ===== beam reorder, then self-attention ===================================================================================================
// After wh_launch_beam_reorder at position g - 1 (rows 0 .. g - 1 of a clip's beams become those of their parents, the position becomes g) a
// self-attention launch must leave out, kc and vc equal, bit for bit, to the same launch on caches permuted on the host.  2 clips x 3 beams: clip 0
// with two rows sharing a parent, clip 1 complete (done: its rows must not move).
static void reorder_host(SData& s, const int* parent, const int* done, int K) {   // rows 0 .. g - 1 of dst row j = those of src row parent[j]
    const SC& c = s.c;
    const std::vector<double> K0 = s.K, V0 = s.V;
    const std::vector<unsigned char> k0 = s.KC.h0, v0 = s.VC.h0;
    for (int b = 0; b < c.B; b++) {
        const int r0 = b / K * K, src = r0 + parent[b];
        if (done[r0] || src == b) continue;
        for (int h = 0; h < c.H; h++) for (int r = 0; r < c.g; r++) for (int e = 0; e < 64; e++) {
            s.K[s.ci(b, h, r, e)] = K0[s.ci(src, h, r, e)]; s.V[s.ci(b, h, r, e)] = V0[s.ci(src, h, r, e)];
            memcpy(&s.KC.h0[s.ci(b, h, r, e) * esz(s.T)], &k0[s.ci(src, h, r, e) * esz(s.T)], esz(s.T));
            memcpy(&s.VC.h0[s.ci(b, h, r, e) * esz(s.T)], &v0[s.ci(src, h, r, e) * esz(s.T)], esz(s.T));
        }
    }
}
static int reorder_case(Mode md, int g) {
    const int K = 3, clips = 2, parent[6] = {1, 1, 0, 2, 0, 1}, done[6] = {0, 0, 0, 1, 1, 1};
    SC c; c.what = "permuted on the host"; c.mode = md; c.g = g; c.B = clips * K;
    SData hs, dv;
    self_prepare(hs, c);
    c.what = "after k_beam_reorder";
    self_prepare(dv, c);   // (the same seed: the same caches and qkv)
    reorder_host(hs, parent, done, K);
    self_launch(hs);
    {   // the device's turn: the un-permuted caches, the reorder at position g - 1, then the self-attention at the position it left
        std::vector<int> pos(1, g - 1), tick(1, 0), par(parent, parent + 6), dn(done, done + 6);
        void *dq = to_dev(dv.hqkv), *dp = to_dev(pos), *dt = to_dev(tick), *dpar = to_dev(par), *ddn = to_dev(dn);
        dv.KC.up(); dv.VC.up(); dv.O.up();
        wh_launch_beam_reorder(0, (int)esz(dv.T), dv.KC.d, dv.VC.d, (const int*)dpar, (const int*)ddn, K, clips, 1, c.H, c.tc, (int*)dp, (int*)dt);
        wh_launch_dec_self_attn(0, prec_of(md), dq, dv.KC.d, dv.VC.d, dv.O.d, (const int*)dp, c.d, c.H, c.tc, c.B, c.mpad, nullptr);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        CK(hipMemcpy(pos.data(), dp, 4, hipMemcpyDeviceToHost));
        dv.KC.down(); dv.VC.down(); dv.O.down(); dev_free({dq, dp, dt, dpar, ddn});
        if (pos[0] != g) { printf("k_beam_reorder left position %d, not %d: MISMATCH\n", pos[0], g); return 1; }
    }
    // the reference history and the bytes that must come back unchanged are the permuted ones
    dv.K = hs.K; dv.V = hs.V; dv.KC.h0 = hs.KC.h0; dv.VC.h0 = hs.VC.h0;
    const SRes rh = self_verify(hs), rd = self_verify(dv);
    const bool same = rh.h[0] == rd.h[0] && rh.h[1] == rd.h[1] && rh.h[2] == rd.h[2];
    printf("reorder ");
    int bad = self_report(hs, rh);
    printf("reorder ");
    bad |= self_report(dv, rd, same ? "  hashes equal" : "  hashes DIFFERENT: MISMATCH") | !same;
    return bad;
}
static int group_reorder() {
    int bad = 0;
    for (Mode md : {BF16, F32}) for (int g : {1, 64, 65, 130}) bad |= reorder_case(md, g);
    return bad;
}

// ===== cross-attention =====================================================================================================================
enum CKind { K_ATTN, K_CG, K_C8 };
enum CDefect { CD_NONE, CD_TAIL, CD_NORESCALE, CD_DENHEAD, CD_NOSKIP, CD_ODDPAR, CD_KVB, CD_PITCH, CD_KSCALE, CD_SVHEAD0, CD_AMAXROW };
struct CC {
    const char* what = ""; Mode mode = BF16; int d = 128, H = 2, S = 17, splits = 1, B = 2, mpad = 64, rpc = 1, unroll = 4, peaked = 0; bool nt = false, eqq = false;
    int zero_head = -1, outlier = 0;   // fp8: head zero_head all zero (K of clip 0, V of clip 1); head 1's V maximum a single outlier at row min(124, S - 1)
    int defect = CD_NONE;
};
struct CData {
    CC c; Fmt T, TO; int clips, kind, KPI, UN, streams; char kern[48];
    std::vector<double> q, K, V;   // q [B][d]; K, V [clips][S][d] as the contract sees them (fp8: code x scale)
    std::vector<unsigned char> hq, hk, hv; std::vector<float> amax;   // fp8: amax [2][B][H] as the quantiser left it
    Out P, ML, O;
    size_t ki(int cl, int j, int n) const { return ((size_t)cl * c.S + j) * c.d + n; }
    // key r of a range -> (stream, register set) by the kernel's dealing
    void deal(int r, int& st, int& set) const {
        if (kind == K_ATTN) { const int grp = r / UN; st = grp % 4; set = grp / 4; }
        else if (kind == K_CG) { const int grp = r / 2 / UN; st = grp % 4 * 2 + r % 2; set = grp / 4; }
        else { const int grp = r / KPI / UN; st = grp % 4 * KPI + r % KPI; set = grp / 4; }
    }
};
static void cross_form(CData& x) {
    const CC& c = x.c;
    x.KPI = 1; x.UN = 4; x.kind = K_ATTN;
    if (c.mode == FP8) {
        const int ch = c.d / 16;
        x.kind = K_C8; x.KPI = ch == 32 ? 2 : ch == 16 ? 4 : ch == 8 ? 8 : 1; x.UN = ch == 32 ? 4 : ch == 16 ? 2 : ch == 8 ? 1 : ch <= 64 ? 4 : 2;
        snprintf(x.kern, sizeof x.kern, "k_dec_cross_attn8<%d, %d, %d, %s>", x.KPI, ch <= 64 ? 1 : 2, x.UN, c.nt ? "nt" : "  ");
    } else if (c.mode == BF16) {
        const int nch = (c.d / 8 + 63) / 64;
        if (nch == 1) { x.UN = c.unroll == 8 ? 8 : c.unroll == 2 ? 2 : 4; snprintf(x.kern, sizeof x.kern, "k_dec_cross_attn<bf16, 1, %d, %s>    ", x.UN, c.nt ? "nt" : "  "); }
        else if (c.d % 256 == 0) { x.kind = K_CG; snprintf(x.kern, sizeof x.kern, "k_dec_cross_attn_cg<4, %s>         ", c.nt ? "nt" : "  "); }
        else { x.UN = 2; snprintf(x.kern, sizeof x.kern, "k_dec_cross_attn<bf16, 3, 2, %s>    ", c.nt ? "nt" : "  "); }
    } else {
        const int nch = (c.d / 4 + 63) / 64;
        x.UN = nch == 1 ? 4 : nch == 2 ? 2 : 1;
        snprintf(x.kern, sizeof x.kern, "k_dec_cross_attn<float, %d, %d, %s%s>", nch == 1 ? 1 : nch == 2 ? 2 : 5, x.UN, c.nt ? "nt" : "  ", c.mode == X3 ? ", h2" : "    ");
    }
    x.streams = x.kind == K_CG ? 8 : 4 * x.KPI;
}
static void cross_outputs(CData& x) {
    const CC& c = x.c;
    x.TO = c.mode == F32 ? F_F32 : c.mode == X3 ? F_H2 : F_BF16;
    x.P.make(F_F32, (size_t)c.B * c.splits * c.d); x.ML.make(F_F32, (size_t)c.B * c.splits * c.H * 2); x.O.make(x.TO, (size_t)c.d * c.mpad);
    if (c.splits == 1) { for (int b = 0; b < c.B; b++) for (int n = 0; n < c.d; n++) x.O.live[slab(b, n, c.mpad)] = 1; }
    else { for (size_t i = 0; i < (size_t)c.B * c.splits * c.d; i++) x.P.live[i] = 1; for (size_t i = 0; i < (size_t)c.B * c.splits * c.H * 2; i++) x.ML.live[i] = 1; }
}
static unsigned cross_seed(const CC& c) {   // (not of B: the rows a small and a large launch share hold the same values)
    return 40503u * c.S + 977u * c.d + 7u * c.mode + 3u * c.peaked + 131u * c.rpc + 1013u * (c.zero_head + 1) + 37u * c.outlier;
}
// the queries of clip cl's rows, after its keys: peaked = a key of the clip scaled so that their score is 30 (odd rows: the last key)
static void cross_queries(CData& x, int cl, const std::vector<double>& Ksrc) {
    const CC& c = x.c;
    for (int b = cl * c.rpc; b < (cl + 1) * c.rpc; b++) for (int h = 0; h < c.H; h++) {
        const int win = b % 2 ? c.S - 1 : (int)(rnd() % (unsigned)c.S);
        double n2 = 1e-30;
        for (int e = 0; e < 64; e++) n2 += Ksrc[x.ki(cl, win, 64 * h + e)] * Ksrc[x.ki(cl, win, 64 * h + e)];
        for (int e = 0; e < 64; e++) {
            const float v = c.peaked ? (float)(Ksrc[x.ki(cl, win, 64 * h + e)] * 30.0 / n2) : frand(0.25f);
            const size_t i = (size_t)b * c.d + 64 * h + e;
            x.q[i] = put(x.hq.data(), x.T, i, v);
            if (c.eqq && b % c.rpc == 1) { x.q[i] = x.q[i - c.d]; memcpy(&x.hq[i * esz(x.T)], &x.hq[(i - c.d) * esz(x.T)], esz(x.T)); }   // the clip's second row repeats its first
        }
    }
}
static void cross_prepare(CData& x, const CC& c) {
    x.c = c; x.T = c.mode == BF16 ? F_BF16 : F_F32; x.clips = c.B / c.rpc;
    cross_form(x); cross_outputs(x);
    rs = cross_seed(c);
    const size_t nkv = (size_t)x.clips * c.S * c.d;
    x.q.assign((size_t)c.B * c.d, 0.0); x.hq.assign(x.q.size() * esz(x.T), 0);
    x.K.assign(nkv, 0.0); x.V.assign(nkv, 0.0); x.hk.assign(nkv * esz(x.T), 0); x.hv.assign(nkv * esz(x.T), 0);
    for (int cl = 0; cl < x.clips; cl++) {
        for (int j = 0; j < c.S; j++) for (int n = 0; n < c.d; n++) x.K[x.ki(cl, j, n)] = put(x.hk.data(), x.T, x.ki(cl, j, n), frand(1.0f));
        for (int j = 0; j < c.S; j++) for (int n = 0; n < c.d; n++) x.V[x.ki(cl, j, n)] = put(x.hv.data(), x.T, x.ki(cl, j, n), frand(1.0f));
        cross_queries(x, cl, x.K);
    }
}
static void cross_launch(CData& x) {
    const CC& c = x.c;
    void *dq = to_dev(x.hq), *dk = to_dev(x.hk), *dv = to_dev(x.hv), *da = to_dev(x.amax);
    x.P.up(); x.ML.up(); x.O.up();
    if (c.mode == FP8)
        wh_launch_dec_cross_attn8(0, dq, dk, dv, (const float*)da, (const float*)da + (size_t)c.B * c.H, (float*)x.P.d, (float*)x.ML.d, c.S, c.d, c.H, c.splits, c.B, x.O.d, c.mpad, c.nt);
    else {
        wh_dbg_cross_unroll = c.unroll;
        wh_launch_dec_cross_attn(0, prec_of(c.mode), dq, dk, dv, (float*)x.P.d, (float*)x.ML.d, c.S, c.d, c.H, c.splits, c.B, x.O.d, c.mpad, c.nt, c.rpc);
        wh_dbg_cross_unroll = 4;
    }
    CK(hipGetLastError()); CK(hipDeviceSynchronize());
    x.P.down(); x.ML.down(); x.O.down(); dev_free({dq, dk, dv, da});
}
static float fscale(float am) { return am > 0.0f ? am / 448.0f : 1.0f; }
static float e4m3_value(unsigned char c) {
    const int e = (c >> 3) & 15, m = c & 7;
    const float v = e == 0 ? ldexpf((float)m, -9) : ldexpf((float)(8 + m), e - 10);
    return c & 0x80 ? -v : v;
}
// the kernels' streams in float on the host: every stream keeps an online softmax over its register sets, then the streams are merged
static void cross_emulate(CData& x) {
    const CC& c = x.c;
    const int d = c.d, H = c.H, S = c.S, per = (S + c.splits - 1) / c.splits, ns = x.streams;
    const bool round_p = c.mode == BF16;
    const int epl = c.mode == BF16 ? 8 : c.mode == FP8 ? 16 : 4;   // elements of a head per lane
    x.P.up(); x.ML.up(); x.O.up();
    for (int b = 0; b < c.B; b++) for (int sp = 0; sp < c.splits; sp++) {
        const int cl = c.defect == CD_KVB ? b % x.clips : b / c.rpc, ks = sp * per, j1 = std::min(S, ks + per), n = std::max(0, j1 - ks);
        std::vector<std::vector<std::vector<int>>> keys(ns);
        for (int r = 0; r < n; r++) { int st, set; x.deal(r, st, set); if ((int)keys[st].size() <= set) keys[st].resize(set + 1); keys[st][set].push_back(ks + r); }
        if (c.defect == CD_TAIL) for (auto& st : keys) if (!st.empty() && !st.back().empty()) while ((int)st.back().size() < x.UN) st.back().push_back(j1 - 1);
        std::vector<float> wm((size_t)ns * H, -INFINITY), wl((size_t)ns * H, 0.0f), wo((size_t)ns * d, 0.0f);
        for (int h = 0; h < H; h++) {
            float qf[64], sk = 1.0f, sv = 1.0f;
            if (c.mode == FP8) { sk = fscale(x.amax[(size_t)b * H + h]); sv = fscale(x.amax[(size_t)(c.B + b) * H + (c.defect == CD_SVHEAD0 ? 0 : h)]); }
            for (int e = 0; e < 64; e++) qf[e] = c.mode == FP8 && c.defect != CD_KSCALE ? (float)x.q[(size_t)b * d + 64 * h + e] * sk : (float)x.q[(size_t)b * d + 64 * h + e];
            auto kval = [&](int j, int e) { const size_t i = x.ki(cl, j, 64 * h + e); return c.mode == FP8 ? e4m3_value(x.hk[i]) : (float)x.K[i]; };
            auto vval = [&](int j, int e) { const size_t i = x.ki(cl, j, 64 * h + e); return c.mode == FP8 ? e4m3_value(x.hv[i]) : (float)x.V[i]; };
            for (int st = 0; st < ns; st++) {
                float mrun = -INFINITY, lrun = 0.0f, o[64] = {0};
                for (auto& set : keys[st]) {
                    if (set.empty()) continue;
                    float s[16], mx = mrun;
                    for (size_t u = 0; u < set.size(); u++) {   // a lane's epl products in a chain, then the head's lanes pairwise
                        float part[16];
                        for (int l = 0; l < 64 / epl; l++) { float t = 0.0f; for (int e = l * epl; e < (l + 1) * epl; e++) t += qf[e] * kval(set[u], e); part[l] = t; }
                        for (int o = 1; o < 64 / epl; o *= 2) for (int l = 0; l < 64 / epl; l += 2 * o) part[l] += part[l + o];
                        s[u] = part[0]; mx = fmaxf(mx, part[0]);
                    }
                    const float scale = expf(mrun - mx);
                    lrun *= scale;
                    for (int e = 0; e < 64; e++) o[e] *= scale;
                    for (size_t u = 0; u < set.size(); u++) {
                        const float p = expf(s[u] - mx), pr = round_p ? bf2f(f2bf(p)) : p;
                        lrun += p;
                        for (int e = 0; e < 64; e++) o[e] += pr * vval(set[u], e);
                    }
                    mrun = mx;
                }
                wm[(size_t)st * H + h] = mrun; wl[(size_t)st * H + h] = lrun;
                for (int e = 0; e < 64; e++) wo[(size_t)st * d + 64 * h + e] = o[e];
            }
            float M = -INFINITY;
            for (int st = 0; st < ns; st++) M = fmaxf(M, wm[(size_t)st * H + h]);
            float num[64] = {0}, den = 0.0f;
            for (int st = 0; st < ns; st++) {
                if (c.defect == CD_ODDPAR && st % 2) continue;
                const float mw = wm[(size_t)st * H + h];
                const float sc = mw == -INFINITY ? (c.defect == CD_NOSKIP ? expf(mw - M) : 0.0f) : c.defect == CD_NORESCALE ? 1.0f : expf(mw - M);
                for (int e = 0; e < 64; e++) num[e] += sc * wo[(size_t)st * d + 64 * h + e];
                den += sc * wl[(size_t)st * H + (c.defect == CD_DENHEAD ? (h + 1) % H : h)];
            }
            if (c.defect == CD_DENHEAD && h + 1 < H) {   // (the neighbour's sums are not there yet in this loop order: take them from its keys directly)
                den = 0.0f;
                for (int j = ks; j < j1; j++) { float t = 0.0f; for (int e = 0; e < 64; e++) t += (float)x.q[(size_t)b * d + 64 * (h + 1) + e] * (float)x.K[x.ki(cl, j, 64 * (h + 1) + e)]; den += expf(t - M); }
            }
            for (int e = 0; e < 64; e++) {
                const float v = c.mode == FP8 ? num[e] * sv : num[e];
                if (c.splits == 1) x.O.set(slab(b, 64 * h + e, c.defect == CD_PITCH ? c.B : c.mpad), v / den);
                else x.P.set(((size_t)b * c.splits + sp) * d + 64 * h + e, v);
            }
            if (c.splits != 1) { x.ML.set(((size_t)b * c.splits + sp) * H * 2 + h, M); x.ML.set(((size_t)b * c.splits + sp) * H * 2 + H + h, den); }
        }
    }
}
struct CRes { double ratio = 0, r_m = 0, r_den = 0; long guard = 0; unsigned long long h[3] = {0, 0, 0}; bool ok() const { return ratio <= 1.0 && r_m <= 1.0 && r_den <= 1.0 && guard == 0; } };
static CRes cross_verify(const CData& x) {
    const CC& c = x.c;
    const int d = c.d, H = c.H, S = c.S, per = (S + c.splits - 1) / c.splits;
    CRes r;
    std::vector<double> rm((size_t)c.B * c.splits * H, 0.0), rd(rm.size(), 0.0);
    r.ratio = par_rows((long)c.B * c.splits * H, [&](long i) {
        const int h = (int)(i % H), sp = (int)(i / H % c.splits), b = (int)(i / H / c.splits), cl = b / c.rpc;
        const int ks = sp * per, j1 = std::min(S, ks + per), n = j1 - ks;
        const size_t pi = ((size_t)b * c.splits + sp) * d + 64 * h, mi = ((size_t)b * c.splits + sp) * H * 2;
        if (n <= 0) {   // an empty range: exactly {0, -inf, 0}
            bool ok = x.ML.at(mi + h) == -INFINITY && x.ML.at(mi + H + h) == 0.0;
            for (int e = 0; e < 64; e++) ok = ok && x.P.at(pi + e) == 0.0;
            return ok ? 0.0 : 1e30;
        }
        std::vector<double> sc(n), mag(n);
        for (int j = 0; j < n; j++) {
            double a = 0, m = 0;
            for (int e = 0; e < 64; e++) { const double t = x.q[(size_t)b * d + 64 * h + e] * x.K[x.ki(cl, ks + j, 64 * h + e)]; a += t; m += fabs(t); }
            sc[j] = a; mag[j] = m;
        }
        std::vector<int> cnt(x.streams, 0);
        int kps = 0;
        for (int j = 0; j < n; j++) { int st, set; x.deal(j, st, set); kps = std::max(kps, ++cnt[st]); }
        const double nsets = (kps + x.UN - 1) / x.UN;
        Soft f;
        soft_ref(n, sc.data(), mag.data(), [&](int j, int e) { return x.V[x.ki(cl, ks + j, 64 * h + e)]; }, c.mode == FP8 ? 24 : 12,c.mode == BF16 ? ldexp(1.0, -8) : 0.0,
                 2.0 * kps + 3 * nsets + x.streams + 16 + (c.mode == FP8 ? 1 : 0), kps + 3 * nsets + x.streams + 16, f);
        Worst w;
        if (c.splits == 1) {
            for (int e = 0; e < 64; e++) w.see(x.O.at(slab(b, 64 * h + e, c.mpad)), f.want[e], f.eb[e] + half_ulp(x.TO, fabs(f.want[e]) + f.eb[e]));
        } else {
            const double dg = x.ML.at(mi + H + h);
            for (int e = 0; e < 64; e++) w.see(x.P.at(pi + e) / dg, f.want[e], f.eb[e] + U * (fabs(f.want[e]) + f.eb[e]));
            Worst wm, wd;
            wm.see(x.ML.at(mi + h), f.m, f.e_m); wd.see(dg, f.den, f.e_den + U * f.den);
            rm[i] = wm.ratio; rd[i] = wd.ratio;
        }
        return w.ratio;
    });
    r.r_m = *std::max_element(rm.begin(), rm.end()); r.r_den = *std::max_element(rd.begin(), rd.end());
    r.guard = x.P.guard() + x.ML.guard() + x.O.guard();
    r.h[0] = x.O.hash(); r.h[1] = x.P.hash(); r.h[2] = x.ML.hash();
    return r;
}
static unsigned long long cross_row_hash(const CData& x, int b) {   // everything the kernel wrote for row b
    const CC& c = x.c;
    if (c.splits == 1) return slab_row_hash(x.O, b, c.d, c.mpad);
    return fnv1a(&x.ML.h[(size_t)b * c.splits * c.H * 2 * 4], (size_t)c.splits * c.H * 2 * 4, fnv1a(&x.P.h[(size_t)b * c.splits * c.d * 4], (size_t)c.splits * c.d * 4));
}
static double worst_cross = 0;
static int cross_report(const CData& x, const CRes& r, const char* tag = "") {
    const CC& c = x.c;
    printf("%s %s %-18s d %4d H %2d S %4d splits %2d B %2d rpc %d %s: err/bound out %.3f m %.3f den %.3f guard %ld  out %016llx part %016llx ml %016llx  %s%s\n", x.kern, mode_name[c.mode], c.what, c.d,
           c.H, c.S, c.splits, c.B, c.rpc, c.peaked ? "peaked" : "small ", r.ratio, r.r_m, r.r_den, r.guard, r.h[0], r.h[1], r.h[2], r.ok() ? "ok" : "MISMATCH", tag);
    worst_cross = std::max(worst_cross, std::max(r.ratio, std::max(r.r_m, r.r_den)));
    return r.ok() ? 0 : 1;
}
static int cross_case(const CC& c, CData* keep = nullptr) {
    CData local; CData& x = keep ? *keep : local;
    cross_prepare(x, c); cross_launch(x);
    return cross_report(x, cross_verify(x));
}
static CC cc(const char* what, Mode md, int d, int S, int splits, bool nt = false, int peaked = 0) {
    CC c; c.what = what; c.mode = md; c.d = d; c.H = d / 64; c.S = S; c.splits = splits; c.nt = nt; c.peaked = peaked;
    return c;
}
static int group_cross() {
    int bad = 0, k = 0;
    // bf16, one chunk per lane
    for (int d : {128, 256, 512}) {
        for (int S : {1, 5, 16, 17, 33, 1500}) for (int sp : {1, 4}) bad |= cross_case(cc(S == 5 ? "three waves idle" : "small", BF16, d, S, sp, (k++ & 1) != 0));
        bad |= cross_case(cc("32 ranges", BF16, d, 1500, 32, true));
        bad |= cross_case(cc("7 ranges empty", BF16, d, 100, 32));
        bad |= cross_case(cc("peaked", BF16, d, 1500, 4, false, 1));
    }
    for (int S : {5, 17, 33, 1500}) for (int sp : {1, 4}) {   // the three unrolls agree within the bounds; whether their bits agree is printed, not required
        unsigned long long hh[3]; int i = 0;
        for (int un : {2, 4, 8}) { CC c = cc("unroll", BF16, 128, S, sp, S == 33); c.unroll = un; c.peaked = S == 17; CData x; bad |= cross_case(c, &x); hh[i++] = x.c.splits == 1 ? x.O.hash() : x.P.hash(); }
        printf("    unroll 2 / 4 / 8 at S %d splits %d: hashes %s\n", S, sp, hh[0] == hh[1] && hh[1] == hh[2] ? "agree" : "differ");
    }
    // bf16, d = 640: <bf16, 3, 2>
    for (int S : {1, 5, 17, 1500}) for (int sp : {1, 4}) bad |= cross_case(cc("d 640", BF16, 640, S, sp, (k++ & 1) != 0, S == 1500 && sp == 4));
    // bf16 wide: _cg
    for (int d : {768, 1280}) {
        for (int S : {1, 2, 15, 16, 17}) bad |= cross_case(cc(S == 1 ? "odd parity idle" : "wide", BF16, d, S, S == 17 ? 4 : 1, (k++ & 1) != 0));
        for (int sp : {1, 3, 8}) bad |= cross_case(cc(sp == 3 ? "odd range lengths" : "wide", BF16, d, 1500, sp, (k++ & 1) != 0, sp == 8));
    }
    // f32 and f16x3
    for (int d : {128, 512, 768, 1280}) for (int S : {1, 5, 17, 1500}) for (int sp : {1, 4}) bad |= cross_case(cc(d == 768 ? "idle chunks" : "f32", F32, d, S, sp, (k++ & 1) != 0, S == 1500 && sp == 1));
    for (int d : {128, 1280}) for (int S : {5, 1500}) bad |= cross_case(cc("h2 slab", X3, d, S, 1, (k++ & 1) != 0, S == 5));
    // beam rows: three rows per clip, the second repeating the first
    for (int d : {128, 768}) for (int sp : {1, 4}) {
        CC c = cc("beam rows", BF16, d, 33, sp); c.B = 6; c.rpc = 3; c.eqq = true;
        CData x; bad |= cross_case(c, &x);
        const bool eq = cross_row_hash(x, 0) == cross_row_hash(x, 1) && cross_row_hash(x, 3) == cross_row_hash(x, 4), ne = cross_row_hash(x, 0) != cross_row_hash(x, 2) && cross_row_hash(x, 0) != cross_row_hash(x, 3);
        printf("    rows 0 = 1 and 3 = 4 (equal q, one clip): row hashes %s; rows 0, 2, 3: %s\n", eq ? "equal" : "DIFFERENT: MISMATCH", ne ? "distinct" : "EQUAL: MISMATCH");
        bad |= !eq || !ne;
    }
    // more than 512 workgroups: the 72 KB LDS reservation in force; the rows a small launch shares must come out the same
    {
        CC big = cc("640 workgroups", BF16, 128, 100, 32); big.B = 20;
        CC sm = cc("the same, 2 rows", BF16, 128, 100, 32);
        CData xb, xs; bad |= cross_case(big, &xb); bad |= cross_case(sm, &xs);
        const bool eq = cross_row_hash(xb, 0) == cross_row_hash(xs, 0) && cross_row_hash(xb, 1) == cross_row_hash(xs, 1);
        printf("    rows 0 and 1 of the large and the small launch: row hashes %s\n", eq ? "equal" : "DIFFERENT: MISMATCH");
        bad |= !eq;
    }
    printf("worst err/bound cross %.3f\n", worst_cross);
    return bad;
}

// ===== fp8: the quantiser, then the attention over its codes ===============================================================================
static unsigned char e4m3_quant(float f) {   // OCP e4m3, round to nearest even, saturating
    const unsigned char sign = std::signbit(f) ? 0x80 : 0;
    const float a = fminf(fabsf(f), 448.0f);
    if (!(a == a)) return sign | 0x7f;
    if (a < ldexpf(1.0f, -6)) return sign | (unsigned char)nearbyintf(ldexpf(a, 9));   // subnormals, step 2^-9 (8 steps reach the smallest normal's code)
    int ex; frexpf(a, &ex); ex -= 1;                                                   // a = 1.xxx 2^ex
    int m = (int)nearbyintf(ldexpf(a, 3 - ex));                                        // 8 .. 16
    if (m == 16) { m = 8; ex += 1; }
    return sign | (unsigned char)(((ex + 7) << 3) | (m - 8));
}
struct QRes { long amax_bad = 0, diff = 0, ties = 0, guard = 0; unsigned long long h[2] = {0, 0}; bool ok() const { return amax_bad == 0 && diff == ties && guard == 0; } };
// planes: K then V, [2][B][S][d] bf16.  Runs the quantiser (device, or host with the defect), checks it, leaves x ready for the attention.
static QRes fp8_quantise(CData& x, const CC& c) {
    x.c = c; x.T = F_BF16; x.clips = c.B;
    cross_form(x); cross_outputs(x);
    rs = cross_seed(c);
    const int B = c.B, S = c.S, d = c.d, H = c.H;
    const size_t nkv = (size_t)B * S * d;
    std::vector<double> src(2 * nkv); std::vector<unsigned char> hsrc(2 * nkv * 2);
    x.q.assign((size_t)B * d, 0.0); x.hq.assign(x.q.size() * 2, 0);
    for (int cl = 0; cl < B; cl++) {
        for (int pl = 0; pl < 2; pl++) for (int j = 0; j < S; j++) for (int n = 0; n < d; n++) {   // the planes' maxima differ: K within 1, V within 2
            float v = frand(pl ? 2.0f : 1.0f);
            if (c.zero_head == n / 64 && cl == pl) v = 0.0f;
            if (c.outlier && pl == 1 && n / 64 == 1 % H) v = (j == std::min(124, S - 1) && n % 64 == 7 + cl) ? -3.0f : v * 0.01f;
            src[pl * nkv + x.ki(cl, j, n)] = put(hsrc.data(), F_BF16, pl * nkv + x.ki(cl, j, n), v);
        }
        cross_queries(x, cl, src);
    }
    Out AM, C8;
    AM.make(F_F32, (size_t)2 * B * H); C8.make(F_U8, 2 * nkv);
    for (size_t i = 0; i < (size_t)2 * B * H; i++) { AM.live[i] = 1; memset(&AM.h0[4 * i], 0, 4); }   // the caller zeroes amax
    for (size_t i = 0; i < 2 * nkv; i++) C8.live[i] = 1;
    AM.up(); C8.up();
    auto host_amax = [&](size_t pb, int h, bool defect) {
        float am = 0.0f;
        for (int j = 0; j < S; j++) { if (defect && j % 125 == 124) continue; for (int e = 0; e < 64; e++) am = fmaxf(am, fabsf((float)src[(pb * S + j) * d + 64 * h + e])); }
        return am;
    };
    if (g_host) {
        for (size_t pb = 0; pb < (size_t)2 * B; pb++) for (int h = 0; h < H; h++) AM.set(pb * H + h, host_amax(pb, h, c.defect == CD_AMAXROW));
        for (size_t i = 0; i < 2 * nkv; i++) { const float sc = fscale((float)AM.at(i / ((size_t)S * d) * H + i % d / 64)); C8.h[i] = e4m3_quant((float)src[i] / sc); }
    } else {
        void* ds = to_dev(hsrc);
        wh_launch_kv_quant(0, ds, (unsigned*)AM.d, C8.d, 2L * B, S, d, H);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        dev_free({ds});
    }
    AM.down(); C8.down();
    QRes r;
    for (size_t pb = 0; pb < (size_t)2 * B; pb++) for (int h = 0; h < H; h++) { const float want = host_amax(pb, h, false); r.amax_bad += memcmp(&want, &AM.h[4 * (pb * H + h)], 4) != 0; }
    for (size_t i = 0; i < 2 * nkv && r.amax_bad == 0; i++) {
        const float sc = fscale((float)AM.at(i / ((size_t)S * d) * H + i % d / 64)), qf = (float)src[i] / sc;
        const unsigned char want = e4m3_quant(qf), got = C8.h[i];
        if (want == got) continue;
        r.diff++;
        // one code step apart, the exact quotient within one f32 ulp of the tie between the two codes
        const double qd = src[i] / (double)sc, mid = 0.5 * ((double)e4m3_value(want) + (double)e4m3_value(got)), ulp = ldexp(1.0, std::ilogb(fabs(qd) > 0 ? fabs(qd) : 1e-30) - 23);
        if ((want ^ got) < 0x80 && abs((int)(want & 0x7f) - (int)(got & 0x7f)) == 1 && fabs(qd - mid) <= ulp) r.ties++;
    }
    r.guard = AM.guard() + C8.guard(); r.h[0] = AM.hash(); r.h[1] = C8.hash();
    // the attention's operands: the codes and scales as the quantiser left them
    x.amax.resize((size_t)2 * B * H);
    for (size_t i = 0; i < x.amax.size(); i++) x.amax[i] = (float)AM.at(i);
    x.hk.assign(C8.h.begin(), C8.h.begin() + nkv); x.hv.assign(C8.h.begin() + nkv, C8.h.begin() + 2 * nkv);
    x.K.resize(nkv); x.V.resize(nkv);
    for (size_t i = 0; i < nkv; i++) {
        const size_t cl = i / ((size_t)S * d); const int h = (int)(i % d / 64);
        x.K[i] = (double)e4m3_value(x.hk[i]) * (double)fscale(x.amax[cl * H + h]);
        x.V[i] = (double)e4m3_value(x.hv[i]) * (double)fscale(x.amax[(B + cl) * H + h]);
    }
    return r;
}
static int quant_report(const CData& x, const QRes& r) {
    const CC& c = x.c;
    printf("k_kv_absmax + k_kv_quant          %s %-18s d %4d H %2d S %4d planes x clips %d: amax differing %ld  codes differing %ld (at a tie: %ld) guard %ld  amax %016llx codes %016llx  %s\n", mode_name[FP8],
           c.what, c.d, c.H, c.S, 2 * c.B, r.amax_bad, r.diff, r.ties, r.guard, r.h[0], r.h[1], r.ok() ? "ok" : "MISMATCH");
    return r.ok() ? 0 : 1;
}
static int cross8_case(const CC& c) {
    CData x;
    int bad = quant_report(x, fp8_quantise(x, c));
    cross_launch(x);
    return bad | cross_report(x, cross_verify(x));
}
static int group_cross8() {
    int bad = 0, k = 0;
    worst_cross = 0;
    for (int d : {128, 256, 512, 768, 1280}) {
        for (int S : {1, 9, 125, 126, 1500}) for (int sp : {1, 4}) {
            CC c = cc(S == 126 ? "rows_per_wg edge" : "small", FP8, d, S, sp, (k++ & 1) != 0, S == 1500 && sp == 4);
            if (S == 9) { c.what = "an all-zero head"; c.zero_head = 1; }
            if (S == 125 || S == 126) c.outlier = 1;
            bad |= cross8_case(c);
        }
    }
    printf("worst err/bound cross8 %.3f\n", worst_cross);
    return bad;
}

// ===== --selftest: host only ===============================================================================================================
static double st_worst[3] = {0, 0, 0};
static int self_line(int fam, const char* what, bool defect, double ratio, long exact) {
    static const char* family[] = {"self", "cross", "cross8"};
    const bool caught = ratio > 1.0 || exact != 0;
    if (!defect) {
        st_worst[fam] = std::max(st_worst[fam], ratio);
        printf("selftest %-6s clean: %-66s err/bound %.3f exact %ld  %s\n", family[fam], what, ratio, exact, caught ? "MISMATCH" : "ok");
        return caught ? 1 : 0;
    }
    printf("selftest %-6s defect: %-65s err/bound %.3g exact %ld  %s\n", family[fam], what, ratio, exact, caught ? "caught" : "NOT CAUGHT");
    return caught ? 0 : 1;
}
static int selftest() {
    g_host = true;
    int bad = 0;
    auto self = [&](Mode md, int g, int peaked, bool pfx, int defect, const char* what) {
        SC c; c.mode = md; c.g = g; c.peaked = peaked; c.pfx = pfx; c.defect = defect;
        if (pfx) { c.off[0] = 0; c.off[1] = 5; c.off[2] = g + 7; }
        SData s; self_prepare(s, c); self_emulate(s);
        const SRes r = self_verify(s);
        bad |= self_line(0, what, defect != SD_NONE, r.ratio, r.guard + r.append);
    };
    for (Mode md : {BF16, F32, X3}) for (int pk : {0, 1}) self(md, 129, pk, false, SD_NONE, (std::string(pk ? "g 129, peaked, " : "g 129, small, ") + mode_name[md]).c_str());
    for (Mode md : {BF16, F32}) self(md, 70, 0, true, SD_NONE, (std::string("g 70, prefixes 0 / 5 / idle, ") + mode_name[md]).c_str());
    self(F32, 447, 0, false, SD_NONE, "g 447, the last row of the plane, f32");
    self(F32, 129, 0, false, SD_NOCUR, "1 the current key left out");
    self(BF16, 129, 0, false, SD_ONEMORE, "2 one cache row too many read (j <= pos)");
    self(BF16, 70, 0, true, SD_NOADV, "3 prefixes: adv ignored");
    self(BF16, 70, 0, false, SD_MASKMUL, "4 a masked V row multiplied in, not selected out");
    self(BF16, 70, 0, true, SD_LOCALROW, "5 the append at the local row");
    {   // the prefixed rows against their un-prefixed launches, in the emulation
        const int off[3] = {0, 5, 70};
        bad |= self_pfx_case(BF16, 70, off, true);
    }

    auto cross = [&](CC c, int defect, const char* what) {
        c.defect = defect;
        CData x; cross_prepare(x, c); cross_emulate(x);
        const CRes r = cross_verify(x);
        bad |= self_line(1, what, defect != CD_NONE, std::max(r.ratio, std::max(r.r_m, r.r_den)), r.guard);
    };
    cross(cc("", BF16, 128, 1500, 1), CD_NONE, "bf16 d 128 S 1500, slab");
    cross(cc("", BF16, 128, 1500, 4, false, 1), CD_NONE, "bf16 d 128 S 1500 splits 4, peaked");
    cross(cc("", BF16, 128, 100, 32), CD_NONE, "bf16 d 128 S 100 splits 32 (7 empty)");
    cross(cc("", BF16, 640, 17, 1), CD_NONE, "bf16 d 640 S 17");
    cross(cc("", BF16, 768, 1500, 3, false, 1), CD_NONE, "_cg d 768 S 1500 splits 3, peaked");
    cross(cc("", BF16, 768, 1, 1), CD_NONE, "_cg d 768 S 1");
    cross(cc("", F32, 128, 1500, 1, false, 1), CD_NONE, "f32 d 128 S 1500, peaked");
    cross(cc("", F32, 768, 17, 4), CD_NONE, "f32 d 768 S 17 splits 4");
    cross(cc("", X3, 128, 1500, 1), CD_NONE, "f16x3 d 128 S 1500, h2 slab");
    cross(cc("", F32, 128, 17, 1), CD_TAIL, "6 the clamped tail key counted");
    cross(cc("", F32, 128, 1500, 4, false, 1), CD_NORESCALE, "7 waves merged without exp(m - M)");
    cross(cc("", F32, 128, 17, 4), CD_DENHEAD, "8 the denominator from the neighbouring head");
    cross(cc("", BF16, 128, 100, 32), CD_NOSKIP, "9 an empty wave's -inf not skipped");
    cross(cc("", BF16, 768, 17, 1), CD_ODDPAR, "10 _cg: the odd-parity stream dropped");
    { CC c = cc("", BF16, 128, 33, 1); c.B = 6; c.rpc = 3; cross(c, CD_NONE, "beam rows, 3 per clip"); cross(c, CD_KVB, "11 beam: kvb = b"); }
    cross(cc("", BF16, 128, 17, 1), CD_PITCH, "12 the slab indexed with pitch B instead of mpad");

    auto c8 = [&](CC c, int defect, const char* what) {
        c.defect = defect;
        CData x;
        const QRes q = fp8_quantise(x, c);
        cross_emulate(x);
        const CRes r = cross_verify(x);
        bad |= self_line(2, what, defect != CD_NONE, std::max(r.ratio, std::max(r.r_m, r.r_den)), r.guard + q.amax_bad + (q.diff - q.ties) + q.guard);
    };
    { CC c = cc("", FP8, 128, 126, 1); c.outlier = 1; c8(c, CD_NONE, "fp8 d 128 S 126, an outlier maximum"); c8(c, CD_AMAXROW, "15 fp8: amax off by one row at a workgroup boundary"); c8(c, CD_SVHEAD0, "14 fp8: V's scale from head 0"); }
    { CC c = cc("", FP8, 512, 1500, 4, false, 1); c8(c, CD_NONE, "fp8 d 512 S 1500 splits 4, peaked"); }
    { CC c = cc("", FP8, 1280, 9, 1); c.zero_head = 1; c8(c, CD_NONE, "fp8 d 1280 S 9, an all-zero head"); }
    c8(cc("", FP8, 256, 125, 4), CD_KSCALE, "13 fp8: K's scale not applied");
    printf("selftest worst err/bound of the emulation: self %.3f cross %.3f cross8 %.3f\n", st_worst[0], st_worst[1], st_worst[2]);
    printf("selftest %s\n", bad ? "FAILED" : "passed");
    return bad;
}

// ===== --time: whisper-base decode shapes, 64 clips, bf16 ==================================================================================
static int timing() {
    const int B = 64, d = 512, H = 8, tc = 448, S = 1500, splits = 4, mpad = 64;
    void *qkv, *kc, *vc, *o, *ck, *cv; float *part, *ml; int* pos;
    const size_t cache = (size_t)B * H * tc * 64 * 2, kv = (size_t)B * S * d * 2;
    CK(hipMalloc(&qkv, (size_t)B * 3 * d * 2)); CK(hipMalloc(&kc, cache)); CK(hipMalloc(&vc, cache)); CK(hipMalloc(&o, (size_t)d * mpad * 2)); CK(hipMalloc(&ck, kv)); CK(hipMalloc(&cv, kv));
    CK(hipMalloc((void**)&part, (size_t)B * splits * d * 4)); CK(hipMalloc((void**)&ml, (size_t)B * splits * H * 2 * 4)); CK(hipMalloc((void**)&pos, 4));
    CK(hipMemset(qkv, 0, (size_t)B * 3 * d * 2)); CK(hipMemset(kc, 0, cache)); CK(hipMemset(vc, 0, cache)); CK(hipMemset(ck, 0, kv)); CK(hipMemset(cv, 0, kv));
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
        printf("time %-44s median %9.1f us  min %9.1f  max %9.1f\n", name, us[12], us.front(), us.back());
    };
    for (int g : {4, 64, 447}) {
        CK(hipMemcpy(pos, &g, 4, hipMemcpyHostToDevice));
        char name[64]; snprintf(name, sizeof name, "k_dec_self_attn bf16 64 clips x 8 heads g %d", g);
        timed(name, [&]() { wh_launch_dec_self_attn(0, WH_PREC_BF16, qkv, kc, vc, o, pos, d, H, tc, B, mpad, nullptr); });
    }
    for (bool nt : {false, true})
        timed(nt ? "k_dec_cross_attn bf16 64 clips splits 4 nt" : "k_dec_cross_attn bf16 64 clips splits 4", [&]() { wh_launch_dec_cross_attn(0, WH_PREC_BF16, qkv, ck, cv, part, ml, S, d, H, splits, B, o, mpad, nt, 1); });
    CK(hipGetLastError());
    dev_free({qkv, kc, vc, o, ck, cv, part, ml, pos});
    return 0;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::string arg = argc > 1 ? argv[1] : "";
    if (arg == "--selftest") return selftest() ? 1 : 0;
    if (arg == "--time") return timing();
    if (!arg.empty() && arg != "self" && arg != "reorder" && arg != "cross" && arg != "cross8") { fprintf(stderr, "usage: dec_attn_check [self | reorder | cross | cross8 | --selftest | --time]\n"); return 2; }
    int bad = 0;
    for (const char* grp : {"self", "reorder", "cross", "cross8"}) {
        if (!arg.empty() && arg != grp) continue;
        const auto t0 = std::chrono::steady_clock::now();
        bad |= !strcmp(grp, "self") ? group_self() : !strcmp(grp, "reorder") ? group_reorder() : !strcmp(grp, "cross") ? group_cross() : group_cross8();
        printf("group %s: %.1f s wall\n", grp, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    return bad ? 1 : 0;
}
