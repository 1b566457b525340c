// lm_check.cpp — the kernels that turn hidden rows into a token, each alone through the library's own launchers: k_lm_head (wh_lm_head.hip),
// k_lm_head_tile (wh_gemm8.hip), k_lm_head_tile_x3 (wh_gemm8x.hip) with their shared epilogue (wh_lm_tile.h), k_argmax_finish with the fused
// next-position embedding, k_nospeech_finish, k_lang_head / k_lang_finish and k_dec_embed (wh_lm_head.hip).  The program links libwhisper_hip.so and calls only launchers declared in wh_kernels.h, steered by wh_dbg_lm_mt,
// wh_dbg_lm_blocks_per_cu and WH_LM_TILE_MIN_ROWS (read at every launch decision), so the same source builds against any revision of the library.
// Data come from the program's own LCG: no model, no Python.
//
// Two levels, so that GEMM rounding and selection logic stay apart:
//
//  VALUES.  For every operand set one plain k_lm_head launch keeps every logit (the reference row set L0).  Each logit is held to a float64
//   product of the operands as the kernel sees them (rounded to bf16, fp16 limb pairs decoded exactly, or f32), with the final LayerNorm restated
//   from ln_part, ln_s and bias.  Per element the bound is built from the operands, as tools/dec_gemm_check.cpp does (U = 2^-24):
//     accumulator  ((c K + 8) U) sum|x w|, c = 1, or 3 for limb pairs, + 4 U sum|x w| for their dropped lo.lo term;
//     LN fold      mean and rstd carry the f32 error of their own sums (tiles + 2 additions, the E[x^2] - mean^2 difference, one rsqrt), each operation
//                  of rstd (acc - mean s) + c one U of its result; one more U for the stored f32.
//   A NaN or infinite expectation must be met exactly (NaN by a NaN).
//
//  SELECTION is exact on the kernel's own logits.  Every other launch of the operand set — any RULES x LP x REP variant, any position, any row
//   grouping, the tile kernels — must store logits that are bit for bit L0's (two NaNs count as equal) and nothing else, and from L0's f32
//   values the host recomputes what the contract says of everything else: the allowed ranges (rule 4 at gen 0, the row state later), the suppress
//   mask of the position (mask_first at gen 0, else mask_base) OR-ed with the row's touched bits, the masked argmax with the lowest index winning
//   a tie, the timestamp logits (-inf where not allowed), the side logits of the touched ids, the probe.  These must be equal, not close.
//   Partials are implementation detail: their host merge is checked, not their layout — the merged (max, index) exactly, the merged sum of
//   exp(v - max) within the bound below.  Every slot the contract leaves alone (rows m >= M of a [part][x_mpad] array, logits rows of a row with
//   logits_sel = -1 or of a position that is not kept, side entries of untouched ids, timestamp rows m >= M) and 64 guard words on BOTH sides of
//   every output buffer must come back unchanged.
//   Every LP launch of k_lm_head carries a probe, on an id the masks suppress, the tile kernels' where they write one.  The tile kernels write a probe only without the rules and without the
//   bitmap (their rules variants have none, and with the bitmap a touched id's accumulator is NaN by the time the probe is read: measured here, a
//   touched probe id came out NaN where k_lm_head gives the raw logit), so they decline such a call (WhLmTile::applicable) and wh_launch_lm_head
//   gives it to k_lm_head.  Every launch here goes through wh_launch_lm_head; the tool asks the library which kernel that is, requires the answer
//   above, and prints the kernel that ran.
//
//  The bound of anything that went through ts_exp (wh_common.h: exp(x) = v_exp_f32(x * log2 e), x <= 0).  The accuracy taken for
//   v_exp_f32, 1 ulp, is an ASSUMPTION: no document this project keeps states it (it is the figure usual for the transcendental unit); the
//   device used 13 % of the bound built on it (profiles/lm_check.txt), so an instruction several ulp off would still pass.  x itself is an f32 difference (U |x|), log2 e is a rounded constant (U relative) and the product is rounded
//   (U relative): the argument of the exponential is off by at most 3 U |x| log2 e, which the exponential turns into a relative error of 3 U |x|;
//   the instruction adds 2 U (one ulp).  A term exp(v - m) that is later moved to a larger maximum (s * ts_exp(m - m')) picks up the same again
//   for each move — but the moves' arguments all have one sign and add up to v - max, so over L evaluations and L multiplications the term's
//   relative error is at most (3 |v - max| + 3 L) U.  Each f32 addition that the term's partial sum passes through adds U.  With A additions:
//       |sum - exact| <= sum over the ids of exp(v - max) (3 |v - max| + 3 L + A) U   (+ 1e-37: results below the normal range may be flushed)
//   L and A follow from the kernel's structure: k_lm_head keeps an online pair per lane (at most one move per logit the lane sees, one more to the
//   row's maximum: L = 4 tiles + 2, A = 4 tiles + 2); the tile kernels add exp(v - row maximum) in a second pass (L = 1, A = 16 + 2) and merge four
//   waves (L + 3, A + 3).  Nothing is fitted to what the kernels give.  A row whose maximum is +inf has no sum to check (exp(inf - inf)).
//
//   lm_check [head | tile | finish | lang | embed]   one group (none: all); one line per case with the worst err/bound ratios, the count of
//                                           exact conditions that failed, the guard result and an FNV-1a hash of each raw output; MISMATCH in the
//                                           line and a non-zero exit status on failure
//   lm_check --selftest   host only (no HIP call): each contract carried out in the kernels' working precision (f32 accumulation, f32 LayerNorm
//                         statistics in the kernels' quarter order, exp through exp2f(x * log2 e) in f32, the lanes' online pairs and the
//                         partial layout of each kernel) must stay within the bounds, and the same with one defect at a time must exceed a bound
//                         or fail an exact condition.
//   lm_check --time       launch times on the whisper-base shapes (informational)
// Build: hipcc --offload-arch=gfx950 -O2 -std=c++17 tools/lm_check.cpp -o tools/lm_check -Lwhisper-rust-ort_amd -lwhisper_hip -Wl,-rpath,'$ORIGIN/../whisper-rust-ort_amd'
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
static const long GUARD = 64;                     // guard words on both sides of every output buffer
static const int NONE_IDX = 0x7fffffff;
enum Mode { BF16, F32, H2 };
static const char* mode_name[] = {"bf16", "f32 ", "h2  "};
static bool g_host = false;                       // --selftest: no device, the outputs come from the host emulation

static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0; return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }   // RNE
static unsigned fbits(float f) { unsigned u; memcpy(&u, &f, 4); return u; }
static float bitsf(unsigned u) { float f; memcpy(&f, &u, 4); return f; }
static bool same_f(float a, float b) { return fbits(a) == fbits(b) || (a != a && b != b); }
static unsigned rs = 1;
static unsigned rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static float frand(float a) { return ((int)(rnd() & 0xffff) - 32768) / 32768.0f * a; }
static unsigned long long fnv1a(const void* p, size_t n, unsigned long long h = 1469598103934665603ull) {
    for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}
static size_t esz(Mode f) { return f == BF16 ? 2 : 4; }
static int prec_of(Mode m) { return m == BF16 ? WH_PREC_BF16 : m == F32 ? WH_PREC_F32 : WH_PREC_F16X3; }
// h2 (wh_common.h): 32 consecutive elements take 128 bytes, [32 x fp16 hi | 32 x fp16 lo]
static size_t h2_hi(size_t i) { return (i >> 5) * 128 + (i & 31) * 2; }
// stores v in the mode's operand format; hi / lo = what the kernel sees (lo = 0 unless limb pairs)
static void put(unsigned char* b, Mode f, size_t i, float v, float& hi, float& lo) {
    lo = 0.0f;
    if (f == BF16) { const unsigned short h = f2bf(v); memcpy(b + 2 * i, &h, 2); hi = bf2f(h); return; }
    if (f == F32) { memcpy(b + 4 * i, &v, 4); hi = v; return; }
    const _Float16 h = (_Float16)v, l = (_Float16)(v - (float)h);
    memcpy(b + h2_hi(i), &h, 2); memcpy(b + h2_hi(i) + 64, &l, 2);
    hi = (float)h; lo = (float)l;
}
static void get(const unsigned char* b, Mode f, size_t i, float& hi, float& lo) {
    lo = 0.0f;
    if (f == BF16) { unsigned short h; memcpy(&h, b + 2 * i, 2); hi = bf2f(h); return; }
    if (f == F32) { memcpy(&hi, b + 4 * i, 4); return; }
    _Float16 h, l; memcpy(&h, b + h2_hi(i), 2); memcpy(&l, b + h2_hi(i) + 64, 2);
    hi = (float)h; lo = (float)l;
}
static size_t slab(int m, int k, int mpad) { return ((size_t)(k >> 5) * mpad + m) * 32 + (k & 31); }
// the kernels' exp (wh_common.h ts_exp) in f32 on the host
static float ts_exp_h(float x) { return exp2f(x * 1.44269504088896341f); }

struct Worst {
    double ratio = 0;
    void see(double got, double want, double bound) {
        double r;
        if (want != want) r = got != got ? 0.0 : 1e30;
        else if (std::isinf(want)) r = got == want ? 0.0 : 1e30;
        else r = fabs(got - want) <= 1e300 ? fabs(got - want) / bound : 1e30;
        if (r > ratio) ratio = r;
    }
};

// rows 0 .. n - 1 over at most 16 host threads
template <typename F> static void par_rows(long n, F f) {
    const int nt = (int)std::min<long>(std::min(16u, std::max(1u, std::thread::hardware_concurrency())), std::max<long>(1, n));
    std::atomic<long> next{0};
    auto body = [&]() { for (;;) { const long i = next.fetch_add(1); if (i >= n) break; f(i); } };
    if (nt == 1) { body(); return; }
    std::vector<std::thread> th;
    for (int t = 0; t < nt; t++) th.emplace_back(body);
    for (auto& t : th) t.join();
}

template <typename V> static void* to_dev(const V& v) {   // an input: its bytes, then a zeroed tail
    if (g_host) return nullptr;
    void* p; const size_t n = v.size() * sizeof(v[0]);
    CK(hipMalloc(&p, n + 256)); CK(hipMemset(p, 0, n + 256)); if (n) CK(hipMemcpy(p, v.data(), n, hipMemcpyHostToDevice));
    return p;
}
static void dev_free(std::initializer_list<void*> ps) { if (!g_host) for (void* p : ps) if (p) CK(hipFree(p)); }

// An output buffer of 32-bit words between two guard regions, filled with a pattern: every word the contract writes is marked live, everything
// else (both guards included) must come back unchanged.
struct Buf {
    long n = 0; std::vector<unsigned> h0, h; std::vector<unsigned char> live; char* d = nullptr;
    void make(long words, bool upload = true) {
        n = words;
        h0.resize(n + 2 * GUARD);
        for (size_t i = 0; i < h0.size(); i++) h0[i] = 0xa5c30000u + (unsigned)((i * 40503u) & 0xffffu);
        live.assign(n, 0);
        if (upload) up();
    }
    // state the kernel reads and rewrites: the caller fills it between make(words, false) and up()
    void init(long i, unsigned v) { h0[GUARD + i] = v; }
    void up() {
        h = h0;
        if (!g_host) { CK(hipMalloc((void**)&d, h0.size() * 4)); CK(hipMemcpy(d, h0.data(), h0.size() * 4, hipMemcpyHostToDevice)); }
    }
    void mark_all() { std::fill(live.begin(), live.end(), 1); }
    void* dev() const { return d ? d + GUARD * 4 : nullptr; }
    void down() { if (!g_host && d) { CK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost)); CK(hipFree(d)); d = nullptr; } }
    void peek() { if (!g_host && d) CK(hipMemcpy(h.data(), d, h.size() * 4, hipMemcpyDeviceToHost)); }   // (a chain of launches: the buffer stays)
    float f(long i) const { return bitsf(h[GUARD + i]); }
    int i32(long i) const { return (int)h[GUARD + i]; }
    unsigned u32(long i) const { return h[GUARD + i]; }
    bool written(long i) const { return h[GUARD + i] != h0[GUARD + i]; }
    // (the emulation: a store outside the buffer lands in a guard, or nowhere)
    void setu(long i, unsigned v) { if (i >= -GUARD && i < n + GUARD) h[GUARD + i] = v; }
    void setf(long i, float v) { setu(i, fbits(v)); }
    void mark(long i) { live[i] = 1; }
    long guard() const {
        long bad = 0;
        for (long i = 0; i < n; i++) bad += !live[i] && h[GUARD + i] != h0[GUARD + i];
        for (long i = 0; i < GUARD; i++) bad += (h[i] != h0[i]) + (h[GUARD + n + i] != h0[GUARD + n + i]);
        return bad;
    }
    unsigned long long hash(unsigned long long s = 1469598103934665603ull) const { return fnv1a(h.data() + GUARD, (size_t)n * 4, s); }
};

// ===== the LM heads ==========================================================================================================================
struct Spec { int tie_a = -1, tie_b = -1, nan_id = -1, ninf_id = -1, pinf_id = -1; };
struct Ops {
    Mode mode = BF16; int M = 0, N = 0, K = 0, mpad = 0, words = 0, ln_tiles = 0; bool ln = true; Spec sp; int sup_id = 17;
    std::vector<unsigned char> hX, hW;
    std::vector<float> Xh, Xl, Wh, Wl;   // the operands as the kernel sees them: [M][K], [N][K]
    std::vector<float> lnp, lns, bias;
    std::vector<unsigned> mfirst, mbase, rep;   // rep [M][words]
    std::vector<float> L0;               // [M][N] the reference logits (a plain k_lm_head launch; --selftest: the emulation)
    void *dX = nullptr, *dW = nullptr, *dlnp = nullptr, *dlns = nullptr, *dbias = nullptr, *dmf = nullptr, *dmb = nullptr;
    void release() { dev_free({dX, dW, dlnp, dlns, dbias, dmf, dmb}); dX = dW = dlnp = dlns = dbias = dmf = dmb = nullptr; }
};
static void setbit(std::vector<unsigned>& w, long base, int id, bool on) { if (on) w[base + (id >> 5)] |= 1u << (id & 31); else w[base + (id >> 5)] &= ~(1u << (id & 31)); }
static bool getbit(const std::vector<unsigned>& w, long base, int id) { return (w[base + (id >> 5)] >> (id & 31)) & 1u; }

static void make_ops(Ops& o, Mode mode, int M, int N, int K, bool ln, Spec sp) {
    o.mode = mode; o.M = M; o.N = N; o.K = K; o.ln = ln; o.sp = sp;
    const int mpad = o.mpad = (M / 192 + 1) * 192;   // > M, and whole row groups of 16, 32, 48 or 64 rows
    o.words = (N + 31) / 32; o.ln_tiles = K / 16;
    rs = 7919u * mode + 131u * M + 17u * N + K + 3u * ln + 1000003u * (sp.tie_a + 2) + 29u * (sp.tie_b + 2) + 5u * (sp.nan_id + 2) + 11u * (sp.pinf_id + 2);
    o.hX.assign((size_t)(K / 32) * mpad * 32 * esz(mode), 0); o.hW.assign((size_t)N * K * esz(mode), 0);
    o.Xh.resize((size_t)M * K); o.Xl.resize((size_t)M * K); o.Wh.resize((size_t)N * K); o.Wl.resize((size_t)N * K);
    for (int m = 0; m < M; m++) {
        const float off = ln ? frand(0.5f) : 0.0f;   // a row mean for the LayerNorm fold to remove
        for (int k = 0; k < K; k++) put(o.hX.data(), mode, slab(m, k, mpad), frand(1.0f) + off, o.Xh[(size_t)m * K + k], o.Xl[(size_t)m * K + k]);
    }
    for (size_t i = 0; i < o.Wh.size(); i++) put(o.hW.data(), mode, i, frand(0.5f), o.Wh[i], o.Wl[i]);
    o.lns.resize(N); o.bias.resize(N);
    for (auto& v : o.lns) v = frand(1.0f);
    for (auto& v : o.bias) v = frand(0.5f);
    auto copy_row = [&](int dst, int src) {
        for (int k = 0; k < K; k++) {
            const size_t s = (size_t)src * K + k, d = (size_t)dst * K + k;
            put(o.hW.data(), mode, d, o.Wh[s] + o.Wl[s], o.Wh[d], o.Wl[d]);   // (hi + lo of a stored pair splits into the same pair)
        }
        o.lns[dst] = o.lns[src]; o.bias[dst] = o.bias[src];
    };
    if (sp.tie_a >= 0) { o.bias[sp.tie_a] = 40.0f; copy_row(sp.tie_b, sp.tie_a); }   // two bit-identical logits, the maximum of every row
    if (sp.nan_id >= 0) {
        const size_t i = (size_t)sp.nan_id * K + 3;
        if (mode == BF16) { const unsigned short h = 0x7fc0; memcpy(&o.hW[2 * i], &h, 2); }
        else if (mode == F32) { const unsigned u = 0x7fc00000u; memcpy(&o.hW[4 * i], &u, 4); }
        else { const unsigned short h = 0x7e00; memcpy(&o.hW[h2_hi(i)], &h, 2); memcpy(&o.hW[h2_hi(i) + 64], &h, 2); }
        get(o.hW.data(), mode, i, o.Wh[i], o.Wl[i]);
    }
    if (sp.ninf_id >= 0) o.bias[sp.ninf_id] = -INFINITY;
    if (sp.pinf_id >= 0) o.bias[sp.pinf_id] = INFINITY;
    // the producer's partial sums of these very rows, per 16 columns
    o.lnp.assign((size_t)o.ln_tiles * mpad * 2, 0.0f);
    for (int t = 0; t < o.ln_tiles; t++) for (int m = 0; m < M; m++) {
        double s1 = 0, s2 = 0;
        for (int k = 16 * t; k < 16 * t + 16; k++) { const double x = (double)o.Xh[(size_t)m * K + k] + o.Xl[(size_t)m * K + k]; s1 += x; s2 += x * x; }
        o.lnp[((size_t)t * mpad + m) * 2] = (float)s1; o.lnp[((size_t)t * mpad + m) * 2 + 1] = (float)s2;
    }
    // the suppress masks (about one id in 16, different at the first position; the bits of the last word past N are set in mask_first and clear in
    // mask_base: nothing may read them either way) and the rows' touched bits (about one id in 64, bits past N set; half of the suppressed ids of
    // row 0 touched as well)
    o.mfirst.assign(o.words, 0); o.mbase.assign(o.words, 0); o.rep.assign((size_t)M * o.words, 0);
    for (int n = 0; n < o.words * 32; n++) { setbit(o.mfirst, 0, n, n >= N || (rnd() & 15) == 0); setbit(o.mbase, 0, n, n < N && (rnd() & 15) == 0); }
    for (int m = 0; m < M; m++) for (int n = 0; n < o.words * 32; n++) setbit(o.rep, (long)m * o.words, n, n >= N || (rnd() & 63) == 0 || (m == 0 && getbit(o.mbase, 0, n) && (n & 1)));
    if (M >= 3) for (int n = 0; n < o.words * 32; n++) { setbit(o.rep, (long)1 * o.words, n, true); setbit(o.rep, (long)2 * o.words, n, n != N - 1); }   // row 1: every id; row 2: all but the last
    o.sup_id = std::min(17, N - 1);
    setbit(o.mfirst, 0, o.sup_id, true); setbit(o.mbase, 0, o.sup_id, true);
    for (int id : {sp.tie_a, sp.tie_b}) if (id >= 0) { setbit(o.mfirst, 0, id, false); setbit(o.mbase, 0, id, false); for (int m = 0; m < M; m++) if (M < 3 || (m != 1 && m != 2)) setbit(o.rep, (long)m * o.words, id, false); }
    o.dX = to_dev(o.hX); o.dW = to_dev(o.hW); o.dlnp = to_dev(o.lnp); o.dlns = to_dev(o.lns); o.dbias = to_dev(o.bias); o.dmf = to_dev(o.mfirst); o.dmb = to_dev(o.mbase);
}

// one launch of an operand set
enum { D_NONE = 0, D_MASKBASE = 1, D_TIEHIGH, D_NOGUARD, D_SUPSUM, D_STRADDLE, D_HIEXCL, D_TEXTLO, D_TOUCHED, D_SIDEPITCH, D_NORESCALE, D_SELSLOT0, D_PARTPITCH, D_LNROW };
struct Var {
    const char* what = ""; bool rules = false, lp = false, rep = false; int gen = 1;
    int lmode = 1, lrows = 2;   // logits kept: 0 none, 1 [M][lrows][N], 2 logits_sel with -1 entries, 3 logits_cur
    int mt = 4, bpc = 2, kern = 0;   // kern 1: the tile kernel of the mode
    int tb = 0, tmax = -1, probe = -1, mmode = 0;   // mmode 1: every id suppressed, 2: only the last column allowed
    int defect = D_NONE;
};
static const int N_PROMPT = 4;
struct HOut { Buf logits, pval, pidx, psum, tsl, side, probe; int n_parts = 0, L = 0, A = 0; std::vector<int> sel; };

static std::vector<int> state_for(const Ops& o, const Var& v) {   // [mpad][4] {text_lo, ts_lo, ts_hi, last timestamp}
    std::vector<int> st((size_t)o.mpad * 4, 0);
    for (int m = 0; m < o.mpad; m++) {
        int* s = &st[4 * m];
        if (m % 3 == 0) { s[0] = 0; s[1] = v.tb; s[2] = o.N - 1; s[3] = -1; }
        else if (m % 3 == 1) { s[0] = std::max(v.tb - 17, 0); s[1] = std::min(v.tb + 5, o.N); s[2] = o.N - 1; s[3] = v.tb + 5; }   // after a single timestamp (text_lo inside a tile and a wave's 64 columns)
        else { s[0] = 0; s[1] = o.N; s[2] = o.N - 1; s[3] = v.tb + 2; }   // after a pair: no timestamp
    }
    return st;
}
static std::vector<unsigned> rep_for(const Ops& o, const Var& v) {   // with the rules on a timestamp is never touched (RepFinish::exempt_from)
    std::vector<unsigned> r = o.rep;
    if (v.rules) for (int m = 0; m < o.M; m++) for (int n = v.tb; n < o.N; n++) setbit(r, (long)m * o.words, n, false);
    return r;
}
static std::vector<unsigned> mask_for(const Ops& o, const Var& v) {   // the mask this position reads, as the contract has it
    std::vector<unsigned> mk = v.gen == 0 ? o.mfirst : o.mbase;
    if (v.mmode) for (int n = 0; n < o.N; n++) setbit(mk, 0, n, !(v.mmode == 2 && n == o.N - 1));
    return mk;
}
static void ranges_for(const Ops& o, const Var& v, const std::vector<int>& st, int m, int& tlo, int& slo, int& shi) {
    if (v.gen == 0) { tlo = v.tb; slo = v.tb; shi = (v.tmax >= 0 && v.tmax < o.N - 1 - v.tb) ? v.tb + v.tmax : o.N - 1; }
    else { tlo = st[4 * m]; slo = st[4 * m + 1]; shi = st[4 * m + 2]; }
}

// ---- the emulation (--selftest): the contract in the kernels' working precision and order ------------------------------------------------------
static void emu_logits(const Ops& o, std::vector<float>& L, int defect) {
    const int M = o.M, N = o.N, K = o.K;
    L.assign((size_t)M * N, 0.0f);
    std::vector<float> mean(M, 0.0f), rstd(M, 1.0f);
    if (o.ln) for (int m = 0; m < M; m++) {
        float q1[4] = {0, 0, 0, 0}, q2[4] = {0, 0, 0, 0};
        for (int t = 0; t < o.ln_tiles; t++) { q1[t & 3] += o.lnp[((size_t)t * o.mpad + m) * 2]; q2[t & 3] += o.lnp[((size_t)t * o.mpad + m) * 2 + 1]; }
        const float s1 = (q1[0] + q1[1]) + (q1[2] + q1[3]), s2 = (q2[0] + q2[1]) + (q2[2] + q2[3]);
        mean[m] = s1 / (float)K;
        const float ex2 = s2 / (float)K, var = ex2 - mean[m] * mean[m];
        rstd[m] = 1.0f / sqrtf(fmaxf(var, 0.0f) + 1e-5f);
    }
    par_rows(M, [&](long m) {
        const int ms = defect == D_LNROW ? (int)((m + 1) % M) : (int)m;
        for (int n = 0; n < N; n++) {
            const float *xh = &o.Xh[(size_t)m * K], *xl = &o.Xl[(size_t)m * K], *wh = &o.Wh[(size_t)n * K], *wl = &o.Wl[(size_t)n * K];
            float acc = 0.0f;
            for (int k0 = 0; k0 < K; k0 += 32) {   // per k-step: lo.hi, hi.lo, hi.hi (limb pairs; else the lo terms are zero)
                if (o.mode == H2) { for (int k = k0; k < k0 + 32; k++) acc += wl[k] * xh[k]; for (int k = k0; k < k0 + 32; k++) acc += wh[k] * xl[k]; }
                for (int k = k0; k < k0 + 32; k++) acc += wh[k] * xh[k];
            }
            float v = acc;
            if (o.ln) { const float p = mean[ms] * o.lns[n], t = acc - p, u = rstd[ms] * t; v = u + o.bias[n]; }
            L[(size_t)m * N + n] = v;
        }
    });
}
static void lp_acc_h(float v, float m, float& s) { if (v > m) s = s * ts_exp_h(m - v) + 1.0f; else if (v > -INFINITY) s += ts_exp_h(v - m); }
static float lp_rescale_h(float s, float m, float mx) { return m == -INFINITY ? 0.0f : s * ts_exp_h(m - mx); }
static float lp_merge_h(float m, float s, float m1, float s1) { const float mx = fmaxf(m, m1); return lp_rescale_h(s, m, mx) + lp_rescale_h(s1, m1, mx); }

static void emu_head(const Ops& o, const Var& v, const std::vector<int>& st, const std::vector<unsigned>& rep, HOut& r) {
    const int M = o.M, N = o.N, d = v.defect;
    std::vector<unsigned> mk = (v.gen == 0 && d != D_MASKBASE) ? o.mfirst : o.mbase;
    if (v.mmode) mk = mask_for(o, v);
    const bool tiehigh = d == D_TIEHIGH;
    auto better = [&](float v1, int i1, float v0, int i0) { return v1 > v0 || (v1 == v0 && ((tiehigh && i0 != NONE_IDX && i1 != NONE_IDX) ? i1 > i0 : i1 < i0)); };
    const int lrow = v.lmode == 3 ? std::min(v.gen, 0) : v.gen;
    const long ppitch = d == D_PARTPITCH ? M : o.mpad, spitch = d == D_SIDEPITCH ? 32L * o.words : N;
    for (int m = 0; m < M; m++) {
        int tlo, slo, shi;
        ranges_for(o, v, st, m, tlo, slo, shi);
        const float* Lr = &o.L0[(size_t)m * N];
        // one logit of a lane: everything the epilogue does with it; returns false past the vocabulary
        struct Lane { float bv = -INFINITY; int bi = NONE_IDX; float ls = 0.0f; };
        auto visit = [&](Lane& ln, int nn, int group_start, bool online) {
            if (nn >= N && d != D_NOGUARD) return;
            const float val = Lr[std::min(nn, N - 1)];   // (the clamped last weight row again)
            if (nn < N && v.lmode && lrow >= 0 && lrow < v.lrows) {
                int slot = v.lmode == 2 ? r.sel[m] : m;
                if (slot < 0 && d == D_SELSLOT0) slot = 0;
                if (slot >= 0) r.logits.setf(((long)slot * v.lrows + lrow) * N + nn, val);
            }
            const bool touched = v.rep && nn < o.words * 32 && getbit(rep, (long)m * o.words, nn);
            if (touched && nn < N) r.side.setf((long)m * spitch + nn, val);
            const bool sup = (nn < o.words * 32 && getbit(mk, 0, nn)) || (touched && d != D_TOUCHED);
            if (v.lp) {
                if (nn == v.probe) r.probe.setf(m, val);
                const bool text_ok = v.rules ? ((!sup || d == D_SUPSUM) && (nn >= tlo || d == D_TEXTLO) && nn < v.tb) : (!sup || d == D_SUPSUM);
                if (text_ok && online) lp_acc_h(val, ln.bv, ln.ls);
            }
            if (v.rules) {
                const bool text_only = d == D_STRADDLE ? group_start < v.tb : group_start + 16 <= v.tb;
                if (text_only || nn < v.tb) { if (!sup && nn >= tlo && (val > ln.bv || (tiehigh && val == ln.bv && val > -INFINITY))) { ln.bv = val; ln.bi = nn; } }
                else r.tsl.setf((long)m * (N - v.tb) + nn - v.tb, (!sup && nn >= slo && (d == D_HIEXCL ? nn < shi : nn <= shi)) ? val : -INFINITY);
            } else if (!sup && (val > ln.bv || (tiehigh && val == ln.bv && val > -INFINITY))) { ln.bv = val; ln.bi = nn; }
        };
        if (v.kern == 0) {   // k_lm_head: part = a wave, its tiles n_parts apart, one online pair per lane group
            const int n_tiles = (N + 15) / 16;
            for (int p = 0; p < r.n_parts; p++) {
                Lane g[4];
                for (int tile = p; tile < n_tiles; tile += r.n_parts)
                    for (int fg = 0; fg < 4; fg++) for (int e = 0; e < 4; e++) visit(g[fg], tile * 16 + 4 * fg + e, tile * 16, true);
                float bv = g[0].bv; int bi = g[0].bi;
                for (int fg = 1; fg < 4; fg++) if (better(g[fg].bv, g[fg].bi, bv, bi)) { bv = g[fg].bv; bi = g[fg].bi; }
                r.pval.setf(p * ppitch + m, bv); r.pidx.setu(p * ppitch + m, (unsigned)bi);
                if (v.lp) {
                    float s[4];
                    for (int fg = 0; fg < 4; fg++) s[fg] = d == D_NORESCALE ? g[fg].ls : lp_rescale_h(g[fg].ls, g[fg].bv, bv);
                    r.psum.setf(p * ppitch + m, (s[0] + s[1]) + (s[2] + s[3]));
                }
            }
        } else {   // the tile kernels: part = a 256-column tile, four waves of 64 columns; the sums in a second pass at the wave's row maximum
            for (int ct = 0; ct < r.n_parts; ct++) {
                float bv = -INFINITY, ls = 0.0f; int bi = NONE_IDX;
                for (int wn = 0; wn < 4; wn++) {
                    Lane g[4];
                    const int nw0 = ct * 256 + wn * 64;
                    for (int fg = 0; fg < 4; fg++) for (int j = 0; j < 4; j++) for (int e = 0; e < 4; e++) visit(g[fg], nw0 + j * 16 + 4 * fg + e, nw0 + j * 16, false);
                    float wv = g[0].bv; int wi = g[0].bi;
                    for (int fg = 1; fg < 4; fg++) if (better(g[fg].bv, g[fg].bi, wv, wi)) { wv = g[fg].bv; wi = g[fg].bi; }
                    float ws = 0.0f;
                    if (v.lp) {
                        float s[4] = {0, 0, 0, 0};
                        for (int fg = 0; fg < 4; fg++) for (int j = 0; j < 4; j++) for (int e = 0; e < 4; e++) {
                            const int nn = nw0 + j * 16 + 4 * fg + e;
                            if (nn >= N) continue;
                            const bool sup = getbit(mk, 0, nn) || (v.rep && getbit(rep, (long)m * o.words, nn));
                            const bool ok = !sup && nn >= ((v.rules && d != D_TEXTLO) ? tlo : 0) && nn < (v.rules ? std::min(v.tb, N) : N) && Lr[nn] > -INFINITY;
                            if (ok) s[fg] += ts_exp_h(Lr[nn] - wv);
                        }
                        ws = (s[0] + s[1]) + (s[2] + s[3]);
                    }
                    if (wn == 0) { bv = wv; bi = wi; ls = ws; continue; }
                    if (v.lp) ls = lp_merge_h(bv, ls, wv, ws);
                    if (better(wv, wi, bv, bi)) { bv = wv; bi = wi; }
                }
                r.pval.setf(ct * ppitch + m, bv); r.pidx.setu(ct * ppitch + m, (unsigned)bi);
                if (v.lp) r.psum.setf(ct * ppitch + m, ls);
            }
        }
    }
}

// ---- one launch (device, or the emulation) and its check --------------------------------------------------------------------------------------
struct Res { double rv = 0, rs = 0; long exact = 0, guard = 0, nosum = 0; int ran = 0, mt = 0; bool compared = false; unsigned long long h[4] = {0, 0, 0, 0}; bool ok() const { return rv <= 1.0 && rs <= 1.0 && exact == 0 && guard == 0; } };

static Res run_head(const Ops& o, const Var& v, std::vector<float>* keep_logits = nullptr) {
    const int M = o.M, N = o.N, prec = prec_of(o.mode);
    HOut r;
    const std::vector<int> st = state_for(o, v);
    const std::vector<unsigned> rep = rep_for(o, v), mk = mask_for(o, v);
    // the masks of this launch: mmode replaces the one the position reads
    std::vector<unsigned> mf = o.mfirst, mb = o.mbase;
    if (v.mmode) (v.gen == 0 ? mf : mb) = mk;
    int n_sel = 0;
    r.sel.assign(M, 0);
    for (int m = 0; m < M; m++) r.sel[m] = (v.lmode == 2 && m % 3 == 1) ? -1 : n_sel++;
    const int lrows = v.lmode == 3 ? 1 : v.lrows;
    Var vv = v; vv.lrows = lrows;
    SkinnyArgs a;
    a.X = o.dX; a.x_mpad = o.mpad; a.W = o.dW; a.M = M; a.N = N; a.K = o.K;
    if (o.ln) { a.ln_part = (const float*)o.dlnp; a.ln_tiles = o.ln_tiles; a.ln_s = (const float*)o.dlns; a.bias = (const float*)o.dbias; }
    a.n_prompt = N_PROMPT;
    wh_dbg_lm_mt = v.mt; wh_dbg_lm_blocks_per_cu = v.bpc;
    setenv("WH_LM_TILE_MIN_ROWS", v.kern ? "1" : "0", 1);
    // The launch decision reads WHICH variant pointers are set, never what they point to: a copy with placeholders asks the library (also on the host).
    static float placeholder[4];
    SkinnyArgs qa = a;
    if (!qa.X) qa.X = placeholder;
    if (v.lp) { qa.part_sum = placeholder; qa.probe_id = v.probe; }
    if (v.rules) qa.ts_logits = placeholder;
    if (v.rep) qa.rep_bits = (const unsigned*)placeholder;
    bool tile = false;
    if (v.kern) {
        SkinnyArgs plain = qa; plain.probe_id = -1;
        const bool can = o.mode == BF16 ? wh_lm_head_tile_applicable(plain) : o.mode == H2 ? wh_lm_head_tile_x3_applicable(plain) : false;
        if (!can) { fprintf(stderr, "the tile kernel does not take M %d N %d K %d %s\n", M, N, o.K, mode_name[o.mode]); exit(2); }
        // false here: a probe together with the rules or the bitmap, which the tile kernels decline and wh_launch_lm_head gives to k_lm_head
        tile = o.mode == BF16 ? wh_lm_head_tile_applicable(qa) : wh_lm_head_tile_x3_applicable(qa);
        if (tile != !(v.lp && v.probe >= 0 && (v.rules || v.rep))) { fprintf(stderr, "unexpected launch decision for a probe with rules %d bitmap %d\n", (int)v.rules, (int)v.rep); exit(2); }
    }
    vv.kern = tile ? 1 : 0;
    r.n_parts = wh_lm_head_parts(prec, qa);   // of the kernel wh_launch_lm_head picks for this call
    if (tile) { r.L = 1 + 3; r.A = 18 + 3; }   // one partial per 256-column tile
    else {
        const int tiles = ((N + 15) / 16 + r.n_parts - 1) / r.n_parts;
        r.L = 4 * tiles + 2; r.A = 4 * tiles + 2;
    }
    // the row groups lm_row_groups settles on (wh_lm_head.hip): the request, the rows, then 150 KB of LDS
    int eff_mt = std::min(v.mt, (M + 15) / 16);
    { const size_t es = o.mode == BF16 ? 2 : 4; while (eff_mt > 1 && (size_t)eff_mt * 16 * o.K * es + (size_t)eff_mt * 16 * 2 * 4 * 5 > 150 * 1024) eff_mt--; }
    const long pw = (long)r.n_parts * o.mpad;
    r.logits.make(v.lmode ? (long)(v.lmode == 2 ? n_sel : M) * lrows * N : 0);
    r.pval.make(pw); r.pidx.make(pw); r.psum.make(v.lp ? pw : 0);
    r.tsl.make(v.rules ? (long)o.mpad * (N - v.tb) : 0); r.side.make(v.rep ? (long)M * N : 0); r.probe.make(v.lp && v.probe >= 0 ? M : 0);
    if (!g_host) {
        const int pos = v.gen + N_PROMPT - 1;
        std::vector<int> posv = {pos};
        void *dpos = to_dev(posv), *dst = to_dev(st), *drep = to_dev(rep), *dsel = to_dev(r.sel), *dmf = to_dev(mf), *dmb = to_dev(mb);
        a.pos_p = (const int*)dpos; a.mask_first = (const unsigned*)dmf; a.mask_base = (const unsigned*)dmb;
        if (v.lmode) { a.logits = (float*)r.logits.dev(); a.logits_rows = lrows; a.logits_cur = v.lmode == 3; if (v.lmode == 2) a.logits_sel = (const int*)dsel; }
        a.part_val = (float*)r.pval.dev(); a.part_idx = (int*)r.pidx.dev();
        if (v.rules) { a.ts_state = (const int*)dst; a.ts_logits = (float*)r.tsl.dev(); a.ts_ld = N - v.tb; a.ts_begin = v.tb; a.ts_max_init = v.tmax; }
        if (v.lp) { a.part_sum = (float*)r.psum.dev(); a.probe_id = v.probe; a.probe_out = (float*)r.probe.dev(); }
        if (v.rep) { a.rep_bits = (const unsigned*)drep; a.rep_side = (float*)r.side.dev(); a.rep_words = o.words; }
        wh_launch_lm_head(0, prec, a);   // (WH_LM_TILE_MIN_ROWS decides between k_lm_head and the mode's tile kernel)
        CK(hipGetLastError());
        CK(hipDeviceSynchronize());
        for (Buf* b : {&r.logits, &r.pval, &r.pidx, &r.psum, &r.tsl, &r.side, &r.probe}) b->down();
        dev_free({dpos, dst, drep, dsel, dmf, dmb});
    } else emu_head(o, vv, st, rep, r);
    wh_dbg_lm_mt = 4; wh_dbg_lm_blocks_per_cu = 2;

    Res q;
    q.ran = tile ? 1 : 0; q.mt = tile ? 0 : eff_mt;
    if (keep_logits) {   // the reference launch (plain, gen 0, one logits row per row): hand the logits out, the values are checked by the caller
        keep_logits->resize((size_t)M * N);
        for (long i = 0; i < (long)M * N; i++) { (*keep_logits)[i] = r.logits.f(i); r.logits.mark(i); }
    }
    const std::vector<float>& L0 = keep_logits ? *keep_logits : o.L0;
    // ---- logits: bit for bit L0 where the contract keeps them ----
    const int lrow = v.lmode == 3 ? std::min(v.gen, 0) : v.gen;
    q.compared = v.lmode && lrow >= 0 && lrow < lrows && !keep_logits;
    if (q.compared)
        for (int m = 0; m < M; m++) {
            if (r.sel[m] < 0) continue;
            const long base = ((long)r.sel[m] * lrows + lrow) * N;
            for (int n = 0; n < N; n++) { r.logits.mark(base + n); q.exact += !same_f(r.logits.f(base + n), L0[(size_t)m * N + n]); }
        }
    // ---- selection, from L0 ----
    Worst ws;
    for (int m = 0; m < M; m++) {
        int tlo = 0, slo = 0, shi = 0;
        if (v.rules) ranges_for(o, v, st, m, tlo, slo, shi);
        const float* Lr = &L0[(size_t)m * N];
        float bv = -INFINITY; int bi = NONE_IDX;
        const int text_hi = v.rules ? std::min(v.tb, N) : N;
        auto sup = [&](int n) { return getbit(mk, 0, n) || (v.rep && getbit(rep, (long)m * o.words, n)); };
        for (int n = v.rules ? std::max(tlo, 0) : 0; n < text_hi; n++) if (!sup(n) && Lr[n] > bv) { bv = Lr[n]; bi = n; }
        float gv = -INFINITY; int gi = NONE_IDX;
        for (int p = 0; p < r.n_parts; p++) {
            const long i = (long)p * o.mpad + m;
            r.pval.mark(i); r.pidx.mark(i); if (v.lp) r.psum.mark(i);
            const float pv = r.pval.f(i); const int pi = r.pidx.i32(i);
            if (pv > gv || (pv == gv && pi < gi)) { gv = pv; gi = pi; }
        }
        q.exact += !(fbits(gv) == fbits(bv) && gi == bi);
        if (v.lp) {
            if (bv == INFINITY) q.nosum++;
            else {
                double want = 0, bound = 1e-37, got = 0;
                for (int n = v.rules ? std::max(tlo, 0) : 0; n < text_hi; n++) if (!sup(n) && Lr[n] > -INFINITY) {
                    const double dlt = (double)Lr[n] - bv, e = exp(dlt);
                    want += e; bound += e * (3 * fabs(dlt) + 3 * r.L + r.A) * U;
                }
                for (int p = 0; p < r.n_parts; p++) {
                    const long i = (long)p * o.mpad + m;
                    if (r.pval.f(i) > -INFINITY) got += (double)r.psum.f(i) * exp((double)r.pval.f(i) - bv);   // (an empty partial's sum counts for nothing)
                }
                ws.see(got, want, bound);
            }
            if (v.probe >= 0) { r.probe.mark(m); q.exact += !same_f(r.probe.f(m), Lr[v.probe]); }
        }
        if (v.rules) for (int n = v.tb; n < N; n++) {
            const long i = (long)m * (N - v.tb) + n - v.tb;
            r.tsl.mark(i);
            q.exact += !same_f(r.tsl.f(i), (!sup(n) && n >= slo && n <= shi) ? Lr[n] : -INFINITY);
        }
        if (v.rep) for (int n = 0; n < N; n++) if (getbit(rep, (long)m * o.words, n)) { r.side.mark((long)m * N + n); q.exact += !same_f(r.side.f((long)m * N + n), Lr[n]); }
    }
    q.rs = ws.ratio;
    for (Buf* b : {&r.logits, &r.pval, &r.pidx, &r.psum, &r.tsl, &r.side, &r.probe}) q.guard += b->guard();
    q.h[0] = r.logits.hash(); q.h[1] = r.psum.hash(r.pidx.hash(r.pval.hash())); q.h[2] = r.tsl.hash(); q.h[3] = r.probe.hash(r.side.hash());
    return q;
}

// the values of the reference logits against the float64 product
static double check_values(const Ops& o, const std::vector<float>& L) {
    const int M = o.M, N = o.N, K = o.K;
    std::vector<double> worst(M, 0.0);
    par_rows(M, [&](long m) {
        double mean = 0, rstd = 1, emean = 0, erstd = 0;
        if (o.ln) {
            double s1 = 0, s2 = 0, a1 = 0;
            for (int t = 0; t < o.ln_tiles; t++) { s1 += o.lnp[((size_t)t * o.mpad + m) * 2]; a1 += fabs(o.lnp[((size_t)t * o.mpad + m) * 2]); s2 += o.lnp[((size_t)t * o.mpad + m) * 2 + 1]; }
            mean = s1 / K;
            const double ex2 = s2 / K, var = ex2 - mean * mean, tl = (o.ln_tiles + 2) * U;
            emean = tl * a1 / K + U * fabs(mean);
            const double evar = tl * ex2 + 2 * fabs(mean) * emean + 3 * U * (ex2 + mean * mean);
            rstd = 1.0 / sqrt(fmax(var, 0.0) + 1e-5);
            erstd = rstd * (0.5 * evar / (fmax(var, 0.0) + 1e-5) + 4 * U);
        }
        Worst w;
        for (int n = 0; n < N; n++) {
            double acc = 0, A = 0;
            for (int k = 0; k < K; k++) {
                const double x = (double)o.Xh[(size_t)m * K + k] + o.Xl[(size_t)m * K + k], wv = (double)o.Wh[(size_t)n * K + k] + o.Wl[(size_t)n * K + k];
                acc += x * wv; A += fabs(x * wv);
            }
            double e = ((o.mode == H2 ? 3.0 : 1.0) * K + 8) * U * A + (o.mode == H2 ? 4 * U * A : 0.0), v = acc;
            if (o.ln) {
                const double p = mean * o.lns[n], ep = fabs(p) * U + fabs(o.lns[n]) * emean, t = acc - p, et = e + ep + U * fabs(t), u = rstd * t;
                v = u + o.bias[n];
                e = rstd * et + fabs(t) * erstd + U * fabs(u) + U * fabs(v);
            }
            w.see(L[(size_t)m * N + n], v, e + U * fabs(v));
        }
        worst[m] = w.ratio;
    });
    return *std::max_element(worst.begin(), worst.end());
}

static double worst_val[2] = {0, 0}, worst_sum[2] = {0, 0};
static long tile_cases = 0, tile_diff = 0;
static const char* kern_of(const Ops& o, int ran) { return !ran ? "k_lm_head        " : o.mode == BF16 ? "k_lm_head_tile   " : "k_lm_head_tile_x3"; }
static int line_head(const Ops& o, const Var& v, const Res& q, double rv, const char* tag) {
    const bool ok = q.ok() && rv <= 1.0;
    printf("%s %s M %3d N %5d K %4d mt %d (ran %d) bpc %d %s%s%s gen %2d tb %5d logits %d %-34s: err/bound logits %.3f sum %.3f exact %ld guard %ld  logits %016llx parts %016llx ts %016llx side %016llx  %s%s\n",
           kern_of(o, q.ran), mode_name[o.mode], o.M, o.N, o.K, v.mt, q.mt, v.bpc, v.rules ? "R" : "-", v.lp ? "L" : "-", v.rep ? "P" : "-", v.gen, v.tb, v.lmode, v.what, rv, q.rs, q.exact, q.guard,
           q.h[0], q.h[1], q.h[2], q.h[3], ok ? "ok" : "MISMATCH", tag);
    worst_val[q.ran] = std::max(worst_val[q.ran], rv); worst_sum[q.ran] = std::max(worst_sum[q.ran], q.rs);
    return ok ? 0 : 1;
}
// the reference launch of an operand set: plain k_lm_head at gen 0, every logit kept and held to the float64 product
static int reference(Ops& o, int defect = D_NONE, double* ratio = nullptr) {
    Var v; v.what = "reference: every logit kept"; v.gen = 0; v.lmode = 1; v.lrows = 1;
    Res q;
    if (g_host) { emu_logits(o, o.L0, defect); q = run_head(o, v); }   // (the emulation's launches store these very logits)
    else { std::vector<float> L; q = run_head(o, v, &L); o.L0 = L; }
    const double rv = check_values(o, o.L0);
    if (ratio) { *ratio = rv; return 0; }
    return line_head(o, v, q, rv, "");
}
static int variant(const Ops& o, Var v) {
    if (v.lp && v.probe < 0 && !v.kern) v.probe = o.sup_id;   // every LP launch of k_lm_head carries a probe, on an id both masks suppress
    const Res q = run_head(o, v);
    if (q.ran && q.compared) { tile_cases++; tile_diff += q.exact != 0; }   // (launches that stored a logits row, which was compared)
    return line_head(o, v, q, 0.0, q.nosum ? "  (a +inf maximum: no sum)" : "");
}
static Var var(const char* what, bool rules, bool lp, bool rep, int gen, int tb, int kern = 0) { Var v; v.what = what; v.rules = rules; v.lp = lp; v.rep = rep; v.gen = gen; v.tb = tb; v.kern = kern; return v; }

static int group_head() {
    int bad = 0;
    for (Mode md : {BF16, F32, H2}) {
        {   // M 5, N 1003 (a last tile of 11 columns, a last mask word used partly), K 128: every variant, position, logits form, ts_begin
            Ops o; make_ops(o, md, 5, 1003, 128, true, Spec());
            bad |= reference(o);
            for (int c = 0; c < 8; c++) { Var v = var("all eight variants", c & 1, c & 2, c & 4, 1, 903); v.probe = o.sup_id; bad |= variant(o, v); }
            { Var v = var("prompt position: no logits row", false, true, false, -1, 0); v.probe = o.sup_id; bad |= variant(o, v); }
            { Var v = var("prompt position, logits_cur", false, false, false, -1, 0); v.lmode = 3; bad |= variant(o, v); }
            { Var v = var("gen 0: mask_first, rule 4 unbounded", true, true, true, 0, 903); bad |= variant(o, v); }
            { Var v = var("gen 0: ts_max_init 3", true, true, false, 0, 903); v.tmax = 3; bad |= variant(o, v); }
            { Var v = var("gen 7 > logits_rows", true, false, true, 7, 896); bad |= variant(o, v); }
            { Var v = var("gen 7, logits_cur", false, true, true, 7, 0); v.lmode = 3; bad |= variant(o, v); }
            { Var v = var("logits_sel with -1 entries", true, true, true, 1, 768); v.lmode = 2; bad |= variant(o, v); }
            { Var v = var("no logits kept", false, true, false, 1, 0); v.lmode = 0; bad |= variant(o, v); }
            for (int tb : {768, 896}) { Var v = var(tb == 768 ? "ts_begin on a multiple of 256" : "ts_begin on a multiple of 16", true, true, false, 1, tb); bad |= variant(o, v); }
            for (int mm : {1, 2}) for (int c : {0, 3, 7}) { Var v = var(mm == 1 ? "every id suppressed" : "only the last column allowed", c & 1, c & 2, c & 4, 1, 903); v.mmode = mm; bad |= variant(o, v); }
            o.release();
        }
        // exact ties as the row maximum: the same lane, two lane groups of a tile, two waves, two workgroups
        for (int tb2 : {9, 13, 24, 72}) {
            Ops o; Spec sp; sp.tie_a = 8; sp.tie_b = tb2; make_ops(o, md, 5, 1003, 128, true, sp);
            bad |= reference(o);
            bad |= variant(o, var("tie 8 = x", false, true, false, 1, 0));
            bad |= variant(o, var("tie 8 = x", true, true, true, 1, 903));
            o.release();
        }
        {   // a weight row with a NaN, a bias of -inf; then a bias of +inf
            Ops o; Spec sp; sp.nan_id = 100; sp.ninf_id = 200; make_ops(o, md, 5, 1003, 128, true, sp);
            bad |= reference(o);
            bad |= variant(o, var("NaN row 100, bias -inf 200", false, true, false, 1, 0));
            bad |= variant(o, var("NaN row 100, bias -inf 200", true, true, true, 1, 96));
            o.release();
            Ops p; Spec sq; sq.pinf_id = 300; make_ops(p, md, 5, 1003, 128, true, sq);
            bad |= reference(p);
            bad |= variant(p, var("bias +inf 300", false, true, false, 1, 0));
            bad |= variant(p, var("bias +inf 300", true, false, true, 1, 903));
            p.release();
        }
        {   // no LayerNorm fold (a.ln_part == nullptr)
            Ops o; make_ops(o, md, 1, 1003, 128, false, Spec());
            bad |= reference(o);
            bad |= variant(o, var("one row, no LayerNorm fold", false, true, false, 1, 0));
            o.release();
        }
        // K: fewer k-steps than DEPTH (384), one full chunk (512), three chunks with the last one cut and the second staging pass (1280; bf16 at
        // 52 rows: MT = 3); M 16 / 17 / 52 (a cut row tile inside the last group); every forced row grouping
        struct { int M, K; } shp[] = {{17, 384}, {16, 512}, {52, 1280}};
        for (auto& s : shp) {
            Ops o; make_ops(o, md, s.M, 1003, s.K, true, Spec());
            bad |= reference(o);
            bad |= variant(o, var("rules", true, false, false, 1, 903));
            bad |= variant(o, var("log-probabilities", false, true, false, 1, 0));
            bad |= variant(o, var("repetition", false, false, true, 1, 0));
            if (s.M == 52) for (int mt : {1, 2, 3}) { Var v = var("forced row groups", true, true, true, 1, 903); v.mt = mt; v.lmode = 2; bad |= variant(o, v); }
            o.release();
        }
        {   // every row grouping in every dtype: at K = 128 the LDS limit cuts none (at K = 1280 f32 and limb pairs fit one 16-row group only)
            Ops o; make_ops(o, md, 52, 1003, 128, true, Spec());
            bad |= reference(o);
            for (int mt : {1, 2, 3, 4}) { Var v = var("forced row groups, K 128", true, true, true, 1, 903); v.mt = mt; v.lmode = 2; v.probe = o.sup_id; bad |= variant(o, v); }
            o.release();
        }
        {   // N 4099 at 256 rows, one workgroup per CU: some waves walk two tiles, some one; a tie in two tiles of one wave
            Ops o; Spec sp; sp.tie_a = 5; sp.tie_b = 4098; make_ops(o, md, 256, 4099, 128, true, sp);
            bad |= reference(o);
            { Var v = var("one and two tiles per wave, tie 5 = 4098", false, true, false, 1, 0); v.bpc = 1; bad |= variant(o, v); }
            { Var v = var("one and two tiles per wave, tie 5 = 4098", true, true, true, 1, 4000); v.bpc = 1; v.lmode = 2; bad |= variant(o, v); }
            o.release();
        }
    }
    {   // one full vocabulary at 16 rows, one workgroup per CU: three and four tiles per wave (odd and even unit counts)
        Ops o; make_ops(o, BF16, 16, 51866, 128, true, Spec());
        bad |= reference(o);
        { Var v = var("three and four tiles per wave", false, true, false, 1, 0); v.bpc = 1; v.probe = 50362; bad |= variant(o, v); }
        { Var v = var("three and four tiles per wave", true, true, true, 1, 50364); v.bpc = 1; v.lmode = 2; bad |= variant(o, v); }
        o.release();
    }
    printf("worst err/bound head: logits %.3f sum of exp %.3f\n", worst_val[0], worst_sum[0]);
    return bad;
}

static int group_tile() {
    int bad = 0;
    struct { int M, N, K, tie_b; } shp[] = {{256, 1003, 128, -1}, {260, 4099, 128, -1}, {260, 1003, 512, 700}, {256, 4099, 512, 9}};
    for (Mode md : {BF16, H2})
        for (auto& s : shp) {
            Ops o; Spec sp; sp.nan_id = 100; sp.ninf_id = 200;
            if (s.tie_b >= 0) { sp.tie_a = 5; sp.tie_b = s.tie_b; }
            make_ops(o, md, s.M, s.N, s.K, true, sp);
            bad |= reference(o);   // k_lm_head's logits: every tile launch below must store the same bits
            const int tb = s.N == 1003 ? 903 : 4000;
            if (s.K == 128 && s.N == 1003) for (int c = 0; c < 8; c++) { Var v = var("all eight variants", c & 1, c & 2, c & 4, 1, tb, 1); v.probe = (c & 5) ? -1 : o.sup_id; bad |= variant(o, v); }
            else {
                bad |= variant(o, var("plain", false, false, false, 1, 0, 1));
                { Var v = var("log-probabilities, probe", false, true, false, -1, 0, 1); v.probe = o.sup_id; bad |= variant(o, v); }
                { Var v = var("rules + log-probabilities + repetition", true, true, true, 1, tb, 1); v.lmode = 2; bad |= variant(o, v); }
            }
            // a probe with the rules or the bitmap: the tile kernels decline, the same call runs k_lm_head and the probe is the raw logit
            for (int c : {3, 6, 7}) { Var v = var("probe declined by the tile kernel", c & 1, c & 2, c & 4, 1, tb, 1); v.probe = o.sup_id; bad |= variant(o, v); }
            { Var v = var("gen 0: ts_max_init 3", true, true, false, 0, tb, 1); v.tmax = 3; bad |= variant(o, v); }
            { Var v = var("only the last column allowed", true, true, true, 1, tb, 1); v.mmode = 2; bad |= variant(o, v); }
            o.release();
        }
    printf("tile logits bit-identical to k_lm_head: %ld launches, %ld differing  %s\n", tile_cases, tile_diff, tile_diff == 0 && tile_cases > 0 ? "ok" : "MISMATCH");
    printf("worst err/bound tile: sum of exp %.3f (logits: k_lm_head's, %.3f)\n", worst_sum[1], worst_val[0]);
    return bad | (tile_diff != 0);
}

// ===== the language head and the language finish =============================================================================================
// k_lang_head gathers the LM head's weight rows by id: each listed id's logit must be bit for bit what k_lm_head gave that id (the operand set's
// reference logits, which are held to the float64 product).  The columns between n_lang and the next multiple of 16 hold the padding ids' logits.
enum { D_LANGTIE = 24, D_LANGSRC = 25, D_PFXCLAMP = 26 };
static long lang_cases = 0, lang_diff = 0;
static std::vector<int> lang_ids(int N) {   // WH_LANG_LD ids, distinct, not ascending (ids[1] > ids[2])
    std::vector<int> ids(WH_LANG_LD);
    for (int j = 0; j < WH_LANG_LD; j++) ids[j] = (7 + 37 * j) % N;
    std::swap(ids[1], ids[2]);
    return ids;
}
static int lang_head_case(const Ops& o, int n_lang, int mt, double rv) {
    std::vector<int> ids = lang_ids(o.N);
    for (int j = n_lang; j < WH_LANG_LD; j++) ids[j] = ids[0];   // padded with a listed id
    Buf out; out.make((long)o.mpad * WH_LANG_LD);
    if (!g_host) {
        void* dids = to_dev(ids);
        LangHeadArgs a;
        a.X = o.dX; a.x_mpad = o.mpad; a.W = o.dW; a.bias = (const float*)o.dbias; a.ln_s = (const float*)o.dlns; a.ln_part = (const float*)o.dlnp; a.ln_tiles = o.ln_tiles;
        a.ids = (const int*)dids; a.n_lang = n_lang; a.M = o.M; a.K = o.K; a.out = (float*)out.dev();
        wh_dbg_lm_mt = mt;
        wh_launch_lang_head(0, prec_of(o.mode), a);
        wh_dbg_lm_mt = 4;
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        out.down(); dev_free({dids});
    } else for (int m = 0; m < o.M; m++) for (int j = 0; j < (n_lang + 15) / 16 * 16; j++) out.setf((long)m * WH_LANG_LD + j, o.L0[(size_t)m * o.N + ids[j]]);
    long exact = 0;
    for (int m = 0; m < o.M; m++) for (int j = 0; j < (n_lang + 15) / 16 * 16; j++) { out.mark((long)m * WH_LANG_LD + j); exact += !same_f(out.f((long)m * WH_LANG_LD + j), o.L0[(size_t)m * o.N + ids[j]]); }
    const long guard = out.guard();
    const bool ok = exact == 0 && guard == 0 && rv <= 1.0;
    lang_cases++; lang_diff += exact != 0;
    printf("k_lang_head       %s M %3d K %4d n_lang %3d mt %d: err/bound logits %.3f (k_lm_head's reference) differing %ld guard %ld  out %016llx  %s\n", mode_name[o.mode], o.M, o.K, n_lang, mt, rv,
           exact, guard, out.hash(), ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

struct LF { const char* what; int n_lang, src_row; bool pos; int defect; };
static double worst_lang = 0;
static int lang_finish_case(const LF& c) {
    const int B = 5, tok_ld = 6, tok_pos = 2, nl = c.n_lang;
    const std::vector<int> ids = lang_ids(1003);
    rs = 4242u + 31u * nl + c.src_row;
    std::vector<float> lg((size_t)B * WH_LANG_LD);
    for (auto& v : lg) v = frand(4.0f);
    if (nl > 2) { lg[1] = 9.0f; lg[2] = 9.0f; }   // row 0: a tie between list positions 1 and 2, ids[2] < ids[1]
    for (int j : {0, 4}) if (j < nl) lg[WH_LANG_LD + j] = NAN;   // row 1: NaN entries
    for (int j = 0; j < WH_LANG_LD; j++) lg[2 * WH_LANG_LD + j] = (j & 1) ? NAN : -INFINITY;   // row 2: nothing finite
    for (int j : {2, 7}) if (j < nl) lg[3 * WH_LANG_LD + j] = INFINITY;   // row 3: a +inf maximum
    Buf probs, chosen, feed, outt, pos;
    probs.make((long)B * nl); chosen.make(B); feed.make(B * tok_ld); outt.make(B * tok_ld); pos.make(1);
    if (!g_host) {
        void *dlg = to_dev(lg), *dids = to_dev(ids);
        const int p0 = 2;
        CK(hipMemcpy(pos.dev(), &p0, 4, hipMemcpyHostToDevice));
        wh_launch_lang_finish(0, (const float*)dlg, (const int*)dids, nl, c.src_row, (float*)probs.dev(), (int*)chosen.dev(), (int*)feed.dev(), (int*)outt.dev(), tok_ld, tok_pos, B,
                              c.pos ? (int*)pos.dev() : nullptr);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        for (Buf* b : {&probs, &chosen, &feed, &outt, &pos}) b->down();
        dev_free({dlg, dids});
    } else {   // the kernel in f32
        pos.setu(0, 2);
        for (int b = 0; b < B; b++) {
            const float* row = &lg[(size_t)((c.src_row >= 0 && c.defect != D_LANGSRC) ? c.src_row : b) * WH_LANG_LD];
            float bv = -INFINITY; int bi = NONE_IDX, lo = NONE_IDX;
            for (int j = 0; j < nl; j++) { lo = std::min(lo, ids[j]); if (row[j] > bv || (row[j] == bv && c.defect != D_LANGTIE && ids[j] < bi)) { bv = row[j]; bi = ids[j]; } }
            const bool none = bv == -INFINITY;
            std::vector<float> e(nl); float s = 0.0f;
            for (int j = 0; j < nl; j++) { e[j] = (none || row[j] != row[j]) ? 0.0f : bv == INFINITY ? (row[j] == INFINITY ? 1.0f : 0.0f) : ts_exp_h(row[j] - bv); s += e[j]; }
            for (int j = 0; j < nl; j++) probs.setf((long)b * nl + j, none ? 0.0f : e[j] / s);
            const int tok = none ? lo : bi;
            chosen.setu(b, tok); feed.setu(b * tok_ld + tok_pos, tok); outt.setu(b * tok_ld + tok_pos, tok);
        }
        if (c.pos) pos.setu(0, 3);
    }
    long exact = 0;
    Worst w;
    for (int b = 0; b < B; b++) {
        const float* row = &lg[(size_t)(c.src_row >= 0 ? c.src_row : b) * WH_LANG_LD];
        double bv = -INFINITY; int bi = NONE_IDX, lo = NONE_IDX;
        for (int j = 0; j < nl; j++) { lo = std::min(lo, ids[j]); if (row[j] > bv || (row[j] == bv && ids[j] < bi)) { bv = row[j]; bi = ids[j]; } }
        const bool none = bv == -INFINITY;
        const int tok = none ? lo : bi;
        chosen.mark(b); feed.mark(b * tok_ld + tok_pos); outt.mark(b * tok_ld + tok_pos);
        exact += (chosen.i32(b) != tok) + (feed.i32(b * tok_ld + tok_pos) != tok) + (outt.i32(b * tok_ld + tok_pos) != tok);
        double S = 0, eS = 0, psum = 0, pb = 0;
        int n_inf = 0;
        for (int j = 0; j < nl; j++) {
            if (none || row[j] != row[j]) continue;
            if (bv == INFINITY) { n_inf += row[j] == INFINITY; continue; }
            const double d = (double)row[j] - bv, e = exp(d);
            S += e; eS += e * (3 * fabs(d) + 3 + 8) * U;   // one exponential; the lane's two terms and the wave's six steps
        }
        for (int j = 0; j < nl; j++) {
            probs.mark((long)b * nl + j);
            double want = 0, bound = 1e-37;
            if (!none && row[j] == row[j]) {
                if (bv == INFINITY) want = row[j] == INFINITY ? 1.0 / n_inf : 0.0, bound += 2 * U * want;
                else { const double d = (double)row[j] - bv; want = exp(d) / S; bound += want * ((3 * fabs(d) + 3) * U + eS / S + 2 * U); }
            }
            w.see(probs.f((long)b * nl + j), want, bound);
            psum += probs.f((long)b * nl + j); pb += bound;
        }
        w.see(psum, none ? 0.0 : 1.0, pb + nl * U);   // the probabilities sum to 1
    }
    pos.mark(0);
    exact += pos.i32(0) != (c.pos ? 3 : 2);
    long guard = 0;
    for (Buf* b : {&probs, &chosen, &feed, &outt, &pos}) guard += b->guard();
    const bool ok = w.ratio <= 1.0 && exact == 0 && guard == 0;
    worst_lang = std::max(worst_lang, c.defect ? 0.0 : w.ratio);
    if (!c.defect || !g_host)
        printf("k_lang_finish     n_lang %3d src_row %2d pos_p %d %-28s: err/bound %.3f exact %ld guard %ld  probs %016llx chosen %016llx  %s\n", nl, c.src_row, (int)c.pos, c.what, w.ratio, exact, guard,
               probs.hash(), chosen.hash(), ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

static int group_lang() {
    int bad = 0;
    for (Mode md : {BF16, F32, H2})
        for (int K : {128, 1280}) for (int M : {3, 52}) {
            Ops o; make_ops(o, md, M, 1003, K, true, Spec());
            double rv = 0;
            reference(o, D_NONE, &rv);
            for (int nl : {1, 16, 17, 99, 128}) bad |= lang_head_case(o, nl, 4, rv);
            if (M == 52) bad |= lang_head_case(o, 99, 2, rv);
            o.release();
        }
    printf("language logits bit-identical to k_lm_head: %ld launches, %ld differing  %s\n", lang_cases, lang_diff, lang_diff == 0 && lang_cases > 0 ? "ok" : "MISMATCH");
    for (int nl : {1, 16, 17, 99, 128}) bad |= lang_finish_case({"tie, NaN, nothing finite, +inf", nl, -1, nl != 17, 0});
    bad |= lang_finish_case({"every row takes row 0 (the tie)", 99, 0, false, 0});
    bad |= lang_finish_case({"every row takes row 3 (+inf)", 128, 3, true, 0});
    printf("worst err/bound lang: probabilities %.3f (logits: k_lm_head's)\n", worst_lang);
    return bad | (lang_diff != 0);
}

// ===== k_dec_embed ==========================================================================================================================
// x = E[token] + P[position] is one f32 addition per element: exact.  The row's mean (shift given) is a sum of d terms: whatever the order,
// |error| <= d U sum|x| / d + U |mean|; the slab copy (x - mean) gamma: the mean's error, one U for the difference, one for the product, half
// an ulp of the stored type; the sums of the centred row and of its squares: the elements' errors added, + d U of the sums of magnitudes.
// The embedding of one row in f32 (--selftest).  order 1, the kernels': a thread takes four columns of every 1024 and the four waves' sums are
// added as (0 + 1) + (2 + 3) (embed_next_row; k_dec_embed, where a lane stands for four threads); order 0, the defect: a lane takes four columns
// of every 256 and 64 lanes are added.
static void emu_embed_row(Mode mode, const float* eh, const float* el, const float* pr, const float* xg, bool shift, int d, int r, int mpad, int order, Buf& x, Buf& xs, Buf& stt, Buf& sh) {
    const int NL = order ? 256 : 64;
    std::vector<float> v(d), l0(NL, 0.0f), l1(NL, 0.0f), l2(NL, 0.0f);
    auto total = [&](const std::vector<float>& l) {
        if (!order) { float s = 0; for (float t : l) s += t; return s; }
        float w[4] = {0, 0, 0, 0};
        for (int t = 0; t < 256; t++) w[t >> 6] += l[t];
        return (w[0] + w[1]) + (w[2] + w[3]);
    };
    for (int k = 0; k < d; k++) { v[k] = (eh[k] + el[k]) + pr[k]; x.setf((long)r * d + k, v[k]); }
    for (int k = 0; k < d; k += 4) l0[(k / 4) % NL] += (v[k] + v[k + 1]) + (v[k + 2] + v[k + 3]);
    const float mean = shift ? total(l0) / (float)d : 0.0f;
    for (int k = 0; k < d; k += 4) {
        float u[4];
        for (int e = 0; e < 4; e++) u[e] = v[k + e] - mean;
        l1[(k / 4) % NL] += (u[0] + u[1]) + (u[2] + u[3]);
        l2[(k / 4) % NL] += (u[0] * u[0] + u[1] * u[1]) + (u[2] * u[2] + u[3] * u[3]);
        for (int e = 0; e < 4; e++) { float hi, lo; put((unsigned char*)(xs.h.data() + GUARD), mode, slab(r, k + e, mpad), u[e] * (xg ? xg[k + e] : 1.0f), hi, lo); }
    }
    stt.setf(2 * r, total(l1)); stt.setf(2 * r + 1, total(l2));
    if (shift) sh.setf(r, mean);
}
struct EC { const char* what; Mode mode; int rows, d; bool gamma, shift, pfx; int defect; };
static double worst_embed = 0;
static double half_ulp_t(Mode f, double v) { return f == BF16 ? ldexp(fabs(v), -8) : f == F32 ? U * fabs(v) : ldexp(fabs(v), -22) + ldexp(1.0, -24); }
static int embed_case(const EC& c) {
    const int rows = c.rows, d = c.d, vocab = 40, ctx = 16, feed_ld = 12, pos = 9, mpad = (rows / 64 + 1) * 64;   // mpad != rows
    rs = 99991u + 7u * c.mode + 13u * rows + d + 2u * c.gamma + 4u * c.shift + 8u * c.pfx;
    std::vector<unsigned char> hE((size_t)vocab * d * esz(c.mode));
    std::vector<float> Eh((size_t)vocab * d), El((size_t)vocab * d), P((size_t)ctx * d), xg(d);
    for (size_t i = 0; i < Eh.size(); i++) put(hE.data(), c.mode, i, frand(1.0f) + 0.25f, Eh[i], El[i]);
    for (auto& v : P) v = frand(0.5f);
    for (auto& v : xg) v = 0.5f + fabsf(frand(1.0f));
    std::vector<int> feed((size_t)rows * feed_ld), off(rows);
    for (auto& v : feed) v = (int)(rnd() % vocab);
    for (int r = 0; r < rows; r++) off[r] = r % 4 == 0 ? 0 : r % 4 == 1 ? 4 : r % 4 == 2 ? pos + 1 : pos;   // (pos + 1: an idle row, embedded at position 0)
    Buf x, xs, stt, sh;
    const long slab_words = (long)(d / 32) * mpad * 32 * (long)esz(c.mode) / 4;
    x.make((long)rows * d); xs.make(slab_words); stt.make((long)mpad * 2); sh.make(c.shift ? mpad : 0);
    auto mpos_of = [&](int r, bool clamp) { return c.pfx ? (clamp ? std::max(pos - std::max(off[r], 0), 0) : (pos - off[r] + ctx) % ctx) : pos; };
    if (!g_host) {
        std::vector<int> pv = {pos};
        void *dE = to_dev(hE), *dP = to_dev(P), *dxg = to_dev(xg), *dfeed = to_dev(feed), *doff = to_dev(off), *dpos = to_dev(pv);
        wh_launch_dec_embed(0, prec_of(c.mode), dE, (const float*)dP, (const int*)dfeed, feed_ld, (const int*)dpos, (float*)x.dev(), xs.dev(), (float*)stt.dev(), rows, d, mpad,
                            c.gamma ? (const float*)dxg : nullptr, c.shift ? (float*)sh.dev() : nullptr, c.pfx ? (const int*)doff : nullptr);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        for (Buf* b : {&x, &xs, &stt, &sh}) b->down();
        dev_free({dE, dP, dxg, dfeed, doff, dpos});
    } else {
        for (int r = 0; r < rows; r++) {
            const int tok = feed[(size_t)r * feed_ld + pos], mp = mpos_of(r, c.defect != D_PFXCLAMP);
            emu_embed_row(c.mode, &Eh[(size_t)tok * d], &El[(size_t)tok * d], &P[(size_t)mp * d], c.gamma ? xg.data() : nullptr, c.shift, d, r, mpad, 1, x, xs, stt, sh);
        }
    }
    long exact = 0;
    Worst w;
    for (int r = 0; r < rows; r++) {
        const int tok = feed[(size_t)r * feed_ld + pos], mp = mpos_of(r, true);
        double sum = 0, mag = 0;
        std::vector<double> v(d);
        for (int k = 0; k < d; k++) {
            const float want = (Eh[(size_t)tok * d + k] + El[(size_t)tok * d + k]) + P[(size_t)mp * d + k];
            x.mark((long)r * d + k); exact += fbits(x.f((long)r * d + k)) != fbits(want);
            v[k] = want; sum += want; mag += fabs(want);
        }
        const double mean = c.shift ? sum / d : 0.0, emean = c.shift ? U * mag + U * fabs(mean) : 0.0;
        if (c.shift) { sh.mark(r); w.see(sh.f(r), mean, emean); }
        double s1 = 0, s2 = 0, b1 = 0, b2 = 0, m1 = 0, m2 = 0;
        for (int k = 0; k < d; k++) {
            const double u = v[k] - mean, eu = emean + U * fabs(u), g = c.gamma ? xg[k] : 1.0, y = u * g, ey = eu * fabs(g) + U * fabs(y);
            float hi, lo; get((const unsigned char*)(xs.h.data() + GUARD), c.mode, slab(r, k, mpad), hi, lo);
            w.see((double)hi + lo, y, ey + half_ulp_t(c.mode, fabs(y) + ey));
            xs.mark((long)(slab(r, k, mpad) * esz(c.mode) / 4));
            if (c.mode == H2) xs.mark((long)((h2_hi(slab(r, k, mpad)) + 64) / 4)), xs.mark((long)(h2_hi(slab(r, k, mpad)) / 4));
            s1 += u; b1 += eu; m1 += fabs(u); s2 += u * u; b2 += 2 * fabs(u) * eu + eu * eu + U * u * u; m2 += u * u;
        }
        stt.mark(2 * r); stt.mark(2 * r + 1);
        w.see(stt.f(2 * r), s1, b1 + d * U * m1);
        w.see(stt.f(2 * r + 1), s2, b2 + d * U * m2);
    }
    long guard = 0;
    for (Buf* b : {&x, &xs, &stt, &sh}) guard += b->guard();
    const bool ok = w.ratio <= 1.0 && exact == 0 && guard == 0;
    worst_embed = std::max(worst_embed, c.defect ? 0.0 : w.ratio);
    if (!c.defect || !g_host)
        printf("k_dec_embed       %s rows %3d d %4d mpad %3d %s%s%s %-12s: err/bound %.3f x differing %ld guard %ld  x %016llx slab %016llx stats %016llx shift %016llx  %s\n", mode_name[c.mode], rows, d, mpad,
               c.gamma ? "G" : "-", c.shift ? "S" : "-", c.pfx ? "P" : "-", c.what, w.ratio, exact, guard, x.hash(), xs.hash(), stt.hash(), sh.hash(), ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}
static int group_embed() {
    int bad = 0;
    for (Mode md : {BF16, F32, H2}) {
        for (int d : {128, 384, 1280}) for (int rows : {1, 4, 5, 260}) {
            const int k = (d / 128 + rows) % 4;   // the options rotate over the shapes; every combination on rows 5, d 384 below
            bad |= embed_case({"", md, rows, d, (k & 1) != 0, (k & 2) != 0, rows >= 4, 0});
        }
        for (int k = 0; k < 8; k++) bad |= embed_case({"all options", md, 5, 384, (k & 1) != 0, (k & 2) != 0, (k & 4) != 0, 0});
    }
    printf("worst err/bound embed: %.3f\n", worst_embed);
    return bad;
}

// ===== k_argmax_finish, k_nospeech_finish =======================================================================================================
// k_argmax_finish on synthetic partials: text ids below 500, 100 timestamps, EOT 490.  Everything the kernel decides is recomputed from its f32
// inputs and must be equal: the merged (max, index) with the lowest index on ties; the touched ids of the history with their penalised side logits
// (one f32 multiplication), bans, masks and text_lo; the token; out_tokens, n_out, done, feed[pos + 1]; the next row state; the next bitmap, word
// for word; the position and the ticket.  Rule 5 compares the timestamps' log-sum-exp with the best text logit: the decided side is taken from
// the float64 log-sum-exp, and every case is built with a margin above the bound of the kernel's f32 value (a case without one counts as a
// failure); a single allowed timestamp has the sum 1 and the log-sum-exp is its logit exactly.  The log-probability is -log of a sum of exp whose
// terms passed at most L = 14 + passes evaluations of ts_exp and A = 24 + passes additions (the thread's loop over 2048 partials per pass, the
// eight pairwise folds, the history merges, the 8-level tree, the last merge of the two sides), plus 4 U |log| for logf and its argument.
// The fused next-position embedding must equal a k_dec_embed launch of the same token and position bit for bit.
enum { D_FTIELATE = 14, D_F2048, D_RULE5MAX, D_LPTEXT, D_PENPOS, D_DUPTWICE, D_BANKEEP, D_DONEREC, D_FORCEDEOT, D_NSNAN, D_EMBORDER = 27 };
static const int FV = 600, FTB = 500, FEOT = 490, FWORDS = 19, FB = 5, FMPAD = 64;
struct FC {
    const char* what = ""; Mode mode = BF16; int n_parts = 5, gen = 3; bool rules = false, lp = false, rep = false, pfx = false, last = false, nothing = false;
    int ngram = 0; float pen = 1.0f; int n_forced = 0, d = 384; int defect = 0;
};
static void rep_bans_h(const std::vector<int>& hs, int L, int n, int exempt, std::vector<unsigned char>& ban) {
    ban.assign(L + 1, 0);
    for (int i = 0; i < L; i++) {
        bool b = n > 0 && L >= n - 1 && i >= n - 1 && hs[i] < exempt;
        for (int k = 0; b && k < n - 1; k++) b = hs[i - (n - 1) + k] == hs[L - (n - 1) + k];
        ban[i] = b;
    }
}
static void ts_next_state_h(int next, bool pen_ts, int prev_last_t, int tb, int eot, int vocab, int* s) {
    const bool last_ts = next >= tb;
    const int last_t = last_ts ? next : prev_last_t;
    int text_lo = 0, ts_lo = tb;
    if (last_ts && pen_ts) ts_lo = vocab; else if (last_ts) text_lo = eot;
    if (last_t >= 0 && ts_lo < vocab) ts_lo = std::max(ts_lo, (last_ts && !pen_ts) ? last_t : last_t + 1);
    s[0] = text_lo; s[1] = ts_lo; s[2] = vocab - 1; s[3] = last_t;
}
// the touched bits a row carries into a position whose history is hs[0 .. L): the penalised ids and the banned ones
static void rep_bits_h(const std::vector<int>& hs, int L, const FC& c, int exempt, unsigned* bits) {
    std::vector<unsigned char> ban;
    rep_bans_h(hs, L, c.ngram, exempt, ban);
    for (int w = 0; w < FWORDS; w++) bits[w] = 0;
    for (int i = 0; i < L; i++) if (hs[i] >= 0 && hs[i] < FV && ((c.pen != 1.0f && hs[i] < std::min(exempt, FV)) || ban[i])) bits[hs[i] >> 5] |= 1u << (hs[i] & 31);
}
static double worst_fin = 0;
static long fin_embed_cases = 0, fin_embed_diff = 0;

static int finish_case(const FC& c) {
    const int B = FB, mpad = FMPAD, NP = c.n_parts, n_prompt = 4, pos = c.gen + n_prompt - 1, tok_ld = c.last ? pos + 1 : pos + 3, ctx = tok_ld + 2, d = c.d, ts_ld = FV - FTB;
    const int exempt = c.rules ? FTB : 0x7fffffff, passes = (NP + 2047) / 2048, histL = std::min(std::max(c.gen, 0), WH_REP_MAX_HIST);
    const float inv = 1.0f / c.pen;
    rs = 31337u + 7u * NP + 13u * c.gen + 3u * c.rules + 5u * c.lp + 11u * c.rep + 17u * c.ngram + c.n_forced;
    // ---- inputs ----
    std::vector<float> pval((size_t)NP * mpad, -INFINITY), psum((size_t)NP * mpad, 0.0f);
    std::vector<int> pidx((size_t)NP * mpad, NONE_IDX);
    for (int p = 0; p < NP; p++) for (int b = 0; b < B; b++) {
        if (c.nothing || p % 7 == 3) continue;
        pval[(size_t)p * mpad + b] = frand(3.0f); pidx[(size_t)p * mpad + b] = (int)(rnd() % 480); psum[(size_t)p * mpad + b] = 1.0f + fabsf(frand(2.0f));
    }
    auto plant = [&](int p, int b, float v, int id) { pval[(size_t)p * mpad + b] = v; pidx[(size_t)p * mpad + b] = id; psum[(size_t)p * mpad + b] = 1.25f; };
    if (!c.nothing) {
        if (NP >= 3) { plant(1, 0, 7.5f, 120); plant(NP - 1, 0, 7.5f, 300); plant(1, 1, 7.5f, 300); plant(NP - 1, 1, 7.5f, 120); }   // ties between partials
        plant(NP - 1, 2, 8.25f, FEOT);   // the maximum in the last partial; the row chooses EOT
    }
    std::vector<int> feed((size_t)B * tok_ld, 1), done(B, 0), n_out(B, n_prompt + std::max(c.gen, 0)), forced(std::max(c.n_forced, 1)), state((size_t)mpad * 4, 0), off(B);
    done[3] = 1;
    for (int i = 0; i < c.n_forced; i++) forced[i] = 77 + i;
    std::vector<std::vector<int>> hist(B, std::vector<int>(histL + 1, 0));
    for (int b = 0; b < B; b++) {
        for (int i = 0; i < histL; i++) hist[b][i] = (i % 9 == 8) ? FTB + (int)(rnd() % 50) : 10 + (int)(rnd() % 20);
        if (histL >= 5) { hist[b][0] = 11; hist[b][1] = 12; hist[b][2] = 13; hist[b][histL - 2] = 11; hist[b][histL - 1] = 12; }   // 13 closes a repeated trigram
        for (int i = 0; i < histL && n_prompt + i < tok_ld; i++) feed[(size_t)b * tok_ld + n_prompt + i] = hist[b][i];
        int* s = &state[4 * b];
        s[0] = b == 4 ? 15 : 0; s[1] = FTB; s[2] = FV - 1; s[3] = -1;
        off[b] = b == 0 ? 0 : b == 1 ? pos + 1 : b == 2 ? pos + 2 : b - 2;
    }
    std::vector<unsigned> bits((size_t)B * FWORDS, 0), mfirst(FWORDS, 0), mbase(FWORDS, 0);
    mbase[0] |= 1u << 20; mfirst[0] |= 1u << 21;
    std::vector<float> side((size_t)B * FV, 0.0f);
    if (c.rep) for (int b = 0; b < B; b++) {
        rep_bits_h(hist[b], histL, c, exempt, &bits[(size_t)b * FWORDS]);
        for (int id = 0; id < FV; id++) side[(size_t)b * FV + id] = frand(4.0f);
        if (histL >= 2 && !c.nothing) side[(size_t)b * FV + hist[b][1]] = b & 1 ? 30.0f : -0.001f;   // a penalised id that can win; a negative one
        if (c.nothing) for (int id = 0; id < FV; id++) side[(size_t)b * FV + id] = -INFINITY;
    }
    // ---- the contract on the host: text side ----
    struct Row { float bv = -INFINITY; int bi = NONE_IDX; double S = 0, eS = 1e-37; int tok = 0, next = 0; double lp = -INFINITY, elp = 0; bool take = false; };
    std::vector<Row> ex(B);
    const int Lf = 14 + passes, Af = 24 + passes;
    const unsigned* pmask = c.gen == 0 ? mfirst.data() : mbase.data();
    for (int b = 0; b < B; b++) {
        Row& r = ex[b];
        std::vector<std::pair<float, double>> cand;   // (value, weight)
        std::vector<int> cid;
        for (int p = 0; p < NP; p++) { cand.push_back({pval[(size_t)p * mpad + b], psum[(size_t)p * mpad + b]}); cid.push_back(pidx[(size_t)p * mpad + b]); }
        if (c.rep) {
            std::vector<unsigned char> ban;
            rep_bans_h(hist[b], histL, c.ngram, exempt, ban);
            const int text_lo = c.rules ? (c.gen > 0 ? state[4 * b] : FTB) : 0;
            for (int i = 0; i < histL; i++) {
                const int id = hist[b][i];
                bool first = true, banned = false;
                for (int j = 0; j < histL; j++) if (hist[b][j] == id) { first = first && j >= i; banned = banned || ban[j]; }
                if (!first || id < 0 || id >= FV || !((bits[(size_t)b * FWORDS + (id >> 5)] >> (id & 31)) & 1u)) continue;
                if (banned || ((pmask[id >> 5] >> (id & 31)) & 1u) || id < text_lo) continue;
                float v = side[(size_t)b * FV + id];
                v = v > 0.0f ? v * inv : v * c.pen;
                if (!(v > -INFINITY)) continue;
                cand.push_back({v, 1.0}); cid.push_back(id);
            }
        }
        for (size_t i = 0; i < cand.size(); i++) if (cand[i].first > r.bv || (cand[i].first == r.bv && cid[i] < r.bi)) { r.bv = cand[i].first; r.bi = cid[i]; }
        for (size_t i = 0; i < cand.size(); i++) if (cand[i].first > -INFINITY) {
            const double dl = (double)cand[i].first - r.bv, e = cand[i].second * exp(dl);
            r.S += e; r.eS += e * (3 * fabs(dl) + 3 * Lf + Af) * U;
        }
    }
    // ---- timestamps: built around the text side so that rule 5 has a margin ----
    std::vector<float> tsl((size_t)mpad * ts_ld, -INFINITY);
    long nomargin = 0;
    if (c.rules && !c.nothing) for (int b = 0; b < B; b++) {
        const float T = ex[b].bv > -INFINITY ? ex[b].bv : 0.0f;
        float* t = &tsl[(size_t)b * ts_ld];
        if (b == 0 || b == 1) for (int j : {10, 20, 30, 40}) t[j] = T - logf(4.0f) + (b == 0 ? 0.01f : -0.01f);   // log-sum-exp just above / just below the text maximum
        else if (b == 2) t[33] = T;   // a tie between the best text id and the only timestamp
        else if (b == 4) for (int j : {3, 50, 51, 98, 99}) t[j] = T - 3.0f + frand(0.5f);
    }
    // ---- device (or the emulation) ----
    Buf o_out, o_nout, o_done, o_feed, o_lp, o_state, o_bits, o_pos, o_x, o_xs, o_st, o_sh;
    auto fill = [&](Buf& bf, const std::vector<int>& v) { bf.make((long)v.size(), false); for (size_t i = 0; i < v.size(); i++) bf.init((long)i, (unsigned)v[i]); bf.up(); bf.mark_all(); };
    // (one row more: the slot of the last position, n_prompt + gen == tok_ld, is the next row's first)
    o_out.make((long)(B + 1) * tok_ld); o_lp.make(c.lp ? (long)(B + 1) * tok_ld : 0);
    fill(o_nout, n_out); fill(o_done, done); fill(o_feed, feed); fill(o_state, state);
    { std::vector<int> bi(bits.begin(), bits.end()); fill(o_bits, bi); }
    fill(o_pos, std::vector<int>{pos, 0});   // {position, ticket}
    const long slab_words = (long)(d / 32) * mpad * 32 * (long)esz(c.mode) / 4;
    o_x.make((long)B * d); o_xs.make(slab_words); o_st.make((long)mpad * 2); o_sh.make(mpad);
    Buf r_x, r_xs, r_st, r_sh;   // the same rows by k_dec_embed
    r_x.make((long)B * d); r_xs.make(slab_words); r_st.make((long)mpad * 2); r_sh.make(mpad);
    std::vector<unsigned char> hE((size_t)FV * d * esz(c.mode));
    std::vector<float> Eh((size_t)FV * d), El((size_t)FV * d), P((size_t)ctx * d), xg(d);
    for (size_t i = 0; i < Eh.size(); i++) put(hE.data(), c.mode, i, frand(1.0f) + 0.25f, Eh[i], El[i]);
    for (auto& v : P) v = frand(0.5f);
    for (auto& v : xg) v = 0.5f + fabsf(frand(1.0f));
    const bool gamma = c.gen & 1;
    auto mpos_of = [&](int b) { return c.pfx ? std::max(pos + 1 - std::max(off[b], 0), 0) : pos + 1; };
    if (!g_host) {
        void *dpv = to_dev(pval), *dpi = to_dev(pidx), *dps = to_dev(psum), *dforced = to_dev(forced), *dtsl = to_dev(tsl), *dside = to_dev(side), *dmf = to_dev(mfirst), *dmb = to_dev(mbase),
             *dE = to_dev(hE), *dP = to_dev(P), *dxg = to_dev(xg), *doff = to_dev(off);
        DecodeState st;
        st.feed = (int*)o_feed.dev(); st.out_tokens = (int*)o_out.dev(); st.n_out = (int*)o_nout.dev(); st.done = (int*)o_done.dev(); st.forced = (const int*)dforced; st.n_forced = c.n_forced;
        st.n_prompt = n_prompt; st.eot = FEOT; st.tok_ld = tok_ld; st.logprob = c.lp ? (float*)o_lp.dev() : nullptr;
        NextEmbed ne;
        ne.tok_emb = dE; ne.pos_emb = (const float*)dP; ne.x = (float*)o_x.dev(); ne.xslab = o_xs.dev(); ne.stats = (float*)o_st.dev(); ne.shift = (float*)o_sh.dev();
        ne.xgamma = gamma ? (const float*)dxg : nullptr; ne.d = d; ne.mpad = mpad; ne.off = c.pfx ? (const int*)doff : nullptr;
        TsFinish ts;
        if (c.rules) { ts.rules = true; ts.ts_logits = (const float*)dtsl; ts.ts_ld = ts_ld; ts.state = (int*)o_state.dev(); ts.ts_begin = FTB; ts.vocab = FV; }
        RepFinish rp;
        if (c.rep) { rp.on = true; rp.bits = (unsigned*)o_bits.dev(); rp.side = (const float*)dside; rp.words = FWORDS; rp.vocab = FV; rp.p = c.pen; rp.inv = inv; rp.ngram = c.ngram; rp.exempt_from = exempt;
                     rp.mask_first = (const unsigned*)dmf; rp.mask_base = (const unsigned*)dmb; }
        int* dpos = (int*)o_pos.dev();
        wh_launch_argmax_finish(0, prec_of(c.mode), (const float*)dpv, (const int*)dpi, NP, mpad, dpos, dpos + 1, st, B, ne, ts, c.lp ? (const float*)dps : nullptr, rp);
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        for (Buf* bf : {&o_out, &o_nout, &o_done, &o_feed, &o_lp, &o_state, &o_bits, &o_pos, &o_x, &o_xs, &o_st, &o_sh}) bf->down();
        // the reference embedding: k_dec_embed of the tokens the kernel fed, at position pos + 1 (a one-column token table, so the last position has one too)
        std::vector<int> f2(B), p2 = {pos + 1};
        for (int b = 0; b < B; b++) f2[b] = c.last ? -1 : o_feed.i32((long)b * tok_ld + pos + 1);
        if (!c.last) {
            std::vector<int> ftab((size_t)B * (pos + 2), 0);
            for (int b = 0; b < B; b++) ftab[(size_t)b * (pos + 2) + pos + 1] = std::min(std::max(f2[b], 0), FV - 1);
            void *dft = to_dev(ftab), *dp2 = to_dev(p2);
            wh_launch_dec_embed(0, prec_of(c.mode), dE, (const float*)dP, (const int*)dft, pos + 2, (const int*)dp2, (float*)r_x.dev(), r_xs.dev(), (float*)r_st.dev(), B, d, mpad,
                                gamma ? (const float*)dxg : nullptr, (float*)r_sh.dev(), c.pfx ? (const int*)doff : nullptr);
            CK(hipGetLastError()); CK(hipDeviceSynchronize());
            dev_free({dft, dp2});
        }
        for (Buf* bf : {&r_x, &r_xs, &r_st, &r_sh}) bf->down();
        dev_free({dpv, dpi, dps, dforced, dtsl, dside, dmf, dmb, dE, dP, dxg, doff});
    } else {   // the kernel in f32, one partial after the other
        const int df = c.defect;
        for (int b = 0; b < B; b++) {
            float bv = -INFINITY, bs = 0.0f; int bi = NONE_IDX;
            auto merge = [&](float v, int id, float s) {
                if (c.lp) bs = lp_merge_h(bv, bs, v, s);
                if (v > bv || (v == bv && (df == D_FTIELATE ? v > -INFINITY : id < bi))) { bv = v; bi = id; }
            };
            for (int p = 0; p < (df == D_F2048 ? std::min(NP, 2048) : NP); p++) merge(pval[(size_t)p * mpad + b], pidx[(size_t)p * mpad + b], psum[(size_t)p * mpad + b]);
            std::vector<unsigned char> ban;
            if (c.rep) {
                rep_bans_h(hist[b], histL, c.ngram, exempt, ban);
                const int text_lo = c.rules ? (c.gen > 0 ? state[4 * b] : FTB) : 0;
                for (int i = 0; i < histL; i++) {
                    const int id = hist[b][i];
                    bool first = true, banned = false;
                    for (int j = 0; j < histL; j++) if (hist[b][j] == id) { first = first && j >= i; banned = banned || ban[j]; }
                    if ((!first && df != D_DUPTWICE) || id < 0 || id >= FV || !((bits[(size_t)b * FWORDS + (id >> 5)] >> (id & 31)) & 1u)) continue;
                    if (banned || ((pmask[id >> 5] >> (id & 31)) & 1u) || id < text_lo) continue;
                    float v = side[(size_t)b * FV + id];
                    v = (v > 0.0f) == (df != D_PENPOS) ? v * inv : v * c.pen;
                    if (!(v > -INFINITY)) continue;
                    const float sv = bv; const int si = bi;
                    if (c.lp) bs = lp_merge_h(bv, bs, v, 1.0f);
                    if (v > sv || (v == sv && id < si)) { bv = v; bi = id; }
                }
            }
            int tok = bi == NONE_IDX ? 0 : bi;
            float lp = -INFINITY;
            if (c.rules) {
                float tm = -INFINITY, tsum = 0.0f; int ti = NONE_IDX;
                for (int j = 0; j < ts_ld; j++) { const float v = tsl[(size_t)b * ts_ld + j]; if (v > tm) { tsum = tsum * ts_exp_h(tm - v) + 1.0f; tm = v; ti = FTB + j; } else if (v > -INFINITY) tsum += ts_exp_h(v - tm); }
                const float lse = tm == -INFINITY ? -INFINITY : df == D_RULE5MAX ? tm : tm + logf(tsum);
                int w;
                if (lse > bv) w = ti; else w = (tm > bv || (tm == bv && ti < bi)) ? ti : bi;
                tok = w == NONE_IDX ? 0 : w;
                if (c.lp && w != NONE_IDX) lp = -logf((lse > bv && df != D_LPTEXT) ? tsum : lp_merge_h(bv, bs, tm, tsum));
            } else if (c.lp && bi != NONE_IDX) lp = -logf(bs);
            int next = tok;
            if (!done[b] || df == D_DONEREC) {
                o_out.setu((long)b * tok_ld + n_prompt + c.gen, tok); o_nout.setu(b, n_prompt + c.gen + 1);
                if (c.lp) o_lp.setf((long)b * tok_ld + n_prompt + c.gen, lp);
            }
            if (!done[b]) {
                const bool is_forced = c.gen < c.n_forced;
                if (is_forced) next = forced[c.gen];
                if (tok == FEOT && (!is_forced || df == D_FORCEDEOT)) o_done.setu(b, 1);
            }
            if (pos + 1 < tok_ld) o_feed.setu((long)b * tok_ld + pos + 1, next);
            if (c.rules) { int s[4]; ts_next_state_h(next, c.gen == 0 || feed[(size_t)b * tok_ld + pos] >= FTB, c.gen == 0 ? -1 : state[4 * b + 3], FTB, FEOT, FV, s); for (int k = 0; k < 4; k++) o_state.setu(4 * b + k, s[k]); }
            if (c.rep) {
                std::vector<unsigned> w(bits.begin() + (size_t)b * FWORDS, bits.begin() + (size_t)(b + 1) * FWORDS);
                const bool pen = c.pen != 1.0f;
                if (!pen && df != D_BANKEEP) for (int i = 0; i < histL; i++) if (ban[i]) w[hist[b][i] >> 5] &= ~(1u << (hist[b][i] & 31));
                std::vector<int> h2v = hist[b]; h2v[histL] = next;
                std::vector<unsigned char> ban2;
                rep_bans_h(h2v, histL + 1, c.ngram, exempt, ban2);
                if (pen && next >= 0 && next < std::min(exempt, FV)) w[next >> 5] |= 1u << (next & 31);
                for (int i = 0; i < histL + 1; i++) if (ban2[i] && h2v[i] >= 0 && h2v[i] < FV) w[h2v[i] >> 5] |= 1u << (h2v[i] & 31);
                for (int k = 0; k < FWORDS; k++) o_bits.setu((long)b * FWORDS + k, w[k]);
            }
            const int ntok = std::min(std::max(next, 0), FV - 1);
            emu_embed_row(c.mode, &Eh[(size_t)ntok * d], &El[(size_t)ntok * d], &P[(size_t)mpos_of(b) * d], gamma ? xg.data() : nullptr, true, d, b, mpad, df == D_EMBORDER ? 0 : 1, o_x, o_xs, o_st, o_sh);
            if (!c.last) emu_embed_row(c.mode, &Eh[(size_t)ntok * d], &El[(size_t)ntok * d], &P[(size_t)mpos_of(b) * d], gamma ? xg.data() : nullptr, true, d, b, mpad, 1, r_x, r_xs, r_st, r_sh);
        }
        o_pos.setu(0, pos + 1); o_pos.setu(1, 0);
    }
    // ---- the check ----
    long exact = 0;
    Worst w;
    std::vector<int> e_feed = feed, e_done = done, e_nout = n_out, e_state = state;
    std::vector<unsigned> e_bits = bits;
    for (int b = 0; b < B; b++) {
        Row& r = ex[b];
        int tok = r.bi == NONE_IDX ? 0 : r.bi;
        if (c.rules) {
            double tm = -INFINITY, tS = 0, etS = 1e-37; int ti = NONE_IDX, cnt = 0;
            const float* t = &tsl[(size_t)b * ts_ld];
            for (int j = 0; j < ts_ld; j++) if (t[j] > tm) { tm = t[j]; ti = FTB + j; }
            for (int j = 0; j < ts_ld; j++) if (t[j] > -INFINITY) { const double dl = (double)t[j] - tm, e = exp(dl); tS += e; etS += e * (3 * fabs(dl) + 3 * 10 + 10) * U; cnt++; }
            const double lse = cnt ? tm + log(tS) : -INFINITY;
            bool take;
            if (cnt <= 1) take = lse > r.bv;   // (one timestamp: the sum is 1 and the log-sum-exp its logit, exactly)
            else {
                const double e_lse = etS / tS + 4 * U * fabs(log(tS)) + 2 * U * fabs(lse);
                if (!(fabs(lse - (double)r.bv) > e_lse)) nomargin++;
                take = lse > r.bv;
            }
            const int wv = take ? ti : ((tm > r.bv || (tm == r.bv && ti < r.bi)) ? ti : r.bi);
            tok = wv == NONE_IDX ? 0 : wv;
            if (c.lp && wv != NONE_IDX) {
                double S, eS;
                if (take) { S = tS; eS = etS; }
                else { const double mx = std::max((double)r.bv, tm), a = r.bv > -INFINITY ? exp(r.bv - mx) : 0.0, q = cnt ? exp(tm - mx) : 0.0; S = r.S * a + tS * q; eS = (r.eS + 8 * U * r.S) * a + (etS + 8 * U * tS) * q; }
                r.lp = -log(S); r.elp = eS / S + 4 * U * fabs(r.lp) + 2 * U;
            }
        } else if (c.lp && r.bi != NONE_IDX) { r.lp = -log(r.S); r.elp = r.eS / r.S + 4 * U * fabs(r.lp) + 2 * U; }
        int next = tok;
        if (!done[b]) {
            const long slot = (long)b * tok_ld + n_prompt + c.gen;
            o_out.mark(slot); exact += o_out.i32(slot) != tok;
            e_nout[b] = n_prompt + c.gen + 1;
            if (c.lp) { o_lp.mark(slot); w.see(o_lp.f(slot), r.lp, r.elp); }
            if (c.gen < c.n_forced) next = forced[c.gen]; else if (tok == FEOT) e_done[b] = 1;
        }
        if (pos + 1 < tok_ld) e_feed[(size_t)b * tok_ld + pos + 1] = next;
        if (c.rules) ts_next_state_h(next, c.gen == 0 || feed[(size_t)b * tok_ld + pos] >= FTB, c.gen == 0 ? -1 : state[4 * b + 3], FTB, FEOT, FV, &e_state[4 * b]);
        if (c.rep) {
            unsigned* wd = &e_bits[(size_t)b * FWORDS];
            std::vector<unsigned char> ban, ban2;
            rep_bans_h(hist[b], histL, c.ngram, exempt, ban);
            const bool pen = c.pen != 1.0f;
            if (!pen) for (int i = 0; i < histL; i++) if (ban[i]) wd[hist[b][i] >> 5] &= ~(1u << (hist[b][i] & 31));
            std::vector<int> h2v = hist[b]; h2v[histL] = next;
            rep_bans_h(h2v, histL + 1, c.ngram, exempt, ban2);
            if (pen && next >= 0 && next < std::min(exempt, FV)) wd[next >> 5] |= 1u << (next & 31);
            for (int i = 0; i < histL + 1; i++) if (ban2[i] && h2v[i] >= 0 && h2v[i] < FV) wd[h2v[i] >> 5] |= 1u << (h2v[i] & 31);
        }
        r.tok = tok; r.next = next;
    }
    exact += nomargin;
    for (int b = 0; b < B; b++) exact += (o_nout.i32(b) != e_nout[b]) + (o_done.i32(b) != e_done[b]);
    for (size_t i = 0; i < e_feed.size(); i++) exact += o_feed.i32((long)i) != e_feed[i];
    for (size_t i = 0; i < e_state.size(); i++) exact += o_state.i32((long)i) != e_state[i];
    for (size_t i = 0; i < e_bits.size(); i++) exact += o_bits.u32((long)i) != e_bits[i];
    exact += (o_pos.i32(0) != pos + 1) + (o_pos.i32(1) != 0);   // the position advances exactly once, the ticket is re-armed
    // the fused embedding: bit for bit k_dec_embed's
    long ediff = 0;
    for (int b = 0; b < B; b++) {
        for (int k = 0; k < d; k++) o_x.mark((long)b * d + k);
        for (long i = 0; i < slab_words; i++) {   // the row's words of the slab: 32 elements of every k-slab
            const long per_row = 32 * (long)esz(c.mode) / 4, blk = i / per_row;
            if (blk % mpad == b) { o_xs.mark(i); if (!c.last) ediff += o_xs.u32(i) != r_xs.u32(i); }
        }
        o_st.mark(2 * b); o_st.mark(2 * b + 1); o_sh.mark(b);
        if (!c.last) {
            for (int k = 0; k < d; k++) ediff += o_x.u32((long)b * d + k) != r_x.u32((long)b * d + k);
            ediff += (o_st.u32(2 * b) != r_st.u32(2 * b)) + (o_st.u32(2 * b + 1) != r_st.u32(2 * b + 1)) + (o_sh.u32(b) != r_sh.u32(b));
        }
    }
    if (!c.last) { fin_embed_cases++; fin_embed_diff += ediff != 0; }
    long guard = 0;
    for (Buf* bf : {&o_out, &o_nout, &o_done, &o_feed, &o_lp, &o_state, &o_bits, &o_pos, &o_x, &o_xs, &o_st, &o_sh}) guard += bf->guard();
    const bool ok = w.ratio <= 1.0 && exact == 0 && guard == 0 && ediff == 0;
    if (!c.defect) worst_fin = std::max(worst_fin, w.ratio);
    if (!c.defect || !g_host)
        printf("k_argmax_finish   %s parts %4d gen %3d %s%s%s%s ngram %d pen %.2f forced %d %-34s: err/bound logprob %.3f exact %ld (no margin %ld) embed differing %ld guard %ld  tokens %016llx logprob %016llx state %016llx bits %016llx x %016llx  %s\n",
               mode_name[c.mode], NP, c.gen, c.rules ? "R" : "-", c.lp ? "L" : "-", c.pfx ? "X" : "-", c.rep ? "P" : "-", c.ngram, c.pen, c.n_forced, c.what, w.ratio, exact, nomargin, ediff, guard,
               o_feed.hash(o_out.hash()), o_lp.hash(), o_state.hash(), o_bits.hash(), o_sh.hash(o_st.hash(o_xs.hash(o_x.hash()))), ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

// k_nospeech_finish: prob = exp(probe - max - log(sum)) from the row's (max, sum) partials.  The sum's terms pass at most L = 8 + n_parts / 64
// evaluations and as many additions; logf and expf (1 ulp each, and the rounding of their arguments) add 4 U (|log| + |x| + 1) relative.
static int nospeech_case(int NP, int kind, int defect) {
    const int B = 3, mpad = FMPAD;
    rs = 777u + NP + 10u * kind;
    std::vector<float> pval((size_t)NP * mpad), psum((size_t)NP * mpad), probe(B);
    for (int p = 0; p < NP; p++) for (int b = 0; b < B; b++) {
        const bool empty = kind == 2 || (kind == 1 && (p == 0 || p == NP / 2) && NP > 1 && b != 1);
        pval[(size_t)p * mpad + b] = empty ? -INFINITY : frand(4.0f); psum[(size_t)p * mpad + b] = empty ? 0.0f : 1.0f + fabsf(frand(3.0f));
    }
    for (auto& v : probe) v = frand(3.0f);
    Buf prob, pos;
    prob.make(B); pos.make(1, false); pos.init(0, 3); pos.up(); pos.mark(0);
    if (!g_host) {
        void *dpv = to_dev(pval), *dps = to_dev(psum), *dpr = to_dev(probe);
        wh_launch_nospeech_finish(0, (const float*)dpv, (const float*)dps, NP, mpad, (const float*)dpr, (float*)prob.dev(), B, (int*)pos.dev());
        CK(hipGetLastError()); CK(hipDeviceSynchronize());
        prob.down(); pos.down(); dev_free({dpv, dps, dpr});
    } else {
        for (int b = 0; b < B; b++) {
            float m = -INFINITY, s = 0.0f;
            for (int p = 0; p < NP; p++) {
                const float m1 = pval[(size_t)p * mpad + b], s1 = psum[(size_t)p * mpad + b], mx = fmaxf(m, m1);
                s = defect == D_NSNAN ? s * ts_exp_h(m - mx) + s1 * ts_exp_h(m1 - mx) : lp_merge_h(m, s, m1, s1);
                m = mx;
            }
            prob.setf(b, (m == -INFINITY && defect != D_NSNAN) ? 0.0f : expf(probe[b] - m - logf(s)));
        }
        pos.setu(0, 4);
    }
    Worst w;
    for (int b = 0; b < B; b++) {
        double m = -INFINITY, S = 0, eS = 1e-37;
        for (int p = 0; p < NP; p++) m = std::max(m, (double)pval[(size_t)p * mpad + b]);
        for (int p = 0; p < NP; p++) if (pval[(size_t)p * mpad + b] > -INFINITY) {
            const double dl = pval[(size_t)p * mpad + b] - m, e = psum[(size_t)p * mpad + b] * exp(dl);
            S += e; eS += e * (3 * fabs(dl) + 4 * (8 + NP / 64 + 1)) * U;
        }
        prob.mark(b);
        if (m == -INFINITY) { w.see(prob.f(b), 0.0, 1e-37); continue; }
        const double x = probe[b] - m - log(S), want = exp(x);
        w.see(prob.f(b), want, want * (eS / S + 4 * U * (fabs(log(S)) + fabs(x) + fabs(m) + fabs((double)probe[b]) + 1)) + 1e-37);
    }
    const long exact = pos.i32(0) != 4, guard = prob.guard() + pos.guard();
    const bool ok = w.ratio <= 1.0 && !exact && !guard;
    if (!defect) worst_fin = std::max(worst_fin, w.ratio);
    if (!defect || !g_host)
        printf("k_nospeech_finish parts %3d %-22s: err/bound %.3f exact %ld guard %ld  prob %016llx  %s\n", NP, kind == 0 ? "" : kind == 1 ? "-inf partials" : "every partial -inf", w.ratio, exact, guard, prob.hash(),
               ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

// The chain: k_lm_head<RULES, LP, REP> -> k_argmax_finish<RULES, LP, REP> over six positions on device buffers that only the kernels write after
// the start — the position and its ticket, feed, the row state, the repetition bitmap, done, n_out.  What one kernel writes is what the next one
// reads: the finish's row state and bitmap steer the next LM head, the LM head's partials, timestamp and side logits feed the finish.  The host
// keeps its own copy of all of it, advanced per position from the operand set's reference logits alone (the activations do not change, so every
// position's logits are L0): allowed ranges, masks, touched ids, penalties, bans, rule 5 (with the margin condition of the finish cases), the
// token, the forced first position (a timestamp, so the next position may emit none), a row that is done from the start.  After every position
// the device's arrays must equal the host's, word for word; the log-probability within the sum bound with both kernels' L and A added.
enum { D_CHAINSTATE = 28 };
static int chain_case(Mode md, int defect) {
    const int B = 5, N = 1003, K = 128, tb = 903, eot = 890, n_prompt = N_PROMPT, G = 6, tok_ld = n_prompt + G + 1, ngram = 2, ts_ld = N - tb;
    const float pen = 1.3f, inv = 1.0f / pen;
    Ops o; make_ops(o, md, B, N, K, true, Spec());
    double rv = 0;
    reference(o, D_NONE, &rv);
    const int words = o.words, mpad = o.mpad, prec = prec_of(md);
    const std::vector<int> forced = {905};
    HOut r;
    r.sel.resize(B);
    for (int b = 0; b < B; b++) r.sel[b] = b;
    static float placeholder[4];
    SkinnyArgs a;
    a.X = g_host ? (const void*)placeholder : o.dX; a.x_mpad = mpad; a.W = o.dW; a.M = B; a.N = N; a.K = K;
    a.ln_part = (const float*)o.dlnp; a.ln_tiles = o.ln_tiles; a.ln_s = (const float*)o.dlns; a.bias = (const float*)o.dbias; a.n_prompt = n_prompt;
    setenv("WH_LM_TILE_MIN_ROWS", "0", 1);
    r.n_parts = wh_lm_head_parts(prec, a);
    const int tiles = ((N + 15) / 16 + r.n_parts - 1) / r.n_parts;
    r.L = 4 * tiles + 2; r.A = 4 * tiles + 2;
    const long pw = (long)r.n_parts * mpad;
    r.logits.make((long)B * G * N); r.pval.make(pw); r.pidx.make(pw); r.psum.make(pw); r.tsl.make((long)mpad * ts_ld); r.side.make((long)B * N); r.probe.make(0);
    // the state, as a call's start leaves it
    std::vector<int> e_state((size_t)mpad * 4, 0), e_feed((size_t)B * tok_ld, 0), e_out((size_t)B * tok_ld, 0), e_nout(B, n_prompt), e_done(B, 0);
    std::vector<unsigned> e_bits((size_t)B * words, 0);
    for (int b = 0; b < B; b++) for (int i = 0; i < n_prompt; i++) e_feed[(size_t)b * tok_ld + i] = e_out[(size_t)b * tok_ld + i] = 1 + b + i;
    e_done[3] = 1;
    Buf o_state, o_feed, o_out, o_nout, o_done, o_bits, o_pos, o_lp;
    auto fill = [&](Buf& bf, const std::vector<int>& v) { bf.make((long)v.size(), false); for (size_t i = 0; i < v.size(); i++) bf.init((long)i, (unsigned)v[i]); bf.up(); bf.mark_all(); };
    fill(o_state, e_state); fill(o_feed, e_feed); fill(o_out, e_out); fill(o_nout, e_nout); fill(o_done, e_done); fill(o_bits, std::vector<int>(e_bits.begin(), e_bits.end()));
    fill(o_pos, std::vector<int>{n_prompt - 1, 0});
    o_lp.make((long)B * tok_ld);
    void* dforced = to_dev(forced);
    long exact = 0, nomargin = 0;
    Worst w;
    for (int g = 0; g < G; g++) {
        const int pos = n_prompt - 1 + g;
        const unsigned* mask = g == 0 ? o.mfirst.data() : o.mbase.data();
        if (!g_host) {
            a.pos_p = (const int*)o_pos.dev(); a.mask_first = (const unsigned*)o.dmf; a.mask_base = (const unsigned*)o.dmb;
            a.logits = (float*)r.logits.dev(); a.logits_rows = G;
            a.part_val = (float*)r.pval.dev(); a.part_idx = (int*)r.pidx.dev(); a.part_sum = (float*)r.psum.dev();
            a.ts_state = (const int*)o_state.dev(); a.ts_logits = (float*)r.tsl.dev(); a.ts_ld = ts_ld; a.ts_begin = tb; a.ts_max_init = -1;
            a.rep_bits = (const unsigned*)o_bits.dev(); a.rep_side = (float*)r.side.dev(); a.rep_words = words;
            wh_launch_lm_head(0, prec, a);
            DecodeState st;
            st.feed = (int*)o_feed.dev(); st.out_tokens = (int*)o_out.dev(); st.n_out = (int*)o_nout.dev(); st.done = (int*)o_done.dev(); st.forced = (const int*)dforced; st.n_forced = 1;
            st.n_prompt = n_prompt; st.eot = eot; st.tok_ld = tok_ld; st.logprob = (float*)o_lp.dev();
            TsFinish ts; ts.rules = true; ts.ts_logits = (const float*)r.tsl.dev(); ts.ts_ld = ts_ld; ts.state = (int*)o_state.dev(); ts.ts_begin = tb; ts.vocab = N;
            RepFinish rp; rp.on = true; rp.bits = (unsigned*)o_bits.dev(); rp.side = (const float*)r.side.dev(); rp.words = words; rp.vocab = N; rp.p = pen; rp.inv = inv; rp.ngram = ngram;
            rp.exempt_from = tb; rp.mask_first = (const unsigned*)o.dmf; rp.mask_base = (const unsigned*)o.dmb;
            int* dpos = (int*)o_pos.dev();
            wh_launch_argmax_finish(0, prec, (const float*)r.pval.dev(), (const int*)r.pidx.dev(), r.n_parts, mpad, dpos, dpos + 1, st, B, NextEmbed(), ts, (const float*)r.psum.dev(), rp);
            CK(hipGetLastError()); CK(hipDeviceSynchronize());
            for (Buf* bf : {&r.logits, &o_state, &o_feed, &o_out, &o_nout, &o_done, &o_bits, &o_pos, &o_lp}) bf->peek();
        } else {   // both kernels in f32, on the emulation's own state
            std::vector<int> st(o_state.h.begin() + GUARD, o_state.h.begin() + GUARD + (long)mpad * 4);
            std::vector<unsigned> rep(o_bits.h.begin() + GUARD, o_bits.h.begin() + GUARD + (long)B * words);
            Var v = var("", true, true, true, g, tb); v.lmode = 1; v.lrows = G;
            emu_head(o, v, st, rep, r);
            for (int b = 0; b < B; b++) {
                float bv = -INFINITY, bs = 0.0f; int bi = NONE_IDX;
                for (int p = 0; p < r.n_parts; p++) {
                    const float pv = r.pval.f((long)p * mpad + b); const int pi = r.pidx.i32((long)p * mpad + b);
                    bs = lp_merge_h(bv, bs, pv, r.psum.f((long)p * mpad + b));
                    if (pv > bv || (pv == bv && pi < bi)) { bv = pv; bi = pi; }
                }
                std::vector<int> hs(g + 1, 0);
                for (int i = 0; i < g; i++) hs[i] = o_feed.i32((long)b * tok_ld + n_prompt + i);
                std::vector<unsigned char> ban;
                rep_bans_h(hs, g, ngram, tb, ban);
                const int text_lo = g > 0 ? st[4 * b] : tb;
                for (int i = 0; i < g; i++) {
                    const int id = hs[i];
                    bool first = true, banned = false;
                    for (int j = 0; j < g; j++) if (hs[j] == id) { first = first && j >= i; banned = banned || ban[j]; }
                    if (!first || id < 0 || id >= N || !getbit(rep, (long)b * words, id)) continue;
                    if (banned || ((mask[id >> 5] >> (id & 31)) & 1u) || id < text_lo) continue;
                    float v1 = r.side.f((long)b * N + id);
                    v1 = v1 > 0.0f ? v1 * inv : v1 * pen;
                    if (!(v1 > -INFINITY)) continue;
                    bs = lp_merge_h(bv, bs, v1, 1.0f);
                    if (v1 > bv || (v1 == bv && id < bi)) { bv = v1; bi = id; }
                }
                float tm = -INFINITY, tsum = 0.0f; int ti = NONE_IDX;
                for (int j = 0; j < ts_ld; j++) { const float v1 = r.tsl.f((long)b * ts_ld + j); if (v1 > tm) { tsum = tsum * ts_exp_h(tm - v1) + 1.0f; tm = v1; ti = tb + j; } else if (v1 > -INFINITY) tsum += ts_exp_h(v1 - tm); }
                const float lse = tm == -INFINITY ? -INFINITY : tm + logf(tsum);
                const int wv = lse > bv ? ti : ((tm > bv || (tm == bv && ti < bi)) ? ti : bi);
                const int tok = wv == NONE_IDX ? 0 : wv;
                const float lp = wv == NONE_IDX ? -INFINITY : -logf(lse > bv ? tsum : lp_merge_h(bv, bs, tm, tsum));
                int next = tok;
                if (!o_done.i32(b)) {
                    o_out.setu((long)b * tok_ld + n_prompt + g, tok); o_nout.setu(b, n_prompt + g + 1); o_lp.setf((long)b * tok_ld + n_prompt + g, lp);
                    if (g < 1) next = forced[g]; else if (tok == eot) o_done.setu(b, 1);
                }
                if (pos + 1 < tok_ld) o_feed.setu((long)b * tok_ld + pos + 1, next);
                if (defect != D_CHAINSTATE) { int s[4]; ts_next_state_h(next, g == 0 || o_feed.i32((long)b * tok_ld + pos) >= tb, g == 0 ? -1 : st[4 * b + 3], tb, eot, N, s); for (int k = 0; k < 4; k++) o_state.setu(4 * b + k, s[k]); }
                hs[g] = next;
                std::vector<unsigned char> ban2;
                rep_bans_h(hs, g + 1, ngram, tb, ban2);
                std::vector<unsigned> wd(rep.begin() + (size_t)b * words, rep.begin() + (size_t)(b + 1) * words);
                if (next >= 0 && next < std::min(tb, N)) wd[next >> 5] |= 1u << (next & 31);
                for (int i = 0; i < g + 1; i++) if (ban2[i] && hs[i] >= 0 && hs[i] < N) wd[hs[i] >> 5] |= 1u << (hs[i] & 31);
                for (int k = 0; k < words; k++) o_bits.setu((long)b * words + k, wd[k]);
            }
            o_pos.setu(0, pos + 1);
        }
        // ---- the host's own step, from L0 and its own state ----
        const int Ls = r.L + 15, As = r.A + 25;
        const std::vector<int> p_state = e_state, p_feed = e_feed;
        for (int b = 0; b < B; b++) {
            const float* Lr = &o.L0[(size_t)b * N];
            for (int n = 0; n < N; n++) { r.logits.mark(((long)b * G + g) * N + n); exact += !same_f(r.logits.f(((long)b * G + g) * N + n), Lr[n]); }
            const int tlo = g == 0 ? tb : p_state[4 * b], slo = g == 0 ? tb : p_state[4 * b + 1], shi = g == 0 ? N - 1 : p_state[4 * b + 2];
            auto masked = [&](int n) { return ((mask[n >> 5] >> (n & 31)) & 1u) != 0; };
            auto touched = [&](int n) { return ((e_bits[(size_t)b * words + (n >> 5)] >> (n & 31)) & 1u) != 0; };
            std::vector<std::pair<float, int>> cand;
            for (int n = std::max(tlo, 0); n < tb; n++) if (!masked(n) && !touched(n) && Lr[n] > -INFINITY) cand.push_back({Lr[n], n});
            std::vector<int> hs(g + 1, 0);
            for (int i = 0; i < g; i++) hs[i] = p_feed[(size_t)b * tok_ld + n_prompt + i];
            std::vector<unsigned char> ban, ban2;
            rep_bans_h(hs, g, ngram, tb, ban);
            for (int i = 0; i < g; i++) {
                const int id = hs[i];
                bool first = true, banned = false;
                for (int j = 0; j < g; j++) if (hs[j] == id) { first = first && j >= i; banned = banned || ban[j]; }
                if (!first || id < 0 || id >= N || !touched(id) || banned || masked(id) || id < tlo) continue;
                float v1 = Lr[id];
                v1 = v1 > 0.0f ? v1 * inv : v1 * pen;
                if (v1 > -INFINITY) cand.push_back({v1, id});
            }
            float bv = -INFINITY; int bi = NONE_IDX;
            for (auto& c : cand) if (c.first > bv || (c.first == bv && c.second < bi)) { bv = c.first; bi = c.second; }
            double S = 0, eS = 1e-37;
            for (auto& c : cand) { const double dl = (double)c.first - bv, e = exp(dl); S += e; eS += e * (3 * fabs(dl) + 3 * Ls + As) * U; }
            double tm = -INFINITY, tS = 0, etS = 1e-37; int ti = NONE_IDX, cnt = 0;
            for (int n = tb; n < N; n++) if (!masked(n) && n >= slo && n <= shi && Lr[n] > tm) { tm = Lr[n]; ti = n; }
            for (int n = tb; n < N; n++) if (!masked(n) && n >= slo && n <= shi && Lr[n] > -INFINITY) { const double dl = (double)Lr[n] - tm, e = exp(dl); tS += e; etS += e * (3 * fabs(dl) + 3 * 10 + 10) * U; cnt++; }
            const double lse = cnt ? tm + log(tS) : -INFINITY;
            if (cnt > 1 && !(fabs(lse - (double)bv) > etS / tS + 4 * U * fabs(log(tS)) + 2 * U * fabs(lse))) nomargin++;
            const bool take = lse > bv;
            const int wv = take ? ti : ((tm > bv || (tm == bv && ti < bi)) ? ti : bi);
            const int tok = wv == NONE_IDX ? 0 : wv;
            int next = tok;
            if (!e_done[b]) {
                const long slot = (long)b * tok_ld + n_prompt + g;
                e_out[slot] = tok; e_nout[b] = n_prompt + g + 1;
                double lp = -INFINITY, elp = 0;
                if (wv != NONE_IDX) {
                    double Sm, eSm;
                    if (take) { Sm = tS; eSm = etS; }
                    else { const double mx = std::max((double)bv, tm), qa = bv > -INFINITY ? exp(bv - mx) : 0.0, qb = cnt ? exp(tm - mx) : 0.0; Sm = S * qa + tS * qb; eSm = (eS + 8 * U * S) * qa + (etS + 8 * U * tS) * qb; }
                    lp = -log(Sm); elp = eSm / Sm + 4 * U * fabs(lp) + 2 * U;
                }
                o_lp.mark(slot); w.see(o_lp.f(slot), lp, elp);
                if (g < 1) next = forced[g]; else if (tok == eot) e_done[b] = 1;
            }
            if (pos + 1 < tok_ld) e_feed[(size_t)b * tok_ld + pos + 1] = next;
            ts_next_state_h(next, g == 0 || p_feed[(size_t)b * tok_ld + pos] >= tb, g == 0 ? -1 : p_state[4 * b + 3], tb, eot, N, &e_state[4 * b]);
            hs[g] = next;
            rep_bans_h(hs, g + 1, ngram, tb, ban2);
            unsigned* wd = &e_bits[(size_t)b * words];
            if (next >= 0 && next < std::min(tb, N)) wd[next >> 5] |= 1u << (next & 31);
            for (int i = 0; i < g + 1; i++) if (ban2[i] && hs[i] >= 0 && hs[i] < N) wd[hs[i] >> 5] |= 1u << (hs[i] & 31);
        }
        for (size_t i = 0; i < e_state.size(); i++) exact += o_state.i32((long)i) != e_state[i];
        for (size_t i = 0; i < e_feed.size(); i++) exact += (o_feed.i32((long)i) != e_feed[i]) + (o_out.i32((long)i) != e_out[i]);
        for (size_t i = 0; i < e_bits.size(); i++) exact += o_bits.u32((long)i) != e_bits[i];
        for (int b = 0; b < B; b++) exact += (o_nout.i32(b) != e_nout[b]) + (o_done.i32(b) != e_done[b]);
        exact += (o_pos.i32(0) != pos + 1) + (o_pos.i32(1) != 0);
    }
    exact += nomargin;
    for (Buf* bf : {&r.logits, &r.pval, &r.pidx, &r.psum, &r.tsl, &r.side, &o_state, &o_feed, &o_out, &o_nout, &o_done, &o_bits, &o_pos, &o_lp}) bf->down();
    // what the LM head may have written of its own outputs over the chain (held to the contract one launch at a time in the group head)
    for (int m = 0; m < B; m++) {
        for (int p = 0; p < r.n_parts; p++) { r.pval.mark((long)p * mpad + m); r.pidx.mark((long)p * mpad + m); r.psum.mark((long)p * mpad + m); }
        for (int j = 0; j < ts_ld; j++) r.tsl.mark((long)m * ts_ld + j);
        for (int n = 0; n < tb; n++) r.side.mark((long)m * N + n);
    }
    long guard = 0;
    for (Buf* bf : {&r.logits, &r.pval, &r.pidx, &r.psum, &r.tsl, &r.side, &o_state, &o_feed, &o_out, &o_nout, &o_done, &o_bits, &o_pos, &o_lp}) guard += bf->guard();
    dev_free({dforced});
    o.release();
    const bool ok = w.ratio <= 1.0 && exact == 0 && guard == 0 && rv <= 1.0;
    if (!defect) worst_fin = std::max(worst_fin, w.ratio);
    if (!defect || !g_host)
        printf("chain k_lm_head -> k_argmax_finish %s RLP %d positions, %d rows: err/bound logprob %.3f logits %.3f exact %ld (no margin %ld) guard %ld  tokens %016llx logprob %016llx state %016llx bits %016llx  %s\n",
               mode_name[md], G, B, w.ratio, rv, exact, nomargin, guard, o_feed.hash(o_out.hash()), o_lp.hash(), o_state.hash(), o_bits.hash(), ok ? "ok" : "MISMATCH");
    return ok ? 0 : 1;
}

static FC fc(const char* what, int n_parts, int gen, bool rules, bool lp, bool rep, bool pfx) { FC c; c.what = what; c.n_parts = n_parts; c.gen = gen; c.rules = rules; c.lp = lp; c.rep = rep; c.pfx = pfx; return c; }
static int group_finish() {
    int bad = 0;
    for (int np : {1, 5, 256, 257, 2048, 2049}) for (int k = 0; k < 2; k++) bad |= finish_case(fc("ties between partials, the last partial", np, 3, k, true, false, false));
    for (Mode md : {BF16, F32, H2}) {
        for (int k = 0; k < 16; k++) { FC c = fc("every variant", 257, 6, k & 1, k & 2, k & 4, k & 8); c.mode = md; c.ngram = 3; c.pen = 1.5f; c.d = md == BF16 ? 384 : md == F32 ? 128 : 1280; bad |= finish_case(c); }
    }
    { FC c = fc("nothing allowed: token 0, -inf", 5, 3, true, true, true, false); c.nothing = true; c.pen = 1.5f; bad |= finish_case(c); c.rules = false; bad |= finish_case(c); }
    { FC c = fc("forced position, EOT does not stop", 5, 2, false, true, false, false); c.n_forced = 3; bad |= finish_case(c); c.rules = true; bad |= finish_case(c); }
    { FC c = fc("last position: no feed", 5, 3, true, true, false, true); c.last = true; bad |= finish_case(c); }
    { FC c = fc("gen 0: rule 4's text_lo, seq[-2] absent", 5, 0, true, true, true, true); c.pen = 1.5f; c.ngram = 3; bad |= finish_case(c); }
    for (int h : {0, 1, 255, 256, 257, WH_REP_MAX_HIST})
        for (int ng : {0, 1, 3}) {
            FC c = fc("history length", 5, h, (h + ng) & 1, true, true, false); c.ngram = ng; c.pen = ng == 1 ? 1.0f : 1.3f; bad |= finish_case(c);
            if (ng == 3) { c.pen = 1.0f; c.what = "bans only: the clear path"; bad |= finish_case(c); }
        }
    printf("fused next embedding bit-identical to k_dec_embed: %ld launches, %ld differing  %s\n", fin_embed_cases, fin_embed_diff, fin_embed_diff == 0 && fin_embed_cases > 0 ? "ok" : "MISMATCH");
    for (Mode md : {BF16, F32, H2}) bad |= chain_case(md, 0);
    for (int np : {1, 63, 64, 65}) for (int kind : {0, 1, 2}) bad |= nospeech_case(np, kind, 0);
    printf("worst err/bound finish: %.3f\n", worst_fin);
    return bad;
}

// ===== --selftest: host only ==================================================================================================================
static int st_bad = 0;
static void st_line(const char* fam, const char* what, int defect, bool caught, double ratio, long exact) {
    if (!defect) { printf("selftest %-6s clean: %-58s err/bound %.3f exact %ld  %s\n", fam, what, ratio, exact, caught ? "MISMATCH" : "ok"); st_bad |= caught; }
    else { printf("selftest %-6s defect: %d %s  err/bound %.3g exact %ld  %s\n", fam, defect, what, ratio, exact, caught ? "caught" : "NOT CAUGHT"); st_bad |= !caught; }
}
static void st_head(const Ops& o, Var v, const char* name) {
    const Res q = run_head(o, v);
    st_line("head", name, v.defect, !q.ok(), std::max(q.rv, q.rs), q.exact + q.guard);
}
static int selftest() {
    g_host = true;
    // the groups themselves on the emulation: every bound must hold
    const int b_head = group_head(), b_tile = group_tile(), b_fin = group_finish(), b_lang = group_lang(), b_embed = group_embed();
    st_line("head", "every case of the group", 0, b_head != 0, std::max(worst_val[0], worst_sum[0]), (long)b_head);
    st_line("tile", "every case of the group", 0, b_tile != 0, worst_sum[1], (long)b_tile);
    st_line("finish", "every case of the group", 0, b_fin != 0, worst_fin, (long)b_fin);
    st_line("lang", "every case of the group", 0, b_lang != 0, worst_lang, (long)b_lang);
    st_line("embed", "every case of the group", 0, b_embed != 0, worst_embed, (long)b_embed);
    {   // the LM head's defects, each on a case of the group's list
        Ops o; make_ops(o, BF16, 5, 1003, 128, true, Spec());
        reference(o, D_NONE, nullptr);
        { double rv; Ops p; make_ops(p, BF16, 5, 1003, 128, true, Spec()); reference(p, D_LNROW, &rv); st_line("head", "LayerNorm statistics of the neighbouring row", D_LNROW, rv > 1.0, rv, 0); p.release(); }
        Var all = var("", true, true, true, 1, 903);
        { Var v = var("", true, true, true, 0, 903); v.defect = D_MASKBASE; st_head(o, v, "gen 0 reads mask_base"); }
        { Var v = var("", false, true, false, 1, 0); v.defect = D_NOGUARD; st_head(o, v, "the nn < N guard dropped, so the clamped last weight row is counted again"); }
        { Var v = var("", false, true, false, 1, 0); v.defect = D_SUPSUM; st_head(o, v, "a suppressed id enters the sum of exp"); }
        { Var v = all; v.defect = D_STRADDLE; st_head(o, v, "a tile that straddles ts_begin treated as text-only"); }
        { Var v = var("", true, true, false, 0, 903); v.tmax = 3; v.defect = D_HIEXCL; st_head(o, v, "ts_hi taken as exclusive"); }
        {   // (k_lm_head's online pairs restart at a lane's first allowed id, and a lane's ids ascend: the tile kernels' second pass is where this shows)
            Ops p; make_ops(p, BF16, 256, 1003, 128, true, Spec());
            reference(p, D_NONE, nullptr);
            Var v = var("", true, true, false, 1, 903, 1); v.defect = D_TEXTLO; st_head(p, v, "text below text_lo in the LP sum");
            p.release();
        }
        { Var v = all; v.defect = D_TOUCHED; st_head(o, v, "a touched id left in the partials"); }
        { Var v = all; v.defect = D_SIDEPITCH; st_head(o, v, "the rep_side row pitch is 32 * rep_words instead of N"); }
        { Var v = var("", false, true, false, 1, 0); v.defect = D_NORESCALE; st_head(o, v, "lane-group sums added without rescaling to the row maximum"); }
        { Var v = all; v.lmode = 2; v.defect = D_SELSLOT0; st_head(o, v, "a logits_sel of -1 stored to slot 0"); }
        { Var v = var("", false, false, false, 1, 0); v.defect = D_PARTPITCH; st_head(o, v, "partials at pitch M instead of x_mpad"); }
        o.release();
        Ops t; Spec sp; sp.tie_a = 8; sp.tie_b = 13; make_ops(t, BF16, 5, 1003, 128, true, sp);
        reference(t, D_NONE, nullptr);
        { Var v = var("", false, true, false, 1, 0); v.defect = D_TIEHIGH; st_head(t, v, "a tie kept by the higher index"); }
        t.release();
    }
    {   // the finish kernels' defects
        auto fin = [&](FC c, int defect, const char* name) { c.defect = defect; st_line("finish", name, defect, finish_case(c) != 0, 0, 1); };
        FC all = fc("", 257, 6, true, true, true, true); all.ngram = 3; all.pen = 1.5f;
        fin(fc("", 257, 3, false, true, false, false), D_FTIELATE, "finish: a tie between partials goes to the later one");
        fin(fc("", 2049, 3, false, true, false, false), D_F2048, "finish: partials past 2048 dropped");
        fin(all, D_RULE5MAX, "rule 5 on the timestamp maximum instead of its log-sum-exp");
        fin(all, D_LPTEXT, "LP under rule 5 includes the text sum");
        fin(all, D_PENPOS, "a positive logit multiplied by p");
        { FC c = all; c.rules = false; fin(c, D_DUPTWICE, "a duplicated history id merged twice"); }
        { FC c = all; c.pen = 1.0f; fin(c, D_BANKEEP, "bans not cleared with the penalty off"); }
        fin(all, D_DONEREC, "a done row records its token");
        { FC c = fc("", 5, 2, false, true, false, false); c.n_forced = 3; fin(c, D_FORCEDEOT, "a forced EOT sets done"); }
        st_line("finish", "no-speech: a -inf partial yields NaN", D_NSNAN, nospeech_case(64, 2, D_NSNAN) != 0, 0, 1);
        fin(all, D_EMBORDER, "the fused next embedding differs from k_dec_embed in the sum order");
        st_line("finish", "chain: the finish leaves the row state of the previous position", D_CHAINSTATE, chain_case(BF16, D_CHAINSTATE) != 0, 0, 1);
    }
    lang_finish_case({"", 99, -1, true, 0});
    st_line("lang", "language: a tie goes to the lowest list position", D_LANGTIE, lang_finish_case({"", 99, -1, true, D_LANGTIE}) != 0, 0, 1);
    st_line("lang", "language: src_row ignored", D_LANGSRC, lang_finish_case({"", 99, 0, false, D_LANGSRC}) != 0, 0, 1);
    st_line("embed", "embed PFX: position pos - off not clamped at 0", D_PFXCLAMP, embed_case({"", BF16, 5, 384, false, true, true, D_PFXCLAMP}) != 0, 0, 1);
    printf("selftest worst err/bound of the emulation: head %.3f tile %.3f finish %.3f lang %.3f embed %.3f\n", std::max(worst_val[0], worst_sum[0]), worst_sum[1], worst_fin, worst_lang, worst_embed);
    printf("selftest %s\n", st_bad ? "FAILED" : "passed");
    return st_bad;
}

// ===== --time: whisper-base shapes (vocabulary 51865, d_model 512), bf16 =======================================================================
static int timing() {
    const int N = 51865, K = 512;
    void *X, *W; float *pv, *lnp, *lns, *bias; int *pi, *pos; unsigned* mask;
    CK(hipMalloc(&X, (size_t)K * 1024 * 2)); CK(hipMalloc(&W, (size_t)N * K * 2)); CK(hipMalloc((void**)&pv, (size_t)4096 * 1024 * 4)); CK(hipMalloc((void**)&pi, (size_t)4096 * 1024 * 4));
    CK(hipMalloc((void**)&lnp, (size_t)32 * 1024 * 8)); CK(hipMalloc((void**)&lns, N * 4)); CK(hipMalloc((void**)&bias, N * 4)); CK(hipMalloc((void**)&pos, 4)); CK(hipMalloc((void**)&mask, (N + 31) / 32 * 4));
    CK(hipMemset(X, 0, (size_t)K * 1024 * 2)); CK(hipMemset(W, 0, (size_t)N * K * 2)); CK(hipMemset(lnp, 0, (size_t)32 * 1024 * 8)); CK(hipMemset(lns, 0, N * 4)); CK(hipMemset(bias, 0, N * 4));
    CK(hipMemset(pos, 0, 4)); CK(hipMemset(mask, 0, (N + 31) / 32 * 4));
    for (int rows : {16, 64, 256, 1024}) {
        SkinnyArgs a;
        a.X = X; a.x_mpad = 1024; a.W = W; a.M = rows; a.N = N; a.K = K; a.ln_part = lnp; a.ln_tiles = K / 16; a.ln_s = lns; a.bias = bias; a.pos_p = pos; a.n_prompt = 4;
        a.mask_first = mask; a.mask_base = mask; a.part_val = pv; a.part_idx = pi;
        unsetenv("WH_LM_TILE_MIN_ROWS");
        for (int i = 0; i < 3; i++) wh_launch_lm_head(0, WH_PREC_BF16, a);
        CK(hipDeviceSynchronize());
        std::vector<double> us;
        for (int r = 0; r < 15; r++) {
            const auto t0 = std::chrono::steady_clock::now();
            for (int i = 0; i < 10; i++) wh_launch_lm_head(0, WH_PREC_BF16, a);
            CK(hipDeviceSynchronize());
            us.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() / 10 * 1e6);
        }
        std::sort(us.begin(), us.end());
        printf("time %s bf16 rows %4d N %d K %d: median %9.1f us  min %9.1f  max %9.1f\n", wh_lm_head_tile_applicable(a) ? "k_lm_head_tile" : "k_lm_head     ", rows, N, K, us[7], us.front(), us.back());
    }
    CK(hipGetLastError());
    dev_free({X, W, pv, pi, lnp, lns, bias, pos, mask});
    return 0;
}

int main(int argc, char** argv) {
    setvbuf(stdout, nullptr, _IOLBF, 0);
    const std::string arg = argc > 1 ? argv[1] : "";
    if (arg == "--selftest") return selftest() ? 1 : 0;
    if (arg == "--time") return timing();
    const char* groups[] = {"head", "tile", "finish", "lang", "embed"};
    bool known = arg.empty();
    for (const char* g : groups) known |= arg == g;
    if (!known) { fprintf(stderr, "usage: lm_check [head | tile | finish | lang | embed | --selftest | --time]\n"); return 2; }
    int bad = 0;
    for (const char* grp : groups) {
        if (!arg.empty() && arg != grp) continue;
        const auto t0 = std::chrono::steady_clock::now();
        bad |= !strcmp(grp, "head") ? group_head() : !strcmp(grp, "tile") ? group_tile() : !strcmp(grp, "finish") ? group_finish() : !strcmp(grp, "lang") ? group_lang() : group_embed();
        printf("group %s: %.1f s wall\n", grp, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
    }
    return bad ? 1 : 0;
}
