// wh_es_common.h — what the encoder-state cross-attention kernels share: k_dec_cross_attn_es (bf16) and k_dec_cross_attn_es2 (two fp16 limbs,
// both wh_cross_es.hip), k_dec_cross_attn_es8 (e4m3, wh_cross_es8.hip) and k_dec_cross_attn_es3 (fp16 + e4m3 remainder, wh_cross_es3.hip) differ
// in their operand side — key-row layout and swizzle, how queries and probabilities become MFMA operands, which MFMA runs, how the 8 x 8 blocks
// are transposed, the type of the output slab.  Everything around that is here once: the format description and the LDS carve, the LOADER ROLE
// (ring bookkeeping, the vmcnt and barrier schedule), the tile / clip walk of the computing waves, the score exchange's addressing, the online
// softmax of a tile, the accumulator rescale, the clip end, the query read, the final LayerNorm of the two fp16 writers and the launcher.
// Each kernel keeps its own main loop (register-tuned: es3 sits at 256 VGPRs) and calls these pieces between its operand code.
//
// Every function is force-inlined into its kernel and takes scalars (or locals of the kernel by reference, which vanish when inlined); kernel
// arguments are passed by value, as in wh_lm_tile.h.  The header is compiled inside the three translation units and so gets their -fno-honor-nans.
//
// The pipeline (stated at k_dec_cross_attn_es): waves 0-3 compute, waves 4 .. 3 + NL only load.  Iteration g of the computing waves works on
// the scores of tile g + 1 and the softmax + output of tile g behind ONE barrier, which the loaders meet too: the barriers of loader() and of a
// kernel's loop (prologue_barriers() before it, tile_barrier() at the top of every iteration) must match one for one.
#pragma once
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "wh_common.h"
#include "wh_kernels.h"

namespace wh_es {

typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int D = 512, H = 8;                          // whisper-base geometry: d_model, heads
constexpr float LOG2E = 1.44269504088896341f;
constexpr float REM = 16.0f, REM_INV = 1.0f / 16.0f;   // scale of the e4m3 remainder rows of queries and probabilities

// ---- small helpers ---------------------------------------------------------------------------------------------------------------------------
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
template <int AUX>
__device__ __forceinline__ void glds16(const void* src, char* lds_wave_base) {   // one LDS-DMA piece: 64 lanes x 16 bytes, written linearly from lds_wave_base
    __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)lds_wave_base, 16, 0, AUX);
}
// 512-byte e4m3 rows: LDS chunk (16 bytes) p of tile row r holds chunk p ^ swz8(r) — both ds_read_b64 patterns of the kernels (8 dims of a key per
// lane: keys across fl for the scores, dims across fl for the output blocks) then touch 32 distinct 8-byte units per 32-lane service group
__device__ __forceinline__ int swz8(int r) { return (r & 15) ^ (((r >> 4) & 1) << 3); }
__device__ __forceinline__ float ror8(float v) {    // v of lane ^ 8 (same 16-lane row): DPP row_ror:8
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, true));
}
__device__ __forceinline__ unsigned ror8u(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true); }
__device__ __forceinline__ float sum32(float v) {   // v(lane) + v(lane ^ 32), in every lane
    const wh_u32x2 t = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
    return __uint_as_float(t.x) + __uint_as_float(t.y);
}
// four f32 -> four e4m3 bytes (byte u = v[u])
__device__ __forceinline__ unsigned pack4(float a, float b, float c, float d) {
    int p = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    return (unsigned)__builtin_amdgcn_cvt_pk_fp8_f32(c, d, p, true);
}
// the remainder limb of four values whose head limb is `hi`: e4m3(16 (v - hi))
__device__ __forceinline__ unsigned rem4(unsigned hi, float a, float b, float c, float d) {
    const float h0 = __builtin_amdgcn_cvt_f32_fp8((int)hi, 0), h1 = __builtin_amdgcn_cvt_f32_fp8((int)hi, 1);
    const float h2_ = __builtin_amdgcn_cvt_f32_fp8((int)hi, 2), h3 = __builtin_amdgcn_cvt_f32_fp8((int)hi, 3);
    return pack4((a - h0) * REM, (b - h1) * REM, (c - h2_) * REM, (d - h3) * REM);
}
__device__ __forceinline__ long join(unsigned lo, unsigned hi) { return (long)(((unsigned long long)hi << 32) | lo); }
// head 4 (fg & 1) + i's value of v, i = 0 .. 3, where head q's value sits in lane q: through SGPRs (v_readlane)
// (the selects are written out: with a loop index the two reads of vh become one read at a selected address, and vh goes to scratch)
__device__ __forceinline__ void head4(float v, int fg, float (&o)[4]) {
    float vh[8];
#pragma unroll
    for (int q = 0; q < 8; q++) vh[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), q));
    const bool up = fg & 1;
    o[0] = up ? vh[4] : vh[0];
    o[1] = up ? vh[5] : vh[1];
    o[2] = up ? vh[6] : vh[2];
    o[3] = up ? vh[7] : vh[3];
}

// ---- a kernel's format: its tiles, its ring, its LDS -------------------------------------------------------------------------------------------
struct Format {
    int tk;        // key rows per tile
    int tileb;     // bytes per tile (a ring slot)
    int nstage;    // ring depth: nstage - 1 tiles are staged ahead of the one being consumed
    bool qs;       // the next clip's expanded queries are prefetched into LDS ([8][512] f32 behind the score exchange)
    int scp;       // floats per (partial, head) row of the score exchange (the tile's keys + pad)
    constexpr int pieces() const { return tileb / 1024; }   // LDS-DMA pieces per tile
    constexpr int scb() const { return 4 * H * scp; }       // floats per score-exchange buffer: [4 partials][head][scp]
    constexpr int lds() const { return nstage * tileb + 2 * scb() * 4 + (qs ? H * D * 4 : 0); }   // ring + two exchange buffers + next queries
};
struct Lds {
    float* sc;   // [2 tiles][scb]
    float* Qs;   // [8][512] f32 (formats with qs)
};
template <const Format& F>
__device__ __forceinline__ Lds carve(char* smem) {
    Lds l;
    l.sc = reinterpret_cast<float*>(smem + F.nstage * F.tileb);
    l.Qs = l.sc + 2 * F.scb();
    return l;
}

// ---- the walk of a workgroup over its tiles: clips blockIdx.x, + gridDim.x, ... as ONE tile sequence ---------------------------------------------
template <const Format& F>
struct Walk {
    int ntile, G, total;    // tiles per clip, workgroups, tiles of this workgroup
    int g, clip, t, slot;   // the tile being consumed: number g of the walk = tile t of `clip`, in ring slot `slot`
    __device__ __forceinline__ Walk(int S, int B) {
        ntile = (S + F.tk - 1) / F.tk;
        G = gridDim.x;
        total = ((B - (int)blockIdx.x + G - 1) / G) * ntile;
        g = 0; clip = blockIdx.x; t = 0; slot = 0;
    }
    __device__ __forceinline__ bool done() const { return g >= total; }
    __device__ __forceinline__ bool more() const { return g + 1 < total; }
    __device__ __forceinline__ int nslot() const { return slot + 1 == F.nstage ? 0 : slot + 1; }
    __device__ __forceinline__ bool last_tile() const { return t == ntile - 1; }   // of the clip (wave-uniform)
    // tile g + 1 is the next clip's first: it is scored with the next clip's queries, which the caller reads now
    __device__ __forceinline__ bool next_queries() const { return last_tile() && more(); }
    // a kernel's loop: for (; !w.done(); w.next()) { ...; if (!w.advance()) continue; <the clip ended: store>; w.next_clip(); }
    __device__ __forceinline__ void next() { g++; }
    __device__ __forceinline__ bool advance() { slot = nslot(); return ++t == ntile; }
    __device__ __forceinline__ void next_clip() { t = 0; clip += G; }
};

// ---- the loader role -------------------------------------------------------------------------------------------------------------------------------
// Runs a loader wave's whole schedule.  issue(slot_base, clip, t) puts this wave's share (pieces() / NL) of tile t of `clip` into the ring slot
// at slot_base with glds16 — the addressing is the format's own.  Tiles are staged strictly in sequence, nstage - 1 ahead; formats with qs also
// get each clip's 16 KiB of queries into Qs a clip ahead.  vmcnt retires in issue order (and holds at most 63), so "all but the youngest n
// pieces" is a statement about whole tiles: the prologue waits for the queries and tile 0, iteration g for tile g + 1 (conservative where the
// next clip's queries are among the younger loads: the count then also covers a few pieces of tile g + 2).
// stamp(0 .. 3) is called at the top of an iteration, behind its wait, behind its barrier and at its end (tools/es_bench.hip's phase stamps).
struct NoStamp { __device__ __forceinline__ void operator()(int) const {} };
template <const Format& F, int NL, typename Issue, typename Stamp = NoStamp>
__device__ __forceinline__ void loader(char* smem, const float* qe, int lw, int lane, int B, Walk<F> w, Issue issue, Stamp stamp = Stamp()) {
    constexpr int LA = F.nstage - 1;
    constexpr int PPT = F.pieces() / NL;   // pieces per loader wave and tile
    constexpr int QPP = 16 / NL;           // pieces of a clip's queries per loader wave
    static_assert(LA >= 2 && F.pieces() % NL == 0, "iteration g needs tile g + 1: at least two tiles ahead");
    const int ntile = w.ntile, total = w.total, G = w.G;
    int st_clip = blockIdx.x, st_t = 0, st_slot = 0;
    auto stage_next = [&]() __attribute__((always_inline)) {
        issue(smem + st_slot * F.tileb, st_clip, st_t);
        st_slot = st_slot + 1 == F.nstage ? 0 : st_slot + 1;
        if (++st_t == ntile) { st_t = 0; st_clip += G; }
    };
    auto stage_q = [&](int clip) __attribute__((always_inline)) {
        const float* src = qe + (long)clip * (H * D);
        char* Qs = reinterpret_cast<char*>(carve<F>(smem).Qs);
#pragma unroll
        for (int j = 0; j < QPP; j++) glds16<0>(src + ((lw * QPP + j) * 64 + lane) * 4, Qs + (lw * QPP + j) * 1024);
    };
    if constexpr (F.qs) stage_q(blockIdx.x);
#pragma unroll
    for (int t = 0; t < LA; t++)
        if (t < total) stage_next();
    if (total >= LA) wait_vm<(PPT * (LA - 1) < 63 ? PPT * (LA - 1) : 63)>(); else wait_vm<0>();
    if constexpr (F.qs) __builtin_amdgcn_s_barrier();   // P1: the first clip's queries are in Qs
    __builtin_amdgcn_s_barrier();                       // P2: tile 0 is in the ring
    int clip = blockIdx.x, t = 0;
    for (int g = 0; g < total; g++) {
        stamp(0);
        if (g + 1 < total) {   // tile g + 1 has landed; the younger tiles stay in flight
            if (total - 2 - g >= LA - 2) wait_vm<PPT * (LA - 2)>(); else wait_vm<0>();
        }
        stamp(1);
        __builtin_amdgcn_s_barrier();
        stamp(2);
        if (g + LA < total) stage_next();
        if constexpr (F.qs) {
            if (t == 0 && clip + G < B) stage_q(clip + G);   // Qs was read (if at all) before this barrier
            if (++t == ntile) { t = 0; clip += G; }
        }
        stamp(3);
    }
}

// ---- the computing waves' side of the barriers ------------------------------------------------------------------------------------------------------
// prologue_barriers(read_q): P1, read_q() (the first clip's queries, from Qs where the format has it), P2
template <const Format& F, typename ReadQ>
__device__ __forceinline__ void prologue_barriers(ReadQ read_q) {
    if constexpr (F.qs) __builtin_amdgcn_s_barrier();
    read_q();
    __builtin_amdgcn_s_barrier();
}
// top of iteration g: tile g + 1 and the scores of tile g visible to all; every wave is done with tile g - 1
__device__ __forceinline__ void tile_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
}

// ---- the query read ------------------------------------------------------------------------------------------------------------------------------
// A computing wave's slice of a clip's expanded queries q [8][512] f32 (Qs, or global memory) as MFMA row operands: lane -> row fl = head fl & 7
// (rows 0-7 carry head limbs, rows 8-15 remainders: the caller's pack(s, v) chooses by fl >= 8), dims 256 hf + 32 s + 8 fg .. + 7 for contraction
// step s, in log2 units (p = exp2(s - m)).  Four steps' reads are in flight at a time; FENCE keeps them so (left alone, the compiler keeps two).
template <bool FENCE, typename Pack>
__device__ __forceinline__ void read_queries(const float* q, int fl, int fg, int hf, Pack pack) {
    const float* qp = q + (fl & 7) * D + 256 * hf + 8 * fg;
#pragma unroll
    for (int s0 = 0; s0 < 8; s0 += 4) {
        f32x4 r[4][2];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            r[s][0] = *reinterpret_cast<const f32x4*>(qp + 32 * (s0 + s));
            r[s][1] = *reinterpret_cast<const f32x4*>(qp + 32 * (s0 + s) + 4);
        }
        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) v[u] = r[s][u >> 2][u & 3] * LOG2E;
            pack(s0 + s, v);
        }
        if constexpr (FENCE) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- the score exchange: per tile [4 partials][8 heads][scp] f32, two buffers (tile parity) ------------------------------------------------------------
// writer: the address of partial `part`, head 4 (fg & 1), key `key`; rows i = 0 .. 3 (heads 4 (fg & 1) + i) are F.scp floats apart
template <const Format& F>
__device__ __forceinline__ float* exch_dst(float* sc, int buf, int part, int fg, int key) {
    return sc + buf * F.scb() + (part * H + 4 * (fg & 1)) * F.scp + key;
}
// reader: the four partials of keys kq .. kq + 3 of head h
struct Partials { f32x4 p[4]; };
template <const Format& F>
__device__ __forceinline__ Partials exch_read(const float* sc, int buf, int h, int kq) {
    const float* s0 = sc + buf * F.scb() + h * F.scp + kq;
    Partials r;
#pragma unroll
    for (int i = 0; i < 4; i++) r.p[i] = *reinterpret_cast<const f32x4*>(s0 + i * H * F.scp);
    return r;
}

// ---- the online softmax of a tile ------------------------------------------------------------------------------------------------------------------
// lane -> head fl & 7, keys key0 .. key0 + 3 of the clip (lanes fl and fl ^ 8 share a head and a lane group's eight keys; the four lane groups
// together hold the tile).  sv: the four scores; S masks the keys past the clip's end (last_tile: wave-uniform).  Updates the running maximum,
// returns the probabilities exp2(sv - m) (masked key: exp2(-inf) = 0), their sum and the factor of what was accumulated so far (first tile: 0).
struct Soft { float pv[4]; float ps, alpha; };
__device__ __forceinline__ Soft softmax_tile(float (&sv)[4], int key0, int S, bool last_tile, float& m_run) {
    float tmax = -INFINITY;
    if (last_tile) {
#pragma unroll
        for (int u = 0; u < 4; u++) sv[u] = (key0 + u < S) ? sv[u] : -INFINITY;
    }
#pragma unroll
    for (int u = 0; u < 4; u++) tmax = fmaxf(tmax, sv[u]);
    tmax = fmaxf(tmax, ror8(tmax));   // the head's other four keys of this lane group
    tmax = xrow_max(tmax);            // over the four lane groups: all keys of the tile
    const float m_new = fmaxf(m_run, tmax);
    Soft r;
    r.alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    r.ps = 0.0f;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        r.pv[u] = __builtin_amdgcn_exp2f(sv[u] - m_new);
        r.ps += r.pv[u];
    }
    m_run = m_new;
    return r;
}
// What was accumulated so far takes the tile's factor, behind the kernel's operand code (the running sum's update then fills MFMA gaps instead of
// standing in front of them): the running sum, which also takes the tile's own, and the accumulators — one or more sets (es3: one per plane) of
// rows 4 fg + i = heads 4 (fg & 1) + i, head h's factor sitting in lane h; only when some running maximum moved (wave-uniform).
template <typename... Acc>
__device__ __forceinline__ void rescale(Soft sm, int fg, float& l_run, Acc&... acc) {
    l_run = l_run * sm.alpha + sm.ps;
    if (__builtin_amdgcn_ballot_w64(sm.alpha != 1.0f) != 0) {
        float a4[4];
        head4(sm.alpha, fg, a4);
#pragma unroll
        for (int e = 0; e < 8; e++) {
#pragma unroll
            for (int i = 0; i < 4; i++) ((acc[e][i] *= a4[i]), ...);
        }
    }
}
template <typename... Acc>
__device__ __forceinline__ void clear(Acc&... acc) {
#pragma unroll
    for (int e = 0; e < 8; e++) ((acc[e] = f32x4{0, 0, 0, 0}), ...);
}

// ---- the clip end -----------------------------------------------------------------------------------------------------------------------------------
// 1 / (sum of the head's probabilities) for rows i = 0 .. 3 of this lane's accumulators.  DUP (es2): lane groups fg and fg ^ 1 hold the same eight
// keys, every key is counted twice, exactly.
template <bool DUP = false>
__device__ __forceinline__ void clip_inv4(float l_run, int fg, float (&inv4)[4]) {
    const float lh = l_run + ror8(l_run);   // the head's two key quartets of this lane group
    const float inv = 1.0f / (DUP ? xrow_sum(lh) * 0.5f : xrow_sum(lh));
    head4(inv, fg, inv4);
}
// where row i of lane group fg (< 2) stores its eight dims 128 wave + 8 fl .. + 7 of head 4 fg + i: the decode GEMM's operand slab
// [8 * 512 / 32][mpad][32], column h * 512 + dim
template <typename T>
__device__ __forceinline__ T* slab_dst(T* out, int fg, int i, int wave, int fl, int mpad, int clip) {
    const int k = (4 * fg + i) * D + 128 * wave + 8 * fl;
    return out + ((long)(k >> 5) * mpad + clip) * 32 + (k & 31);
}

// ---- the final LayerNorm of the fp16 state writers (k_layernorm_es2, k_layernorm_es3) -----------------------------------------------------------------
// One wave per row of d_model 512, 8 columns per lane: store(output row, first column, the 8 values).  [3P] torch LayerNorm eps 1e-5, biased
// variance, two-pass in f32 — k_layernorm's arithmetic (wh_gemm.hip).  in_blk > 0: input rows in blocks of in_blk go to blocks of out_blk.
template <typename Store>
__device__ __forceinline__ void layernorm_row(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, long rows, int in_blk, int out_blk, Store store) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63, c = lane * 8;
    const float* xr = x + row * D;
    const f32x4 v0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xr + c)), v1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(xr + c + 4));
    const float mean = dpp_wave_sum((v0[0] + v0[1] + v0[2] + v0[3]) + (v1[0] + v1[1] + v1[2] + v1[3])) / (float)D;
    float q = 0.0f;
#pragma unroll
    for (int e = 0; e < 4; e++) { const float t0 = v0[e] - mean, t1 = v1[e] - mean; q += t0 * t0; q += t1 * t1; }
    const float rstd = rsqrtf(dpp_wave_sum(q) / (float)D + 1e-5f);
    const f32x4 w0 = *reinterpret_cast<const f32x4*>(w + c), w1 = *reinterpret_cast<const f32x4*>(w + c + 4);
    const f32x4 b0 = *reinterpret_cast<const f32x4*>(b + c), b1 = *reinterpret_cast<const f32x4*>(b + c + 4);
    f32x8 o;
#pragma unroll
    for (int e = 0; e < 4; e++) { o[e] = (v0[e] - mean) * rstd * w0[e] + b0[e]; o[4 + e] = (v1[e] - mean) * rstd * w1[e] + b1[e]; }
    store(in_blk > 0 ? (row / in_blk) * out_blk + row % in_blk : row, c, o);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------------------------
// an A/B switch of the launchers, for a function-local static: read once per process
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
// one persistent workgroup per CU walks its clips (n_cus <= 0: the context did not say — a whole MI355X)
inline int persistent_grid(int B, int n_cus) { return std::min(B, n_cus <= 0 ? 256 : n_cus); }
// pick(AUX, NL) returns the kernel's instantiation for two std::integral_constant<int>: AUX = the LDS-DMA cache policy of the state stream
// (2: nontemporal), NL = loader waves per workgroup (1 or 2)
template <typename Pick, typename... Args>
void launch(hipStream_t s, int grid, bool two_loaders, bool stream_nt, int lds, Pick pick, Args... args) {
    wh_with_flags([&](auto NT, auto TWO) {
        constexpr int AUX = decltype(NT)::value ? 2 : 0, NL = decltype(TWO)::value ? 2 : 1;
        void (*kfn)(Args...) = pick(std::integral_constant<int, AUX>{}, std::integral_constant<int, NL>{});
        wh_ensure_dyn_lds((const void*)kfn, lds);
        hipLaunchKernelGGL(kfn, dim3(grid), dim3(256 + 64 * NL), lds, s, args...);
    }, stream_nt, two_loaders);
}

}  // namespace wh_es
