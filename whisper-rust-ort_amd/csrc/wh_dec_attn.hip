// wh_dec_attn.hip — the decoder's attention for gfx950, one position per launch: self-attention over the KV cache and
// cross-attention over the encoder states.  How a decode step is launched, and why every kernel reads the position from device
// memory: the header of wh_dec_gemm.hip.
#include <stdlib.h>

#include "wh_common.h"
#include "wh_dec_epilogue.h"
#include "wh_kernels.h"

// tuning knob (tools/microbench.cpp flips it; product code leaves the default)
int wh_dbg_cross_unroll = 4;

namespace {

// ---- decoder self-attention, one position ([3P] :417-425, 468-475): one wave per (head, clip) ---
// qkv: [B][3d] (q pre-scaled | k | v) of the current position.
// K cache [B][H][TC][64]  (lane j scores key j: its row is 8 x 16-byte loads, issued before anything else)
// V cache [B][H][TC][64]  (lane e reads column e of every cached row: one 128-byte line per wave load)
// The new k / v are appended (present.{i}.decoder.{key,value}) and used straight from registers.
// PFX (per-clip prefixes): row b's history starts at cache row off[b] of its (clip, head) plane, not at row 0.  With
// adv = min(off[b], g) at the global position g = *pos_p the kernel advances both plane pointers by adv rows and runs on the local
// position g - adv — so which lane scores which key, the prefetch groups and every summation order are
// those of an un-prefixed row at that model position (bit-identical results).  An idle row (g < off[b]) has adv = g: local position 0,
// it attends to its current key only and appends its k / v at cache row g < off[b], which no later position of the row reads.
// Invariants, for any row and any off[b] (clamped to >= 0 here; the host guarantees off[b] <= Nmax and g < tc):
//   * 0 <= adv <= g, so the row appended is cache row adv + (g - adv) = g < tc of the row's own plane — nothing outside it is written;
//   * every cached row read is adv + r with r < g - adv, a live row below g: the V loads of masked lanes are clamped to the
//     last live row, local row g - adv - 1, and at local position 0 no cache row is loaded at all — nothing outside the plane is read, nor
//     the row this launch appends;
//   * sc[] is indexed by local positions < tc <= 512.
template <typename T, typename TO = T, bool PFX = false>   // TO: the attention output as the out-projection's operand (slab layout)
__global__ __launch_bounds__(64) void k_dec_self_attn(const T* __restrict__ qkv, T* __restrict__ kc,
                                                      T* __restrict__ vc, TO* __restrict__ out,
                                                      const int* __restrict__ pos_p, int d, int n_heads, int tc_plane,
                                                      int mpad, const int* __restrict__ off) {
    constexpr int HD = WH_HEAD_DIM;
    typedef typename FragT<T>::type frag_t;
    __shared__ __attribute__((aligned(16))) float qs[HD];
    __shared__ __attribute__((aligned(16))) float sc[512];
    const int h = blockIdx.x, b = blockIdx.y, lane = threadIdx.x, gpos = *pos_p;
    int adv = 0;   // cache rows of the plane below the row's first key
    if constexpr (PFX) adv = min(max(off[b], 0), gpos);
    const int pos = gpos - adv;   // local position
    const T* row = qkv + (long)b * 3 * d;
    T* kcb = kc + (((long)b * n_heads + h) * tc_plane + adv) * HD;
    T* vcb = vc + (((long)b * n_heads + h) * tc_plane + adv) * HD;
    // 1. the cached K rows of this lane's first two keys go in flight before anything else
    frag_t kr[2][HD / 8];
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int j = lane + 64 * i;
        if (j < pos) {
#pragma unroll
            for (int e = 0; e < HD / 8; e++) kr[i][e] = load_frag<T>(kcb + (long)j * HD + e * 8);
        }
    }
    // ... and so do the first NPRE * RPI cached V rows, 16 bytes per lane: lane = (row slot, 16-byte chunk of the row), one
    // wave instruction covers RPI whole rows (8 for bf16, 4 for f32) instead of one row as 64 two-byte loads
    constexpr int EPC = 16 / (int)sizeof(T), CPR = HD / EPC, RPI = 64 / CPR, NPRE = 8;
    typedef __attribute__((ext_vector_type(EPC))) T vrow_t;
    const int rslot = lane / CPR, chunk = lane % CPR;
    vrow_t vpre[NPRE] = {};
    if (pos > 0) {   // (wave-uniform) live rows only: a slot whose row is >= pos re-reads the last live row, pos - 1, and is masked below
#pragma unroll
        for (int u = 0; u < NPRE; u++)
            vpre[u] = *reinterpret_cast<const vrow_t*>(vcb + (long)min(u * RPI + rslot, pos - 1) * HD + chunk * EPC);
    }
    const vrow_t vcur_v = *reinterpret_cast<const vrow_t*>(row + 2 * d + h * HD + chunk * EPC);
    const T kcur = row[d + h * HD + lane], vcur = row[2 * d + h * HD + lane];
    qs[lane] = cvt_in<T>(row[h * HD + lane]);
    kcb[(long)pos * HD + lane] = kcur;
    vcb[(long)pos * HD + lane] = vcur;
    __syncthreads();
    // 2. scores of the past: lane owns keys lane, lane+64, ... (the first two already loaded)
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const int j = lane + 64 * i;
        if (j < pos) {
            float s = 0.0f;
#pragma unroll
            for (int e = 0; e < HD / 8; e++)
#pragma unroll
                for (int u = 0; u < 8; u++) s += qs[e * 8 + u] * (float)kr[i][e][u];
            sc[j] = s;
            mx = fmaxf(mx, s);
        }
    }
    for (int j = lane + 128; j < pos; j += 64) {
        float s = 0.0f;
#pragma unroll
        for (int e = 0; e < HD / 8; e++) {
            const frag_t kk = load_frag<T>(kcb + (long)j * HD + e * 8);
#pragma unroll
            for (int u = 0; u < 8; u++) s += qs[e * 8 + u] * (float)kk[u];
        }
        sc[j] = s;
        mx = fmaxf(mx, s);
    }
    const float scur = dpp_wave_sum(qs[lane] * cvt_in<T>(kcur));
    mx = fmaxf(dpp_wave_max(mx), scur);
    float sum = 0.0f;
    for (int j = lane; j < pos; j += 64) {
        const float p = __expf(sc[j] - mx);
        sc[j] = p;
        sum += p;
    }
    const float pcur = __expf(scur - mx);
    sum = dpp_wave_sum(sum) + pcur;
    __syncthreads();
    // 3. P·V: lane accumulates its chunk's EPC columns over the rows of its slot; the RPI slots are summed at the end
    float o[EPC];
#pragma unroll
    for (int e = 0; e < EPC; e++) o[e] = (rslot == 0) ? pcur * cvt_in<T>(vcur_v[e]) : 0.0f;
#pragma unroll
    for (int u = 0; u < NPRE; u++) {
        const int r = u * RPI + rslot;
        const float pr = (r < pos) ? sc[min(r, 511)] : 0.0f;  // select: a row beyond pos contributes exactly 0
#pragma unroll
        for (int e = 0; e < EPC; e++) o[e] += (r < pos) ? pr * cvt_in<T>(vpre[u][e]) : 0.0f;
    }
    for (int j = NPRE * RPI; j < pos; j += NPRE * RPI) {  // later rows: NPRE wide loads in flight, clamped to the last live row and masked
        vrow_t v[NPRE];
#pragma unroll
        for (int u = 0; u < NPRE; u++)
            v[u] = *reinterpret_cast<const vrow_t*>(vcb + (long)min(j + u * RPI + rslot, pos - 1) * HD + chunk * EPC);
#pragma unroll
        for (int u = 0; u < NPRE; u++) {
            const int r = j + u * RPI + rslot;
            const float pr = (r < pos) ? sc[min(r, 511)] : 0.0f;
#pragma unroll
            for (int e = 0; e < EPC; e++) o[e] += (r < pos) ? pr * cvt_in<T>(v[u][e]) : 0.0f;
        }
    }
    // sum over the row slots (lanes with equal chunk): lane ^ 8 inside a 16-lane row by DPP (bf16 only: 8 chunks per
    // row), then across the four rows of the wave
#pragma unroll
    for (int e = 0; e < EPC; e++) {
        float t = o[e];
        if (CPR == 8) t += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, t), 0x128, 0xF, 0xF, true));  // row_ror:8
        o[e] = xrow_sum(t);
    }
    if (rslot == 0) {
        const float inv = 1.0f / sum;
        if constexpr (EPC == 4) {   // f32 caches: 4 columns per lane, in the operand type of the consumer
            store4(out + slab_idx(b, h * HD + chunk * EPC, mpad), o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
        } else {
            vrow_t ov;
#pragma unroll
            for (int e = 0; e < EPC; e++) ov[e] = cvt_out<T>(o[e] * inv);
            *reinterpret_cast<vrow_t*>(out + slab_idx(b, h * HD + chunk * EPC, mpad)) = ov;
        }
    }
}

// ---- decoder cross-attention, one position ([3P] :433-440, 478-491) -----------------------------
// The HBM-bound kernel of batched decode: per clip and layer it streams S*d K and S*d V elements
// (18.4 MB per clip per step for whisper-base in bf16) and nothing else of note.
// One workgroup = one clip x one contiguous key range, ALL heads: every key row of K (and V) is one
// contiguous d-element line read once with 16-byte lane accesses; a wave walks its keys UNROLL at a
// time with the K and V rows of all of them in flight (single pass, online softmax in registers).
// The last workgroup of a clip to finish merges the key-range partials (agent-scope release /
// acquire around an arrival ticket) and writes the attention output.
//   ck/cv: [B][S][d]  (head h at columns h*64..h*64+63),   q: [B][d] pre-scaled
//   part : [B][splits][d] unnormalised partial outputs, ml: [B][splits][H][2] (max, sum)
template <typename T, int NCH, int UNROLL, bool NT, typename TO = T>  // NCH = ceil(d*sizeof(T)/16 / 64): 16-B chunks per lane per row; NT: non-temporal K/V loads; TO: type of the slab output
__global__ __launch_bounds__(256) void k_dec_cross_attn(const T* __restrict__ q, const T* __restrict__ ck,
                                                        const T* __restrict__ cv, float* __restrict__ part,
                                                        float* __restrict__ ml, int S, int d, int n_heads,
                                                        int splits, TO* __restrict__ out, int mpad, int rows_per_clip) {
    constexpr int EPC = 16 / (int)sizeof(T);   // elements per 16-B chunk: 8 (bf16) / 4 (f32)
    constexpr int LPH = WH_HEAD_DIM / EPC;     // lanes per head: 8 / 16
    extern __shared__ __attribute__((aligned(16))) float smem[];
    typedef __attribute__((ext_vector_type(EPC))) T vec_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sp = blockIdx.x, b = blockIdx.y;
    const int per = (S + splits - 1) / splits;
    const int ks = sp * per, ke = min(S, ks + per);
    // Key groups of UNROLL consecutive keys are dealt round-robin to the four waves, so at any moment
    // the workgroup reads 4*UNROLL adjacent key rows (one 16 KiB run of K and one of V for bf16 base).
    const int j1 = ke;
    const int chunks = d / EPC;                // 16-B chunks per row

    constexpr bool PACKED = sizeof(T) == 2;  // bf16: packed-pair arithmetic (v_dot2c_f32_bf16, v_perm_b32)
    float qv[NCH][EPC], o[NCH][EPC], mrun[NCH], lrun[NCH];
    wh_u32x4 qd[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int ch = lane + 64 * c;
        mrun[c] = -INFINITY;
        lrun[c] = 0.0f;
        qd[c] = wh_u32x4{0, 0, 0, 0};
        if (PACKED && ch < chunks) qd[c] = *reinterpret_cast<const wh_u32x4*>(q + (long)b * d + ch * EPC);
#pragma unroll
        for (int u = 0; u < EPC; u++) {
            qv[c][u] = (!PACKED && ch < chunks) ? cvt_in<T>(q[(long)b * d + ch * EPC + u]) : 0.0f;
            o[c][u] = 0.0f;
        }
    }
    int kvb = b;   // the clip whose K / V this row reads: the row itself, or (beam search) clip b / rows_per_clip
    if (rows_per_clip != 1) kvb = b / rows_per_clip;
    const T* kb = ck + (long)kvb * S * d;
    const T* vb = cv + (long)kvb * S * d;
    // Software pipeline, two register sets: the K and V rows of the next UNROLL keys are in flight
    // while the current UNROLL keys go through dot / online softmax / P·V.
    vec_t kA[UNROLL][NCH], vA[UNROLL][NCH], kB[UNROLL][NCH], vB[UNROLL][NCH];
    auto load_set = [&](vec_t (&kk)[UNROLL][NCH], vec_t (&vv)[UNROLL][NCH], int j) {
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int jj = min(j + u, j1 - 1);  // tail: re-read the last key, masked in compute_set
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int ch = lane + 64 * c;
                if (ch < chunks) {
                    // read-once stream: non-temporal, so that the K/V bytes of a launch (hundreds of MB) do not evict the
                    // decode weights and activations from L2 / the Infinity Cache between the surrounding small GEMMs
                    // (only when the whole cross K/V set is larger than the Infinity Cache: a small batch re-reads it from there)
                    if constexpr (NT) {
                        kk[u][c] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(kb + (long)jj * d + ch * EPC));
                        vv[u][c] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(vb + (long)jj * d + ch * EPC));
                    } else {
                        kk[u][c] = *reinterpret_cast<const vec_t*>(kb + (long)jj * d + ch * EPC);
                        vv[u][c] = *reinterpret_cast<const vec_t*>(vb + (long)jj * d + ch * EPC);
                    }
                }
            }
        }
    };
    auto compute_set = [&](const vec_t (&kk)[UNROLL][NCH], const vec_t (&vv)[UNROLL][NCH], int j) {
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const int ch = lane + 64 * c;
            float s[UNROLL];
            float mx = mrun[c];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) {
                float t = 0.0f;
                if (ch < chunks) {
                    if constexpr (PACKED) {  // 4 x v_dot2c_f32_bf16 on the packed pairs, no conversions
                        t = dot8_bf16(as_u32x4(kk[u][c]), qd[c], t);
                    } else {
#pragma unroll
                        for (int e = 0; e < EPC; e++) t += qv[c][e] * (float)kk[u][c][e];
                    }
                }
                t = dpp_group_sum<LPH>(t);  // every lane of the head's lane group gets the full dot product
                s[u] = (j + u < j1) ? t : -INFINITY;
                mx = fmaxf(mx, s[u]);
            }
            const float scale = __expf(mrun[c] - mx);  // first chunk: exp(-inf) = 0
            float ls = lrun[c] * scale;
#pragma unroll
            for (int e = 0; e < EPC; e++) o[c][e] *= scale;
            if constexpr (PACKED && (UNROLL % 2 == 0)) {
                // P·V two keys at a time: pair the same element of both keys with v_perm_b32, then one
                // v_dot2c_f32_bf16 against the packed (p_u, p_u+1) per output element
#pragma unroll
                for (int u = 0; u < UNROLL; u += 2) {
                    const float p0 = __expf(s[u] - mx), p1 = __expf(s[u + 1] - mx);
                    ls += p0 + p1;
                    const bf16x2 pp = bf16x2{(bf16)p0, (bf16)p1};
                    if (ch < chunks) {
                        const wh_u32x4 va = as_u32x4(vv[u][c]), vb = as_u32x4(vv[u + 1][c]);
                        pv2_bf16(va.x, vb.x, pp, o[c][0], o[c][1]);
                        pv2_bf16(va.y, vb.y, pp, o[c][2], o[c][3]);
                        pv2_bf16(va.z, vb.z, pp, o[c][4], o[c][5]);
                        pv2_bf16(va.w, vb.w, pp, o[c][6], o[c][7]);
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < UNROLL; u++) {
                    const float p = __expf(s[u] - mx);
                    ls += p;
                    if (ch < chunks) {
#pragma unroll
                        for (int e = 0; e < EPC; e++) o[c][e] += p * (float)vv[u][c][e];
                    }
                }
            }
            mrun[c] = mx;
            lrun[c] = ls;
        }
    };
    constexpr int GS = 4 * UNROLL;             // stride between this wave's consecutive key groups
    const int j0 = ks + wave * UNROLL;
    if (j0 < j1) load_set(kA, vA, j0);
    for (int j = j0; j < j1; j += 2 * GS) {
        const bool hasB = j + GS < j1;
        if (hasB) load_set(kB, vB, j + GS);
        compute_set(kA, vA, j);
        if (hasB) {
            if (j + 2 * GS < j1) load_set(kA, vA, j + 2 * GS);
            compute_set(kB, vB, j + GS);
        }
    }
    // merge the four waves of this key range (LDS): wm/wl [4][H], wo [4][d]
    float* wm = smem;
    float* wl = wm + 4 * n_heads;
    float* wo = wl + 4 * n_heads;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int ch = lane + 64 * c;
        if (ch < chunks) {
            if ((lane % LPH) == 0) {
                wm[wave * n_heads + ch / LPH] = mrun[c];
                wl[wave * n_heads + ch / LPH] = lrun[c];
            }
#pragma unroll
            for (int e = 0; e < EPC; e++) wo[wave * d + ch * EPC + e] = o[c][e];
        }
    }
    __syncthreads();
    // this key range's partial (unnormalised output, running max, running sum); the consumer GEMM merges
    // the ranges of a clip while it builds its MFMA operand (frag_from_partials), so nothing is exchanged
    // between workgroups here and the kernel ends with its last store
    float* pp = part + ((long)b * splits + sp) * d;
    float* mp = ml + ((long)b * splits + sp) * n_heads * 2;
    for (int n = tid; n < d; n += 256) {
        const int h = n / WH_HEAD_DIM;
        const float M = fmaxf(fmaxf(wm[h], wm[n_heads + h]), fmaxf(wm[2 * n_heads + h], wm[3 * n_heads + h]));
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const float mw = wm[w * n_heads + h];
            const float sc = (mw == -INFINITY) ? 0.0f : __expf(mw - M);  // a wave may own no keys
            num += sc * wo[w * d + n];
            den += sc * wl[w * n_heads + h];
        }
        if (out) {  // one key range per clip: this IS the attention output (slab layout, compute dtype)
            store1(out + slab_idx(b, n, mpad), num / den);
            continue;
        }
        pp[n] = num;
        if ((n % WH_HEAD_DIM) == 0) {
            mp[h] = M;
            mp[n_heads + h] = den;
        }
    }
}

// ---- the same for wide models (d_model > 512, bf16): one workgroup = one clip x one key range x one COLUMN GROUP of
// 256 columns (4 heads).  With all heads in one workgroup a d = 1280 row needs 2.5 wave-instructions (three chunks per
// lane, a sixth of the lanes idle in the last) and the register sets allow only two keys in flight per wave: 0.42 of the
// HBM roof at whisper-large-v3 width.  Here a wave-instruction reads the 512-byte segments of TWO key rows (lanes 0-31 the
// even key, 32-63 the odd key of a pair), UNROLL pairs per register set, two sets: the base kernel's 16 KiB in flight per
// wave, every lane busy.  The two parities of a wave keep separate online-softmax states; 4 waves x 2 parities merge
// through LDS.  Output layout unchanged (partials [B][splits][d], {max, sum} [B][splits][H][2], or the slab when splits == 1).
template <int UNROLL, bool NT>
__global__ __launch_bounds__(256) void k_dec_cross_attn_cg(const bf16* __restrict__ q, const bf16* __restrict__ ck,
                                                           const bf16* __restrict__ cv, float* __restrict__ part,
                                                           float* __restrict__ ml, int S, int d, int n_heads,
                                                           int splits, bf16* __restrict__ out, int mpad, int rows_per_clip) {
    constexpr int CGW = 256, HPG = CGW / WH_HEAD_DIM;   // columns / heads per group
    __shared__ __attribute__((aligned(16))) float wm[8][HPG], wl[8][HPG], wo[8][CGW];
    typedef __attribute__((ext_vector_type(8))) bf16 vec_t;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int par = lane >> 5, chunk = lane & 31;
    const int sp = blockIdx.x, b = blockIdx.y, cg = blockIdx.z;
    const int per = (S + splits - 1) / splits;
    const int ks = sp * per, j1 = min(S, ks + per);
    const int col0 = cg * CGW + chunk * 8;
    const wh_u32x4 qd = *reinterpret_cast<const wh_u32x4*>(q + (long)b * d + col0);
    float o[8], mrun = -INFINITY, lrun = 0.0f;
#pragma unroll
    for (int e = 0; e < 8; e++) o[e] = 0.0f;
    int kvb = b;   // (as in k_dec_cross_attn)
    if (rows_per_clip != 1) kvb = b / rows_per_clip;
    const bf16* kb = ck + (long)kvb * S * d + col0;
    const bf16* vb = cv + (long)kvb * S * d + col0;
    vec_t kA[UNROLL], vA[UNROLL], kB[UNROLL], vB[UNROLL];
    auto load_set = [&](vec_t (&kk)[UNROLL], vec_t (&vv)[UNROLL], int j) {
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            const int jj = min(j + 2 * u + par, j1 - 1);   // tail: re-read the last key, masked in compute_set
            if constexpr (NT) {
                kk[u] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(kb + (long)jj * d));
                vv[u] = __builtin_nontemporal_load(reinterpret_cast<const vec_t*>(vb + (long)jj * d));
            } else {
                kk[u] = *reinterpret_cast<const vec_t*>(kb + (long)jj * d);
                vv[u] = *reinterpret_cast<const vec_t*>(vb + (long)jj * d);
            }
        }
    };
    auto compute_set = [&](const vec_t (&kk)[UNROLL], const vec_t (&vv)[UNROLL], int j) {
        float s[UNROLL];
        float mx = mrun;
#pragma unroll
        for (int u = 0; u < UNROLL; u++) {
            float t = dot8_bf16(as_u32x4(kk[u]), qd, 0.0f);
            t = dpp_group_sum<8>(t);
            s[u] = (j + 2 * u + par < j1) ? t : -INFINITY;
            mx = fmaxf(mx, s[u]);
        }
        const float scale = (mx == -INFINITY) ? 1.0f : __expf(mrun - mx);   // nothing seen yet (this parity's keys all masked): keep zeros
        float ls = lrun * scale;
#pragma unroll
        for (int e = 0; e < 8; e++) o[e] *= scale;
#pragma unroll
        for (int u = 0; u < UNROLL; u += 2) {
            const float p0 = (s[u] == -INFINITY) ? 0.0f : __expf(s[u] - mx), p1 = (s[u + 1] == -INFINITY) ? 0.0f : __expf(s[u + 1] - mx);
            ls += p0 + p1;
            const bf16x2 pp = bf16x2{(bf16)p0, (bf16)p1};
            const wh_u32x4 va = as_u32x4(vv[u]), vb2 = as_u32x4(vv[u + 1]);
            pv2_bf16(va.x, vb2.x, pp, o[0], o[1]);
            pv2_bf16(va.y, vb2.y, pp, o[2], o[3]);
            pv2_bf16(va.z, vb2.z, pp, o[4], o[5]);
            pv2_bf16(va.w, vb2.w, pp, o[6], o[7]);
        }
        mrun = mx;
        lrun = ls;
    };
    constexpr int GS = 4 * UNROLL * 2;   // keys per round of the four waves
    const int j0 = ks + wave * UNROLL * 2;
    if (j0 < j1) load_set(kA, vA, j0);
    for (int j = j0; j < j1; j += 2 * GS) {
        const bool hasB = j + GS < j1;
        if (hasB) load_set(kB, vB, j + GS);
        compute_set(kA, vA, j);
        if (hasB) {
            if (j + 2 * GS < j1) load_set(kA, vA, j + 2 * GS);
            compute_set(kB, vB, j + GS);
        }
    }
    // merge the 4 waves x 2 parities of this key range (LDS)
    const int st = wave * 2 + par;
    if ((chunk & 7) == 0) { wm[st][chunk >> 3] = mrun; wl[st][chunk >> 3] = lrun; }
#pragma unroll
    for (int e = 0; e < 8; e++) wo[st][chunk * 8 + e] = o[e];
    __syncthreads();
    float* pp = part + ((long)b * splits + sp) * d + cg * CGW;
    float* mp = ml + ((long)b * splits + sp) * n_heads * 2;
    {
        const int n = tid, hl = n / WH_HEAD_DIM, h = cg * HPG + hl;   // 256 threads = 256 columns of the group
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 8; w++) M = fmaxf(M, wm[w][hl]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const float mw = wm[w][hl];
            const float sc = (mw == -INFINITY) ? 0.0f : __expf(mw - M);   // a stream may own no keys
            num += sc * wo[w][n];
            den += sc * wl[w][hl];
        }
        if (out) {
            out[slab_idx(b, cg * CGW + n, mpad)] = (bf16)(num / den);
        } else {
            pp[n] = num;
            if ((n % WH_HEAD_DIM) == 0) { mp[h] = M; mp[n_heads + h] = den; }
        }
    }
}

}  // namespace

void wh_launch_dec_self_attn(hipStream_t s, int prec, const void* qkv, void* kc, void* vc, void* out, const int* pos_p,
                             int d, int n_heads, int tc, int B, int mpad, const int* off) {
    dim3 grid(n_heads, B);
    wh_with_flags([&](auto pfx) {
        constexpr bool PFX = decltype(pfx)::value;
        if (prec == WH_PREC_F16X3)   // f32 q/k/v and caches (no matrix-core work here), the output as the out-projection's fp16-limb operand
            hipLaunchKernelGGL((k_dec_self_attn<float, h2, PFX>), grid, dim3(64), 0, s, (const float*)qkv, (float*)kc, (float*)vc, (h2*)out, pos_p, d, n_heads, tc, mpad, off);
        else if (prec == WH_PREC_F32)
            hipLaunchKernelGGL((k_dec_self_attn<float, float, PFX>), grid, dim3(64), 0, s, (const float*)qkv, (float*)kc, (float*)vc, (float*)out, pos_p, d, n_heads, tc, mpad, off);
        else
            hipLaunchKernelGGL((k_dec_self_attn<bf16, bf16, PFX>), grid, dim3(64), 0, s, (const bf16*)qkv, (bf16*)kc, (bf16*)vc, (bf16*)out, pos_p, d, n_heads, tc, mpad, off);
    }, off != nullptr);
}

// Occupancy cap of the cross-attention stream.  With more than two workgroups resident per CU (1024 clips = 4 per CU) every one
// keeps 32 KB of K/V rows in flight and the memory system queues far more requests than the ~7 MB its latency x bandwidth
// needs; measured at 1024 clips (profiles/r03_cross_attn_occupancy.txt): 474.5 us per launch with 4 resident workgroups per
// CU, 493.4 with 3, 464.2 with 2, 477.0 with 1.  The cap is an LDS reservation: a launch with more than 2 x 256 workgroups
// asks for 72 KB of dynamic LDS per workgroup (the kernels use only their own first bytes), so two fit a CU's 160 KB and a
// third does not.  WH_CROSS_WGS_PER_CU=0 removes the cap, 1 reserves for one workgroup per CU.  Results do not depend on it.
size_t wh_cross_lds_reserve(long total_wgs, size_t own_bytes) {
    static const int cap = [] { const char* e = getenv("WH_CROSS_WGS_PER_CU"); return e ? atoi(e) : 2; }();
    if (cap <= 0 || cap > 2 || total_wgs <= (long)cap * 256) return own_bytes;
    const size_t target = cap == 1 ? (size_t)150 * 1024 : (size_t)72 * 1024;
    return own_bytes > target ? own_bytes : target;
}

void wh_launch_dec_cross_attn(hipStream_t s, int prec, const void* q, const void* ck, const void* cv, float* part,
                              float* ml, int S, int d, int n_heads, int splits, int B, void* out, int mpad, bool stream_nt, int rows_per_clip) {
    dim3 grid(splits, B);
    const bool f32_layout = prec == WH_PREC_F32 || prec == WH_PREC_F16X3;   // (no matrix-core work in this kernel: the f32 form serves both)
    const long wgs = (long)splits * B * ((!f32_layout && d > 512 && d % 256 == 0) ? d / 256 : 1);
    const size_t sm = wh_cross_lds_reserve(wgs, sizeof(float) * ((size_t)8 * n_heads + 4 * (size_t)d));
#define WH_CA2(T_, N_, U_, NT_, TO_) do { set_max_smem(k_dec_cross_attn<T_, N_, U_, NT_, TO_>, sm);                                                 \
                                     hipLaunchKernelGGL((k_dec_cross_attn<T_, N_, U_, NT_, TO_>), grid, dim3(256), sm, s, (const T_*)q, (const T_*)ck, \
                                             (const T_*)cv, part, ml, S, d, n_heads, splits, (TO_*)(splits == 1 ? out : nullptr), mpad, rows_per_clip); } while (0)
#define WH_CA1(T_, N_, U_, NT_) WH_CA2(T_, N_, U_, NT_, T_)
    static const int nt_env = [] { const char* e = getenv("WH_CROSS_NT"); return e ? atoi(e) : -1; }();   // (A/B runs: force the non-temporal K/V loads off / on)
    if (nt_env >= 0) stream_nt = nt_env != 0;
#define WH_CA(T_, N_, U_) do { if (stream_nt) WH_CA1(T_, N_, U_, true); else WH_CA1(T_, N_, U_, false); } while (0)
    if (prec == WH_PREC_F16X3) {   // the f32 kernel (no matrix-core work); one key range per clip writes the out-projection's fp16-limb operand
#define WH_CAX(N_, U_) do { if (stream_nt) WH_CA2(float, N_, U_, true, h2); else WH_CA2(float, N_, U_, false, h2); } while (0)
        const int nch = (d / 4 + 63) / 64;
        if (nch == 1) WH_CAX(1, 4);
        else if (nch == 2) WH_CAX(2, 2);
        else WH_CAX(5, 1);
#undef WH_CAX
    } else if (f32_layout) {
        const int nch = (d / 4 + 63) / 64;  // f32: 4 elements per chunk
        if (nch == 1) WH_CA(float, 1, 4);
        else if (nch == 2) WH_CA(float, 2, 2);
        else WH_CA(float, 5, 1);
    } else {
        const int nch = (d / 8 + 63) / 64;
        static const int unroll_env = [] { const char* e = getenv("WH_CROSS_UNROLL"); return e ? atoi(e) : 0; }();   // (A/B runs)
        if (nch == 1) {
            const int un = unroll_env ? unroll_env : wh_dbg_cross_unroll;
            if (un == 8) WH_CA(bf16, 1, 8);
            else if (un == 2) WH_CA(bf16, 1, 2);
            else WH_CA(bf16, 1, 4);
        }
        else if (d % 256 == 0 && getenv("WH_CROSS_ALLHEADS") == nullptr) {   // wide models: one workgroup per 256-column group
            dim3 g3(splits, B, d / 256);
            bf16* o = (bf16*)(splits == 1 ? out : nullptr);
            const size_t smcg = wh_cross_lds_reserve(wgs, 12 * 1024) - 12 * 1024;   // (the kernel's own ~10 KB are static: only the reserve is dynamic)
            if (stream_nt) { set_max_smem(k_dec_cross_attn_cg<4, true>, smcg); hipLaunchKernelGGL((k_dec_cross_attn_cg<4, true>), g3, dim3(256), smcg, s, (const bf16*)q, (const bf16*)ck, (const bf16*)cv, part, ml, S, d, n_heads, splits, o, mpad, rows_per_clip); }
            else { set_max_smem(k_dec_cross_attn_cg<4, false>, smcg); hipLaunchKernelGGL((k_dec_cross_attn_cg<4, false>), g3, dim3(256), smcg, s, (const bf16*)q, (const bf16*)ck, (const bf16*)cv, part, ml, S, d, n_heads, splits, o, mpad, rows_per_clip); }
        } else WH_CA(bf16, 3, 2);
    }
#undef WH_CA
#undef WH_CA1
#undef WH_CA2
}
