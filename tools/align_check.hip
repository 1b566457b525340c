// align_check.hip — the three score kernels of wh_align.hip (k_align_scores_f32, k_align_scores_bf16<64>, k_align_scores_bf16<512, split>)
// against a double-precision host restatement on random data: P[g][s] = softmax over s < S_b of q_g . k_s, with the exact operands the
// kernel reads (f32 queries, f32 or bf16 keys).  2 clips x 2 heads, 37 rows of a capacity of 40, S_b = 203 and 77 of S = 208 (no multiple of
// the 16-frame tile), a clip pitch with padding rows as in the encoder-state form.
//   Tolerance 5e-5 on probabilities.  What an exact kernel leaves: the f32 accumulation of dk <= 512 products (queries U(-0.5, 0.5), keys
//   U(-1, 1): a product has sigma 0.17, a score sigma 3.8 at dk = 512) — about sqrt(512) * 0.17 * 2^-24 ~ 2e-7 per score and the expf / divide
//   roundings, 1e-6 relative — and, for the split query, its 16 significant bits: sqrt(512) * 0.17 * 2^-17 ~ 3e-5 on a score, times the
//   probability it belongs to (at most 1) = 3e-5 at the very worst, 1e-6 measured.  A query that entered as its bf16 hi limb alone (8 bits) would move a score by 4e-3 and the larger
//   probabilities by ~1e-3: twenty times the tolerance.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -I whisper-rust-ort_amd/csrc tools/align_check.hip -o tools/align_check
#include "../whisper-rust-ort_amd/csrc/wh_align.hip"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
void wh_set_error(const char* f, ...) { fprintf(stderr, "error: %s\n", f); }
static unsigned rs = 777;
static float uni() { rs = rs * 1664525u + 1013904223u; return ((int)((rs >> 8) & 0xffff) - 32768) / 32768.0f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16; return (unsigned short)u; }
static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// form: WH_ALIGN_*; dk 64 (keys = one head's 64 columns of a d-wide plane) or 512 (the whole encoder-state row)
static int check(int form, const char* name) {
    const int nb = 2, nh = 2, cap = 40, n_gen = 37, S = 208, Sp = 208, dk = form == WH_ALIGN_ES_BF16 ? 512 : 64, d = 512, rows = S + 20, n_prompt = 5;
    const int sb_h[nb] = {203, 77}, nout_h[nb] = {n_prompt + n_gen, n_prompt + n_gen};
    const bool kf32 = form == WH_ALIGN_KV_F32;
    std::vector<float> q((size_t)nh * nb * cap * dk), kf((size_t)nb * rows * d);
    for (auto& v : kf) v = kf32 ? uni() : bf2f(f2bf(uni()));
    for (auto& v : q) { v = 0.5f * uni(); if (form == WH_ALIGN_KV_BF16) v = bf2f(f2bf(v)); }   // (the K/V form's queries were bf16 in the loop)
    std::vector<unsigned short> kb(kf.size());
    for (size_t i = 0; i < kf.size(); i++) kb[i] = f2bf(kf[i]);
    float *dq, *dP; void* dK; int *dn, *dsb;
    const size_t pn = (size_t)nb * nh * cap * Sp;
    CK(hipMalloc(&dq, q.size() * 4)); CK(hipMalloc(&dP, pn * 4)); CK(hipMalloc(&dK, kf.size() * 4)); CK(hipMalloc(&dn, nb * 4)); CK(hipMalloc(&dsb, nb * 4));
    CK(hipMemcpy(dq, q.data(), q.size() * 4, hipMemcpyHostToDevice));
    if (kf32) CK(hipMemcpy(dK, kf.data(), kf.size() * 4, hipMemcpyHostToDevice)); else CK(hipMemcpy(dK, kb.data(), kb.size() * 2, hipMemcpyHostToDevice));
    CK(hipMemcpy(dn, nout_h, nb * 4, hipMemcpyHostToDevice)); CK(hipMemcpy(dsb, sb_h, nb * 4, hipMemcpyHostToDevice));
    CK(hipMemset(dP, 0xff, pn * 4));
    const int head_col[nh] = {dk == 64 ? 64 * 3 : 0, dk == 64 ? 64 * 6 : 0};   // heads 3 and 6 of the plane; the encoder-state form reads whole rows
    AlignArgs a;
    a.q = dq; a.dk = dk;
    for (int h = 0; h < nh; h++) a.k_base[h] = (const char*)dK + (size_t)head_col[h] * (kf32 ? 4 : 2);
    a.k_clip_pitch = (long)rows * d; a.k_row_pitch = d;
    a.n_out = dn; a.n_prompt = n_prompt; a.cap = cap; a.sb = dsb; a.nb = nb; a.n_heads = nh; a.S = S; a.Sp = Sp; a.clip0 = 0; a.P = dP;
    if (wh_launch_align_scores(0, form, a, nb) != WH_OK) return 1;
    CK(hipDeviceSynchronize());
    std::vector<float> P(pn);
    CK(hipMemcpy(P.data(), dP, pn * 4, hipMemcpyDeviceToHost));
    double worst = 0, pmax = 0;
    std::vector<double> sc(S);
    for (int b = 0; b < nb; b++)
        for (int h = 0; h < nh; h++)
            for (int g = 0; g < n_gen; g++) {
                double mx = -1e300, sum = 0;
                for (int s = 0; s < sb_h[b]; s++) {
                    double acc = 0;
                    for (int k = 0; k < dk; k++) acc += (double)q[(((size_t)h * nb + b) * cap + g) * dk + k] * (double)kf[((size_t)b * rows + s) * d + head_col[h] + k];
                    sc[s] = acc; mx = std::max(mx, acc);
                }
                for (int s = 0; s < sb_h[b]; s++) sum += exp(sc[s] - mx);
                for (int s = 0; s < sb_h[b]; s++) {
                    const double ref = exp(sc[s] - mx) / sum, got = P[(((size_t)b * nh + h) * cap + g) * Sp + s];
                    worst = std::max(worst, fabs(got - ref)); pmax = std::max(pmax, ref);
                }
            }
    const bool ok = worst <= 5e-5;
    printf("%s: max |P - ref| %.3g (largest probability %.3g, tolerance 5e-5) %s\n", name, worst, pmax, ok ? "ok" : "MISMATCH");
    hipFree(dq); hipFree(dP); hipFree(dK); hipFree(dn); hipFree(dsb);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0;
    bad += check(WH_ALIGN_KV_F32, "k_align_scores_f32");
    bad += check(WH_ALIGN_KV_BF16, "k_align_scores_bf16<64>");
    bad += check(WH_ALIGN_ES_BF16, "k_align_scores_bf16<512, split>");
    return bad ? 1 : 0;
}
