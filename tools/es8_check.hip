// es8_check.hip — k_dec_cross_attn_es8 (wh_cross_es8.hip) against a host restatement on random data, then its launch time at 2048 clips.
//   ctx_h[dim] = sum_key softmax_key(qe_h . E[key]) E[key][dim],  E = e4m3 codes decoded exactly on the host; the kernel carries queries and
//   probabilities as e4m3 head + remainder pairs (~8 significant bits) and stores bf16
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -I whisper-rust-ort_amd/csrc tools/es8_check.hip -o tools/es8_check
#include "../whisper-rust-ort_amd/csrc/wh_cross_es8.hip"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
bool wh_ensure_dyn_lds(const void* k, size_t b) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b) == hipSuccess; }
void wh_set_error(const char* f, ...) { fprintf(stderr, "error: %s\n", f); }
static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static float e4m3(unsigned char b) {   // OCP e4m3fn
    const int s = b >> 7, e = (b >> 3) & 15, m = b & 7;
    float v = e == 0 ? ldexpf((float)m / 8.0f, -6) : ldexpf(1.0f + (float)m / 8.0f, e - 7);
    return s ? -v : v;
}
static unsigned rs = 4242;
static unsigned rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static unsigned long long fnv1a(const void* p, size_t n) {   // 64-bit FNV-1a of the raw output buffer: equal across builds that compute the same bits
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int check(int B, int S, int n_cus) {
    const int e_rows = S + 20, mpad = ((B + 63) / 64) * 64, H = 8, D = 512;
    std::vector<unsigned char> E((size_t)B * e_rows * D);
    for (auto& b : E) { unsigned x = rnd(); unsigned char c = (unsigned char)(x & 0xff); if ((c & 0x78) > 0x40) c = (unsigned char)((c & 0x87) | 0x38); b = c; }   // |values| <= 3.75, no NaN codes
    std::vector<float> qe((size_t)B * H * D);
    for (auto& v : qe) v = ((int)(rnd() & 0xffff) - 32768) / 32768.0f * 0.12f;
    unsigned char* dE; float* dq; unsigned short* dout;
    const size_t out_n = (size_t)(H * D / 32) * mpad * 32;
    CK(hipMalloc(&dE, E.size())); CK(hipMalloc(&dq, qe.size() * 4)); CK(hipMalloc(&dout, out_n * 2));
    CK(hipMemcpy(dE, E.data(), E.size(), hipMemcpyHostToDevice)); CK(hipMemcpy(dq, qe.data(), qe.size() * 4, hipMemcpyHostToDevice)); CK(hipMemset(dout, 0, out_n * 2));
    wh_launch_dec_cross_attn_es8(0, dq, dE, dout, S, e_rows, B, mpad, true, n_cus);
    CK(hipDeviceSynchronize());
    std::vector<unsigned short> out(out_n);
    CK(hipMemcpy(out.data(), dout, out_n * 2, hipMemcpyDeviceToHost));
    double worst = 0, scale = 0;
    std::vector<double> sc(S), ctx(D);
    for (int b = 0; b < B; b++)
        for (int h = 0; h < H; h++) {
            double mx = -1e30;
            for (int k = 0; k < S; k++) {
                double s = 0;
                for (int d = 0; d < D; d++) s += (double)qe[((size_t)b * H + h) * D + d] * e4m3(E[((size_t)b * e_rows + k) * D + d]);
                sc[k] = s; mx = fmax(mx, s);
            }
            double l = 0;
            for (int d = 0; d < D; d++) ctx[d] = 0;
            for (int k = 0; k < S; k++) {
                const double p = exp(sc[k] - mx);
                l += p;
                for (int d = 0; d < D; d++) ctx[d] += p * e4m3(E[((size_t)b * e_rows + k) * D + d]);
            }
            for (int d = 0; d < D; d++) {
                const int kcol = h * D + d;
                const double got = bf2f(out[((size_t)(kcol >> 5) * mpad + b) * 32 + (kcol & 31)]), want = ctx[d] / l;
                if (!(fabs(got - want) <= 1e30)) worst = 1e30;   // NaN
                worst = fmax(worst, fabs(got - want)); scale = fmax(scale, fabs(want));
            }
        }
    const bool ok = worst <= 0.02 * scale + 1e-3;
    printf("check B %3d S %4d on %3d workgroups: max |ctx - host| %.3e (|ctx| up to %.3f)  %s  hash %016llx\n", B, S, std::min(B, n_cus), worst, scale, ok ? "ok" : "MISMATCH", fnv1a(out.data(), out_n * 2));
    hipFree(dE); hipFree(dq); hipFree(dout);
    return ok ? 0 : 1;
}

int main(int argc, char** argv) {
    if (check(3, 64, 256) | check(5, 1500, 256) | check(7, 1500, 2) | check(4, 333, 3)) return 1;
    const int B = argc > 1 ? atoi(argv[1]) : 2048, S = 1500, e_rows = 1520, mpad = B;
    unsigned char* dE; float* dq; unsigned short* dout;
    CK(hipMalloc(&dE, (size_t)B * e_rows * 512)); CK(hipMalloc(&dq, (size_t)B * 4096 * 4)); CK(hipMalloc(&dout, (size_t)128 * mpad * 32 * 2));
    std::vector<unsigned char> hb(1 << 24);
    for (auto& b : hb) { unsigned char c = (unsigned char)(rnd() & 0xff); if ((c & 0x78) > 0x40) c = (unsigned char)((c & 0x87) | 0x38); b = c; }
    for (size_t off = 0; off < (size_t)B * e_rows * 512; off += hb.size()) CK(hipMemcpy(dE + off, hb.data(), std::min(hb.size(), (size_t)B * e_rows * 512 - off), hipMemcpyHostToDevice));
    std::vector<float> hq((size_t)B * 4096);
    for (auto& v : hq) v = ((int)(rnd() & 0xffff) - 32768) / 32768.0f * 0.12f;
    CK(hipMemcpy(dq, hq.data(), hq.size() * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) wh_launch_dec_cross_attn_es8(0, dq, dE, dout, S, e_rows, B, mpad, true, 256);
    CK(hipEventRecord(e0, 0));
    const int reps = 10;
    for (int i = 0; i < reps; i++) wh_launch_dec_cross_attn_es8(0, dq, dE, dout, S, e_rows, B, mpad, true, 256);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = ms / reps * 1e3, bytes = (double)B * S * 512;
    printf("k_dec_cross_attn_es8, %d clips: %.1f us per launch, %.2f TB/s of e4m3 encoder states (the bf16 form: 472-478 us for twice the bytes)\n", B, us, bytes / us * 1e-6);
    return 0;
}
