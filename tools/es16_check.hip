// es16_check.hip — k_dec_cross_attn_es (bf16 encoder states) and k_dec_cross_attn_es2 (two fp16 limb planes, the WH_ES3=0 form), both wh_cross_es.hip,
// against a host restatement on random data, then their launch times at 2048 clips.
//   ctx_h[dim] = sum_key softmax_key(qe_h . E[key]) E[key][dim].  bf16: the states are rounded to bf16 on the host (exact for the kernel); es2: f32
//   states are split into the limb planes on the device with the library's own split (x3_split) and decoded exactly on the host.
//   Bounds: the bf16 form carries queries as bf16 head + remainder and probabilities as bf16 — at least es8_check's operands, so its bound; the es2
//   form carries more bits than the fp16 + e4m3 form, so es3_check's bound.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -fno-honor-nans -I whisper-rust-ort_amd/csrc tools/es16_check.hip -o tools/es16_check
#include "../whisper-rust-ort_amd/csrc/wh_cross_es.hip"
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
bool wh_ensure_dyn_lds(const void* k, size_t b) { return hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b) == hipSuccess; }
void wh_set_error(const char* f, ...) { fprintf(stderr, "error: %s\n", f); }
// the other formats' kernels live in their own files: the dispatcher's references to them are never taken here
bool wh_es3_enabled() { return false; }
void wh_launch_dec_cross_attn_es3(hipStream_t, const float*, const void*, void*, int, int, int, int, bool, int) { fprintf(stderr, "es16_check: the es3 kernel is not in this binary\n"); abort(); }
void wh_launch_dec_cross_attn_es8(hipStream_t, const float*, const void*, void*, int, int, int, int, bool, int) { fprintf(stderr, "es16_check: the es8 kernel is not in this binary\n"); abort(); }

static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); return (unsigned short)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16); }   // RNE (finite inputs)
static unsigned rs = 1616;
static unsigned rnd() { rs = rs * 1664525u + 1013904223u; return rs >> 8; }
static float frand(float a) { return ((int)(rnd() & 0xffff) - 32768) / 32768.0f * a; }
static unsigned long long fnv1a(const void* p, size_t n) {
    unsigned long long h = 1469598103934665603ull;
    for (size_t i = 0; i < n; i++) { h ^= ((const unsigned char*)p)[i]; h *= 1099511628211ull; }
    return h;
}
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

// f32 rows [rows][512] -> limb planes [rows][hi 512 | lo 512] fp16 (the conversion of k_layernorm_es2 without the LayerNorm)
__global__ void k_pack_es2(const float* __restrict__ x, _Float16* __restrict__ y, long rows) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int c = (threadIdx.x & 63) * 8;
    const xfrag f = x3_split(*reinterpret_cast<const f32x8*>(x + row * 512 + c));
    *reinterpret_cast<f16x8*>(y + row * 1024 + c) = f.hi;
    *reinterpret_cast<f16x8*>(y + row * 1024 + 512 + c) = f.lo;
}

// x3 = false: the bf16 form (bf16 slab out); true: the es2 form (h2 slab out)
static int check(bool x3, int B, int S, int n_cus) {
    const int e_rows = S + 20, mpad = ((B + 63) / 64) * 64, H = 8, D = 512;
    const long rows = (long)B * e_rows;
    const size_t esz = x3 ? 4 : 2, out_b = (size_t)(H * D / 32) * mpad * 32 * esz;
    std::vector<float> Ef((size_t)rows * D), qe((size_t)B * H * D);
    for (auto& v : Ef) v = frand(2.5f);
    for (auto& v : qe) v = frand(0.12f);
    std::vector<unsigned char> E((size_t)rows * D * esz), out(out_b);
    float *dEf = nullptr, *dq; unsigned char *dE, *dout;
    CK(hipMalloc(&dE, E.size())); CK(hipMalloc(&dq, qe.size() * 4)); CK(hipMalloc(&dout, out_b));
    CK(hipMemcpy(dq, qe.data(), qe.size() * 4, hipMemcpyHostToDevice)); CK(hipMemset(dout, 0, out_b));
    if (x3) {
        CK(hipMalloc(&dEf, Ef.size() * 4)); CK(hipMemcpy(dEf, Ef.data(), Ef.size() * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_pack_es2, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, 0, dEf, (_Float16*)dE, rows);
    } else {
        for (size_t i = 0; i < Ef.size(); i++) { const unsigned short h = f2bf(Ef[i]); memcpy(&E[2 * i], &h, 2); }
        CK(hipMemcpy(dE, E.data(), E.size(), hipMemcpyHostToDevice));
    }
    wh_launch_dec_cross_attn_es(0, x3 ? WH_PREC_F16X3 : WH_PREC_BF16, dq, dE, dout, S, e_rows, B, mpad, true, n_cus);
    CK(hipDeviceSynchronize());
    if (x3) CK(hipMemcpy(E.data(), dE, E.size(), hipMemcpyDeviceToHost));
    CK(hipMemcpy(out.data(), dout, out_b, hipMemcpyDeviceToHost));
    auto Eval = [&](long r, int d) -> double {
        if (!x3) { unsigned short h; memcpy(&h, &E[((size_t)r * D + d) * 2], 2); return bf2f(h); }
        _Float16 hi, lo; memcpy(&hi, &E[(size_t)r * 2048 + 2 * d], 2); memcpy(&lo, &E[(size_t)r * 2048 + 1024 + 2 * d], 2);
        return (double)(float)hi + (double)(float)lo;
    };
    double worst = 0, scale = 0, quant = 0;
    std::vector<double> sc(S), ctx(D), Er((size_t)S * D);
    for (int b = 0; b < B; b++) {
        for (int k = 0; k < S; k++) for (int d = 0; d < D; d++) { Er[(size_t)k * D + d] = Eval((long)b * e_rows + k, d); quant = fmax(quant, fabs(Er[(size_t)k * D + d] - Ef[((size_t)b * e_rows + k) * D + d])); }
        for (int h = 0; h < H; h++) {
            double mx = -1e30;
            for (int k = 0; k < S; k++) {
                double s = 0;
                for (int d = 0; d < D; d++) s += (double)qe[((size_t)b * H + h) * D + d] * Er[(size_t)k * D + d];
                sc[k] = s; mx = fmax(mx, s);
            }
            double l = 0;
            for (int d = 0; d < D; d++) ctx[d] = 0;
            for (int k = 0; k < S; k++) { const double p = exp(sc[k] - mx); l += p; for (int d = 0; d < D; d++) ctx[d] += p * Er[(size_t)k * D + d]; }
            for (int d = 0; d < D; d++) {
                const int kcol = h * D + d;
                const size_t el = ((size_t)(kcol >> 5) * mpad + b) * 32 + (kcol & 31);
                double got;
                if (x3) {
                    const size_t byte = el * 4, blk = byte & ~(size_t)127, off = (byte & 127) >> 1;
                    _Float16 oh, ol; memcpy(&oh, &out[blk + off], 2); memcpy(&ol, &out[blk + 64 + off], 2);
                    got = (double)(float)oh + (double)(float)ol;
                } else { unsigned short o; memcpy(&o, &out[el * 2], 2); got = bf2f(o); }
                const double want = ctx[d] / l;
                if (!(fabs(got - want) <= 1e30)) worst = 1e30;   // NaN
                worst = fmax(worst, fabs(got - want)); scale = fmax(scale, fabs(want));
            }
        }
    }
    const bool ok = x3 ? worst <= 2e-4 * scale + 1e-6 : worst <= 0.02 * scale + 1e-3;
    printf("check %s B %3d S %4d on %3d workgroups: max |ctx - host| %.3e (|ctx| up to %.3f; the states' own rounding: %.2e)  %s  hash %016llx\n", x3 ? "es2 " : "bf16", B, S,
           std::min(B, n_cus), worst, scale, quant, ok ? "ok" : "MISMATCH", fnv1a(out.data(), out_b));
    hipFree(dEf); hipFree(dE); hipFree(dq); hipFree(dout);
    return ok ? 0 : 1;
}

static int timing(bool x3, int B) {
    const int S = 1500, e_rows = 1520, mpad = B;
    const size_t rowb = x3 ? 2048 : 1024, esz = x3 ? 4 : 2;
    unsigned char *dE, *dout; float* dq;
    CK(hipMalloc(&dE, (size_t)B * e_rows * rowb)); CK(hipMalloc(&dq, (size_t)B * 4096 * 4)); CK(hipMalloc(&dout, (size_t)128 * mpad * 32 * esz));
    {   // random states, 64 clips at a time: rounded to bf16 on the host, or through the pack kernel
        const int nb = std::min(64, B);
        std::vector<float> hf((size_t)nb * e_rows * 512);
        for (auto& v : hf) v = frand(2.5f);
        std::vector<unsigned short> hb;
        float* df = nullptr;
        if (x3) { CK(hipMalloc(&df, hf.size() * 4)); CK(hipMemcpy(df, hf.data(), hf.size() * 4, hipMemcpyHostToDevice)); }
        else { hb.resize(hf.size()); for (size_t i = 0; i < hf.size(); i++) hb[i] = f2bf(hf[i]); }
        for (int b0 = 0; b0 < B; b0 += nb) {
            const long rows = (long)std::min(nb, B - b0) * e_rows;
            if (x3) hipLaunchKernelGGL(k_pack_es2, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, 0, df, (_Float16*)(dE + (size_t)b0 * e_rows * rowb), rows);
            else CK(hipMemcpy(dE + (size_t)b0 * e_rows * rowb, hb.data(), (size_t)rows * rowb, hipMemcpyHostToDevice));
        }
        CK(hipDeviceSynchronize()); hipFree(df);
    }
    std::vector<float> hq((size_t)B * 4096);
    for (auto& v : hq) v = frand(0.12f);
    CK(hipMemcpy(dq, hq.data(), hq.size() * 4, hipMemcpyHostToDevice));
    const int prec = x3 ? WH_PREC_F16X3 : WH_PREC_BF16;
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 3; i++) wh_launch_dec_cross_attn_es(0, prec, dq, dE, dout, S, e_rows, B, mpad, true, 256);
    CK(hipEventRecord(e0, 0));
    const int reps = 10;
    for (int i = 0; i < reps; i++) wh_launch_dec_cross_attn_es(0, prec, dq, dE, dout, S, e_rows, B, mpad, true, 256);
    CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1));
    float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
    const double us = ms / reps * 1e3, bytes = (double)B * S * rowb;
    printf("k_dec_cross_attn_es%s, %d clips: %.1f us per launch, %.2f TB/s of %s encoder states\n", x3 ? "2" : "", B, us, bytes / us * 1e-6, x3 ? "two-fp16-limb" : "bf16");
    hipFree(dE); hipFree(dq); hipFree(dout);
    return 0;
}

int main(int argc, char** argv) {
    int bad = 0;
    for (int x3 = 0; x3 < 2; x3++) bad |= check(x3, 3, 64, 256) | check(x3, 5, 1500, 256) | check(x3, 7, 1500, 2) | check(x3, 4, 333, 3);
    if (bad) return 1;
    const int B = argc > 1 ? atoi(argv[1]) : 2048;
    return timing(false, B) | timing(true, B);
}
