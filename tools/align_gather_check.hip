// align_gather_check.hip — k_align_gather of wh_align.hip (the forced pass's copy of the alignment heads' queries) against a host
// loop on random operands.  Sources bf16 and f32; dk = 64 (one head's 64 columns of a 512-wide query row: the K/V form) and dk = 512 (a head's
// whole expanded query of an [8][512] row: the encoder-state form); four hypotheses of ragged lengths 1, 2, 17 and Lmax = 23 in one launch,
// with P = 1 and P = 4 prompt positions; two listed heads in slots 1 and 0 of a list of three (slot 2 belongs to another layer).
//   The destination is pre-filled with a sentinel bit pattern.  The kernel is a copy (bf16 -> f32 is exact), so every element the definition
//   names must be bit-equal to its source and every other element must still hold the sentinel: prompt rows before P - 1, the padding of the
//   shorter hypotheses, the slot of the other layer.  The source holds exactly the pass's rows.
//   build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-mfma-vgpr-form=1 -I whisper-rust-ort_amd/csrc tools/align_gather_check.hip -o tools/align_gather_check
#include "../whisper-rust-ort_amd/csrc/wh_align.hip"
#include <cstdio>
#include <cstring>
#include <vector>
void wh_set_error(const char* f, ...) { fprintf(stderr, "error: %s\n", f); }
static unsigned rs = 4242;
static float uni() { rs = rs * 1664525u + 1013904223u; return ((int)((rs >> 8) & 0xffff) - 32768) / 32768.0f; }
static unsigned short f2bf(float f) { unsigned u; memcpy(&u, &f, 4); u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16; return (unsigned short)u; }
static float bf2f(unsigned short h) { unsigned u = (unsigned)h << 16; float f; memcpy(&f, &u, 4); return f; }
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int check(bool bf, int dk, int P) {
    const int G = 4, Lmax = 23, T = P + Lmax - 1, R = G * T, n_model_heads = 8, slots = 3;
    const int len_h[G] = {1, 17, Lmax, 2};
    const long head_pitch = dk, row_pitch = dk == 64 ? 512 : (long)n_model_heads * dk;
    AlignLayerHeads hs;
    hs.n = 2; hs.slot[0] = 1; hs.head[0] = 3; hs.slot[1] = 0; hs.head[1] = 6;
    std::vector<float> src((size_t)R * row_pitch);
    for (auto& v : src) v = bf ? bf2f(f2bf(uni())) : uni();
    std::vector<unsigned short> srcb(src.size());
    for (size_t i = 0; i < src.size(); i++) srcb[i] = f2bf(src[i]);
    const size_t dn = (size_t)slots * G * Lmax * dk;
    const unsigned SENT = 0xFFC0DE77u;
    std::vector<unsigned> want(dn, SENT), got(dn);
    for (int j = 0; j < hs.n; j++)
        for (int g = 0; g < G; g++)
            for (int i = 0; i < len_h[g]; i++)
                for (int k = 0; k < dk; k++) {
                    const float v = src[(size_t)(g * T + P - 1 + i) * row_pitch + hs.head[j] * head_pitch + k];
                    memcpy(&want[(((size_t)hs.slot[j] * G + g) * Lmax + i) * dk + k], &v, 4);
                }
    void* dsrc; float* ddst; int* dlen;
    CK(hipMalloc(&dsrc, src.size() * (bf ? 2 : 4))); CK(hipMalloc(&ddst, dn * 4)); CK(hipMalloc(&dlen, G * 4));
    if (bf) CK(hipMemcpy(dsrc, srcb.data(), srcb.size() * 2, hipMemcpyHostToDevice)); else CK(hipMemcpy(dsrc, src.data(), src.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(dlen, len_h, G * 4, hipMemcpyHostToDevice));
    std::vector<unsigned> fill(dn, SENT);
    CK(hipMemcpy(ddst, fill.data(), dn * 4, hipMemcpyHostToDevice));
    wh_launch_align_gather(0, bf, dsrc, row_pitch, head_pitch, dk, hs, R, T, P, Lmax, dlen, G, ddst);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(got.data(), ddst, dn * 4, hipMemcpyDeviceToHost));
    size_t bad = 0, named = 0, first = dn;
    for (size_t i = 0; i < dn; i++) {
        named += want[i] != SENT;
        if (got[i] != want[i]) { if (!bad) first = i; bad++; }
    }
    printf("k_align_gather %s dk %3d P %d: %d rows, %zu named elements of %zu, %zu differ%s\n", bf ? "bf16" : "f32 ", dk, P, R, named, dn, bad, bad ? " MISMATCH" : " ok");
    if (bad) printf("  first at element %zu: got %08x want %08x\n", first, got[first], want[first]);
    hipFree(dsrc); hipFree(ddst); hipFree(dlen);
    return bad ? 1 : 0;
}

int main() {
    int rc = 0;
    for (int bf = 0; bf < 2; bf++)
        for (int dk : {64, 512})
            for (int P : {1, 4}) rc |= check(bf != 0, dk, P);
    return rc;
}
