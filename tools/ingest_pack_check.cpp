// ingest_pack_check — host-side check of the raw-audio descriptor packing (csrc/wh_ingest_desc.h), a stand-alone program so that it
// can be built with -fsanitize=address,undefined:  g++ -std=c++17 -g -fsanitize=address,undefined tools/ingest_pack_check.cpp -o ingest_pack_check
// Packs batches of clips of mixed formats and odd byte counts, copies each clip's bytes to its offset in a staging buffer of exactly the
// planned size (an offset or a size that is off by one is an out-of-bounds copy), reads every sample back through the descriptor the way the
// kernel indexes it, and checks alignment, order, n_out and the largest-batch arithmetic.  Prints "ok" and returns 0.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../whisper-rust-ort_amd/csrc/wh_ingest_desc.h"

#define CHECK(x)                                                                   \
    do {                                                                           \
        if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); return 1; } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(rng_state >> 33); }

int main() {
    // the lengths the issue pins (src/main.rs:211-212, half away from zero)
    CHECK(wh_resampled_len(1440000, 48000) == 480000 && wh_resampled_len(1440001, 48000) == 480000 && wh_resampled_len(1440002, 48000) == 480001);
    CHECK(wh_resampled_len(1323000, 44100) == 480000 && wh_resampled_len(240001, 8000) == 480002);
    CHECK(wh_resampled_len(1, 44100) == 0 && wh_resampled_len(2, 96000) == 0 && wh_resampled_len(3, 96000) == 1 && wh_resampled_len(7, 16000) == 7);
    CHECK(wh_resampled_len(5, 0) == 0);
    const uint32_t rates[] = {8000, 11025, 15999, 16000, 16001, 22050, 44100, 48000, 96000, 1, 768000};
    const uint16_t fmts[] = {WH_PCM_S16, WH_PCM_U8, WH_PCM_F32};
    for (int round = 0; round < 200; round++) {
        const size_t n = 1 + rnd() % 64;
        std::vector<std::vector<unsigned char>> host(n);
        std::vector<wh_raw_clip> clips(n);
        for (size_t i = 0; i < n; i++) {
            wh_raw_clip& r = clips[i];
            r.format = fmts[rnd() % 3];
            r.channels = (uint16_t)(1 + rnd() % WH_MAX_CHANNELS);
            r.sample_rate = rates[rnd() % (sizeof rates / sizeof rates[0])];
            r.n_frames = 1 + rnd() % 97;
            host[i].resize(r.n_frames * r.channels * wh_pcm_sample_bytes(r.format) + 1);
            for (auto& b : host[i]) b = (unsigned char)rnd();
            r.data = host[i].data() + 1;                      // any alignment
            CHECK(wh_raw_clip_problem(r) == nullptr);
        }
        WhIngestPlan plan;
        wh_ingest_pack(clips.data(), n, WH_CLIP_SAMPLES, plan);
        CHECK(plan.desc.size() == n && plan.bytes.size() == n && plan.total_bytes % WH_INGEST_ALIGN == 0);
        unsigned char* stage = (unsigned char*)malloc(plan.total_bytes);   // exactly the planned size
        CHECK(stage != nullptr);
        size_t max_out = 0, prev_end = 0;
        for (size_t i = 0; i < n; i++) {
            const WhIngestDesc& d = plan.desc[i];
            CHECK(d.raw_off % WH_INGEST_ALIGN == 0 && d.raw_off >= prev_end && d.raw_off - prev_end < WH_INGEST_ALIGN);
            CHECK(plan.bytes[i] == clips[i].n_frames * clips[i].channels * wh_pcm_sample_bytes(clips[i].format));
            CHECK(d.raw_off + plan.bytes[i] <= plan.total_bytes);
            CHECK(d.n_frames == clips[i].n_frames && d.sample_rate == clips[i].sample_rate && d.channels == clips[i].channels && d.format == clips[i].format);
            CHECK(d.dst_row == i && d.row_stride == WH_CLIP_SAMPLES && d.n_out == wh_resampled_len(clips[i].n_frames, clips[i].sample_rate));
            memcpy(stage + d.raw_off, clips[i].data, plan.bytes[i]);
            prev_end = d.raw_off + plan.bytes[i];
            if (d.n_out > max_out) max_out = d.n_out;
        }
        CHECK(plan.max_out == max_out);
        for (size_t i = 0; i < n; i++) {   // every sample through the descriptor, with the element type's own alignment
            const WhIngestDesc& d = plan.desc[i];
            const size_t ne = d.n_frames * d.channels, sb = wh_pcm_sample_bytes(d.format);
            for (size_t e = 0; e < ne; e++) {
                if (d.format == WH_PCM_S16) { const int16_t v = reinterpret_cast<const int16_t*>(stage + d.raw_off)[e]; CHECK(!memcmp(&v, (const char*)clips[i].data + e * sb, sb)); }
                else if (d.format == WH_PCM_F32) { const uint32_t v = reinterpret_cast<const uint32_t*>(stage + d.raw_off)[e]; CHECK(!memcmp(&v, (const char*)clips[i].data + e * sb, sb)); }
                else CHECK(stage[d.raw_off + e] == ((const unsigned char*)clips[i].data)[e]);
            }
        }
        free(stage);
    }
    // a batch past 2^31 bytes: 64 clips of 30 s, 8 channels, 96 kHz, f32 (offsets only; nothing is allocated)
    std::vector<wh_raw_clip> big(64);
    static const float one = 0.0f;
    for (auto& r : big) { r.data = &one; r.n_frames = 2880000; r.sample_rate = 96000; r.channels = 8; r.format = WH_PCM_F32; }
    WhIngestPlan plan;
    wh_ingest_pack(big.data(), big.size(), WH_CLIP_SAMPLES, plan);
    CHECK(plan.bytes[0] == 92160000ull && plan.desc[63].raw_off == 63ull * 92160000ull && plan.total_bytes == 64ull * 92160000ull && plan.total_bytes > (1ull << 31));
    CHECK(plan.max_out == 480000);
    wh_raw_clip bad = big[0];
    bad.data = nullptr; CHECK(wh_raw_clip_problem(bad)); bad = big[0];
    bad.format = 3; CHECK(wh_raw_clip_problem(bad)); bad = big[0];
    bad.channels = 0; CHECK(wh_raw_clip_problem(bad)); bad.channels = 65; CHECK(wh_raw_clip_problem(bad)); bad = big[0];
    bad.sample_rate = 0; CHECK(wh_raw_clip_problem(bad)); bad.sample_rate = 768001; CHECK(wh_raw_clip_problem(bad));
    printf("ok\n");
    return 0;
}
