// wh_ingest_desc.h — the per-clip descriptor of the raw-audio ingest kernel (wh_ingest.hip) and the host-side packing of a batch of
// wh_raw_clip into descriptors + staging offsets.  Plain C++ with no HIP in it: the packing is checked by a stand-alone host
// program (tools/ingest_pack_check.cpp) as well as through the library.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/whisper_hip.h"

constexpr size_t WH_INGEST_ALIGN = 16;   // every clip's raw bytes start at a multiple of this in the staging buffer
constexpr uint32_t WH_MAX_SAMPLE_RATE = 768000;

struct WhIngestDesc {
    uint64_t raw_off;      // byte offset of the clip's first sample in the staging buffer (multiple of WH_INGEST_ALIGN)
    uint64_t n_frames;
    uint64_t row_stride;   // destination: out + dst_row * row_stride, n_out f32 samples
    uint32_t n_out;
    uint32_t dst_row;
    uint32_t sample_rate;
    uint16_t channels;
    uint16_t format;       // WH_PCM_*
};
static_assert(sizeof(WhIngestDesc) == 40, "descriptor layout is shared with the kernel");

inline size_t wh_pcm_sample_bytes(unsigned format) { return format == WH_PCM_S16 ? 2 : format == WH_PCM_U8 ? 1 : format == WH_PCM_F32 ? 4 : 0; }

// resample_linear's output length (src/main.rs:211-212): llround(n * (16000 / rate)), half away from zero; the 16 kHz clip is not resampled
inline size_t wh_resampled_len(size_t n_frames, uint32_t sample_rate) {
    if (sample_rate == 0) return 0;
    if (sample_rate == 16000) return n_frames;
    const double ratio = 16000.0 / (double)sample_rate;
    return (size_t)llround((double)n_frames * ratio);
}

// Checks one clip's fields (not its length): 0, or a message.
inline const char* wh_raw_clip_problem(const wh_raw_clip& r) {
    if (!r.data) return "data is NULL";
    if (wh_pcm_sample_bytes(r.format) == 0) return "unknown sample format";
    if (r.channels < 1 || r.channels > WH_MAX_CHANNELS) return "channels must be 1..64";
    if (r.sample_rate < 1 || r.sample_rate > WH_MAX_SAMPLE_RATE) return "sample_rate must be 1..768000";
    return nullptr;
}

struct WhIngestPlan {
    std::vector<WhIngestDesc> desc;
    std::vector<size_t> bytes;   // raw bytes of each clip (what is copied to desc[i].raw_off)
    size_t total_bytes = 0;      // staging bytes the batch needs
    size_t max_out = 0;          // longest resampled clip
};

// Packs n validated clips back to back, each at the next multiple of WH_INGEST_ALIGN; clip i goes to destination row i.
inline void wh_ingest_pack(const wh_raw_clip* clips, size_t n, size_t row_stride, WhIngestPlan& plan) {
    plan.desc.resize(n);
    plan.bytes.resize(n);
    plan.max_out = 0;
    size_t off = 0;
    for (size_t i = 0; i < n; i++) {
        const wh_raw_clip& r = clips[i];
        WhIngestDesc& d = plan.desc[i];
        const size_t nb = r.n_frames * (size_t)r.channels * wh_pcm_sample_bytes(r.format);
        const size_t n_out = wh_resampled_len(r.n_frames, r.sample_rate);
        d.raw_off = off;
        d.n_frames = r.n_frames;
        d.row_stride = row_stride;
        d.n_out = (uint32_t)n_out;
        d.dst_row = (uint32_t)i;
        d.sample_rate = r.sample_rate;
        d.channels = r.channels;
        d.format = r.format;
        plan.bytes[i] = nb;
        if (n_out > plan.max_out) plan.max_out = n_out;
        off = (off + nb + WH_INGEST_ALIGN - 1) / WH_INGEST_ALIGN * WH_INGEST_ALIGN;
    }
    plan.total_bytes = off;
}
