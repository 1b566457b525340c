// wh_ingest.hip — raw audio ingest: interleaved S16 / U8 / F32 samples of any rate and channel count -> the 16 kHz mono f32 rows the log-mel
// kernels read.  The arithmetic is the reference's load_audio_16k_mono + resample_linear (src/main.rs:207-316), operation
// for operation, so the rows carry the bits the host loader (host/wh_host.h) produces:
//   conv     S16: (float)s / 32768.0f      U8: ((float)u - 128.0f) / 128.0f      F32: the value
//   m(j)     acc = 0.0f; acc += conv(x[j * channels + ch]) for ch = 0 .. channels-1 in order; acc / (float)channels; 0.0f outside the clip
//   16 kHz   out[i] = m(i)
//   else     ratio = 16000.0 / rate; t = (double)i / ratio; i0 = floor(t); a = t - i0; out[i] = (float)(1.0 - a) * m(i0) + (float)a * m(i0 + 1)
// Every f32 operation is a separate IEEE operation (nothing contracts into an FMA), the divisions are correctly rounded, t is one f64
// division per output.  One launch converts a whole batch: blockIdx.y is the clip, consecutive lanes take consecutive outputs (the raw reads
// of a wave then cover one contiguous span of the clip), each lane takes OUT_PER_LANE outputs 256 apart so the descriptor is read once per 1024.
#include "wh_ingest_desc.h"
#include "wh_kernels.h"

namespace {

constexpr int ING_THREADS = 256;
constexpr int OUT_PER_LANE = 4;
constexpr int ING_TILE = ING_THREADS * OUT_PER_LANE;

template <int FMT>
__device__ __forceinline__ float ing_conv(const unsigned char* __restrict__ base, size_t e) {
#pragma clang fp contract(off)
    if (FMT == WH_PCM_S16) return (float)reinterpret_cast<const short*>(base)[e] / 32768.0f;
    if (FMT == WH_PCM_U8) return ((float)base[e] - 128.0f) / 128.0f;
    return reinterpret_cast<const float*>(base)[e];
}

// channel mean of frame j (0.0f outside the clip); the additions run in channel order
template <int FMT>
__device__ __forceinline__ float ing_frame(const unsigned char* __restrict__ base, long long j, unsigned long long n_frames, unsigned channels, float fch) {
#pragma clang fp contract(off)
    if (j < 0 || (unsigned long long)j >= n_frames) return 0.0f;
    const size_t e0 = (size_t)j * channels;
    float acc = 0.0f;
    for (unsigned ch = 0; ch < channels; ch++) acc = acc + ing_conv<FMT>(base, e0 + ch);
    return acc / fch;
}

template <int FMT>
__device__ __forceinline__ void ing_tile(const WhIngestDesc& d, const unsigned char* __restrict__ base, float* __restrict__ out, unsigned i_first) {
#pragma clang fp contract(off)
    const float fch = (float)d.channels;
    if (d.sample_rate == 16000) {
#pragma unroll
        for (int k = 0; k < OUT_PER_LANE; k++) {
            const unsigned i = i_first + k * ING_THREADS;
            if (i < d.n_out) out[i] = ing_frame<FMT>(base, (long long)i, d.n_frames, d.channels, fch);
        }
        return;
    }
    const double ratio = 16000.0 / (double)d.sample_rate;
#pragma unroll
    for (int k = 0; k < OUT_PER_LANE; k++) {
        const unsigned i = i_first + k * ING_THREADS;
        if (i >= d.n_out) continue;
        const double t = (double)i / ratio;
        const double fl = floor(t);
        const long long i0 = (long long)fl;
        const double a = t - fl;
        const float w0 = (float)(1.0 - a), w1 = (float)a;
        const float s0 = ing_frame<FMT>(base, i0, d.n_frames, d.channels, fch);
        const float s1 = ing_frame<FMT>(base, i0 + 1, d.n_frames, d.channels, fch);
        const float p0 = w0 * s0, p1 = w1 * s1;
        out[i] = p0 + p1;
    }
}

__global__ __launch_bounds__(ING_THREADS) void k_ingest(const unsigned char* __restrict__ raw, const WhIngestDesc* __restrict__ descs, float* __restrict__ out) {
    const WhIngestDesc d = descs[blockIdx.y];
    const unsigned long long tile0 = (unsigned long long)blockIdx.x * ING_TILE;
    if (tile0 >= d.n_out) return;
    const unsigned char* base = raw + d.raw_off;
    float* row = out + (size_t)d.dst_row * d.row_stride;
    const unsigned i_first = (unsigned)tile0 + threadIdx.x;
    if (d.format == WH_PCM_S16) ing_tile<WH_PCM_S16>(d, base, row, i_first);
    else if (d.format == WH_PCM_U8) ing_tile<WH_PCM_U8>(d, base, row, i_first);
    else ing_tile<WH_PCM_F32>(d, base, row, i_first);
}

}  // namespace

void wh_launch_ingest(hipStream_t s, const void* raw, const WhIngestDesc* descs, int n_clips, size_t max_out, float* out) {
    if (n_clips <= 0 || max_out == 0) return;
    dim3 grid((unsigned)((max_out + ING_TILE - 1) / ING_TILE), (unsigned)n_clips);
    hipLaunchKernelGGL(k_ingest, grid, dim3(ING_THREADS), 0, s, (const unsigned char*)raw, descs, out);
}
