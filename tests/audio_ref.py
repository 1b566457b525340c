"""Numpy restatement of the raw-audio ingest (the reference's load_audio_16k_mono + resample_linear, src/main.rs:207-316).

Every f32 operation is a separate numpy float32 operation (numpy never contracts a * b + c), the position arithmetic is float64, and n_out is
rounded half away from zero explicitly — not Python's round (half to even) and not floor(x + 0.5) (wrong just below a tie).
tests/test_ingest_cpu.py pins this file to the host loader bit for bit; the GPU tests hold the kernel to it."""
import math

import numpy as np

F32 = np.float32


def n_out(n_frames: int, sample_rate: int) -> int:
    """resample_linear's output length (src/main.rs:211-212); a 16 kHz clip is not resampled."""
    if sample_rate == 16000:
        return int(n_frames)
    ratio = 16000.0 / float(sample_rate)
    x = float(n_frames) * ratio
    t = math.trunc(x)
    return int(t + (1 if x - t >= 0.5 else 0))


def convert(x: np.ndarray) -> np.ndarray:
    """Sample conversion, elementwise, to float32."""
    if x.dtype == np.int16:
        return x.astype(F32) / F32(32768.0)
    if x.dtype == np.uint8:
        return (x.astype(F32) - F32(128.0)) / F32(128.0)
    if x.dtype == np.float32:
        return x
    raise TypeError(x.dtype)


def downmix(x: np.ndarray) -> np.ndarray:
    """[frames, channels] -> [frames]: acc = 0.0f; acc += conv(x[j, ch]) in channel order; acc / (float)channels."""
    x = x.reshape(len(x), -1)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros(x.shape[0], F32)
        for ch in range(x.shape[1]):
            acc = acc + convert(np.ascontiguousarray(x[:, ch]))
        return (acc / F32(x.shape[1])).astype(F32)


def ingest(x: np.ndarray, sample_rate: int) -> np.ndarray:
    """The 16 kHz mono float32 samples of interleaved samples x [frames, channels] (int16 / uint8 / float32) at sample_rate."""
    m = downmix(np.asarray(x))
    if sample_rate == 16000:
        return m
    n = n_out(len(m), sample_rate)
    ratio = np.float64(16000.0) / np.float64(sample_rate)
    i = np.arange(n, dtype=np.float64)
    t = i / ratio
    fl = np.floor(t)
    a = t - fl
    i0 = fl.astype(np.int64)
    mp = np.concatenate([m, np.zeros(2, F32)])              # m(j) = 0 for j >= n_frames; t >= 0, so j < 0 never occurs
    i0c = np.minimum(i0, len(m))
    s0, s1 = mp[i0c], mp[np.minimum(i0c + 1, len(m) + 1)]
    w0, w1 = (np.float64(1.0) - a).astype(F32), a.astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        p0 = w0 * s0
        p1 = w1 * s1
        return (p0 + p1).astype(F32)


def write_wav(path: str, x: np.ndarray, sample_rate: int) -> None:
    """A canonical RIFF/WAVE file of x [frames, channels]: int16 / uint8 as PCM (format 1), float32 as IEEE float (format 3)."""
    import struct
    x = np.ascontiguousarray(np.asarray(x).reshape(len(x), -1))
    fmt = 3 if x.dtype == np.float32 else 1
    ch, bps = x.shape[1], x.dtype.itemsize
    data = x.tobytes()
    pad = b"\0" * (len(data) & 1)
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", 36 + len(data) + len(pad)) + b"WAVEfmt "
                + struct.pack("<IHHIIHH", 16, fmt, ch, sample_rate, sample_rate * ch * bps, ch * bps, 8 * bps)
                + b"data" + struct.pack("<I", len(data)) + data + pad)


def random_clip(rng: np.random.Generator, dtype, frames: int, channels: int) -> np.ndarray:
    """Seeded samples [frames, channels]: int16 clips include -32768 and 32767, uint8 0 and 255 (a one-sample clip: the first of them), float32 values are finite and normal."""
    dtype = np.dtype(dtype)
    if dtype == np.int16:
        x = rng.integers(-32768, 32768, (frames, channels)).astype(np.int16)
        for k, v in zip(rng.choice(x.size, min(2, x.size), replace=False), (-32768, 32767)):
            x.flat[k] = v
    elif dtype == np.uint8:
        x = rng.integers(0, 256, (frames, channels)).astype(np.uint8)
        for k, v in zip(rng.choice(x.size, min(2, x.size), replace=False), (0, 255)):
            x.flat[k] = v
    else:
        x = rng.uniform(-1.0, 1.0, (frames, channels)).astype(np.float32)
        x[np.abs(x) < 1e-3] = np.float32(0.25)
    return x
