"""Raw-audio ingest, the parts that need no GPU: the resampled length, the numpy restatement tests/audio_ref.py pinned to the
host loader (which tests/test_host_cpu.py pins to the reference's formula), and the CLI's parse-only reader."""
import ctypes as C
import os

import numpy as np
import pytest

import audio_ref as ar
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = (8000, 11025, 15999, 16000, 16001, 22050, 44100, 48000, 96000)
FRAMES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097)
# (frames, rate) -> length, computed with the formula: the ties and near-ties around one 30 s window
PINNED = {(1440000, 48000): 480000, (1440002, 48000): 480001, (1323000, 44100): 480000, (240001, 8000): 480002}


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(os.path.join(ROOT, "whisper-rust-ort_amd", "libwh_host.so"))
    L.whh_load_wav.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
    L.whh_read_wav_raw.argtypes = [C.c_char_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]
    return L


def load_wav(H, path, cap):
    out = np.zeros(max(1, cap), np.float32)
    n, dur = C.c_size_t(), C.c_double()
    rc = H.whh_load_wav(path.encode(), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(n), C.byref(dur))
    return rc, out[: min(n.value, out.size)], n.value, dur.value


def test_resampled_samples_is_the_reference_rounding(H, tmp_path):
    lib = wb.load_library()
    pairs = [(f, r) for r in RATES for f in FRAMES] + list(PINNED)
    for f, r in pairs:
        assert lib.wh_resampled_samples(f, r) == ar.n_out(f, r), (f, r)
    for (f, r), want in PINNED.items():
        assert ar.n_out(f, r) == want and lib.wh_resampled_samples(f, r) == want
    assert sum(ar.n_out(f, r) == 0 for r in RATES for f in FRAMES) == 4
    assert lib.wh_resampled_samples(5, 0) == 0
    # ... and the length the host loader returns for a WAV of that many frames (u8 mono keeps the pinned files small)
    p = str(tmp_path / "n.wav")
    for f, r in pairs:
        ar.write_wav(p, np.full((f, 1), 128, np.uint8), r)
        rc, _, n, dur = load_wav(H, p, 1)
        assert rc == 0 and n == ar.n_out(f, r) and dur == n / 16000.0, (f, r)


@pytest.mark.parametrize("dtype", [np.int16, np.uint8, np.float32])
def test_restatement_equals_the_host_loader_bit_for_bit(H, tmp_path, dtype):
    rng = np.random.default_rng(20260 + np.dtype(dtype).itemsize)
    p = str(tmp_path / "x.wav")
    for ch in (1, 2, 3):
        for rate in (8000, 22050, 44100, 16000):
            x = ar.random_clip(rng, dtype, 1531, ch)
            ar.write_wav(p, x, rate)
            want = ar.ingest(x, rate)
            rc, got, n, _ = load_wav(H, p, len(want) + 8)
            assert rc == 0 and n == len(want)
            np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32), err_msg=f"{np.dtype(dtype)} {ch}ch {rate} Hz")


def read_raw(H, path, cap=1 << 20):
    out = np.zeros(cap, np.uint8)
    nb, nfr = C.c_size_t(), C.c_size_t()
    info = (C.c_uint * 3)()
    err = C.create_string_buffer(512)
    rc = H.whh_read_wav_raw(path.encode(), out.ctypes.data, out.size, C.byref(nb), C.byref(nfr), info, err, 512)
    return rc, out[: nb.value], nfr.value, tuple(info), err.value.decode()


def test_read_wav_raw_returns_the_payload_untouched(H, tmp_path):
    rng = np.random.default_rng(77)
    p = str(tmp_path / "r.wav")
    for dtype, fmt in ((np.int16, wb.WH_PCM_S16), (np.uint8, wb.WH_PCM_U8), (np.float32, wb.WH_PCM_F32)):
        for ch, rate in ((1, 8000), (2, 44100), (3, 16000)):
            x = ar.random_clip(rng, dtype, 333, ch)
            ar.write_wav(p, x, rate)
            rc, payload, frames, info, err = read_raw(H, p)
            assert rc == 0, err
            assert frames == 333 and info == (fmt, ch, rate)
            assert payload.tobytes() == x.tobytes()
    # the loader's refusals, with its texts
    import wave
    p24 = str(tmp_path / "s24.wav")
    with wave.open(p24, "wb") as w:
        w.setnchannels(1); w.setsampwidth(3); w.setframerate(16000); w.writeframes(b"\0" * 30)
    rc, _, _, _, err = read_raw(H, p24)
    assert rc == 1 and err == "Unsupported decoded sample format" and load_wav(H, p24, 1)[0] == 1
    rc, _, _, _, err = read_raw(H, "/nonexistent.wav")
    assert rc == 1 and err == "Failed to open audio: /nonexistent.wav" and load_wav(H, "/nonexistent.wav", 1)[0] == 1
    pn = str(tmp_path / "not.wav")
    open(pn, "wb").write(b"OggS" + b"\0" * 64)
    rc, _, _, _, err = read_raw(H, pn)
    assert rc == 1 and err.startswith("Unsupported container (only RIFF/WAVE is decoded here)") and load_wav(H, pn, 1)[0] == 1
    p0 = str(tmp_path / "rate0.wav")
    ar.write_wav(p0, np.zeros((4, 1), np.int16), 0)
    rc, _, _, _, err = read_raw(H, p0)
    assert rc == 1 and err == "Unknown sample rate" and load_wav(H, p0, 1)[0] == 1


def test_raw_clip_helper_builds_the_struct():
    x = np.arange(12, dtype=np.int16).reshape(6, 2)
    buf = np.zeros(64, np.uint8)
    odd = buf[1:1 + 6].view(np.uint8).reshape(6, 1)          # a pointer that is not even 2-byte aligned
    arr, keep = wb.raw_clips([(x, 44100), (odd, 8000), (np.zeros(5, np.float32), 16000)])
    assert (arr[0].n_frames, arr[0].sample_rate, arr[0].channels, arr[0].format) == (6, 44100, 2, wb.WH_PCM_S16)
    assert arr[0].data == x.ctypes.data
    assert arr[1].data == buf.ctypes.data + 1 and arr[1].format == wb.WH_PCM_U8 and arr[1].channels == 1
    assert (arr[2].n_frames, arr[2].channels, arr[2].format) == (5, 1, wb.WH_PCM_F32)
    with pytest.raises(TypeError):
        wb.raw_clips([(np.zeros(4, np.float64), 16000)])


def test_descriptor_packing_program(tmp_path):
    """tools/ingest_pack_check.cpp (alignment, offsets, n_out, a batch past 2^31 bytes) — built plainly here; its header says how to build it
    with the address and undefined-behaviour sanitizers."""
    import subprocess
    exe = str(tmp_path / "ingest_pack_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", os.path.join(ROOT, "tools", "ingest_pack_check.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr
