"""Raw-audio ingest on the GPU (wh_ingest_raw, wh_transcribe_batch_raw*, wh_transcribe_longform_raw, whisper_bench --gpu-ingest; DESIGN.md
§5o).  Run with -m gpu.  The reference is tests/audio_ref.py (pinned to the host loader by tests/test_ingest_cpu.py), never the kernel:
the converted rows are compared as uint32, and everything downstream must equal the f32 entries on the restatement's samples exactly — the
same PCM bits go through the same kernels.

A note on -0.0: the definition starts every frame's sum at +0.0f, so a -0.0 sample of a 16 kHz mono clip comes back as +0.0 — from the host
loader, from the restatement and from the kernel alike; NaN and the infinities come back with the bits they went in with."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import audio_ref as ar
from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
SPEC = "synthetic:nano:7"
B, NEW = 64, 8
PROMPT, EOT = [3, 5, 7, 9], 2
DTYPES = (np.int16, np.uint8, np.float32)
CHANNELS = (1, 2, 3, 6)
RATES = (8000, 11025, 15999, 16000, 16001, 22050, 44100, 48000, 96000)
FRAMES = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 4097)
EMPTY_AUDIO, ERR_ARG = 1, 4


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


_ctx = {}


def ctx_of(prec):
    if prec not in _ctx:
        _ctx[prec] = wb.Context(wb.Model(SPEC, 0, wb.PRECISIONS[prec]), B)
    return _ctx[prec]


def params():
    return wb.DecodeParams(PROMPT, NEW, EOT)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_rows_equal(got, clips, what=""):
    assert len(got) == len(clips)
    for i, (g, (x, r)) in enumerate(zip(got, clips)):
        want = ar.ingest(x, r)
        assert len(g) == len(want), (what, i, x.dtype, x.shape, r, len(g), len(want))
        bad = np.flatnonzero(bits(g) != bits(want))
        assert bad.size == 0, (what, i, x.dtype, x.shape, r, bad[:4], g[bad[:4]], want[bad[:4]])


def derived_clip(k, dtype, channels, rate, seconds):
    """Clip content with some structure: the synthetic clip k read as `rate` Hz audio, a second / third channel of other gains."""
    n = int(seconds * rate)
    src = np.resize(ms.synth_clip(1700 + k), n).astype(np.float32)
    chans = np.stack([src * np.float32(1.0 - 0.3 * c) for c in range(channels)], axis=1)
    if np.dtype(dtype) == np.int16:
        return np.clip(np.round(chans * 32767.0), -32768, 32767).astype(np.int16)
    if np.dtype(dtype) == np.uint8:
        return np.clip(np.round(chans * 127.0 + 128.0), 0, 255).astype(np.uint8)
    return np.ascontiguousarray(chans, np.float32)


def mixed_clips(base):
    spec = [(np.int16, 2, 44100, 3.1), (np.uint8, 1, 8000, 7.3), (np.float32, 3, 22050, 1.7), (np.int16, 1, 16000, 12.0), (np.float32, 6, 48000, 0.9)]
    return [(derived_clip(base + i, d, ch, r, s), r) for i, (d, ch, r, s) in enumerate(spec)]


def host_converted(clips):
    return [ar.ingest(x, r) for x, r in clips]


def test_rows_are_bit_exact_over_the_grid(gpu):
    """Ladder 1: every (format, channels, rate, frames) of the grid, packed into mixed batches of up to 64 in a shuffled order so formats, rates
    and lengths differ within one call; the 4 (rate, frames) pairs that resample to nothing are sent alone and refused."""
    ctx = ctx_of("bf16")
    rng = np.random.default_rng(1234)
    clips, empty = [], []
    for d in DTYPES:
        for ch in CHANNELS:
            for r in RATES:
                for f in FRAMES:
                    (empty if ar.n_out(f, r) == 0 else clips).append((ar.random_clip(rng, d, f, ch), r))
    assert {(x.shape[0], r) for x, r in empty} == {(1, 44100), (1, 48000), (1, 96000), (2, 96000)}
    assert len(empty) == 4 * len(DTYPES) * len(CHANNELS) and len(clips) + len(empty) == 1080
    for c in empty:
        with pytest.raises(wb.WhisperHipError) as e:
            ctx.ingest_raw([c])
        assert e.value.code == EMPTY_AUDIO
    order = rng.permutation(len(clips))
    for b0 in range(0, len(order), B):
        batch = [clips[i] for i in order[b0:b0 + B]]
        assert_rows_equal(ctx.ingest_raw(batch), batch, f"batch at {b0}")


def test_odd_byte_counts_and_unaligned_host_pointers(gpu):
    """Ladder 2: odd byte counts in front of wider formats, every host pointer one byte past an aligned address."""
    ctx = ctx_of("bf16")
    rng = np.random.default_rng(5)
    shapes = [(np.uint8, 1, 1), (np.int16, 3, 2), (np.uint8, 5, 3), (np.float32, 7, 1)]
    clips, keep = [], []
    for d, f, ch in shapes:
        x = ar.random_clip(rng, d, f, ch)
        buf = np.zeros(x.nbytes + 64, np.uint8)
        base = (-buf.ctypes.data) % 16 + 1                       # 16-byte aligned + 1
        buf[base:base + x.nbytes] = np.frombuffer(x.tobytes(), np.uint8)
        view = np.ndarray(x.shape, x.dtype, buffer=buf, offset=base)
        assert view.ctypes.data % 16 == 1 and view.flags.c_contiguous
        keep.append(buf)
        clips.append((view, 16000 if d is np.float32 else 22050))
    assert_rows_equal(ctx.ingest_raw(clips), [(np.array(v), r) for v, r in clips], "odd placement")


def test_non_finite_f32_passes_through(gpu):
    """Ladder 3: 16 kHz mono f32 is not interpolated."""
    ctx = ctx_of("bf16")
    x = np.array([np.nan, np.inf, -np.inf, -0.0, 0.5, 1e-30, -3.0e38], np.float32)
    got = ctx.ingest_raw([(x, 16000), (x[:3], 16000)])[0]
    np.testing.assert_array_equal(bits(got), bits(ar.ingest(x, 16000)))
    np.testing.assert_array_equal(bits(got)[:3], bits(x)[:3])        # NaN and the infinities: the input's bits
    assert bits(got)[3] == 0                                         # -0.0: 0.0f + -0.0f (see the module docstring)
    np.testing.assert_array_equal(bits(got)[4:], bits(x)[4:])


def test_full_window_lengths(gpu):
    """Ladder 4: the lengths around one 30 s window."""
    ctx = ctx_of("bf16")
    rng = np.random.default_rng(99)
    full = [(ar.random_clip(rng, np.int16, 1440000, 2), 48000), (ar.random_clip(rng, np.int16, 1440001, 2), 48000),
            (ar.random_clip(rng, np.int16, 1323000, 1), 44100)]
    got = ctx.ingest_raw(full)
    assert [len(g) for g in got] == [480000] * 3
    assert_rows_equal(got, full, "full window")
    over = (np.zeros((1440002, 2), np.int16), 48000)                 # 480001 samples: one too many for a batch entry
    with pytest.raises(wb.WhisperHipError) as e:
        ctx.transcribe_batch_raw([over], params())
    assert e.value.code == ERR_ARG and "longform" in str(e.value)
    with pytest.raises(wb.WhisperHipError) as e:
        ctx.ingest_raw([over, full[2]])
    assert e.value.code == ERR_ARG
    clips = mixed_clips(0)
    want = ctx.transcribe_batch(host_converted(clips), params())
    got = ctx.transcribe_batch_raw(clips, params())
    assert [t.tolist() for t in got] == [t.tolist() for t in want]


@pytest.mark.parametrize("prec", ["bf16", "f32"])
def test_transcription_equals_the_host_path(gpu, prec):
    """Ladder 5."""
    ctx = ctx_of(prec)
    clips = mixed_clips(10)
    host = host_converted(clips)
    want = ctx.transcribe_batch(host, params())
    got = ctx.transcribe_batch_raw(clips, params())
    assert [t.tolist() for t in got] == [t.tolist() for t in want]
    assert any(len(t) > len(PROMPT) for t in got)
    # once more with the timestamp rules and the log-probabilities on
    prompt, eot, tb, nots = setup("nano")
    p = wb.DecodeParams(prompt, NEW, eot)
    ctx.set_timestamp_rules(tb, nots)
    ctx.set_logprobs()
    try:
        want = ctx.transcribe_batch(host, p)
        want_lp, _ = ctx.logprobs()
        got = ctx.transcribe_batch_raw(clips, p)
        got_lp, _ = ctx.logprobs()
    finally:
        ctx.clear_timestamp_rules()
        ctx.clear_logprobs()
    assert [t.tolist() for t in got] == [t.tolist() for t in want]
    assert len(got_lp) == len(want_lp) == len(clips)
    for a, b in zip(got_lp, want_lp):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_prefetch_hits_misses_and_mixing_with_the_f32_entries(gpu):
    """Ladder 6."""
    ctx = ctx_of("bf16")
    p = params()
    A, Bc, Cc, Dc = mixed_clips(20), mixed_clips(30)[:4], mixed_clips(40)[:3], mixed_clips(50)
    plain = {k: [t.tolist() for t in ctx.transcribe_batch_raw(v, p)] for k, v in (("A", A), ("B", Bc), ("C", Cc))}
    assert [t.tolist() for t in ctx.transcribe_batch_raw(A, p, next_clips=Bc)] == plain["A"]
    assert [t.tolist() for t in ctx.transcribe_batch_raw(Bc, p, next_clips=Cc)] == plain["B"]      # a hit
    assert [t.tolist() for t in ctx.transcribe_batch_raw(Cc, p, prefetch=True)] == plain["C"]      # a hit, nothing announced
    # a miss: the same first pointer, clip 1 announced at another rate
    x1, r1 = Bc[1]
    B2 = [Bc[0], (x1, 16000 if r1 != 16000 else 8000)] + Bc[2:]
    want_B2 = [t.tolist() for t in ctx.transcribe_batch_raw(B2, p)]
    assert [t.tolist() for t in ctx.transcribe_batch_raw(A, p, next_clips=Bc)] == plain["A"]
    assert [t.tolist() for t in ctx.transcribe_batch_raw(B2, p, prefetch=True)] == want_B2
    # the two families on one context: a pending f32 prefetch, then a raw call, then a plain f32 call
    Af, Bf, Df = host_converted(A), host_converted(Bc), host_converted(Dc)
    want_D = [t.tolist() for t in ctx.transcribe_batch(Df, p)]
    assert [t.tolist() for t in ctx.transcribe_batch_next(Af, p, Bf)] == plain["A"]
    assert [t.tolist() for t in ctx.transcribe_batch_raw(Cc, p)] == plain["C"]
    assert [t.tolist() for t in ctx.transcribe_batch(Df, p)] == want_D
    # ... and the other way round: a pending raw prefetch, then the f32 pipelined entry
    assert [t.tolist() for t in ctx.transcribe_batch_raw(A, p, next_clips=Bc)] == plain["A"]
    assert [t.tolist() for t in ctx.transcribe_batch_next(Df, p, None)] == want_D
    assert [t.tolist() for t in ctx.transcribe_batch_raw(Bc, p, prefetch=True)] == plain["B"]


def test_longform_raw_equals_longform_on_the_host_conversion(gpu):
    """Ladder 7: 70 s of 22.05 kHz stereo S16."""
    ctx = ctx_of("bf16")
    x = derived_clip(60, np.int16, 2, 22050, 70.0)
    host = ar.ingest(x, 22050)
    assert len(host) == 70 * 16000
    want = ctx.transcribe_longform(host, params())
    got = ctx.transcribe_longform_raw(x, 22050, params())
    assert len(got) == len(want) == len(wb.longform_plan(len(host))) == 3
    assert [t.tolist() for t in got] == [t.tolist() for t in want]
    np.testing.assert_array_equal(bits(ctx.ingest_raw([(x, 22050)])[0]), bits(host))   # the whole-file conversion itself


def test_refusals_leave_the_context_usable(gpu):
    """Ladder 8."""
    ctx = ctx_of("bf16")
    lib = ctx.lib
    good = mixed_clips(70)[:2]
    want = [t.tolist() for t in ctx.transcribe_batch_raw(good, params())]
    x = np.zeros((100, 1), np.int16)
    ok = dict(data=x.ctypes.data, n_frames=100, sample_rate=16000, channels=1, format=wb.WH_PCM_S16)
    cases = [(dict(ok, data=None), ERR_ARG), (dict(ok, format=3), ERR_ARG), (dict(ok, channels=0), ERR_ARG), (dict(ok, channels=65), ERR_ARG),
             (dict(ok, sample_rate=0), ERR_ARG), (dict(ok, sample_rate=768001), ERR_ARG), (dict(ok, n_frames=0), EMPTY_AUDIO),
             (dict(ok, n_frames=1, sample_rate=48000), EMPTY_AUDIO)]
    p, keep = params().to_c()
    stride = len(PROMPT) + NEW
    toks = np.zeros((B + 1, stride), np.int64)
    n = (C.c_size_t * (B + 1))()
    out = np.zeros((2, 100), np.float32)
    f32p = out.ctypes.data_as(C.POINTER(C.c_float))
    i64p = toks.ctypes.data_as(C.POINTER(C.c_int64))
    for fields, code in cases:
        arr = (wb.WhRawClip * 1)(wb.WhRawClip(**fields))
        assert lib.wh_ingest_raw(ctx.h, arr, 1, f32p, 100, n) == code, fields
        assert lib.wh_transcribe_batch_raw(ctx.h, arr, 1, C.byref(p), i64p, n) == code, fields
        assert lib.wh_transcribe_batch_raw_next(ctx.h, arr, 1, None, 0, C.byref(p), i64p, n) == code, fields
        got = C.c_size_t(0)
        assert lib.wh_transcribe_longform_raw(ctx.h, arr, 30.0, 5.0, C.byref(p), i64p, n, B, C.byref(got)) == code, fields
        assert [t.tolist() for t in ctx.transcribe_batch_raw(good, params())] == want
    one = (wb.WhRawClip * 1)(wb.WhRawClip(**ok))
    many = (wb.WhRawClip * (B + 1))(*[wb.WhRawClip(**ok)] * (B + 1))
    assert lib.wh_ingest_raw(ctx.h, one, 0, f32p, 100, n) == ERR_ARG
    assert lib.wh_ingest_raw(ctx.h, many, B + 1, f32p, 100, n) == ERR_ARG
    assert lib.wh_transcribe_batch_raw(ctx.h, many, B + 1, C.byref(p), i64p, n) == ERR_ARG
    assert lib.wh_transcribe_batch_raw(ctx.h, one, 0, C.byref(p), i64p, n) == ERR_ARG
    assert lib.wh_ingest_raw(ctx.h, one, 1, f32p, 99, n) == ERR_ARG                    # cap_samples too small
    bad_next = (wb.WhRawClip * 1)(wb.WhRawClip(**dict(ok, channels=0)))
    assert lib.wh_transcribe_batch_raw_next(ctx.h, one, 1, bad_next, 1, C.byref(p), i64p, n) == ERR_ARG
    assert [t.tolist() for t in ctx.transcribe_batch_raw(good, params())] == want
    assert lib.wh_ingest_raw(ctx.h, one, 1, f32p, 100, n) == 0 and n[0] == 100 and not out[0].any()


def test_cli_gpu_ingest_prints_what_the_host_path_prints(gpu, tmp_path):
    """Ladder 9: whisper_bench with and without --gpu-ingest on the same directory."""
    adir = tmp_path / "audio"
    adir.mkdir()
    files = {"a_s16_44k.wav": (np.int16, 2, 44100, 2.5), "b_u8_8k.wav": (np.uint8, 1, 8000, 4.0), "c_f32_44k.wav": (np.float32, 1, 44100, 1.2),
             "d_long_u8_8k.wav": (np.uint8, 1, 8000, 41.0), "e_s16_8k.wav": (np.int16, 3, 8000, 6.0), "f_f32_8k.wav": (np.float32, 2, 8000, 3.3)}
    for k, (name, (d, ch, r, s)) in enumerate(files.items()):
        ar.write_wav(str(adir / name), derived_clip(80 + k, d, ch, r, s), r)
    res = {}
    for tag, flags in (("host", []), ("gpu", ["--gpu-ingest"])):
        out = tmp_path / tag
        r = subprocess.run([CLI, "--audio-dir", str(adir), "--onnx-dir", "synthetic:base:1234", "--max-new-tokens", "8", "--max-batch", "4", "--timestamp-rules",
                            "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json")] + flags,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        res[tag] = (json.loads((out / "p.json").read_text()), json.loads((out / "s.json").read_text()))
    rows_h, rows_g = res["host"][0], res["gpu"][0]
    assert [x["file"] for x in rows_h] == sorted(files) and len(rows_g) == len(rows_h)
    for a, b in zip(rows_h, rows_g):
        for key in ("file", "duration_s", "text", "segments"):
            assert a[key] == b[key], (a["file"], key, a[key], b[key])
    assert next(x for x in rows_h if x["file"] == "d_long_u8_8k.wav")["duration_s"] == 41.0
    sum_h, sum_g = res["host"][1], res["gpu"][1]
    assert "gpu_ingest" not in sum_h and sum_g["gpu_ingest"] is True
    assert set(sum_g) == set(sum_h) | {"gpu_ingest"}
    timing = {"latency_end_to_end_s", "breakdown_s", "rtf_end_to_end", "rtfx_end_to_end"}
    gpu_timing = {"wall_s", "throughput_rtfx", "gpu_busy_s", "gpu_throughput_rtfx"}
    for key in set(sum_h) - timing - {"gpu"}:
        assert sum_h[key] == sum_g[key], key
    assert set(sum_h["gpu"]) == set(sum_g["gpu"])
    for key in set(sum_h["gpu"]) - gpu_timing:
        assert sum_h["gpu"][key] == sum_g["gpu"][key], key
