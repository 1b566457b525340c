"""Sequential long-form on the GPU: the resident file set (wh_files_load), windows cut from it by (file, seek)
(k_mel_window, wh_transcribe_windows) and whisper_bench --sequential.

Every comparison is exact equality.  The references are entries this feature does not touch — wh_log_mel for the mels, wh_transcribe_longform for
fixed windows, the staged wh_encode + wh_decode_greedy, per-row calls for a composed batch — and tests/seq_ref.py for the loop."""
import dataclasses
import functools
import json
import os
import subprocess
import wave

import numpy as np
import pytest

import seq_ref
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
NANO_PROMPT, NANO_EOT = [3, 5, 7], 2
NANO_TB = ms.PRESETS["nano"].vocab - 301
NANO_NOTS, NANO_NOSPEECH, NANO_SOT_PREV = NANO_TB - 1, NANO_TB - 2, NANO_TB - 3
BASE_PROMPT, BASE_EOT = [50258, 50259, 50359], 50257
ERR_EMPTY, ERR_STATE, ERR_ARG = 1, 3, 4


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


@functools.lru_cache(maxsize=None)
def long_pcm():
    """70.3 s: three synthetic clips back to back, cut."""
    return np.concatenate([ms.synth_clip(40), ms.synth_clip(41), ms.synth_clip(42)])[:1124800].copy()


@functools.lru_cache(maxsize=None)
def four_files():
    """1 sample, 0.5 s, exactly 30 s, 70.3 s."""
    x = long_pcm()
    return (x[100000:100001].copy(), ms.synth_clip(43)[:8000].copy(), ms.synth_clip(44), x)


def cut(mel, seek):
    """The window's numpy cut: 3000 frames of the normalised whole-file mel from `seek`, zero-filled past the file's end."""
    out = np.zeros((mel.shape[0], 3000), np.float32)
    k = min(3000, mel.shape[1] - seek)
    out[:, :k] = mel[:, seek:seek + k]
    return out


def bf16_round(x):
    """f32 -> bf16 (round to nearest even) -> f32, as the conv1 operand of the bf16 modes holds it (no NaN here)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u >> 16) & 1) + 0x7FFF
    return ((u + r) & 0xFFFF0000).astype(np.uint32).view(np.float32).reshape(x.shape)


def model_of(kind):
    """nano f32 / nano bf16 / nano with 128 mel bins (large-v3's log-mel geometry, tiny otherwise) f32."""
    if kind == "mels128":
        dims = dataclasses.replace(ms.PRESETS["nano"], n_mels=128)
        return wb.Model.from_weights(dims, ms.flatten_state_dict(dims, ms.synth_state_dict(dims, 7)), 0, wb.WH_PREC_F32)
    return wb.Model("synthetic:nano:7", 0, wb.PRECISIONS[kind])


def seeks_of(frames):
    """Tile-aligned and not, the last tile, the file's last frame, full and one-short windows at the end, fewer than 8 valid frames."""
    return [0, 1, 63, 64, 65, 2999, frames - 1, frames - 3000, frames - 2999, frames - 5]


def params(new=8, prompt=NANO_PROMPT, eot=NANO_EOT):
    return wb.DecodeParams(prompt, new, eot, [eot])      # EOT suppressed: every row runs `new` positions


# ---- 1. the mels ---------------------------------------------------------------------------------------------------------------------------------

def test_file_set_mels_are_wh_log_mel_bit_for_bit(gpu):
    files = four_files()
    ctx = wb.Context(model_of("f32"), 4)
    mels = [ctx.whisper_log_mel(f) for f in files]
    frames = ctx.files_load(files)
    assert frames == [int(ctx.lib.wh_mel_frames(f.size)) for f in files] == [1, 50, 3000, 7030]
    for f, mel in enumerate(mels):
        assert np.array_equal(ctx.files_window_mel(f, 0), cut(mel, 0)), f
    for seek in (3000, 4031, 7029):
        assert np.array_equal(ctx.files_window_mel(3, seek), cut(mels[3], seek)), seek
    ctx.whisper_log_mel(files[2])                                  # another whole-file entry in between: the set is its own buffer
    assert np.array_equal(ctx.files_window_mel(1, 17), cut(mels[1], 17))
    # the raw form: the same samples as a file holds them (f32 mono at 16 kHz converts to itself; int16 stereo at 8 kHz through the ingest kernel)
    st = (np.stack([files[1], -files[1]], 1) * 20000).astype(np.int16)
    assert ctx.files_load_raw([(files[3].reshape(-1, 1), 16000), (st, 8000)]) == [7030, int(ctx.lib.wh_mel_frames(16000))]
    assert np.array_equal(ctx.files_window_mel(0, 4031), cut(mels[3], 4031))
    conv = ctx.ingest_raw([(st, 8000)])[0]                         # (through the raw staging buffer and the one-file PCM buffer: the set stays)
    assert np.array_equal(ctx.files_window_mel(1, 3), cut(ctx.whisper_log_mel(conv), 3))
    ctx.close()


# ---- 2. the window cut ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["f32", "bf16", "mels128"])
def test_window_cut_against_numpy(gpu, kind):
    files = four_files()
    ctx = wb.Context(model_of(kind), 4)
    mels = [ctx.whisper_log_mel(f) for f in files]
    assert mels[3].shape[0] == (128 if kind == "mels128" else 80)
    ctx.files_load(files)
    rnd = bf16_round if kind == "bf16" else (lambda x: x)
    for seek in seeks_of(7030):
        assert np.array_equal(ctx.files_window_mel(3, seek), rnd(cut(mels[3], seek))), seek
    for f, seek in ((0, 0), (1, 0), (1, 43), (1, 49), (2, 0), (2, 2936), (2, 2999)):       # one valid frame; a last valid frame inside a tile
        assert np.array_equal(ctx.files_window_mel(f, seek), rnd(cut(mels[f], seek))), (f, seek)
    # through the decode entry: one file in two rows at different seeks decodes as the two rows alone
    p = params()
    both = ctx.transcribe_windows([(3, 65), (3, 4031)], p)
    assert all(len(t) == len(NANO_PROMPT) + 8 for t in both)
    assert both[0].tolist() != both[1].tolist()
    for row, t in zip([(3, 65), (3, 4031)], both):
        assert ctx.transcribe_windows([row], p)[0].tolist() == t.tolist(), row
    ctx.close()


# ---- 3. the fixed plan's windows -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("preset,prec_name", [("nano", "f32"), ("base", "bf16"), ("base", "fp8")])
def test_rows_at_the_fixed_plan_equal_transcribe_longform(gpu, preset, prec_name):
    x = long_pcm()
    nano = preset == "nano"
    model = wb.Model(f"synthetic:{preset}:{7 if nano else 1234}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, 4)
    p = params(8, NANO_PROMPT if nano else BASE_PROMPT, NANO_EOT if nano else BASE_EOT)
    plan = wb.longform_plan(x.size, 30.0, 5.0)
    assert plan == [0, 400000, 800000]
    want = ctx.transcribe_longform(x, p, 30.0, 5.0)
    ctx.files_load([x])
    got = ctx.transcribe_windows([(0, off // 160) for off in plan], p)
    assert [t.tolist() for t in got] == [t.tolist() for t in want]
    assert len({tuple(t.tolist()) for t in got}) == 3
    ctx.close()


# ---- 4. staged -----------------------------------------------------------------------------------------------------------------------------------

def test_rows_equal_the_staged_calls(gpu):
    files = four_files()
    ctx = wb.Context(model_of("f32"), 4)
    ctx.files_load(files)
    p = params()
    rows = [(3, s) for s in seeks_of(7030)]
    pre = [[], [NANO_SOT_PREV, 11], [NANO_SOT_PREV, 12, 13, 14, 15]]
    for at in range(0, len(rows), 4):
        group = rows[at:at + 4]
        prefixes = [pre[(at + i) % 3] for i in range(len(group))]
        ctx.set_prefixes(prefixes)
        got = ctx.transcribe_windows(group, p)
        for row, pf, t in zip(group, prefixes, got):
            mel = ctx.files_window_mel(*row)
            ctx.run_encoder(mel, want_output=False)
            ctx.set_prefixes([pf])
            staged, _ = ctx.greedy_decode_with_past(p)
            assert staged.tolist() == t.tolist(), (row, pf)
    ctx.close()


# ---- 5. composition ------------------------------------------------------------------------------------------------------------------------------

def test_options_compose_as_in_the_per_row_calls(gpu):
    files = four_files()
    ctx = wb.Context(model_of("f32"), 4)
    frames = ctx.files_load(files)
    ctx.set_timestamp_rules(NANO_TB, NANO_NOTS, 50)
    ctx.set_logprobs(NANO_NOSPEECH, 0)
    ctx.set_alignment([(1, 0), (1, 1), (0, 1)])
    p = wb.DecodeParams(NANO_PROMPT, 10, NANO_EOT)
    rows = [(1, 3), (2, 1000), (3, 6900)]
    pre = [[], [NANO_SOT_PREV, 21], [NANO_SOT_PREV, 31, 32, 33, 34]]

    def run(rr, pp):
        ctx.set_prefixes(pp)
        toks = ctx.transcribe_windows(rr, p)
        lps, ns = ctx.logprobs()
        fr, nfr = ctx.token_frames()
        return [t.tolist() for t in toks], [l.tolist() for l in lps], ns.tolist(), [f.tolist() for f in fr], nfr.tolist()

    toks, lps, ns, fr, nfr = run(rows, pre)
    assert nfr == [min(1500, max(8, (min(3000, frames[f] - s) + 1) // 2)) for f, s in rows] == [24, 1000, 65]
    for i, (row, pf) in enumerate(zip(rows, pre)):
        t1, l1, n1, f1, nf1 = run([row], [pf])
        assert (t1[0], l1[0], n1[0], f1[0], nf1[0]) == (toks[i], lps[i], ns[i], fr[i], nfr[i]), row
    assert all(NANO_TB <= t[len(NANO_PROMPT)] <= NANO_TB + 50 for t in toks)          # the rules are on: a first timestamp within 1 s
    ctx.close()


# ---- 6. decoding the resident rows again ---------------------------------------------------------------------------------------------------------

def test_resident_rows_decode_again(gpu):
    ctx = wb.Context(model_of("f32"), 4)
    ctx.files_load(four_files())
    p = params(12)
    rows = [(3, 100), (2, 0), (3, 5000)]
    first = [t.tolist() for t in ctx.transcribe_windows(rows, p)]
    again, _ = ctx.greedy_decode_resident_batch(p)
    assert [t.tolist() for t in again] == first
    ctx.set_sampling(9, [0.0, 1.0, 0.0], row_ids=[5, 6, 7])
    sampled, _ = ctx.greedy_decode_resident_batch(p)
    ctx.clear_sampling()
    assert sampled[0].tolist() == first[0] and sampled[2].tolist() == first[2]
    assert sampled[1].tolist() != first[1]                         # 12 draws at temperature 1 over a flat 1024-id distribution
    ctx.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_context_usable(gpu):
    files = four_files()
    ctx = wb.Context(model_of("f32"), 2)
    p = params()

    def refused(code, call):
        with pytest.raises(wb.WhisperHipError) as e:
            call()
        assert e.value.code == code, e.value
        assert len(ctx.transcribe_batch([files[1]], p)[0]) == len(NANO_PROMPT) + 8       # the context decodes normally afterwards

    refused(ERR_STATE, lambda: ctx.transcribe_windows([(0, 0)], p))
    refused(ERR_STATE, lambda: ctx.files_window_mel(0, 0))
    assert ctx.files_load([files[1], files[2]]) == [50, 3000]
    want = ctx.transcribe_windows([(1, 10)], p)[0].tolist()
    refused(ERR_ARG, lambda: ctx.transcribe_windows([(2, 0)], p))
    refused(ERR_ARG, lambda: ctx.transcribe_windows([(-1, 0)], p))
    refused(ERR_ARG, lambda: ctx.transcribe_windows([(0, 50)], p))
    refused(ERR_ARG, lambda: ctx.transcribe_windows([(0, -1)], p))
    refused(ERR_ARG, lambda: ctx.transcribe_windows([(0, 0), (1, 0), (1, 1)], p))      # more rows than max_batch
    refused(ERR_ARG, lambda: ctx.transcribe_windows([], p))
    refused(ERR_EMPTY, lambda: ctx.files_load([files[1], files[1][:0]]))
    assert ctx.transcribe_windows([(1, 10)], p)[0].tolist() == want                     # the old set is still there
    ctx.set_prefixes([[NANO_SOT_PREV, 4]])
    refused(ERR_ARG, lambda: ctx.transcribe_windows([(0, 0), (1, 0)], p))               # one prefix, two rows
    ctx.clear_prefixes()
    assert ctx.files_load([]) == []
    refused(ERR_STATE, lambda: ctx.transcribe_windows([(1, 10)], p))
    ctx.close()


# ---- 8, 9. the loop end to end -------------------------------------------------------------------------------------------------------------------
# Seed and --max-new-tokens were picked on the GPU from seq_ref's own run (the Python loop below), so that it shows both kinds of advance:
# seed 7 with 12 new tokens gives (advance, window frames) = (582, 3000), (3000, 3000), (562, 2918), (562, 2356), (1794, 1794) for the 65 s
# file, (582, 3000), (562, 2518), (596, 1956), (1360, 1360) for the 31 s file and (562, 400) for the 4 s file — advances taken from a timestamp
# pair, whole-window advances (window 1 of the first file, and the last windows, cut at max_new_tokens before a pair), and one beyond its
# window at a file's end.  (Seeds 7, 11 and 3 at 20 or 32 new tokens show no whole-window advance inside a file; 8 new tokens show one.)
CLI_SEED, CLI_NEW = 7, 12
SPECIAL = {NANO_EOT: "<|endoftext|>", 3: "<|startoftranscript|>", 5: "<|en|>", 7: "<|transcribe|>", NANO_NOTS: "<|notimestamps|>", NANO_NOSPEECH: "<|nospeech|>",
           NANO_SOT_PREV: "<|startofprev|>", NANO_TB: "<|0.00|>"}


def write_wav(path, x):
    q = np.clip(np.round(x * 32767.0), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(16000)
        w.writeframes(q.tobytes())
    return q.astype(np.float32) / np.float32(32768.0)              # what the loader reads back


def cli_inputs(tmp):
    adir = tmp / "audio"
    adir.mkdir()
    c = [wb.cli_synthetic_clip(300 + i) for i in range(3)]
    clips = {"a65.wav": np.concatenate(c)[:1040000], "b31.wav": np.concatenate(c[1:])[:496000], "c04.wav": c[2][200000:264000]}
    pcm = [write_wav(str(adir / k), v) for k, v in sorted(clips.items())]
    vocab = {f"Ġt{i}": i for i in range(ms.PRESETS["nano"].vocab) if i not in SPECIAL}
    tokj = tmp / "tokenizer.json"
    tokj.write_text(json.dumps({"model": {"vocab": vocab}, "added_tokens": [{"id": i, "content": s, "special": True} for i, s in SPECIAL.items()]}))
    return adir, tokj, pcm


def run_cli(tmp, tag, adir, tokj, extra):
    out = tmp / tag
    r = subprocess.run([CLI, "--sequential", "--audio-dir", str(adir), "--onnx-dir", f"synthetic:nano:{CLI_SEED}", "--tokenizer-json", str(tokj), "--precision", "f32",
                        "--max-new-tokens", str(CLI_NEW), "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json")] + extra,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = json.loads((out / "p.json").read_text())
    assert [x["file"] for x in rows] == ["a65.wav", "b31.wav", "c04.wav"]
    return rows


def text_of(ids):
    return " ".join(f"t{i}" for i in ids if i < NANO_TB and i not in SPECIAL)


def test_cli_sequential_follows_the_reference_loop(gpu, tmp_path):
    adir, tokj, pcm = cli_inputs(tmp_path)
    ctx = wb.Context(wb.Model(f"synthetic:nano:{CLI_SEED}", 0, wb.WH_PREC_F32), 4)
    ctx.set_timestamp_rules(NANO_TB, NANO_NOTS, 50)
    frames = ctx.files_load(pcm)
    assert frames == [6500, 3100, 400]
    p = wb.DecodeParams(NANO_PROMPT, CLI_NEW, NANO_EOT)

    def step(rows):
        ctx.set_prefixes([r["prefix"] for r in rows])
        toks = ctx.transcribe_windows([(r["file"], r["seek"]) for r in rows], p)
        return [{"tokens": t[len(NANO_PROMPT):].tolist()} for t in toks]

    want = seq_ref.run_sequential(frames, step, NANO_TB, NANO_EOT, NANO_SOT_PREV, 448, len(NANO_PROMPT), CLI_NEW)
    ctx.close()
    adv = [(w["advance"], w["seg_frames"]) for f in want["files"] for w in f["windows"]]
    print("reference loop: (advance, seg_frames) per window:", adv)
    assert any(a != s for a, s in adv) and any(a == s for a, s in adv)       # the coverage condition, on the reference loop's own output
    assert any(len(w["prefix"]) > 1 for f in want["files"] for w in f["windows"])

    rows4 = run_cli(tmp_path, "mb4", adir, tokj, ["--max-batch", "4"])
    for row, ref in zip(rows4, want["files"]):
        assert len(row["windows"]) == len(ref["windows"]), row["file"]
        for got, w in zip(row["windows"], ref["windows"]):
            assert got["seek_s"] == w["seek"] * 0.01 and got["frames"] == w["seg_frames"] and got["advance_s"] == w["advance"] * 0.01, (row["file"], got, w)
            assert got["tokens"] == w["tokens"] and got["skipped"] is False and got["temperature"] == 0
        segs = [(s["start"], s["end"], text_of(s["ids"])) for s in ref["segments"]]
        assert [(s["start"], s["end"], s["text"]) for s in row["segments"]] == [s for s in segs if s[2]], row["file"]
        assert row["text"] == " ".join(s[2] for s in segs if s[2])
    rows1 = run_cli(tmp_path, "mb1", adir, tokj, ["--max-batch", "1"])
    for a, b in zip(rows1, rows4):
        assert (a["windows"], a["segments"], a["text"]) == (b["windows"], b["segments"], b["text"]), a["file"]
    skipped = run_cli(tmp_path, "skip", adir, tokj, ["--max-batch", "4", "--no-speech-threshold", "0", "--logprob-threshold", "0"])
    for row, nf in zip(skipped, frames):
        assert all(w["skipped"] and w["advance_s"] == w["frames"] * 0.01 for w in row["windows"]) and len(row["windows"]) == -(-nf // 3000)
        assert row["segments"] == [] if "segments" in row else True
        assert row["text"] == ""


def test_cli_ladder_runs_on_multi_window_files(gpu, tmp_path):
    adir, tokj, _ = cli_inputs(tmp_path)
    ladder = ["--temperature", "0,0.4", "--compression-ratio-threshold", "0.05"]          # every window's ratio exceeds it: every window falls back
    rows4 = run_cli(tmp_path, "mb4", adir, tokj, ["--max-batch", "4"] + ladder)
    rows1 = run_cli(tmp_path, "mb1", adir, tokj, ["--max-batch", "1"] + ladder)
    plain = run_cli(tmp_path, "plain", adir, tokj, ["--max-batch", "4"])
    assert len(rows4[0]["windows"]) >= 3
    for a, b in zip(rows1, rows4):
        assert all(w["temperature"] == 0.4 for w in b["windows"]) and b["temperature"] == 0.4
        assert a["windows"] == b["windows"], a["file"]                                    # a row's random stream is (file, window): no --max-batch in it
    assert [w["tokens"] for w in rows4[0]["windows"]] != [w["tokens"] for w in plain[0]["windows"]]
