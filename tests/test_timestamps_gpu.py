"""Whisper's timestamp rules in the GPU token loop (wh_ctx_set_timestamp_rules), held to the numpy restatement in
tests/timestamp_rules_ref.py: the emitted tokens follow the rules on the logits the kernels computed, the rules leave the logits
bit-identical, the f32 mode agrees with the CPU oracle, and the entries / CLI built on top keep their contracts.  Run with -m gpu."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import timestamp_rules_ref as tr
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
BASE_PROMPT, BASE_EOT, BASE_TB, BASE_NOTS = [50258, 50259, 50359], 50257, 50364, 50363
MARGIN = 1e-4   # |lse_ts - max_text| below this: step 5 is decided by rounding, not counted


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def setup(preset):
    """(prompt, eot, tb, no_timestamps) of a preset: the multilingual ids for base / large-v3, a timestamp block of 301 ids at the top of
    the small vocabularies."""
    d = ms.PRESETS[preset]
    if d.vocab > 50400:
        return BASE_PROMPT, BASE_EOT, BASE_TB, BASE_NOTS
    tb = d.vocab - 301
    return [3, 5, 7], 2, tb, tb - 1


def check_rows(toks, logits, rows, P, tb, eot, nots, max_init=50, suppress=(), begin_suppress=()):
    """Every generated position of the given rows: the restatement on the returned logits and the fed history picks the emitted token.
    Returns (positions checked, positions inside MARGIN)."""
    n, near = 0, 0
    for j, r in enumerate(rows):
        gen = [int(t) for t in toks[r][P:]]
        assert len(logits[j]) == len(gen)
        for i, t in enumerate(gen):
            ref, lse, mt = tr.apply_rules(logits[j][i], gen[:i], tb, eot, nots, max_init, suppress, begin_suppress)
            if abs(lse - mt) < MARGIN:
                near += 1
                continue
            assert ref == t, (r, i, gen[: i + 1], ref, lse, mt)
            n += 1
    return n, near


CONFIGS = [   # (preset, precision, clips, WH_LM_TILE_MIN_ROWS): the LM-head kernel each configuration runs
    ("nano", "f32", 1, "256"), ("nano", "f32", 64, "256"),           # k_lm_head<float>
    ("micro", "f16x3", 1, "256"), ("micro", "f16x3", 64, "256"),     # k_lm_head<h2>
    ("base", "bf16", 512, "256"), ("base", "bf16", 512, "0"),        # k_lm_head_tile | k_lm_head<bf16>
    ("base", "fp8", 512, "256"), ("base", "fp8", 512, "0"),
    ("base", "f16x3", 512, "256"),                                   # k_lm_head_tile_x3
    ("large-v3", "bf16", 32, "256"),                                 # K = 1280
]


@pytest.mark.parametrize("preset,prec_name,nb,tile_rows", CONFIGS)
def test_kernel_follows_the_rules(gpu, monkeypatch, preset, prec_name, nb, tile_rows):
    monkeypatch.setenv("WH_LM_TILE_MIN_ROWS", tile_rows)
    prompt, eot, tb, nots = setup(preset)
    model = wb.Model(f"synthetic:{preset}:{7 if preset == 'nano' else 11 if preset == 'micro' else 1234}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    ctx.set_timestamp_rules(tb, nots, 50)
    clips = [ms.synth_clip(1500 + (i % 16)) for i in range(nb)]
    P, total, near = len(prompt), 0, 0
    for max_init, suppress in ((50, [eot]), (-1, [])):   # EOT suppressed: every position runs; then EOT allowed, no first-token bound
        ctx.set_timestamp_rules(tb, nots, max_init)
        p = wb.DecodeParams(prompt, 24, eot, suppress)
        ctx.transcribe_batch(clips, p)
        rows = sorted({0, nb // 2, nb - 1} | set(range(0, nb, max(1, nb // 8))))
        toks, lg = ctx.greedy_decode_resident_rows(p, rows)
        n, k = check_rows(toks, lg, rows, P, tb, eot, nots, max_init, suppress)
        total, near = total + n, near + k
        assert all(tb <= int(t[P]) <= (tb + 50 if max_init == 50 else model.dims.vocab - 1) for t in toks)
    print(f"{preset} {prec_name} {nb} clips (WH_LM_TILE_MIN_ROWS={tile_rows}): {total} positions follow the rules, {near} inside {MARGIN}")
    assert total > 0 and near <= max(3, total // 200)
    ctx.close()


@pytest.mark.parametrize("prec_name,nb", [("bf16", 512), ("f16x3", 64)])
def test_rules_leave_the_logits_bit_identical(gpu, prec_name, nb):
    """One forced history F (a rules-on row's own output, so it holds timestamp pairs) in both runs: every compared row's logits are
    bit-identical with the rules on and off, and the rules-on argmax at each step is the restatement on those logits and F."""
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    clips = [ms.synth_clip(1600 + (i % 16)) for i in range(nb)]
    ctx.set_timestamp_rules(tb, nots, 50)
    free = ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 20, eot, [eot]))
    pairs = lambda F: sum(1 for a, b in zip(F, F[1:]) if a >= tb and b >= tb)
    F = max(([int(t) for t in f[len(prompt):]] for f in free[:64]), key=pairs)
    assert pairs(F) >= 1, F
    rows = list(range(0, nb, max(1, nb // 64)))
    p = wb.DecodeParams(prompt, len(F), eot, [eot], forced=F)
    on_t, on_l = ctx.greedy_decode_resident_rows(p, rows)
    ctx.clear_timestamp_rules()
    off_t, off_l = ctx.greedy_decode_resident_rows(p, rows)
    for j, r in enumerate(rows):
        assert np.array_equal(on_l[j], off_l[j]), r
        gen = [int(t) for t in on_t[r][len(prompt):]]
        for i, t in enumerate(gen):
            ref, lse, mt = tr.apply_rules(on_l[j][i], F[:i], tb, eot, nots, 50, [eot])
            assert ref == t or abs(lse - mt) < MARGIN, (r, i, ref, t)
    ctx.close()


@pytest.mark.parametrize("preset,seed,clip", [("nano", 7, 0), ("micro", 11, 2), ("base", 1234, 0)])
def test_f32_rules_agree_with_the_oracle(gpu, preset, seed, clip):
    """f32 mode: under the GPU's own rules-on history, the oracle's logits are within 1e-3 and the restatement on them makes the same
    choice wherever the deciding margin exceeds 2e-3 (base: the golden vectors' clip 0, tests/golden/base_s1234_c0.npz)."""
    prompt, eot, tb, nots = setup(preset)
    dims = ms.PRESETS[preset]
    model = wb.Model(f"synthetic:{preset}:{seed}", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 1)
    ctx.set_timestamp_rules(tb, nots, 50)
    pcm = ms.synth_clip(clip)
    ctx.transcribe_batch([pcm], wb.DecodeParams(prompt, 24, eot, [eot]))
    toks, lg = ctx.greedy_decode_resident_batch(wb.DecodeParams(prompt, 24, eot, [eot]), want_logits=True)
    gen = [int(t) for t in toks[0][len(prompt):]]
    w = ms.flatten_state_dict(dims, ms.synth_state_dict(dims, seed))
    enc = orc.encoder(dims, w, orc.window_mel(orc.log_mel(pcm, dims.n_mels), 0, 3000))
    _, ref_l = orc.decode_greedy(dims, w, enc, prompt, len(gen), eot, [eot], forced=gen, want_logits=True)
    assert np.abs(np.asarray(ref_l)[: len(gen)] - lg[0]).max() < 1e-3
    decided = 0
    for i, t in enumerate(gen):
        ref, lse, mt = tr.apply_rules(ref_l[i], gen[:i], tb, eot, nots, 50, [eot])
        x = np.where(tr.rule_mask(dims.vocab, gen[:i], tb, eot, nots, 50, [eot]), np.asarray(ref_l[i], np.float64), -np.inf)
        if lse > mt:
            x[:tb] = -np.inf
        top2 = np.sort(x[x > -np.inf])[-2:] if (x > -np.inf).sum() >= 2 else np.array([0.0, np.inf])
        if abs(lse - mt) > 2e-3 and top2[1] - top2[0] > 2e-3:
            assert ref == t, (i, ref, t)
            decided += 1
    assert decided >= 1
    ctx.close()


def _row_ok(gen, tb, nots):
    ts = [t for t in gen if t >= tb]
    run = 0
    for t in gen:
        run = run + 1 if t >= tb else 0
        if run >= 3:
            return False
    return bool(gen) and tb <= gen[0] <= tb + 50 and nots not in gen and ts == sorted(ts)


def test_throughput_configuration_rows_follow_the_rules(gpu):
    """bf16 at 2048 resident clips through wh_transcribe_batch_device: every row starts with a timestamp within 1.0 s, never holds
    <|notimestamps|>, never decreases its timestamps and never has three in a row."""
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 2048)
    ctx.set_timestamp_rules(tb, nots, 50)
    uniq = np.stack([ms.synth_clip(1700 + i) for i in range(32)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (64, 1))))
    try:
        out = ctx.transcribe_batch_device(d_pcm, 2048, wb.DecodeParams(prompt, 48, eot, []))
    finally:
        hip.free(d_pcm)
    P = len(prompt)
    for i, t in enumerate(out):
        gen = [int(x) for x in t[P:]]
        if gen and gen[-1] == eot:
            gen = gen[:-1]
        assert _row_ok(gen, tb, nots), (i, gen)
        assert t.tolist() == out[i % 32].tolist(), i
    ctx.close()


def test_largest_batch_rows_equal_small_calls_with_rules(gpu):
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 1024)
    ctx.set_timestamp_rules(tb, nots, 50)
    uniq = [ms.synth_clip(900 + i) for i in range(24)]
    clips = [uniq[(i * 5) % 24] for i in range(1024)]
    p = wb.DecodeParams(prompt, 48, eot, [eot])
    full = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert all(_row_ok(t[len(prompt):], tb, nots) for t in full)
    assert [t.tolist() for t in ctx.transcribe_batch(clips[5:8], p)] == full[5:8]
    assert [t.tolist() for t in ctx.transcribe_batch(clips[300:400], p)] == full[300:400]
    ctx.close()


def test_toggling_recaptures_the_graph(gpu):
    """Rules on, then off, on one context: the same tokens as a context that never had rules (the captured step is keyed on them)."""
    prompt, eot, tb, nots = setup("micro")
    model = wb.Model("synthetic:micro:11", 0, wb.WH_PREC_F32)
    clips = [ms.synth_clip(1800 + i) for i in range(4)]
    p = wb.DecodeParams(prompt, 20, eot, [eot])
    plain = [t.tolist() for t in wb.Context(model, 4).transcribe_batch(clips, p)]
    ctx = wb.Context(model, 4)
    ctx.set_timestamp_rules(tb, nots, 50)
    on = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert on != plain and all(t[len(prompt)] >= tb for t in on)
    ctx.set_timestamp_rules(tb - 1, nots - 1, 50)       # another tb: recaptured too
    assert all(t.tolist()[len(prompt)] >= tb - 1 for t in ctx.transcribe_batch(clips, p))
    ctx.clear_timestamp_rules()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.set_timestamp_rules(tb, nots, 50)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == on
    ctx.close()


def test_errors_leave_the_context_usable(gpu):
    prompt, eot, tb, nots = setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 2)
    clips = [ms.synth_clip(0), ms.synth_clip(1)]
    p = wb.DecodeParams(prompt, 8, eot, [eot])
    plain = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    bad = wb.WhTimestampRules(wb.C.sizeof(wb.WhTimestampRules) - 8, tb, nots, 50)
    assert ctx.lib.wh_ctx_set_timestamp_rules(ctx.h, wb.C.byref(bad)) == 4          # wrong struct_size: refused, rules stay off
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.set_timestamp_rules(tb, nots, 50)
    good = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    with pytest.raises(wb.WhisperHipError) as ei:                                   # timestamp_begin <= eot for this call
        ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 8, tb, [tb]))
    assert ei.value.code == 4
    with pytest.raises(wb.WhisperHipError) as ei:                                   # <|notimestamps|> in the prompt
        ctx.transcribe_batch(clips, wb.DecodeParams(prompt + [nots], 8, eot, [eot]))
    assert ei.value.code == 4
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == good
    # a first-timestamp bound past the vocabulary is no bound (no tb + bound overflow: the first token stays a timestamp)
    ctx.set_timestamp_rules(tb, nots, -1)
    unbounded = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    ctx.set_timestamp_rules(tb, nots, 2 ** 31 - 1)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == unbounded
    assert all(t[len(prompt)] >= tb for t in unbounded)
    ctx.close()


def test_longform_with_rules_equals_staged_calls(gpu):
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 4)
    ctx.set_timestamp_rules(tb, nots, 50)
    pcm = np.concatenate([ms.synth_clip(40), ms.synth_clip(41), ms.synth_clip(42)[:200000]])  # 72.5 s
    params = wb.DecodeParams(prompt, 16, eot, [eot])
    got = ctx.transcribe_longform(pcm, params)
    offs = wb.longform_plan(pcm.size)
    assert len(got) == len(offs) == 3
    mel_full = ctx.whisper_log_mel(pcm)
    for off, toks in zip(offs, got):
        ctx.run_encoder(orc.window_mel(mel_full, off // 160, 3000), want_output=False)
        alone, _ = ctx.greedy_decode_with_past(params)
        assert toks.tolist() == alone.tolist()
        assert int(toks[len(prompt)]) >= tb
    ctx.close()


def _parse_cues(text, sep):
    cues = []
    for block in text.strip().split("\n\n"):
        lines = block.split("\n")
        if lines[0] == "WEBVTT":
            continue
        m = re.match(r"(\d+):(\d\d):(\d\d)" + re.escape(sep) + r"(\d{3}) --> (\d+):(\d\d):(\d\d)" + re.escape(sep) + r"(\d{3})$", lines[1])
        assert m, lines
        v = [int(x) for x in m.groups()]
        cues.append((int(lines[0]), v[0] * 3600 + v[1] * 60 + v[2] + v[3] / 1000, v[4] * 3600 + v[5] * 60 + v[6] + v[7] / 1000, "\n".join(lines[2:])))
    return cues


def test_cli_writes_srt_and_vtt(gpu, tmp_path):
    out = tmp_path / "res"
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "8", "--max-new-tokens", "24", "--write-srt", "--write-vtt",
                        "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = json.loads((out / "p.json").read_text())
    assert json.loads((out / "s.json").read_text())["timestamp_rules"] is True
    assert len(rows) == 8
    for row in rows:
        base = str(out / row["file"][: row["file"].rfind(".")])
        srt = _parse_cues(open(base + ".srt").read(), ",")
        vtt_text = open(base + ".vtt").read()
        assert vtt_text.startswith("WEBVTT\n\n")
        vtt = _parse_cues(vtt_text, ".")
        segs = row["segments"]
        assert len(segs) == len(srt) == len(vtt) >= 1
        last = 0.0
        for k, (s, a, b) in enumerate(zip(segs, srt, vtt)):
            assert a[0] == b[0] == k + 1 and a[1:] == b[1:]
            assert abs(a[1] - s["start"]) < 1e-3 and abs(a[2] - s["end"]) < 1e-3 and a[3] == s["text"]
            assert 0.0 <= s["start"] <= s["end"] <= row["duration_s"] and s["start"] >= last
            last = s["start"]
