"""Token log-probabilities and the no-speech probability of the GPU token loop (wh_ctx_set_logprobs / wh_get_logprobs), held to the
float64 restatement in tests/logprob_ref.py on the logits the kernels returned, to the f32 oracle, and to each other across the decode
entries and the CLI.  Run with -m gpu.

Bounds (the issue's): 2e-4 absolute against the restatement on the call's own logits — the value is -log S, S >= 1 a sum of at most 51,865
terms in [0, 1]; per-lane runs of <= 128 terms, <= 812 pairwise merges, v_exp_f32 and an f32 argument keep the relative error of S below 5e-5,
which is the absolute error of log S; 2e-4 leaves a factor of four.  2e-3 against the oracle: twice the project's 1e-3 logit tolerance."""
import json
import os
import subprocess

import numpy as np
import pytest

import logprob_ref as lr
import test_timestamps_gpu as tg
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
TOL, TOL_ORACLE = 2e-4, 2e-3
SEEDS = {"nano": 7, "micro": 11, "base": 1234, "large-v3": 1234}


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def no_speech_id(preset):
    d = ms.PRESETS[preset]
    return 50362 if d.vocab > 50400 else d.vocab - 301 - 2


def spread(nb):
    return sorted({0, nb // 2, nb - 1} | set(range(0, nb, max(1, nb // 8))))


def check_rows(toks, logits, lps, rows, P, eot, suppress, rules):
    """Every generated position of the given rows against the restatement on the returned logits.  Returns (positions counted, positions
    inside rule 5's margin, largest |difference|)."""
    n, near, worst = 0, 0, 0.0
    for j, r in enumerate(rows):
        gen = [int(t) for t in toks[r][P:]]
        assert len(logits[j]) == len(gen) == len(lps[r]), (r, len(logits[j]), len(gen), len(lps[r]))
        for i, t in enumerate(gen):
            tok, ref, margin = lr.token_logprob(logits[j][i], gen[:i], eot, suppress, (), rules)
            if rules is not None and margin < tg.MARGIN:
                near += 1
                continue
            got = float(lps[r][i])
            assert tok == t, (r, i, tok, t)
            if ref == -np.inf:
                assert got == -np.inf, (r, i, got)
            else:
                assert abs(got - ref) <= TOL, (r, i, got, ref)
                worst = max(worst, abs(got - ref))
            n += 1
    return n, near, worst


def run_config(ctx, prompt, eot, tb, nots, encode):
    """Rules off and on, EOT suppressed and allowed, on one context whose encoder states `encode(params)` makes resident."""
    P, out = len(prompt), []
    for rules_on in (False, True):
        total = near = 0
        worst = 0.0
        for max_init, suppress in ((50, [eot]), (-1, [])):
            if rules_on:
                ctx.set_timestamp_rules(tb, nots, max_init)
            else:
                ctx.clear_timestamp_rules()
            p = wb.DecodeParams(prompt, 24, eot, suppress)
            encode(p)
            rows = spread(ctx.max_batch)
            toks, lg = ctx.greedy_decode_resident_rows(p, rows)
            lps, ns = ctx.logprobs()
            assert ns is None and len(lps) == len(toks)
            n, k, w = check_rows(toks, lg, lps, rows, P, eot, suppress, (tb, nots, max_init) if rules_on else None)
            total, near, worst = total + n, near + k, max(worst, w)
        out.append((total, near, worst))
        assert total > 0 and near <= max(3, total // 200), (rules_on, total, near)
    return out


@pytest.mark.parametrize("preset,prec_name,nb,tile_rows", tg.CONFIGS)
def test_each_kernel_follows_the_definition(gpu, monkeypatch, preset, prec_name, nb, tile_rows):
    monkeypatch.setenv("WH_LM_TILE_MIN_ROWS", tile_rows)
    prompt, eot, tb, nots = tg.setup(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    ctx.set_logprobs()
    clips = [ms.synth_clip(1500 + (i % 16)) for i in range(nb)]
    res = run_config(ctx, prompt, eot, tb, nots, lambda p: ctx.transcribe_batch(clips, p))
    for name, (total, near, worst) in zip(("rules off", "rules on"), res):
        print(f"{preset} {prec_name} {nb} clips (WH_LM_TILE_MIN_ROWS={tile_rows}) {name}: {total} positions, {near} inside {tg.MARGIN}, max |d logprob| {worst:.3g}")
    ctx.close()


def test_benchmarked_size_follows_the_definition(gpu):
    """bf16 at 2048 resident clips (k_lm_head_tile over eight row blocks)."""
    prompt, eot, tb, nots = tg.setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 2048)
    ctx.set_logprobs()
    uniq = np.stack([ms.synth_clip(1700 + i) for i in range(32)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (64, 1))))
    try:
        res = run_config(ctx, prompt, eot, tb, nots, lambda p: ctx.transcribe_batch_device(d_pcm, 2048, p))
    finally:
        hip.free(d_pcm)
    for name, (total, near, worst) in zip(("rules off", "rules on"), res):
        print(f"base bf16 2048 clips {name}: {total} positions, {near} inside {tg.MARGIN}, max |d logprob| {worst:.3g}")
    ctx.close()


@pytest.mark.parametrize("prec_name,nb", [("bf16", 512), ("f16x3", 64)])
@pytest.mark.parametrize("rules_on", [False, True])
def test_nothing_else_moves(gpu, prec_name, nb, rules_on):
    """One forced history, the feature off then on, on one context: tokens equal, logits bit-identical; on -> off -> on gives the same
    log-probabilities each time (the captured step is recaptured, not reused)."""
    prompt, eot, tb, nots = tg.setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    if rules_on:
        ctx.set_timestamp_rules(tb, nots, 50)
    clips = [ms.synth_clip(1600 + (i % 16)) for i in range(nb)]
    free = ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 20, eot, [eot]))
    F = [int(t) for t in free[0][len(prompt):]]
    rows = list(range(0, nb, max(1, nb // 32)))
    p = wb.DecodeParams(prompt, len(F), eot, [eot], forced=F)
    off_t, off_l = ctx.greedy_decode_resident_rows(p, rows)
    with pytest.raises(wb.WhisperHipError) as ei:     # the call ran with log-probabilities off
        ctx.logprobs()
    assert ei.value.code == 3
    ctx.set_logprobs()
    on_t, on_l = ctx.greedy_decode_resident_rows(p, rows)
    lp1, _ = ctx.logprobs()
    assert [t.tolist() for t in on_t] == [t.tolist() for t in off_t]
    for j in range(len(rows)):
        assert np.array_equal(on_l[j], off_l[j]), rows[j]
    ctx.clear_logprobs()
    again_t, again_l = ctx.greedy_decode_resident_rows(p, rows)
    assert [t.tolist() for t in again_t] == [t.tolist() for t in off_t]
    assert all(np.array_equal(a, b) for a, b in zip(again_l, off_l))
    ctx.set_logprobs()
    ctx.greedy_decode_resident_rows(p, rows)
    lp2, _ = ctx.logprobs()
    assert len(lp1) == len(lp2) == nb and all(np.array_equal(a, b) for a, b in zip(lp1, lp2))
    # with `forced`, the value belongs to the recorded (argmax) token
    n, near, worst = 0, 0, 0.0
    for j, r in enumerate(rows):
        for i in range(len(F)):
            tok, ref, margin = lr.token_logprob(on_l[j][i], F[:i], eot, [eot], (), (tb, nots, 50) if rules_on else None)
            if rules_on and margin < tg.MARGIN:
                near += 1
                continue
            assert tok == int(on_t[r][len(prompt) + i]) and abs(float(lp1[r][i]) - ref) <= TOL, (r, i)
            n += 1
    assert n > 0 and near <= max(3, n // 200)
    ctx.close()


_ORACLE = {}


def oracle_model(preset):
    if preset not in _ORACLE:
        dims = ms.PRESETS[preset]
        _ORACLE[preset] = (dims, ms.flatten_state_dict(dims, ms.synth_state_dict(dims, SEEDS[preset])), {})
    return _ORACLE[preset]


def oracle_encoder(preset, clip):
    dims, w, enc = oracle_model(preset)
    if clip not in enc:
        enc[clip] = orc.encoder(dims, w, orc.window_mel(orc.log_mel(ms.synth_clip(clip), dims.n_mels), 0, 3000))
    return enc[clip]


@pytest.mark.parametrize("preset,prec_name,clip", [("nano", "f32", 0), ("micro", "f32", 2), ("base", "f32", 1900), ("base", "f16x3", 1900)])
def test_f32_against_the_oracle(gpu, preset, prec_name, clip):
    """One clip under the GPU's own history as `forced`: the log-probabilities are within 2e-3 of the restatement on the oracle's logits
    (rules off: every position; rules on: positions whose rule-5 margin on the oracle's logits exceeds 2e-3, where 1e-3 of logit error
    on either side cannot change what rule 5 decides)."""
    prompt, eot, tb, nots = tg.setup(preset)
    dims, w, _ = oracle_model(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, 1)
    ctx.set_logprobs()
    pcm = ms.synth_clip(clip)
    enc = oracle_encoder(preset, clip)
    for rules_on in (False, True):
        if rules_on:
            ctx.set_timestamp_rules(tb, nots, 50)
        p = wb.DecodeParams(prompt, 12, eot, [eot])
        toks = ctx.transcribe_batch([pcm], p)
        lps, _ = ctx.logprobs()
        gen = [int(t) for t in toks[0][len(prompt):]]
        _, ref_l = orc.decode_greedy(dims, w, enc, prompt, len(gen), eot, [eot], forced=gen, want_logits=True)
        counted, worst = 0, 0.0
        for i in range(len(gen)):
            tok, ref, margin = lr.token_logprob(ref_l[i], gen[:i], eot, [eot], (), (tb, nots, 50) if rules_on else None)
            if rules_on and margin <= TOL_ORACLE:
                continue
            worst = max(worst, abs(float(lps[0][i]) - ref))
            assert abs(float(lps[0][i]) - ref) <= TOL_ORACLE, (rules_on, i, float(lps[0][i]), ref)
            counted += 1
        print(f"{preset} {prec_name} rules {'on' if rules_on else 'off'}: {counted} positions, max |d logprob| against the oracle {worst:.3g}")
        assert counted >= 1
    ctx.close()


NS_CASES = [("nano", "f32", 1), ("micro", "f32", 1), ("base", "f32", 1), ("micro", "f16x3", 64), ("base", "f16x3", 512), ("base", "bf16", 512),
            ("base", "bf16", 1), ("base", "fp8", 512)]


@pytest.mark.parametrize("preset,prec_name,nb", NS_CASES)
def test_no_speech_probability(gpu, preset, prec_name, nb):
    """By causality the logits at prompt position k are the first-token logits of a decode whose prompt is prompt[:k + 1]: the probe's value
    against the restatement on those logits (this library's, probe off; in f32 also the oracle's)."""
    prompt, eot, tb, nots = tg.setup(preset)
    ns_id = no_speech_id(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    clips = [ms.synth_clip(1900 + (i % 16)) for i in range(nb)]
    rows = spread(nb)
    p = wb.DecodeParams(prompt, 6, eot, [eot])
    ctx.transcribe_batch(clips, p)
    want = {}
    for k in (0, 1):   # the GPU's own logits of a [sot] and a [sot, lang] prompt
        _, lg = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt[: k + 1], 1, eot, []), rows)
        want[k] = [np.log(lr.no_speech_prob(lg[j][0], ns_id)) for j in range(len(rows))]
    got = {}
    for k, rules_on in ((0, False), (0, True), (1, False)):
        ctx.set_logprobs(ns_id, k)
        if rules_on:
            ctx.set_timestamp_rules(tb, nots, 50)
        else:
            ctx.clear_timestamp_rules()
        toks = ctx.greedy_decode_resident_batch(p)[0]
        lps, ns = ctx.logprobs()
        assert ns is not None and ns.shape == (nb,) and len(lps) == nb
        assert np.all(ns > 0) and np.all(ns <= 1)
        got[(k, rules_on)] = ns.copy()
        worst = max(abs(np.log(float(ns[r])) - want[k][j]) for j, r in enumerate(rows))
        print(f"{preset} {prec_name} {nb} clips sot_index {k} rules {'on' if rules_on else 'off'}: max |d log no_speech_prob| {worst:.3g}")
        assert worst <= TOL
    assert np.array_equal(got[(0, False)], got[(0, True)])
    ctx.clear_timestamp_rules()
    if prec_name == "f32":
        dims, w, _ = oracle_model(preset)
        enc = oracle_encoder(preset, 1900)
        _, ref_l = orc.decode_greedy(dims, w, enc, prompt[:1], 1, eot, [], want_logits=True)
        assert abs(np.log(float(got[(0, False)][0])) - np.log(lr.no_speech_prob(ref_l[0], ns_id))) <= TOL_ORACLE
    # without a probe: the token log-probabilities still come back, a no-speech buffer is refused
    ctx.set_logprobs(-1)
    ctx.greedy_decode_resident_batch(p)
    lps2, ns2 = ctx.logprobs()
    assert ns2 is None and all(np.array_equal(a, b) for a, b in zip(lps2, lps))
    buf, n = np.zeros(nb, np.float32), wb.C.c_size_t(0)
    assert ctx.lib.wh_get_logprobs(ctx.h, None, 0, buf.ctypes.data_as(wb.C.POINTER(wb.C.c_float)), nb, wb.C.byref(n)) == 3
    # a probe position that emits is refused before anything is launched; the context stays usable
    ctx.set_logprobs(ns_id, len(prompt) - 1)
    with pytest.raises(wb.WhisperHipError) as ei:
        ctx.greedy_decode_resident_batch(p)
    assert ei.value.code == 4
    ctx.set_logprobs(ns_id, 0)
    ctx.greedy_decode_resident_batch(p)
    assert np.array_equal(ctx.logprobs()[1], got[(0, False)])
    ctx.close()


def test_setter_refuses_bad_options(gpu):
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 2)
    vocab = model.dims.vocab
    for o in (wb.WhLogprobOpts(wb.C.sizeof(wb.WhLogprobOpts) - 8, -1, 0), wb.WhLogprobOpts(wb.C.sizeof(wb.WhLogprobOpts), vocab, 0),
              wb.WhLogprobOpts(wb.C.sizeof(wb.WhLogprobOpts), -2, 0), wb.WhLogprobOpts(wb.C.sizeof(wb.WhLogprobOpts), 5, -1)):
        assert ctx.lib.wh_ctx_set_logprobs(ctx.h, wb.C.byref(o)) == 4
    ctx.transcribe_batch([ms.synth_clip(0)], wb.DecodeParams([3, 5, 7], 4, 2, [2]))
    with pytest.raises(wb.WhisperHipError) as ei:     # every refusal left the feature off
        ctx.logprobs()
    assert ei.value.code == 3
    ctx.close()


def test_every_entry_returns_the_same_values(gpu):
    """Six clips on a context of four (bf16 base): every decode entry returns through the getter what the resident-batch decode of the
    same clips returns, bit for bit; rows that stopped at EOT have exactly n_tokens - n_prompt entries and 0 past their end."""
    prompt, _, tb, nots = tg.setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 4)
    ns_id = no_speech_id("base")
    ctx.set_logprobs(ns_id, 0)
    clips = [ms.synth_clip(2000 + i) for i in range(6)]
    A, B = clips[:4], clips[4:]
    P, NEW = len(prompt), 24
    # an "EOT" some rows emit early and others late or never: the token row 0 generates at its fifth position
    probe = ctx.transcribe_batch(A, wb.DecodeParams(prompt, NEW, 50257, [50257]))
    eot = int(probe[0][P + 4])
    p = wb.DecodeParams(prompt, NEW, eot, [])

    def resident(batch):
        ctx.transcribe_batch(batch, p)
        toks = ctx.greedy_decode_resident_batch(p)[0][: len(batch)]
        lps, ns = ctx.logprobs()
        return [t.tolist() for t in toks], lps[: len(batch)], ns[: len(batch)]

    def same(toks, ref):
        lps, ns = ctx.logprobs()
        assert [t.tolist() for t in toks] == ref[0]
        assert len(lps) == len(ref[1]) and all(np.array_equal(a, b) for a, b in zip(lps, ref[1]))
        assert np.array_equal(ns, ref[2])
        for t, l in zip(toks, lps):
            assert len(l) == len(t) - P

    ref_a, ref_b = resident(A), resident(B)
    lens = [len(t) - P for t in ref_a[0]]
    assert min(lens) < NEW and ref_a[0][0][-1] == eot, lens        # at least row 0 stopped at its EOT
    # the raw getter: 0 past each clip's end
    raw, nsb, n = np.full((4, NEW + 3), 7.0, np.float32), np.zeros(4, np.float32), wb.C.c_size_t(0)
    ctx.transcribe_batch(A, p)
    f32p = wb.C.POINTER(wb.C.c_float)
    assert ctx.lib.wh_get_logprobs(ctx.h, raw.ctypes.data_as(f32p), NEW + 3, nsb.ctypes.data_as(f32p), 4, wb.C.byref(n)) == 0 and n.value == 4
    for b in range(4):
        assert np.array_equal(raw[b, : lens[b]], ref_a[1][b]) and np.all(raw[b, lens[b]:] == 0)
    assert ctx.lib.wh_get_logprobs(ctx.h, raw.ctypes.data_as(f32p), NEW + 3, nsb.ctypes.data_as(f32p), 3, wb.C.byref(n)) == 4   # too few clips
    assert ctx.lib.wh_get_logprobs(ctx.h, raw.ctypes.data_as(f32p), 1, None, 4, wb.C.byref(n)) == 4                             # too few tokens
    same(ctx.transcribe_batch(A, p), ref_a)                                  # wh_transcribe_batch
    ctx.run_encoder(ctx.whisper_log_mel(A[1]), want_output=False)                # wh_decode_greedy
    one, _ = ctx.greedy_decode_with_past(p)
    lps, ns = ctx.logprobs()
    assert one.tolist() == ref_a[0][1] and np.array_equal(lps[0], ref_a[1][1]) and ns[0] == ref_a[2][1]
    same(ctx.transcribe_batch_next(A, p, B), ref_a)                          # wh_transcribe_batch_next, pipelined
    same(ctx.transcribe_batch_next(B, p), ref_b)
    hip = wb.HipRuntime()
    full = [np.pad(c, (0, wb.WH_CLIP_SAMPLES - c.size)) for c in clips]
    ref_fa, ref_fb = resident(full[:4]), resident(full[4:])
    d_a, d_b = hip.upload(0, np.ascontiguousarray(np.stack(full[:4]))), hip.upload(0, np.ascontiguousarray(np.stack(full[4:])))
    try:
        same(ctx.transcribe_batch_device(d_a, 4, p), ref_fa)                 # wh_transcribe_batch_device
        same(ctx.transcribe_batch_device(d_a, 4, p, d_b, 2), ref_fa)         # wh_transcribe_batch_device_next, pipelined
        same(ctx.transcribe_batch_device(d_b, 2, p), ref_fb)
    finally:
        hip.free(d_a)
        hip.free(d_b)
    # long-form: six windows on a context of four, so two device batches; each window against the staged calls
    pcm = np.concatenate([ms.synth_clip(40 + i) for i in range(5)])[: 25 * 5 * 16000 + 200000]
    got = ctx.transcribe_longform(pcm, p)
    lps, ns = ctx.logprobs()
    offs = wb.longform_plan(pcm.size)
    assert len(got) == len(offs) == len(lps) == len(ns) and len(got) > 4
    mel_full = ctx.whisper_log_mel(pcm)
    for k, off in enumerate(offs):
        ctx.run_encoder(orc.window_mel(mel_full, off // 160, 3000), want_output=False)
        alone, _ = ctx.greedy_decode_with_past(p)
        l1, n1 = ctx.logprobs()
        assert got[k].tolist() == alone.tolist() and np.array_equal(lps[k], l1[0]) and ns[k] == n1[0], k
    ctx.close()


def test_cli_reports_and_applies_the_thresholds(gpu, tmp_path):
    """--logprobs --timestamp-rules rows carry the binding's values for the same clips; a threshold pair chosen from the printed values so
    that it catches some windows and not others empties exactly those."""
    def run(tag, *extra):
        out = tmp_path / tag
        r = subprocess.run([CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "8", "--max-new-tokens", "24", "--logprobs", "--timestamp-rules",
                            "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json"), *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert json.loads((out / "s.json").read_text())["logprobs"] is True
        return json.loads((out / "p.json").read_text())

    rows = run("plain")
    assert len(rows) == 8
    prompt, eot, tb, nots = tg.setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 16)
    ctx.set_timestamp_rules(tb, nots, 50)
    ctx.set_logprobs(50362, 0)
    toks = ctx.transcribe_batch([wb.cli_synthetic_clip(1000 + i) for i in range(8)], wb.DecodeParams(prompt, 24, eot, []))
    lps, ns = ctx.logprobs()
    for i, row in enumerate(rows):
        avg = wb.avg_logprob(lps[i], toks[i][len(prompt):], eot)
        assert row["avg_logprob"] == pytest.approx(avg, rel=1e-5, abs=1e-6) and row["no_speech_prob"] == pytest.approx(float(ns[i]), rel=1e-5), i
        assert row["segments"] and all(s["avg_logprob"] == row["avg_logprob"] and s["no_speech_prob"] == row["no_speech_prob"] for s in row["segments"])
    ctx.close()
    # thresholds between the sorted values: the windows above the no-speech cut and below the log-probability cut, and only those
    nsv, lpv = sorted(r["no_speech_prob"] for r in rows), sorted(r["avg_logprob"] for r in rows)
    x, y = (nsv[3] + nsv[4]) / 2, (lpv[5] + lpv[6]) / 2
    caught = [r["no_speech_prob"] > x and r["avg_logprob"] < y for r in rows]
    assert nsv[3] < nsv[4] and lpv[5] < lpv[6] and any(caught) and not all(caught), (nsv, lpv)
    cut = run("cut", "--no-speech-threshold", repr(x), "--logprob-threshold", repr(y))
    for r0, r1, c in zip(rows, cut, caught):
        assert r1["avg_logprob"] == pytest.approx(r0["avg_logprob"], rel=1e-5, abs=1e-6) and r1["no_speech_prob"] == pytest.approx(r0["no_speech_prob"], rel=1e-5)
        if c:
            assert r1["text"] == "" and r1["segments"] == []
        else:
            assert r1["text"] == r0["text"] and r1["segments"] == r0["segments"]
