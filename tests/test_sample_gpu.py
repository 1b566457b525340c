"""Temperature sampling in the GPU token loop (wh_ctx_set_sampling), held to the numpy restatement in tests/sample_ref.py.
Run with -m gpu.

Ladder:
  1. every draw follows the definition: a call samples and stores its logits in one pass (wh_decode_greedy_rows), and every position of the
     read rows is replayed with sample_ref.step on the GPU's own logits and fed history, so a flip cannot cascade;
  2. T = 0 rows return the greedy call's tokens, inactive rows return n_prompt tokens, T > 0 rows do not depend on their neighbours;
  3. the same seed gives the same tokens, a row id names the stream wherever the clip sits, another seed changes tokens, long-form in two
     device batches equals long-form in one;
  4. every decode entry agrees;
  5. refusals leave the context usable, and clearing the option restores the greedy call bit for bit;
  6. the CLI's ladder replaces the failing windows only and does not depend on --max-batch.

Bounds.  A position whose perturbed margin (best against second-best allowed z + gum, on the reference) is below delta = 8 x the f32 spacing
at max(1, max|z| + max|gum|) is undecided and either outcome passes — two few-ulp logf, one multiplication and one addition on each side of
the comparison; a position whose rule-5 margin is below test_timestamps_gpu.MARGIN is undecided too.  Undecided positions are at most 2 % of
a case's positions.  Log-probabilities: test_logprobs_gpu.TOL."""
import json
import os
import subprocess

import numpy as np
import pytest

import sample_ref as sr
from test_logprobs_gpu import SEEDS, TOL
from test_timestamps_gpu import MARGIN, setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu
NEW = 24
SEED = 0x5EEDC0DE12345678
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


_models, _clips = {}, {}


def model_of(preset, prec_name):
    key = (preset, prec_name)
    if key not in _models:
        _models[key] = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    return _models[key]


def clips_of(n):
    for i in range(min(n, 16)):
        if i not in _clips:
            _clips[i] = ms.synth_clip(1500 + i)
    return [_clips[i % 16] for i in range(n)]


def replay(toks, logits, lps, rows, P, temps, ids, seed, eot, suppress=(), begin_suppress=(), rules=None, forced=None):
    """Ladder 1 over the read rows.  Returns (positions compared, undecided, largest |lp difference| of the decided ones)."""
    n_cmp = n_und = 0
    worst = 0.0
    for j, r in enumerate(rows):
        gen = [int(t) for t in toks[r][P:]]
        fed = list(forced) + gen[len(forced):] if forced else gen
        assert len(logits[j]) == len(gen) == len(lps[r])
        for g, t in enumerate(gen):
            tok, lp, margin, r5, delta = sr.step(logits[j][g], fed[:g], temps[r], seed, ids[r], g, eot, suppress, begin_suppress, rules)
            n_cmp += 1
            if margin < delta or r5 < MARGIN:
                n_und += 1
                continue
            assert tok == t, (r, g, tok, t, margin, delta)
            d = 0.0 if lp == lps[r][g] else abs(lp - float(lps[r][g]))
            assert d <= TOL, (r, g, lp, lps[r][g])
            worst = max(worst, d)
    return n_cmp, n_und, worst


def run_replay(ctx, n_clips, p, temps, rows, ids=None, active=None, rules=None, label="", seed=SEED):
    ids = list(range(n_clips)) if ids is None else ids
    ctx.set_sampling(seed, temps, active, ids)
    first = ctx.transcribe_batch(clips_of(n_clips), p)
    toks, logits = ctx.greedy_decode_resident_rows(p, rows)          # samples and stores in one pass
    lps, _ = ctx.logprobs()
    assert [t.tolist() for t in toks] == [t.tolist() for t in first]
    n_cmp, n_und, worst = replay(toks, logits, lps, rows, len(p.prompt), temps, ids, seed, p.eot, p.suppress_tokens, p.begin_suppress_tokens, rules,
                                 p.forced)
    print(f"{label}: {n_cmp} positions compared, {n_und} undecided, max |d lp| {worst:.3g}")
    assert n_cmp > 0 and n_und <= 0.02 * n_cmp, (n_cmp, n_und)
    return toks, lps


@pytest.mark.parametrize("n", [1, 3])
def test_replay_nano_f32(gpu, n):
    prompt, eot, tb, nots = setup("nano")
    ctx = wb.Context(model_of("nano", "f32"), 3)
    p = wb.DecodeParams(prompt, NEW, eot, [eot], [5])
    toks, _ = run_replay(ctx, n, p, [1.0] * n, list(range(n)), ids=[100 + i for i in range(n)], label=f"nano f32 T=1 clips={n}")
    assert all(len(t) == len(prompt) + NEW for t in toks)
    ctx.close()


def test_replay_micro_f32_with_the_rules(gpu):
    prompt, eot, tb, nots = setup("micro")
    ctx = wb.Context(model_of("micro", "f32"), 16)
    ctx.set_timestamp_rules(tb, nots, 50)
    for suppress in ([eot], []):
        p = wb.DecodeParams(prompt, NEW, eot, suppress)
        run_replay(ctx, 3, p, [0.6] * 3, [0, 1, 2], rules=(tb, nots, 50), label=f"micro f32 rules T=0.6 suppress={suppress}")
    ctx.close()


@pytest.mark.parametrize("es,max_batch", [(False, 16), (True, 256)], ids=["kv", "es-256"])
def test_replay_base_bf16(gpu, es, max_batch):
    prompt, eot, tb, nots = setup("base")
    ctx = wb.Context(model_of("base", "bf16"), max_batch, cross_es=es)
    assert ctx.cross_mode == (1 if es else 0)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    run_replay(ctx, 3, p, [1.0, 0.6, 0.2], [0, 1, 2], label=f"base bf16 es={es} max_batch={max_batch}")
    ctx.close()


def test_replay_base_bf16_tile_lm_head_mixed_temperatures(gpu):
    """max_batch 1024 (the tile LM head and the 1024-row kernels), 1020 clips, temperatures 0 / 0.4 / 1 by row; the first rows, a middle
    block and the last rows are replayed."""
    prompt, eot, tb, nots = setup("base")
    n = 1020
    ctx = wb.Context(model_of("base", "bf16"), 1024)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    temps = [(0.0, 0.4, 1.0)[i % 3] for i in range(n)]
    run_replay(ctx, n, p, temps, [0, 1, 2, 509, 510, 511, 1017, 1018, 1019], label="base bf16 1020 of 1024 rows, T = 0 / 0.4 / 1")
    ctx.close()


def test_replay_rows_end_early_when_four_ids_are_left(gpu):
    """All ids suppressed but four, one of them the stop token: rows draw it and end before max_new_tokens."""
    dims = ms.PRESETS["nano"]
    prompt, eot, tb, nots = setup("nano")
    keep, stop = (11, 12, 13, 14), 14
    ctx = wb.Context(model_of("nano", "f32"), 8)
    p = wb.DecodeParams(prompt, NEW, stop, [i for i in range(dims.vocab) if i not in keep])
    toks, lps = run_replay(ctx, 8, p, [1.0] * 8, list(range(8)), label="nano f32 T=1, four ids left")
    lens = [len(t) - len(prompt) for t in toks]
    print("generated lengths:", lens)
    assert any(n < NEW for n in lens)
    for t, n in zip(toks, lens):
        gen = t[len(prompt):].tolist()
        assert set(gen) <= set(keep) and stop not in gen[:-1] and (gen[-1] == stop or n == NEW)
    ctx.close()


def test_replay_large_v3_bf16(gpu):
    """The column-group cross-attention kernel: 2 clips, 6 tokens."""
    prompt, eot, tb, nots = setup("large-v3")
    ctx = wb.Context(model_of("large-v3", "bf16"), 2)
    p = wb.DecodeParams(prompt, 6, eot, [eot])
    run_replay(ctx, 2, p, [1.0, 1.0], [0, 1], label="large-v3 bf16 T=1")
    ctx.close()


@pytest.mark.parametrize("preset,prec_name", [("base", "fp8"), ("micro", "f16x3")])
def test_replay_fp8_and_f16x3(gpu, preset, prec_name):
    """The two other precision modes take the LM head's current-row store as it is."""
    prompt, eot, tb, nots = setup(preset)
    ctx = wb.Context(model_of(preset, prec_name), 4)
    p = wb.DecodeParams(prompt, 12, eot, [eot])
    run_replay(ctx, 3, p, [1.0, 0.5, 0.0], [0, 1, 2], label=f"{preset} {prec_name}")
    ctx.close()


def test_replay_with_forced_tokens_and_prefixes(gpu):
    """Forced tokens: the recorded token is the sampled one, the fed one the forced one.  Prefixes: the draws use global generated positions."""
    prompt, eot, tb, nots = setup("nano")
    ctx = wb.Context(model_of("nano", "f32"), 3)
    ctx.set_sampling(SEED, [1.0] * 3)
    forced = [9, 10, 11, 12]
    p = wb.DecodeParams(prompt, 10, eot, [eot], forced=forced)
    ctx.transcribe_batch(clips_of(3), wb.DecodeParams(prompt, 10, eot, [eot]))
    toks, logits = ctx.greedy_decode_resident_rows(p, [0, 1, 2])
    lps, _ = ctx.logprobs()
    n_cmp, n_und, _ = replay(toks, logits, lps, [0, 1, 2], len(prompt), [1.0] * 3, [0, 1, 2], SEED, eot, [eot], forced=forced)
    assert n_cmp == 30 and n_und <= 0.02 * n_cmp
    ctx.set_prefixes([[9, 10], [], [4]])
    p = wb.DecodeParams(prompt, 10, eot, [eot])
    toks, logits = ctx.greedy_decode_resident_rows(p, [0, 1, 2])
    lps, _ = ctx.logprobs()
    n_cmp, n_und, _ = replay(toks, logits, lps, [0, 1, 2], len(prompt), [1.0] * 3, [0, 1, 2], SEED, eot, [eot])
    assert n_cmp == 30 and n_und <= 0.02 * n_cmp
    ctx.close()


@pytest.mark.parametrize("preset,prec_name", [("nano", "f32"), ("base", "bf16")])
def test_t0_rows_are_greedy_and_inactive_rows_are_empty(gpu, preset, prec_name):
    prompt, eot, tb, nots = setup(preset)
    ctx = wb.Context(model_of(preset, prec_name), 6)
    ctx.set_logprobs()
    p = wb.DecodeParams(prompt, NEW, eot, [], [5])
    clips = clips_of(6)
    greedy = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    g_lp, _ = ctx.logprobs()
    temps = [0.0, 1.0, 0.0, 1.0, 0.5, 0.0]
    ctx.set_sampling(SEED, temps)
    full = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    active = [1, 1, 0, 1, 0, 1]
    ctx.set_sampling(SEED, temps, active)
    mixed = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    m_lp, _ = ctx.logprobs()
    for b in range(6):
        if not active[b]:
            assert mixed[b] == list(prompt) and len(m_lp[b]) == 0
        elif temps[b] == 0.0:
            assert mixed[b] == greedy[b] == full[b]
            assert np.abs(m_lp[b] - g_lp[b]).max() <= TOL
        else:
            assert mixed[b] == full[b]
    assert any(full[b] != greedy[b] for b in (1, 3, 4))
    # every temperature 0 and every row active: the plain kernels, and (log-probabilities being on) the greedy call's values bit for bit
    ctx.set_sampling(SEED, [0.0] * 6)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == greedy
    t_lp, _ = ctx.logprobs()
    assert all(np.array_equal(a, b) for a, b in zip(t_lp, g_lp))
    ctx.close()


def test_determinism_row_ids_and_seeds(gpu):
    prompt, eot, tb, nots = setup("nano")
    model = model_of("nano", "f32")
    ctx = wb.Context(model, 3)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    clips = clips_of(3)
    ctx.set_sampling(SEED, [1.0] * 3, None, [10, 11, 12])
    a = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == a
    # the same clips at other batch rows, each with its id
    ctx.set_sampling(SEED, [1.0] * 3, None, [12, 10, 11])
    moved = [t.tolist() for t in ctx.transcribe_batch([clips[2], clips[0], clips[1]], p)]
    assert moved == [a[2], a[0], a[1]]
    # ... and in a batch of its own, in another context
    one = wb.Context(model, 1)
    one.set_sampling(SEED, [1.0], None, [11])
    assert one.transcribe_batch([clips[1]], p)[0].tolist() == a[1]
    one.close()
    # a second seed: chosen so that the reference, on the first position's logits (which no seed touches), draws another token for row 0
    ctx.set_sampling(SEED, [1.0] * 3, None, [10, 11, 12])
    ctx.transcribe_batch(clips, p)
    _, lg = ctx.greedy_decode_resident_rows(p, [0])
    t_a, _, m_a, _, d_a = sr.step(lg[0][0], [], 1.0, SEED, 10, 0, eot, [eot])
    assert m_a >= d_a
    other = None
    for s in range(1, 50):
        t_b, _, m_b, _, d_b = sr.step(lg[0][0], [], 1.0, s, 10, 0, eot, [eot])
        if t_b != t_a and m_b >= d_b:
            other = s
            break
    assert other is not None
    ctx.set_sampling(other, [1.0] * 3, None, [10, 11, 12])
    b = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert b[0][len(prompt)] == t_b and b[0] != a[0]
    ctx.close()
    # long-form: 3 windows in two device batches (2 + 1) against one batch of 3 — the window index is the row id
    audio = np.concatenate(clips)[: 16000 * 80]
    assert len(wb.longform_plan(audio.size)) == 3
    two = wb.Context(model, 2)
    two.set_sampling(SEED, [1.0])
    w2 = [t.tolist() for t in two.transcribe_longform(audio, p)]
    lp2, _ = two.logprobs()
    two.close()
    big = wb.Context(model, 3)
    big.set_sampling(SEED, [1.0])
    w3 = [t.tolist() for t in big.transcribe_longform(audio, p)]
    assert w2 == w3 and len(w2) == 3 and len(lp2) == 3
    big.set_sampling(SEED, [0.0])
    g3 = [t.tolist() for t in big.transcribe_longform(audio, p)]
    assert g3 != w3
    big.close()


def test_every_entry_agrees(gpu):
    prompt, eot, tb, nots = setup("nano")
    ctx = wb.Context(model_of("nano", "f32"), 4)
    ctx.set_sampling(SEED, [1.0, 0.7])
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    clips = clips_of(2)
    ref = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert [t.tolist() for t in ctx.transcribe_batch_next(clips, p, clips)] == ref
    assert [t.tolist() for t in ctx.transcribe_batch_next(clips, p)] == ref          # (the prefetched copy)
    hip = wb.HipRuntime()
    d = hip.upload(0, np.stack(clips))
    assert [t.tolist() for t in ctx.transcribe_batch_device(d, 2, p)] == ref
    assert [t.tolist() for t in ctx.transcribe_batch_device(d, 2, p, d, 2)] == ref
    assert [t.tolist() for t in ctx.transcribe_batch_device(d, 2, p)] == ref           # (the prefetched encoder pass)
    hip.free(d)
    assert [t.tolist() for t in ctx.greedy_decode_resident_batch(p)[0]] == ref
    toks, lg = ctx.greedy_decode_resident_batch(p, want_logits=True)
    assert [t.tolist() for t in toks] == ref and all(len(x) == NEW for x in lg)
    ctx.close()


def test_refusals_leave_the_context_usable(gpu):
    prompt, eot, tb, nots = setup("nano")
    ctx = wb.Context(model_of("nano", "f32"), 4)
    p = wb.DecodeParams(prompt, 12, eot, [eot])
    clips = clips_of(2)
    greedy = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    forced = [int(t) for t in greedy[0][len(prompt):]]
    pf = wb.DecodeParams(prompt, 12, eot, [eot], forced=forced)
    _, g_lg = ctx.greedy_decode_resident_batch(pf, want_logits=True)

    def refused(code, fn):
        with pytest.raises(wb.WhisperHipError) as e:
            fn()
        assert e.value.code == code, e.value

    for bad in ([-0.1, 1.0], [float("nan"), 1.0], [float("inf"), 1.0], [], [1.0] * 5):
        refused(4, lambda: ctx.set_sampling(SEED, bad))
    import ctypes as C
    t = np.ones(2, np.float32)
    o = wb.WhSamplingOpts(C.sizeof(wb.WhSamplingOpts) - 8, 1, t.ctypes.data_as(C.POINTER(C.c_float)), None, None, 2)
    assert ctx.lib.wh_ctx_set_sampling(ctx.h, C.byref(o)) == 4
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == greedy      # a refused setter left the option off
    with pytest.raises(wb.WhisperHipError):
        ctx.logprobs()                                                         # ... and nothing recorded log-probabilities
    ctx.set_sampling(SEED, [1.0, 1.0])
    sampled = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert len(ctx.logprobs()[0]) == 2                                         # recorded without wh_ctx_set_logprobs
    refused(4, lambda: ctx.set_sampling(SEED, [-1.0, 1.0]))
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == sampled     # a refused setter left the option as it was
    refused(4, lambda: ctx.transcribe_batch(clips_of(3), p))                   # 3 clips, 2 rows set
    refused(4, lambda: ctx.transcribe_longform(np.concatenate(clips), p))      # long-form takes one row
    ctx.set_beam_search(2)
    refused(8, lambda: ctx.transcribe_batch(clips, p))
    ctx.clear_beam_search()
    ctx.set_repetition(1.3, 3)
    refused(8, lambda: ctx.transcribe_batch(clips, p))
    ctx.clear_repetition()
    ctx.set_alignment([(0, 0)])
    refused(8, lambda: ctx.transcribe_batch(clips, p))
    ctx.clear_alignment()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == sampled
    # cleared: the greedy call's tokens, and the logits of a forced decode, bit for bit
    ctx.clear_sampling()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == greedy
    _, lg = ctx.greedy_decode_resident_batch(pf, want_logits=True)
    assert all(np.array_equal(a, b) for a, b in zip(lg, g_lg))
    ctx.close()


def test_cli_ladder_replaces_the_failing_windows_only(gpu, tmp_path):
    """whisper_bench --temperature 0,1.0 on six synthetic clips with a --logprob-threshold put between two of the rung-0 avg_logprob values:
    the windows above it keep their rung-0 bytes; the ones below carry temperature 1.0 and the tokens of a library call with the same seed and
    the files' indices as row ids; --max-batch 2 and --max-batch 8 write the same rows."""
    keys = ("file", "text", "avg_logprob", "no_speech_prob", "temperature", "compression_ratio")
    n, new, seed = 6, 8, 42

    def run(tag, *extra):
        out = tmp_path / tag
        out.mkdir()
        r = subprocess.run([CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", str(n), "--max-new-tokens", str(new), "--precision", "bf16", "--seed", str(seed),
                            "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json"), *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return json.loads((out / "p.json").read_text()), json.loads((out / "s.json").read_text())

    rows0, s0 = run("rung0", "--logprobs", "--max-batch", "8")
    assert "temperature" not in s0["config_used"] and all("temperature" not in r and "compression_ratio" not in r for r in rows0)
    lpv = sorted(r["avg_logprob"] for r in rows0)
    assert lpv[2] < lpv[3], lpv
    thr = (lpv[2] + lpv[3]) / 2
    failing = [r["avg_logprob"] < thr for r in rows0]
    assert sum(failing) == 3
    rows8, s8 = run("b8", "--temperature", "0,1.0", "--logprob-threshold", repr(thr), "--max-batch", "8")
    rows2, s2 = run("b2", "--temperature", "0,1.0", "--logprob-threshold", repr(thr), "--max-batch", "2")
    assert s8["config_used"]["temperature"] == [0, 1] and s8["seed"] == seed
    assert [{k: r[k] for k in keys} for r in rows8] == [{k: r[k] for k in keys} for r in rows2]
    # the library call of rung 1: the failing rows sampled at T = 1, the others inactive
    prompt, eot = [50258, 50259, 50359, 50363], 50257
    ctx = wb.Context(model_of("base", "bf16"), 8)
    ctx.set_sampling(seed, [1.0 if f else 0.0 for f in failing], [1 if f else 0 for f in failing], list(range(n)))
    toks = ctx.transcribe_batch([wb.cli_synthetic_clip(seed + i) for i in range(n)], wb.DecodeParams(prompt, new, eot, []))
    ctx.close()
    for i, (r0, r8) in enumerate(zip(rows0, rows8)):
        assert r8["compression_ratio"] > 0
        if failing[i]:
            gen = [int(t) for t in toks[i][len(prompt):]]
            if gen and gen[-1] == eot:
                gen.pop()
            assert r8["temperature"] == 1.0 and r8["text"] == "[TOKENS:" + " ".join(map(str, gen)) + "]", (i, r8, gen)
        else:
            assert r8["temperature"] == 0 and all(r8[k] == r0[k] for k in ("file", "text", "avg_logprob", "no_speech_prob")), (i, r0, r8)
            assert len(toks[i]) == len(prompt)
