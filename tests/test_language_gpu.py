"""Language detection in the GPU token loop (wh_ctx_set_language_detection / wh_get_languages), held to the float64 restatement in
tests/language_ref.py on logits the LM head itself returned, to the f32 oracle, to explicit-prompt calls, and to the CLI.  Run with -m gpu.

The id lists.  Hash-seeded weights put one id of the real language block on top for every clip, so each test builds its list from
reference logits L[b] of its own context — a decode with prompt = [sot], max_new_tokens = 1, no suppress, logits read back: the LM head's
logits at prompt position 0, which is where detection reads (sot_index = 0) — with language_ref.pick_ids: a pair of ids whose order
flips between the clips, plus fillers, passed unsorted.  Every test asserts that at least two languages occur among its rows.

Bounds.  The chosen id is compared exactly: a listed id's logit is bit-identical to the LM head's by construction (same K walk, same
epilogue).  Probabilities within 4e-5 of the restatement: the sum has at most 128 terms in [0, 1] and is >= 1; the f32 argument of the
exponential is rounded by |v - m| 2^-24 (|v - m| < 88 for a term that is not 0) and scaled by log2(e) with the same relative error,
v_exp_f32 is within 1 ulp, the sum and the division add 2^-24 each per operation: the relative error stays below 1e-5, and a probability
is at most 1; 4e-5 leaves a factor of four.  Each row's probabilities sum to 1 within 1e-5.  Against the f32 oracle (f32 and f16x3 modes):
the winner's log-probability within 2e-3, the project's TOL_ORACLE (twice its 1e-3 logit tolerance)."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import language_ref as lg
import test_timestamps_gpu as tg
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
TOL_P, TOL_SUM, TOL_ORACLE = 4e-5, 1e-5, 2e-3
SEEDS = {"nano": 7, "micro": 11, "base": 1234, "large-v3": 1234}


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def spread(nb):
    return sorted({0, nb // 2, nb - 1} | set(range(0, nb, max(1, nb // 8))))


def clip_of(i):
    return 1500 + (i % 16)


@functools.lru_cache(maxsize=None)
def _clip(seed):
    return ms.synth_clip(seed)


def clip(i):
    """Row i's clip: sixteen distinct ones, so a batch of hundreds holds every clip many times."""
    return _clip(clip_of(i))


def sot_logits(ctx, sot, eot, rows):
    """L [len(rows)][vocab]: the LM head's logits at prompt position 0 of the resident clips (detection must be off)."""
    _, lgts = ctx.greedy_decode_resident_rows(wb.DecodeParams([sot], 1, eot), rows)
    return np.stack([l[0] for l in lgts])


@functools.lru_cache(maxsize=None)
def oracle_sot_logits(preset, clip):   # clip: the seed
    dims = ms.PRESETS[preset]
    w = ms.flatten_state_dict(dims, ms.synth_state_dict(dims, SEEDS[preset]))
    enc = orc.encoder(dims, w, orc.window_mel(orc.log_mel(_clip(clip), dims.n_mels), 0, 3000))
    prompt, eot, _, _ = tg.setup(preset)
    _, ref_l = orc.decode_greedy(dims, w, enc, [prompt[0]], 1, eot, want_logits=True)
    return np.asarray(ref_l[0], np.float64)


def check_against_ref(langs, probs, toks, rows, L, ids, slot=1):
    worst = 0.0
    for j, r in enumerate(rows):
        ref_id, ref_p = lg.detect(L[j], ids)
        assert int(langs[r]) == ref_id, (r, int(langs[r]), ref_id)
        d = float(np.abs(probs[r].astype(np.float64) - ref_p).max())
        assert d <= TOL_P, (r, d)
        assert abs(float(probs[r].astype(np.float64).sum()) - 1.0) <= TOL_SUM, r
        assert int(toks[r][slot]) == int(langs[r]), (r, toks[r][: slot + 2], int(langs[r]))
        worst = max(worst, d)
    return worst


HEAD_CONFIGS = [   # (preset, precision, clips, WH_LM_TILE_MIN_ROWS, n_lang): the LM-head kernel the reference logits come from
    ("nano", "f32", 1, "256", 5), ("nano", "f32", 3, "256", 17),      # k_lm_head<float>; 3: a partial row tile
    ("micro", "f16x3", 64, "256", 33),                                 # k_lm_head<h2>
    ("base", "bf16", 512, "256", 99), ("base", "bf16", 512, "0", 99),  # k_lm_head_tile | k_lm_head<bf16>
    ("base", "fp8", 512, "256", 99),
    ("base", "f16x3", 512, "256", 99),                                 # k_lm_head_tile_x3
    ("large-v3", "bf16", 32, "256", 100),                              # K = 1280
]


@pytest.mark.parametrize("preset,prec_name,nb,tile_rows,n_lang", HEAD_CONFIGS)
def test_language_head_matches_the_lm_head(gpu, monkeypatch, preset, prec_name, nb, tile_rows, n_lang):
    """Bounds: see the module docstring.  A one-clip context cannot show two languages in one call: it decodes two clips in two calls,
    and the list is built from both."""
    monkeypatch.setenv("WH_LM_TILE_MIN_ROWS", tile_rows)
    prompt, eot, _, _ = tg.setup(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    batches = [[0], [1]] if nb == 1 else [list(range(nb))]
    rows = spread(nb)
    p = wb.DecodeParams(prompt, 4, eot, [eot])
    Ls = []
    for batch in batches:
        ctx.transcribe_batch([clip(i) for i in batch], p)
        Ls.append(sot_logits(ctx, prompt[0], eot, rows))
    ids, gap = lg.pick_ids(np.concatenate(Ls), n_lang)
    ctx.set_language_detection(ids, 0)
    seen, worst, worst_o = set(), 0.0, 0.0
    for batch, L in zip(batches, Ls):
        toks = ctx.transcribe_batch([clip(i) for i in batch], p)
        langs, probs = ctx.languages()
        assert langs.shape == (nb,) and probs.shape == (nb, n_lang)
        worst = max(worst, check_against_ref(langs, probs, toks, rows, L, ids))
        seen |= {int(langs[r]) for r in rows}
        for i in range(nb):   # the same clip in two rows: the same language, the same probabilities
            assert int(langs[i]) == int(langs[i % 16]) and np.array_equal(probs[i], probs[i % 16]), i
        if prec_name in ("f32", "f16x3"):
            for r in rows:
                vo = oracle_sot_logits(preset, clip_of(batch[r]))[ids]
                k = ids.index(int(langs[r]))
                ref = vo[k] - (vo.max() + np.log(np.exp(vo - vo.max()).sum()))
                d = abs(float(np.log(np.float64(probs[r][k]))) - ref)
                assert d <= TOL_ORACLE, (r, d)
                worst_o = max(worst_o, d)
    print(f"{preset} {prec_name} {nb} clips (WH_LM_TILE_MIN_ROWS={tile_rows}) n_lang {n_lang}: pair gap {gap:.3g}, languages {sorted(seen)}, "
          f"max |d prob| {worst:.3g}, max |d logprob| against the oracle {worst_o:.3g}")
    assert len(seen) >= 2, seen
    ctx.close()


def test_list_sizes_and_ties(gpu):
    """nano f32, 3 clips: one language (certain), 128 languages (the largest list), and an exact tie — a model whose embedding row t is a
    copy of row a, so the two logits are the same bits: the lower id wins although the higher one is listed first."""
    prompt, eot, _, _ = tg.setup("nano")
    dims = ms.PRESETS["nano"]
    clips = [clip(i) for i in range(3)]
    rows = [0, 1, 2]
    p = wb.DecodeParams(prompt, 4, eot, [eot])
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 3)
    ctx.transcribe_batch(clips, p)
    L = sot_logits(ctx, prompt[0], eot, rows)
    ids128, _ = lg.pick_ids(L, 128)
    a, b = ids128[-1], ids128[-2]
    ctx.set_language_detection([b], 0)
    toks = ctx.transcribe_batch(clips, p)
    langs, probs = ctx.languages()
    assert langs.tolist() == [b] * 3 and probs.tolist() == [[1.0]] * 3 and all(int(t[1]) == b for t in toks)
    ctx.set_language_detection(ids128, 0)
    toks = ctx.transcribe_batch(clips, p)
    langs, probs = ctx.languages()
    assert probs.shape == (3, 128)
    check_against_ref(langs, probs, toks, rows, L, ids128)
    assert len({int(x) for x in langs}) >= 2
    ctx.close()
    # the tie: t > a copies a's row, and is listed before it
    t = next(x for x in range(a + 1, dims.vocab) if x not in ids128)
    sd = ms.synth_state_dict(dims, 7)
    key = next(k for k in sd if k.endswith("decoder.embed_tokens.weight"))
    sd[key] = sd[key].copy()
    sd[key][t] = sd[key][a]
    tied = wb.Model.from_weights(dims, ms.flatten_state_dict(dims, sd), 0, wb.WH_PREC_F32)
    ctx = wb.Context(tied, 3)
    ctx.transcribe_batch(clips, p)
    L = sot_logits(ctx, prompt[0], eot, rows)
    assert np.array_equal(L[:, t], L[:, a])
    ids = ids128[:6] + [t, b, a]
    ctx.set_language_detection(ids, 0)
    toks = ctx.transcribe_batch(clips, p)
    langs, probs = ctx.languages()
    check_against_ref(langs, probs, toks, rows, L, ids)
    assert t not in langs.tolist() and a in langs.tolist() and len(set(langs.tolist())) >= 2
    for r in rows:
        assert probs[r][6] == probs[r][8]
    ctx.close()


def detect_setup(preset, prec_name, nb, n_lang=20):
    prompt, eot, tb, nots = tg.setup(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    clips = [clip(i) for i in range(nb)]
    ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 1, eot))
    ids, _ = lg.pick_ids(sot_logits(ctx, prompt[0], eot, spread(nb)), n_lang)
    return model, ctx, clips, prompt, eot, tb, nots, ids


def with_lang(prompt, g):
    return [prompt[0], int(g)] + list(prompt[2:])


@pytest.mark.parametrize("preset,prec_name,nb", [("base", "bf16", 512), ("base", "f16x3", 64), ("base", "fp8", 512), ("nano", "f32", 3)])
def test_decode_equals_the_explicit_prompt(gpu, preset, prec_name, nb):
    """Rows grouped by detected language: the detection-off call with that id in the prompt gives the group's rows the same tokens and
    bit-identical logits under one forced history, and the same free-running tokens."""
    model, ctx, clips, prompt, eot, _, _, ids = detect_setup(preset, prec_name, nb)
    P = len(prompt)
    ctx.set_language_detection(ids, 0)
    pf = wb.DecodeParams(prompt, 16, eot, [eot])
    free_on = ctx.transcribe_batch(clips, pf)
    langs, _ = ctx.languages()
    groups = sorted({int(x) for x in langs})
    assert len(groups) >= 2, groups
    F = [int(t) for t in free_on[0][P:]]
    rows = spread(nb)
    assert len({int(langs[r]) for r in rows}) >= 2
    on_t, on_l = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, len(F), eot, [eot], forced=F), rows)
    assert np.array_equal(ctx.languages()[0], langs)
    assert all(int(on_t[i][1]) == int(langs[i]) for i in range(nb))
    ctx.clear_language_detection()
    for g in groups:
        off_t, off_l = ctx.greedy_decode_resident_rows(wb.DecodeParams(with_lang(prompt, g), len(F), eot, [eot], forced=F), rows)
        for j, r in enumerate(rows):
            if int(langs[r]) == g:
                assert on_t[r].tolist() == off_t[r].tolist(), (g, r)
                assert np.array_equal(on_l[j], off_l[j]), (g, r)
        free_off = ctx.transcribe_batch(clips, wb.DecodeParams(with_lang(prompt, g), 16, eot, [eot]))
        for i in range(nb):
            if int(langs[i]) == g:
                assert free_on[i].tolist() == free_off[i].tolist(), (g, i)
    ctx.close()


@pytest.mark.parametrize("prec_name,nb", [("bf16", 512), ("f16x3", 64)])
def test_nothing_else_moves(gpu, prec_name, nb):
    model, ctx, clips, prompt, eot, tb, nots, ids = detect_setup("base", prec_name, nb)
    P = len(prompt)
    rows = spread(nb)
    free = ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 16, eot, [eot]))
    F = [int(t) for t in free[0][P:]]
    p = wb.DecodeParams(prompt, len(F), eot, [eot], forced=F)
    off_t, off_l = ctx.greedy_decode_resident_rows(p, rows)
    with pytest.raises(wb.WhisperHipError) as ei:     # the call ran with detection off
        ctx.languages()
    assert ei.value.code == 3
    # one language, the prompt's own: nothing moves; on -> off -> on gives the same each time
    for k in range(2):
        ctx.set_language_detection([prompt[1]], 0)
        on_t, on_l = ctx.greedy_decode_resident_rows(wb.DecodeParams([prompt[0], 0] + prompt[2:], len(F), eot, [eot], forced=F), rows)   # (the placeholder is ignored)
        langs, probs = ctx.languages()
        assert langs.tolist() == [prompt[1]] * nb and probs.tolist() == [[1.0]] * nb
        ctx.clear_language_detection()
        again_t, again_l = ctx.greedy_decode_resident_rows(p, rows)
        for j, r in enumerate(rows):
            assert on_t[r].tolist() == off_t[r].tolist() == again_t[r].tolist(), (k, r)
            assert np.array_equal(on_l[j], off_l[j]) and np.array_equal(again_l[j], off_l[j]), (k, r)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 16, eot, [eot]))] == [t.tolist() for t in free]
    # log-probabilities + the no-speech probe at the same sot_index + detection, without and with the timestamp rules: what the
    # explicit-prompt call reports for the rows of each language
    ns_id = 50362
    for rules in (False, True):
        if rules:
            ctx.set_timestamp_rules(tb, nots, 50)
        ctx.set_logprobs(ns_id, 0)
        ctx.set_language_detection(ids, 0)
        pf = wb.DecodeParams(prompt, 12, eot, [eot])
        on = ctx.transcribe_batch(clips, pf)
        on_lp, on_ns = ctx.logprobs()
        langs, _ = ctx.languages()
        groups = sorted({int(x) for x in langs})
        assert len(groups) >= 2
        ctx.clear_language_detection()
        for g in groups:
            off = ctx.transcribe_batch(clips, wb.DecodeParams(with_lang(prompt, g), 12, eot, [eot]))
            off_lp, off_ns = ctx.logprobs()
            for i in range(nb):
                if int(langs[i]) == g:
                    assert on[i].tolist() == off[i].tolist(), (rules, g, i)
                    assert np.array_equal(on_lp[i], off_lp[i]) and on_ns[i] == off_ns[i], (rules, g, i)
        ctx.clear_logprobs()
    ctx.close()


@pytest.mark.parametrize("max_batch", [2, 4])
def test_longform_uses_the_first_window(gpu, max_batch):
    """nano f32, 70 s, three windows (max_batch 2: the third window is a second device batch, which decodes with the first batch's
    language as a prompt token).  The windows' reference logits come from the staged calls on the whole file's log-mel (what long-form
    computes per window); the list makes window 1 prefer another language than window 0."""
    prompt, eot, _, _ = tg.setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, max_batch)
    pcm = np.concatenate([ms.synth_clip(1500), ms.synth_clip(1501), ms.synth_clip(1502)[:160000]])   # 70 s
    offs = wb.longform_plan(pcm.size)
    assert len(offs) == 3
    mel_full = ctx.whisper_log_mel(pcm)
    L = []
    for off in offs:
        ctx.run_encoder(orc.window_mel(mel_full, off // 160, 3000), want_output=False)
        _, lgts = ctx.greedy_decode_with_past(wb.DecodeParams([prompt[0]], 1, eot), want_logits=True)
        L.append(lgts[0])
    L = np.stack(L)
    ids, gap = lg.pick_ids(L[:2], 12)
    w = [lg.detect(L[k], ids)[0] for k in range(3)]
    assert w[0] != w[1]
    params = wb.DecodeParams(prompt, 12, eot, [eot])
    ctx.set_language_detection(ids, 0)
    # window 1 alone detects its own language: through the staged entry on the file's log-mel, and as a clip of its own
    ctx.run_encoder(orc.window_mel(mel_full, offs[1] // 160, 3000), want_output=False)
    alone, _ = ctx.greedy_decode_with_past(params)
    assert ctx.languages()[0].tolist() == [w[1]] and int(alone[1]) == w[1]
    ctx.transcribe_batch([pcm[offs[1]: offs[1] + wb.WH_CLIP_SAMPLES]], params)
    print(f"long-form: pair gap {gap:.3g}, windows prefer {w}, window 1 as a clip of its own: {ctx.languages()[0].tolist()}")
    assert ctx.languages()[0].tolist() == [w[1]]
    got = ctx.transcribe_longform(pcm, params)
    langs, probs = ctx.languages()
    assert langs.tolist() == [w[0]] * 3
    ref_p = lg.detect(L[0], ids)[1]
    for k in range(3):
        assert np.array_equal(probs[k], probs[0]) and np.abs(probs[k] - ref_p).max() <= TOL_P
        assert int(got[k][1]) == w[0]
    ctx.clear_language_detection()
    ref = ctx.transcribe_longform(pcm, wb.DecodeParams(with_lang(prompt, w[0]), 12, eot, [eot]))
    assert [t.tolist() for t in got] == [t.tolist() for t in ref]
    # the long-form call leaves nothing behind: a batch call afterwards detects per clip again
    ctx.set_language_detection(ids, 0)
    ctx.transcribe_batch([pcm[: wb.WH_CLIP_SAMPLES], pcm[offs[1]: offs[1] + wb.WH_CLIP_SAMPLES]][:max_batch], params)
    assert len(set(ctx.languages()[0].tolist())) == 2
    ctx.close()


def test_refusals(gpu):
    prompt, eot, _, _ = tg.setup("nano")
    vocab = ms.PRESETS["nano"].vocab
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 2)
    clips = [ms.synth_clip(1500), ms.synth_clip(1501)]
    p = wb.DecodeParams(prompt, 8, eot, [eot])
    plain = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    lib, n = ctx.lib, wb.C.c_size_t(0)
    assert lib.wh_get_languages(ctx.h, None, None, 0, wb.C.byref(n)) == 3       # the call ran with detection off

    def raw_set(ids, sot_index=0, size=wb.C.sizeof(wb.WhLanguageOpts), n_lang=None):
        a = np.ascontiguousarray(ids, np.int64)
        o = wb.WhLanguageOpts(size, a.ctypes.data_as(wb.C.POINTER(wb.C.c_int64)), a.size if n_lang is None else n_lang, sot_index)
        return lib.wh_ctx_set_language_detection(ctx.h, wb.C.byref(o))

    bad = [dict(ids=[5, 6], size=wb.C.sizeof(wb.WhLanguageOpts) - 8), dict(ids=[5], n_lang=0), dict(ids=list(range(129))),
           dict(ids=[5, vocab]), dict(ids=[-1, 5]), dict(ids=[5, 6, 5]), dict(ids=[5, 6], sot_index=-1)]
    for kw in bad:                                                                # refused while off: stays off
        assert raw_set(**kw) == 4, kw
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    assert lib.wh_get_languages(ctx.h, None, None, 0, wb.C.byref(n)) == 3
    ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 1, eot))
    ids, _ = lg.pick_ids(sot_logits(ctx, prompt[0], eot, [0, 1]), 6)
    ctx.set_language_detection(ids, 0)
    good = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    good_l, good_p = ctx.languages()
    assert len(set(good_l.tolist())) == 2
    for kw in bad:                                                                # refused while on: the list in force stays
        assert raw_set(**kw) == 4, kw
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == good
    assert np.array_equal(ctx.languages()[0], good_l) and np.array_equal(ctx.languages()[1], good_p)
    # wh_get_languages: the count alone, too little room
    assert lib.wh_get_languages(ctx.h, None, None, 0, wb.C.byref(n)) == 0 and n.value == 2
    one = np.zeros(1, np.int64)
    assert lib.wh_get_languages(ctx.h, one.ctypes.data_as(wb.C.POINTER(wb.C.c_int64)), None, 1, wb.C.byref(n)) == 4
    two = np.zeros(2, np.int64)
    assert lib.wh_get_languages(ctx.h, two.ctypes.data_as(wb.C.POINTER(wb.C.c_int64)), None, 2, wb.C.byref(n)) == 0 and two.tolist() == good_l.tolist()
    # decode time: sot_index + 1 must be a prompt position
    ctx.set_language_detection(ids, len(prompt) - 1)
    with pytest.raises(wb.WhisperHipError) as ei:
        ctx.transcribe_batch(clips, p)
    assert ei.value.code == 4 and "sot_index" in str(ei.value)
    with pytest.raises(wb.WhisperHipError) as ei:                                 # nothing was decoded: nothing to report
        ctx.languages()
    assert ei.value.code == 3
    ctx.set_language_detection(ids, 0)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == good
    ctx.clear_language_detection()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.close()


def _run_cli(out, *flags):
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "4", "--max-new-tokens", "8", "--max-batch", "16", *flags,
                        "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    return json.loads((out / "p.json").read_text()), (out / "p.csv").read_text(), json.loads((out / "s.json").read_text())


def test_cli_language_auto(gpu, tmp_path):
    """base bf16, 4 synthetic clips: language / language_probability of the rows are the binding's for the same clips (the probability
    printed so that it reads back as the same float).  --language en writes what the flags of before write: the same keys in the same
    order, the same CSV header, the same values (the times of a run are its own)."""
    rows, csv, summary = _run_cli(tmp_path / "auto", "--language", "auto")
    assert summary["language"] == "auto" and len(rows) == 4
    codes, ids = wb.language_table(51865)
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 16)
    ctx.set_language_detection(ids, 0)
    toks = ctx.transcribe_batch([wb.cli_synthetic_clip(1000 + i) for i in range(4)], wb.DecodeParams([50258, 50259, 50359, 50363], 8, 50257))
    langs, probs = ctx.languages()
    assert csv.splitlines()[0] == "file,duration_s,end_to_end_s,rtf,text,language,language_probability"
    for k, row in enumerate(rows):
        j = ids.index(int(langs[k]))
        assert list(row)[:7] == ["file", "duration_s", "end_to_end_s", "rtf", "text", "language", "language_probability"]
        assert row["language"] == codes[j] and np.float32(row["language_probability"]) == probs[k][j], (k, row, codes[j], probs[k][j])
        fields = csv.splitlines()[1 + k].split(",")
        assert fields[-2] == codes[j] and float(fields[-1]) == row["language_probability"]
    ctx.close()
    base_rows, base_csv, base_sum = _run_cli(tmp_path / "base")
    en_rows, en_csv, en_sum = _run_cli(tmp_path / "en", "--language", "en")
    timed = ("end_to_end_s", "rtf")
    assert [list(r) for r in en_rows] == [list(r) for r in base_rows] and "language" not in en_rows[0]
    assert [{k: v for k, v in r.items() if k not in timed} for r in en_rows] == [{k: v for k, v in r.items() if k not in timed} for r in base_rows]
    assert en_csv.splitlines()[0] == base_csv.splitlines()[0] == "file,duration_s,end_to_end_s,rtf,text"
    assert [l.split(",")[0:2] + l.split(",")[4:] for l in en_csv.splitlines()] == [l.split(",")[0:2] + l.split(",")[4:] for l in base_csv.splitlines()]
    assert list(en_sum) == list(base_sum) and en_sum["language"] == base_sum["language"] == "en"
