"""Repetition penalty and no-repeat n-grams in the GPU token loop (wh_ctx_set_repetition), held to the numpy restatement in
tests/repetition_ref.py on the raw logits the kernels returned, composed with the timestamp-rules and log-probability restatements.
Run with -m gpu.

Bounds: tokens are compared exactly — the restatement's penalty is the kernel's float32 multiplication, the ban is -inf, and the argmax has
no tolerance.  The log-probability bound is test_logprobs_gpu.TOL (2e-4), the one that file derives for the same comparison; positions
inside rule 5's margin (test_timestamps_gpu.MARGIN) are skipped under that file's cap."""
import json
import os
import subprocess

import numpy as np
import pytest

import logprob_ref as lr
import repetition_ref as rr
import test_logprobs_gpu as tl
import test_timestamps_gpu as tg
from oracle import oracle as orc
from test_timestamps_gpu import CONFIGS, MARGIN, setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
TOL = tl.TOL
SEEDS = tl.SEEDS


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def check_rows(toks, logits, lps, rows, P, eot, suppress, rules, p, n, hist=None):
    """Every generated position of the given rows: the restatement on the returned raw logits and the row's history (its own generated
    tokens, or `hist` when the call was forced) picks the recorded token exactly; with lps, its log-probability agrees within TOL.
    Returns (positions checked, inside rule 5's margin, with a non-empty touched set, with a ban, largest |d logprob|)."""
    ex = rules[0] if rules is not None else None
    cnt = near = n_touched = n_ban = 0
    worst = 0.0
    for j, r in enumerate(rows):
        gen = [int(t) for t in toks[r][P:]]
        assert len(logits[j]) == len(gen)
        for i, t in enumerate(gen):
            h = gen[:i] if hist is None else list(hist[:i])
            adj = rr.adjust(logits[j][i], h, p, n, ex)
            tok, ref, margin = lr.token_logprob(adj, h, eot, suppress, (), rules)
            if rules is not None and margin < MARGIN:
                near += 1
                continue
            assert tok == t, (r, i, h, tok, t)
            if lps is not None:
                got = float(lps[r][i])
                if ref == -np.inf:
                    assert got == -np.inf, (r, i, got)
                else:
                    assert abs(got - ref) <= TOL, (r, i, got, ref)
                    worst = max(worst, abs(got - ref))
            pen, ban = rr.touched(h, p, n, ex)
            n_touched += bool(pen | ban)
            n_ban += bool(ban)
            cnt += 1
    return cnt, near, n_touched, n_ban, worst


@pytest.mark.parametrize("preset,prec_name,nb,tile_rows", CONFIGS)
def test_each_kernel_follows_the_definition(gpu, monkeypatch, preset, prec_name, nb, tile_rows):
    """{1.3, 3} over 24 tokens, once plain and once with the timestamp rules and the log-probabilities on: free-running, and under a
    forced history that cycles through three of the row's own text ids, so that positions with a ban exist whatever the model repeats."""
    monkeypatch.setenv("WH_LM_TILE_MIN_ROWS", tile_rows)
    prompt, eot, tb, nots = setup(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    ctx.set_repetition(1.3, 3)
    clips = [ms.synth_clip(1500 + (i % 16)) for i in range(nb)]
    P = len(prompt)
    rows = tl.spread(nb)
    p = wb.DecodeParams(prompt, 24, eot, [eot])
    total = near = touched = bans = 0
    cycle = None
    for both_on in (False, True):
        if both_on:
            ctx.set_timestamp_rules(tb, nots, 50)
            ctx.set_logprobs()
        rules = (tb, nots, 50) if both_on else None
        ctx.transcribe_batch(clips, p)
        toks, lg = ctx.greedy_decode_resident_rows(p, rows)
        lps = ctx.logprobs()[0] if both_on else None
        c, k, t, b, w = check_rows(toks, lg, lps, rows, P, eot, [eot], rules, 1.3, 3)
        print(f"{preset} {prec_name} {nb} clips (WH_LM_TILE_MIN_ROWS={tile_rows}) rules+logprobs {both_on}: {c} positions, {k} inside {MARGIN}, "
              f"{t} with touched ids, {b} with a ban, max |d logprob| {w:.3g}")
        total, near, touched, bans = total + c, near + k, touched + t, bans + b
        if cycle is None:   # three distinct text ids the first row generated (ids of its own choosing, so their logits are not far down)
            cycle = list(dict.fromkeys(int(x) for x in toks[0][P:] if x != eot and x < tb))[:3]
            cycle = (cycle + [10, 11, 12])[:3]
        F = (cycle * 8)[:24]
        pf = wb.DecodeParams(prompt, 24, eot, [eot], forced=F)
        toks, lg = ctx.greedy_decode_resident_rows(pf, rows)
        lps = ctx.logprobs()[0] if both_on else None
        c, k, t, b, w = check_rows(toks, lg, lps, rows, P, eot, [eot], rules, 1.3, 3, hist=F)
        print(f"   forced cycle {cycle}: {c} positions, {k} inside {MARGIN}, {t} with touched ids, {b} with a ban, max |d logprob| {w:.3g}")
        total, near, touched, bans = total + c, near + k, touched + t, bans + b
    assert total > 0 and near <= max(3, total // 200)
    assert touched >= 1 and bans >= 1, (touched, bans)
    ctx.close()


@pytest.mark.parametrize("preset,prec_name,nb", [("nano", "f32", 3), ("base", "bf16", 64)])
def test_the_feature_changes_what_it_should(gpu, preset, prec_name, nb):
    """One forced history F with a repeated bigram: the raw logits do not move, the ban and the penalty change the recorded token where
    the bigram closes, and every recorded token is the restatement's."""
    prompt, eot, tb, nots = setup(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    ctx = wb.Context(model, nb)
    clips = [ms.synth_clip(1600 + (i % 16)) for i in range(nb)]
    P = len(prompt)
    free = ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 32, eot, [eot]))
    gens = [[int(t) for t in f[P:]] for f in free]
    star = max(range(nb), key=lambda r: len(rr.repeated_bigrams(gens[r])))
    F = gens[star]
    closing = rr.repeated_bigrams(F)
    assert len(closing) >= 1, F
    rows = sorted({star} | set(tl.spread(nb)))
    p = wb.DecodeParams(prompt, len(F), eot, [eot], forced=F)
    off_t, off_l = ctx.greedy_decode_resident_rows(p, rows)
    assert [int(t) for t in off_t[star][P:]] == F          # the row's own history reproduces itself
    for pen, n in ((1.0, 2), (1000.0, 0)):
        ctx.set_repetition(pen, n)
        on_t, on_l = ctx.greedy_decode_resident_rows(p, rows)
        for j, r in enumerate(rows):
            assert np.array_equal(on_l[j], off_l[j]), (pen, n, r)
        c, _, t, b, _ = check_rows(on_t, on_l, None, rows, P, eot, [eot], None, pen, n, hist=F)
        assert c == len(rows) * len(F) and t >= 1
        for i in closing:
            assert int(on_t[star][P + i]) != F[i], (pen, n, i, F)
            if n:       # the closing id is banned in every row that is fed F
                assert all(int(on_t[r][P + i]) != F[i] for r in rows), (i, F)
    ctx.close()


@pytest.mark.parametrize("preset,prec_name,nb", [("base", "bf16", 64), ("micro", "f16x3", 16)])
def test_nothing_else_moves(gpu, preset, prec_name, nb):
    """Tokens, logits, log-probabilities, no-speech probabilities and languages of a context that never saw the setter, against one with
    the option off, set then cleared, and set to {1.0, 0}."""
    prompt, eot, tb, nots = setup(preset)
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    clips = [ms.synth_clip(1700 + (i % 16)) for i in range(nb)]
    lang_ids = [prompt[1], prompt[1] + 1, prompt[1] + 2]
    rows = tl.spread(nb)
    p = wb.DecodeParams(prompt, 20, eot, [eot])

    def everything(ctx):
        ctx.set_logprobs(tl.no_speech_id(preset), 0)
        ctx.set_language_detection(lang_ids, 0)
        first = ctx.transcribe_batch(clips, p)
        ns0 = ctx.logprobs()[1]
        langs, lprobs = ctx.languages()
        toks, lg = ctx.greedy_decode_resident_rows(p, rows)
        lps, _ = ctx.logprobs()
        return [t.tolist() for t in first], ns0, langs, lprobs, [t.tolist() for t in toks], lg, lps

    def same(a, b):
        assert a[0] == b[0] and a[4] == b[4]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])
        assert all(np.array_equal(x, y) for x, y in zip(a[5], b[5])) and all(np.array_equal(x, y) for x, y in zip(a[6], b[6]))

    fresh = wb.Context(model, nb)
    ref = everything(fresh)
    fresh.close()
    ctx = wb.Context(model, nb)
    same(everything(ctx), ref)                      # option off
    ctx.set_repetition(1.3, 3)
    moved = everything(ctx)
    assert moved[0] != ref[0]                       # (the option was really on: the captured step was the other one)
    ctx.clear_repetition()
    same(everything(ctx), ref)                      # set, then cleared
    ctx.set_repetition(1.0, 0)
    same(everything(ctx), ref)                      # {1.0, 0} is off
    ctx.close()


def test_with_prefixes_the_history_starts_at_the_first_generated_token(gpu):
    """Per-clip prefixes of 0, 1 and 65 ids.  Everything but eight ids S is suppressed, the forced history is one id `a` outside S, and the
    65-id prefix holds the bigram (a, s) for every s in S: had the prefix counted as history, {1.0, 2} would ban all of S at every position
    from the second on.  The restatement with the generated history alone picks every recorded token, and that token is in S."""
    prompt, eot, tb, nots = setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 3)
    clips = [ms.synth_clip(1800 + i) for i in range(3)]
    P, a = len(prompt), 9
    S = list(range(10, 18))
    suppress = [i for i in range(model.dims.vocab) if i not in S]
    U = [a] * 16
    pre = [[], [a], [x for s in S * 5 for x in (a, s)][:65]]
    assert len(pre[2]) == 65
    ctx.set_prefixes(pre)
    p = wb.DecodeParams(prompt, len(U), eot, suppress, forced=U)
    ctx.transcribe_batch(clips, p)
    would = 0
    for pen, n in ((1.0, 2), (1.3, 3)):
        ctx.set_repetition(pen, n)
        toks, lg = ctx.greedy_decode_resident_rows(p, [0, 1, 2])
        c, _, touched, _, _ = check_rows(toks, lg, None, [0, 1, 2], P, eot, suppress, None, pen, n, hist=U)
        assert c == 3 * len(U) and touched >= 1
        for b in range(3):
            for i in range(len(U)):
                t = int(toks[b][P + i])
                assert t in S, (b, i, t)
                would += t in rr.banned_ids(pre[b] + U[:i], n) and t not in rr.banned_ids(U[:i], n)
    assert would >= len(U) - 1        # row 2 under {1.0, 2}: every position from the second on
    ctx.close()


def test_with_language_detection(gpu):
    """The language token is part of the prompt, not of the history, and detection is untouched by the option."""
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 4)
    clips = [ms.synth_clip(1900 + i) for i in range(4)]
    ids = [50259 + k for k in range(8)]
    P = len(prompt)
    ctx.set_language_detection(ids, 0)
    p = wb.DecodeParams(prompt, 20, eot, [eot])
    ctx.transcribe_batch(clips, p)
    l0, p0 = ctx.languages()
    ctx.set_repetition(1.3, 2)
    ctx.transcribe_batch(clips, p)
    l1, p1 = ctx.languages()
    assert np.array_equal(l0, l1) and np.array_equal(p0, p1)
    toks, lg = ctx.greedy_decode_resident_rows(p, [0, 1, 2, 3])
    assert [int(t[1]) for t in toks] == [int(x) for x in l1]
    c, _, t, b, _ = check_rows(toks, lg, None, [0, 1, 2, 3], P, eot, [eot], None, 1.3, 2)
    assert c == 4 * 20 and t >= 1
    ctx.close()


def test_every_entry_agrees(gpu):
    """wh_decode_greedy, wh_decode_greedy_batch, wh_transcribe_batch, wh_transcribe_batch_device_next and long-form on a context of two,
    with the option, the rules and the log-probabilities on: the same tokens for the same clips."""
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 2)
    ctx.set_repetition(1.3, 3)
    ctx.set_timestamp_rules(tb, nots, 50)
    ctx.set_logprobs()
    clips = [ms.synth_clip(2000), ms.synth_clip(2001)]
    p = wb.DecodeParams(prompt, 24, eot, [eot])
    ref = [t.tolist() for t in ctx.transcribe_batch(clips, p)]                                  # wh_transcribe_batch
    ref_lp = ctx.logprobs()[0]
    plain = wb.Context(model, 2)
    plain.set_timestamp_rules(tb, nots, 50)
    assert [t.tolist() for t in plain.transcribe_batch(clips, p)] != ref                        # (the option is on and acts)
    plain.close()
    assert [t.tolist() for t in ctx.greedy_decode_resident_batch(p)[0]] == ref                  # wh_decode_greedy_batch
    assert all(np.array_equal(a, b) for a, b in zip(ctx.logprobs()[0], ref_lp))
    for b in range(2):                                                                          # wh_decode_greedy
        ctx.run_encoder(ctx.whisper_log_mel(clips[b]), want_output=False)
        assert ctx.greedy_decode_with_past(p)[0].tolist() == ref[b]
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.stack(clips)))
    try:                                                                                        # wh_transcribe_batch_device_next, twice
        assert [t.tolist() for t in ctx.transcribe_batch_device(d_pcm, 2, p, next_ptr=d_pcm, next_n=2)] == ref
        assert [t.tolist() for t in ctx.transcribe_batch_device(d_pcm, 2, p, next_ptr=d_pcm, next_n=2)] == ref
    finally:
        hip.free(d_pcm)
    pcm = np.concatenate([ms.synth_clip(40), ms.synth_clip(41), ms.synth_clip(42)[:200000]])    # 72.5 s: three windows, two device batches
    got = ctx.transcribe_longform(pcm, p)
    offs = wb.longform_plan(pcm.size)
    assert len(got) == len(offs) == 3
    mel_full = ctx.whisper_log_mel(pcm)
    for off, toks in zip(offs, got):
        ctx.run_encoder(orc.window_mel(mel_full, off // 160, 3000), want_output=False)
        assert ctx.greedy_decode_with_past(p)[0].tolist() == toks.tolist()
    ctx.close()


def test_refusals_leave_the_context_unchanged(gpu):
    prompt, eot, tb, nots = setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 2)
    clips = [ms.synth_clip(0), ms.synth_clip(1)]
    p = wb.DecodeParams(prompt, 16, eot, [eot])
    plain = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    size = wb.C.sizeof(wb.WhRepetitionOpts)

    def refused(struct_size, pen, n):
        o = wb.WhRepetitionOpts(struct_size, pen, n)
        return ctx.lib.wh_ctx_set_repetition(ctx.h, wb.C.byref(o))

    bad = [(size - 8, 1.3, 3), (size + 8, 1.3, 3), (size, float("nan"), 0), (size, float("inf"), 0), (size, -float("inf"), 0), (size, 0.0, 0),
           (size, -1.3, 2), (size, 1.3, -1), (size, 1.3, wb.WH_MAX_NGRAM + 1)]
    for args in bad:                                   # refused while off: stays off
        assert refused(*args) == 4, args
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.set_repetition(1.3, 3)
    good = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert good != plain
    for args in bad:                                   # refused while on: the earlier setting stays
        assert refused(*args) == 4, args
        assert "wh_ctx_set_repetition" in ctx.lib.wh_last_error(ctx.h).decode()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == good
    ctx.set_repetition(1.0, wb.WH_MAX_NGRAM)           # the largest n-gram is accepted (and never completes in 16 tokens)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.set_repetition(1.0, 0)
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.close()


def test_cli_no_repeat_ngram_size(gpu, tmp_path):
    out = tmp_path / "res"
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "8", "--max-new-tokens", "48", "--max-batch", "8",
                        "--no-repeat-ngram-size", "2", "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"),
                        "--out-summary-json", str(out / "s.json")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    s = json.loads((out / "s.json").read_text())
    assert s["no_repeat_ngram_size"] == 2 and "repetition_penalty" not in s
    rows = json.loads((out / "p.json").read_text())
    assert len(rows) == 8
    n_pairs = 0
    for row in rows:
        assert row["text"].startswith("[TOKENS:") and row["text"].endswith("]")
        gen = [int(t) for t in row["text"][len("[TOKENS:"):-1].split()]
        pairs = [g for g in zip(gen, gen[1:]) if g[0] < tg.BASE_TB and g[1] < tg.BASE_TB]
        assert len(pairs) == len(set(pairs)), gen
        n_pairs += len(pairs)
    assert n_pairs >= 8
