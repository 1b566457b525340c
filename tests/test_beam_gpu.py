"""Beam search in the GPU token loop (wh_ctx_set_beam_search), held to the numpy restatement in tests/beam_ref.py.  Run with
-m gpu.

Ladder:
  1. selection follows the definition position by position: every position of the trace clips is replayed with beam_ref.step on the
     GPU's own logits (read through wh_decode_greedy_rows), histories and parent scores, so a flip cannot cascade;
  2. the rows carry the right histories: the returned hypotheses are forced through an option-off decode, and its logits are compared with
     the rows recorded along each hypothesis's ancestor chain;
  3. K = 1 returns the greedy tokens exactly;
  4. every decode entry agrees, and the ranking follows length_penalty;
  5. refusals leave the context usable, and clearing the option restores the greedy call bit for bit.

Bounds.  A decision whose reference margin is below delta = 8 x the f32 spacing at max(|score|, max|v| + log V) is undecided and either
outcome passes (one rounded addition, one rounded subtraction and a few-ulp logf on each side of a comparison); a position whose rule-5
margin is below test_timestamps_gpu.MARGIN is undecided as a whole.  Undecided decisions are at most 2 % of those compared in a case.
Ladder 2 asserts equality: the same replay of the greedy path against its own call measures 0 (batch rows are bit-identical)."""
import numpy as np
import pytest

import beam_ref as br
from test_logprobs_gpu import SEEDS
from test_timestamps_gpu import MARGIN, setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu
NEW = 24


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


_models = {}


def model_of(preset, prec_name):
    key = (preset, prec_name)
    if key not in _models:
        _models[key] = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    return _models[key]


def clips_of(n):
    return [ms.synth_clip(1500 + (i % 16)) for i in range(n)]


def histories(trace):
    """[g][j] -> generated history of live beam j after position g, from the parents and tokens of the trace."""
    out, prev = [], [[] for _ in range(trace["parents"].shape[1])]
    for par, tok in zip(trace["parents"], trace["tokens"]):
        cur = [prev[p] + [int(t)] if t >= 0 else list(prev[s]) for s, (p, t) in enumerate(zip(par, tok))]
        out.append(cur)
        prev = cur
    return out


def replay(trace, logits, K, C, eot, suppress, begin_suppress, rules):
    """Ladder 1 for one clip.  logits [K][steps][V].  Returns (decisions compared, undecided)."""
    hist = histories(trace)
    n_cmp = n_und = 0
    V = logits.shape[-1]
    for g in range(len(trace["parents"])):
        h_prev = hist[g - 1] if g else [[] for _ in range(K)]
        s_prev = trace["scores"][g - 1] if g else np.array([0.0] + [-np.inf] * (K - 1), np.float32)
        pool_prev = int(trace["pool_size"][g - 1]) if g else 0
        lg = logits[:, g, :]
        live, fin, margins, r5 = br.step(lg, h_prev, [float(s) for s in s_prev], eot, C - pool_prev, suppress, begin_suppress, rules)
        alive = [j for j in range(K) if s_prev[j] > -np.inf]
        vmax = float(np.nanmax(np.abs(np.where(np.isfinite(lg[alive]), lg[alive], 0.0))))
        if r5 < MARGIN:
            n_cmp += len(margins)
            n_und += len(margins)
            continue
        decided_all = True
        for s, (p, t, sc, _) in enumerate(live):
            n_cmp += 1
            d = br.delta(sc if np.isfinite(sc) else 0.0, vmax, V)
            if margins[s] < d:
                n_und += 1
                decided_all = False
                continue
            assert (int(trace["parents"][g][s]), int(trace["tokens"][g][s])) == (p, t), (g, s, trace["parents"][g], trace["tokens"][g], live)
            got = float(trace["scores"][g][s])
            assert got == sc if not np.isfinite(sc) else abs(got - sc) <= d, (g, s, got, sc, d)
        for k, (j, sc, _) in enumerate(fin):
            n_cmp += 1
            if margins[K + k] < br.delta(sc, vmax, V):
                n_und += 1
                decided_all = False
        if decided_all:
            assert int(trace["pool_size"][g]) == pool_prev + len(fin), (g, trace["pool_size"][g], pool_prev, fin)
    return n_cmp, n_und


def run_ladder1(ctx, n_clips, K, patience, trace_clips, params, rules=None, label=""):
    C = int(np.floor(np.float32(K) * np.float32(patience) + np.float32(0.5)))
    ctx.set_beam_search(K, patience, -1.0, trace_clips)
    toks = ctx.transcribe_batch(clips_of(n_clips), params)
    beams = ctx.beams()
    rows = [c * K + j for c in trace_clips for j in range(K)]
    toks2, logits = ctx.decode_resident_rows_raw(params, rows)
    assert [t.tolist() for t in toks] == [t.tolist() for t in toks2]
    P = len(params.prompt)
    n_cmp = n_und = 0
    for k, clip in enumerate(trace_clips):
        tr = ctx.beam_trace(k)
        steps = len(tr["parents"])
        assert 1 <= steps <= params.max_new_tokens and tr["parents"].shape == (steps, K)
        assert tr["pool_size"][-1] >= C or steps == params.max_new_tokens        # the loop ended for one of the two reasons
        assert (np.diff(tr["pool_size"]) >= 0).all() and tr["pool_size"][-1] <= C
        a, b = replay(tr, logits[k * K:(k + 1) * K], K, C, params.eot, params.suppress_tokens, params.begin_suppress_tokens, rules)
        n_cmp, n_und = n_cmp + a, n_und + b
        # what the clip returned is its best hypothesis, and every live hypothesis is a history of the trace
        best = beams[clip][0]
        assert toks[clip][P:].tolist() == best["tokens"].tolist()
        assert 1 <= len(beams[clip]) <= max(K, C)
        final = [h for h, s in zip(histories(tr)[-1], tr["scores"][-1]) if s > -np.inf]
        for h in beams[clip]:
            if h["finished"]:
                assert h["tokens"][-1] == params.eot and params.eot not in h["tokens"][:-1].tolist()
            else:
                assert h["tokens"].tolist() in final
    print(f"{label}: {n_cmp} decisions compared, {n_und} undecided")
    assert n_cmp > 0 and n_und <= 0.02 * n_cmp, (n_cmp, n_und)
    return toks, beams


@pytest.mark.parametrize("K", [1, 2, 5, 8])
def test_selection_nano_f32(gpu, K):
    """Rows below (1 clip) and exactly at (3 clips) max_batch."""
    prompt, eot, tb, nots = setup("nano")
    ctx = wb.Context(model_of("nano", "f32"), 3 * K)
    p = wb.DecodeParams(prompt, NEW, eot, [eot], [5])
    for n in (1, 3):
        run_ladder1(ctx, n, K, 1.0, list(range(n)), p, label=f"nano f32 K={K} clips={n}")
    ctx.close()


@pytest.mark.parametrize("rules_on,patience", [(True, 1.0), (False, 2.0)], ids=["rules", "patience2"])
def test_selection_micro_f32(gpu, rules_on, patience):
    prompt, eot, tb, nots = setup("micro")
    ctx = wb.Context(model_of("micro", "f32"), 16)
    if rules_on:
        ctx.set_timestamp_rules(tb, nots, 50)
    p = wb.DecodeParams(prompt, NEW, eot, [] if patience > 1 else [eot])
    run_ladder1(ctx, 3, 5, patience, [0, 1, 2], p, rules=(tb, nots, 50) if rules_on else None, label=f"micro f32 K=5 rules={rules_on} patience={patience}")
    ctx.close()


@pytest.mark.parametrize("es", [False, True], ids=["kv", "es"])
def test_selection_base_bf16(gpu, es):
    prompt, eot, tb, nots = setup("base")
    ctx = wb.Context(model_of("base", "bf16"), 16, cross_es=es)
    assert ctx.cross_mode == (1 if es else 0)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    run_ladder1(ctx, 3, 5, 1.0, [0, 1, 2], p, label=f"base bf16 K=5 es={es}")
    ctx.close()


def test_selection_base_bf16_tile_gemms(gpu):
    """max_batch 1024 (the tile LM head and the 1024-row kernels), 204 clips x 5 = 1020 rows, trace on the first, a middle and the last clip."""
    prompt, eot, tb, nots = setup("base")
    ctx = wb.Context(model_of("base", "bf16"), 1024)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    run_ladder1(ctx, 204, 5, 1.0, [0, 101, 203], p, label="base bf16 1024 rows K=5")
    ctx.close()


def test_selection_large_v3_bf16(gpu):
    """The column-group cross-attention kernel: 1 clip, K = 2, 6 tokens."""
    prompt, eot, tb, nots = setup("large-v3")
    ctx = wb.Context(model_of("large-v3", "bf16"), 2)
    p = wb.DecodeParams(prompt, 6, eot, [eot])
    run_ladder1(ctx, 1, 2, 1.0, [0], p, label="large-v3 bf16 K=2")
    ctx.close()


def test_dead_beams_when_two_ids_are_left(gpu):
    """Everything but two ids suppressed, K = 5: position 0 has two candidates, so three beams are dead; later positions have four."""
    dims = ms.PRESETS["nano"]
    prompt, eot, tb, nots = setup("nano")
    keep = (11, 12)
    ctx = wb.Context(model_of("nano", "f32"), 5)
    p = wb.DecodeParams(prompt, 8, eot, [i for i in range(dims.vocab) if i not in keep])
    run_ladder1(ctx, 1, 5, 1.0, [0], p, label="nano f32 K=5, two ids left")
    tr = ctx.beam_trace(0)
    assert tr["tokens"][0].tolist()[2:] == [-1, -1, -1] and tr["parents"][0].tolist()[2:] == [2, 3, 4] and (tr["scores"][0][2:] == -np.inf).all()
    assert (tr["tokens"][1] >= 0).sum() == 4 and tr["tokens"][1][4] == -1
    assert set(tr["tokens"][tr["tokens"] >= 0].tolist()) <= set(keep)
    ctx.close()


@pytest.mark.parametrize("patience", [1.0, 2.0])
def test_pool_fills_and_the_clip_completes(gpu, patience):
    """The synthetic models hardly ever emit their EOT, so here all ids but four are suppressed and one of the four is the stop token: EOT
    candidates sit among the best at every position, hypotheses finish mid-walk, the pool fills and the clips complete before
    max_new_tokens (their rows then count as done, and nothing more of them is recorded)."""
    dims = ms.PRESETS["nano"]
    prompt, eot, tb, nots = setup("nano")
    K, n = 5, 3
    C = int(round(K * patience))
    keep, stop = (11, 12, 13, 14), 14
    ctx = wb.Context(model_of("nano", "f32"), 16)
    p = wb.DecodeParams(prompt, NEW, stop, [i for i in range(dims.vocab) if i not in keep])
    toks, beams = run_ladder1(ctx, n, K, patience, list(range(n)), p, label=f"nano f32 K=5 patience={patience}, four ids left, stop token {stop}")
    traces = [ctx.beam_trace(k) for k in range(n)]
    print("pool sizes:", [tr["pool_size"].tolist() for tr in traces])
    assert any(tr["pool_size"][-1] == C and len(tr["parents"]) < NEW for tr in traces)
    for c, tr in zip(beams, traces):
        assert sum(h["finished"] for h in c) == tr["pool_size"][-1]
    ctx.close()


def chains(trace, K, eot):
    """{tuple(history) -> [physical beam index at position 0 .. len-1]} for every live history of every position, and for the finished ones
    (history ++ [eot]: the EOT was a candidate of the parent's row)."""
    out = {}
    rows_prev = [[] for _ in range(K)]
    hist = histories(trace)
    for g, (par, tok) in enumerate(zip(trace["parents"], trace["tokens"])):
        rows = [rows_prev[p] + [int(p)] if t >= 0 else [] for s, (p, t) in enumerate(zip(par, tok))]
        for s in range(K):
            if tok[s] >= 0:
                out[tuple(hist[g][s])] = rows[s]
        h_prev = hist[g - 1] if g else [[] for _ in range(K)]
        for j in range(K):   # a finished hypothesis ends on (live) row j of this position
            if g == 0 and j == 0 or g > 0 and trace["scores"][g - 1][j] > -np.inf:
                out.setdefault(tuple(h_prev[j] + [eot]), rows_prev[j] + [j])
        rows_prev = rows
    return out


@pytest.mark.parametrize("preset,prec_name,es", [("nano", "f32", None), ("base", "bf16", False), ("base", "bf16", True)], ids=["nano-f32", "base-kv", "base-es"])
def test_rows_carry_the_right_histories(gpu, preset, prec_name, es):
    """Ladder 2.  Position g of a hypothesis was computed by physical row chain[g] (the row its ancestor held then): the logits that row
    recorded must be the logits an option-off decode computes when the hypothesis is forced.  Floor: the greedy tokens forced back against
    their own call differ by 0, so equality is asserted."""
    prompt, eot, tb, nots = setup(preset)
    K, n = 5, 3
    ctx = wb.Context(model_of(preset, prec_name), 16, cross_es=es)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    clips = clips_of(n)
    # the floor, on the greedy path
    g_toks = ctx.transcribe_batch(clips, p)
    _, g_lg = ctx.greedy_decode_resident_rows(p, [0])
    forced = [int(t) for t in g_toks[0][len(prompt):]]
    _, f_lg = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, len(forced), eot, [eot], forced=forced), [0])
    floor = float(np.abs(np.asarray(f_lg[0]) - np.asarray(g_lg[0])[: len(forced)]).max())
    print(f"{preset} {prec_name} es={es}: greedy forced-replay floor {floor}")
    assert floor == 0.0
    # the beam run stops on an id the greedy path emits early, so that some hypotheses are finished ones
    stop = int(g_toks[0][len(prompt) + 2])
    p = wb.DecodeParams(prompt, NEW, stop, [])
    ctx.set_beam_search(K, 1.0, -1.0, list(range(n)))
    ctx.transcribe_batch(clips, p)
    beams = ctx.beams()
    rows = [c * K + j for c in range(n) for j in range(K)]
    _, logits = ctx.decode_resident_rows_raw(p, rows)
    traces = [ctx.beam_trace(k) for k in range(n)]
    ctx.clear_beam_search()
    worst, n_pos = 0.0, 0
    print("finished hypotheses per clip:", [sum(h["finished"] for h in c) for c in beams])
    for clip in range(n):
        ch = chains(traces[clip], K, stop)
        for h in beams[clip][:3]:
            toks = [int(t) for t in h["tokens"]]
            chain = ch[tuple(toks)]
            assert len(chain) == len(toks)
            _, f_lg = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, len(toks), stop, [], forced=toks), [clip])
            for g, j in enumerate(chain):
                d = float(np.abs(np.asarray(f_lg[0])[g] - logits[clip * K + j, g]).max())
                worst = max(worst, d)
                n_pos += 1
    print(f"{preset} {prec_name} es={es}: {n_pos} positions along the ancestor chains, max |d logit| {worst}")
    assert n_pos > 0 and worst == 0.0
    ctx.close()


@pytest.mark.parametrize("preset,prec_name", [("nano", "f32"), ("base", "bf16")])
def test_k1_is_greedy(gpu, preset, prec_name):
    prompt, eot, tb, nots = setup(preset)
    ctx = wb.Context(model_of(preset, prec_name), 4)
    ctx.set_logprobs()
    p = wb.DecodeParams(prompt, NEW, eot, [eot], [5])
    clips = clips_of(3)
    greedy = ctx.transcribe_batch(clips, p)
    g_lp = ctx.logprobs()[0]
    ctx.set_beam_search(1)
    beam = ctx.transcribe_batch(clips, p)
    b_lp = ctx.logprobs()[0]
    assert [t.tolist() for t in beam] == [t.tolist() for t in greedy]
    for a, b in zip(g_lp, b_lp):
        assert a.shape == b.shape and np.abs(a - b).max() <= 2e-4   # (test_logprobs_gpu.TOL: the greedy kernels' v_exp_f32 against expf / logf)
    ctx.clear_beam_search()
    again = ctx.transcribe_batch(clips, p)
    assert [t.tolist() for t in again] == [t.tolist() for t in greedy]
    ctx.close()


def test_every_entry_agrees_and_ranking_follows_the_penalty(gpu):
    prompt, eot, tb, nots = setup("nano")
    K = 3
    model = model_of("nano", "f32")
    ctx = wb.Context(model, 6)
    ctx.set_beam_search(K, 1.0, -1.0)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    clips = [ms.synth_clip(1500), ms.synth_clip(1501)]
    assert all(c.size == 480000 for c in clips)
    ref = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    ref_beams = ctx.beams()
    assert [t.tolist() for t in ctx.transcribe_batch_next(clips, p, clips)] == ref
    assert [t.tolist() for t in ctx.transcribe_batch_next(clips, p)] == ref          # (the prefetched copy)
    hip = wb.HipRuntime()
    d = hip.upload(0, np.stack(clips))
    assert [t.tolist() for t in ctx.transcribe_batch_device(d, 2, p)] == ref
    assert [t.tolist() for t in ctx.transcribe_batch_device(d, 2, p, d, 2)] == ref
    assert [t.tolist() for t in ctx.transcribe_batch_device(d, 2, p)] == ref           # (the prefetched encoder pass)
    got = ctx.beams()
    assert [[h["tokens"].tolist() for h in c] for c in got] == [[h["tokens"].tolist() for h in c] for c in ref_beams]
    hip.free(d)
    # long-form: 3 windows on 6 rows = two device batches of max_batch / K = 2 windows, against one batch on 9 rows
    audio = np.concatenate([ms.synth_clip(1500), ms.synth_clip(1501), ms.synth_clip(1502)])[: 16000 * 80]
    assert len(wb.longform_plan(audio.size)) == 3
    two = [t.tolist() for t in ctx.transcribe_longform(audio, p)]
    assert len(ctx.beams()) == 3
    big = wb.Context(model, 9)
    big.set_beam_search(K, 1.0, -1.0)
    assert [t.tolist() for t in big.transcribe_longform(audio, p)] == two
    big.close()
    # ranking: the same hypotheses under every penalty, ordered by the formula in f32
    base = None
    for lpn in (-1.0, 0.0, 1.0):
        ctx.set_beam_search(K, 1.0, lpn)
        ctx.transcribe_batch(clips, p)
        for c in ctx.beams():
            ranks = [h["rank_score"] for h in c]
            assert ranks == sorted(ranks, reverse=True)
            for h in c:
                n = np.float32(max(1, len(h["tokens"]) - (1 if h["finished"] else 0)))
                s = np.float32(h["sum_logprob"])
                want = s / n if lpn < 0 else s / np.power((np.float32(5) + n) / np.float32(6), np.float32(lpn), dtype=np.float32)
                assert abs(h["rank_score"] - float(want)) <= 4 * float(np.spacing(np.float32(abs(want))))
        key = [sorted((h["tokens"].tolist(), h["sum_logprob"]) for h in c) for c in ctx.beams()]
        base = base or key
        assert key == base
    ctx.close()


def test_refusals_leave_the_context_usable(gpu):
    prompt, eot, tb, nots = setup("nano")
    ctx = wb.Context(model_of("nano", "f32"), 4)
    p = wb.DecodeParams(prompt, 12, eot, [eot])
    clips = clips_of(2)
    greedy = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    _, g_lg = ctx.greedy_decode_resident_batch(p, want_logits=True)

    def refused(code, fn):
        with pytest.raises(wb.WhisperHipError) as e:
            fn()
        assert e.value.code == code, e.value

    for bad in [dict(beam_size=0), dict(beam_size=9), dict(beam_size=2, patience=0.0), dict(beam_size=2, patience=float("nan")),
                dict(beam_size=8, patience=2.2), dict(beam_size=2, trace_clips=list(range(9))), dict(beam_size=2, trace_clips=[-1]),
                dict(beam_size=2, length_penalty=float("nan"))]:
        refused(4, lambda: ctx.set_beam_search(**bad))
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == greedy      # a refused setter left the option off
    ctx.set_beam_search(2)
    beam = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    refused(4, lambda: ctx.transcribe_batch(clips_of(3), p))                   # 3 clips x 2 beams > 4 rows
    refused(8, lambda: ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 12, eot, [eot], forced=[7, 8])))
    ctx.set_repetition(1.3, 3)
    refused(8, lambda: ctx.transcribe_batch(clips, p))
    ctx.clear_repetition()
    ctx.set_alignment([(0, 0)])
    refused(8, lambda: ctx.transcribe_batch(clips, p))
    ctx.clear_alignment()
    ctx.set_prefixes([[9, 10], []])
    refused(8, lambda: ctx.transcribe_batch(clips, p))
    ctx.clear_prefixes()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == beam
    # the parity entries that take logits_out: one block per PHYSICAL row.  wh_decode_greedy's buffer holds one row -> refused with K > 1;
    # wh_decode_greedy_batch needs cap_clips >= clips x K -> refused below that, before anything is written
    import ctypes as C
    refused(4, lambda: ctx.greedy_decode_with_past(p, want_logits=True))
    assert ctx.greedy_decode_with_past(p)[0].tolist() == beam[0]                # (without logits the entry decodes clip 0 with its beams)
    ctx.transcribe_batch(clips, p)
    pc, keep = p.to_c()
    cap = len(prompt) + 12
    V = ms.PRESETS["nano"].vocab
    toks = np.zeros((4, cap), np.int64)
    n, got = (C.c_size_t * 4)(), C.c_size_t(0)
    guard = np.full((4, 12, V), 7.0, np.float32)    # room for all four rows, so that a missing check cannot overrun it here
    i64p, f32p = C.POINTER(C.c_int64), C.POINTER(C.c_float)
    for cap_clips in (2, 3):                        # enough for the 2 clips' tokens, not for their 4 rows of logits
        rc = ctx.lib.wh_decode_greedy_batch(ctx.h, C.byref(pc), toks.ctypes.data_as(i64p), cap, n, cap_clips, C.byref(got), guard.ctypes.data_as(f32p), 12)
        assert rc == 4 and (guard == 7.0).all(), rc
    rc = ctx.lib.wh_decode_greedy_batch(ctx.h, C.byref(pc), toks.ctypes.data_as(i64p), cap, n, 2, C.byref(got), None, 0)   # no logits: 2 is enough
    assert rc == 0 and got.value == 2 and [toks[i, : n[i]].tolist() for i in range(2)] == beam
    rc = ctx.lib.wh_decode_greedy_batch(ctx.h, C.byref(pc), toks.ctypes.data_as(i64p), cap, n, 4, C.byref(got), guard.ctypes.data_as(f32p), 12)
    assert rc == 0
    _, rows_lg = ctx.decode_resident_rows_raw(p, [0, 1, 2, 3])
    assert np.array_equal(guard, rows_lg)           # [n * K][rows][vocab]: the physical rows in order
    for preset, prec in (("base", "fp8"), ("micro", "f16x3")):
        c2 = wb.Context(model_of(preset, prec), 4)
        c2.set_beam_search(2)
        mp = wb.DecodeParams(setup(preset)[0], 4, setup(preset)[1])
        refused(8, lambda: c2.transcribe_batch(clips, mp))
        c2.clear_beam_search()
        assert len(c2.transcribe_batch(clips, mp)) == 2
        c2.close()
    # cleared: the greedy call's tokens and logits, bit for bit
    ctx.clear_beam_search()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == greedy
    _, lg = ctx.greedy_decode_resident_batch(p, want_logits=True)
    assert all(np.array_equal(a, b) for a, b in zip(lg, g_lg))
    ctx.close()


def test_cli_writes_hypotheses_and_the_beam_size(gpu, tmp_path):
    """whisper_bench --beam-size 3 --n-best 2 on five synthetic clips in batches of max-batch / 3 = 2 files: every row has its two best
    hypotheses, the first one's text is the row's text, config_used names the beam size — and a run without the flag has neither key."""
    import json
    import os
    import subprocess
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust-ort_amd", "whisper_bench")

    def run(out, extra):
        r = subprocess.run([cli, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "5", "--max-new-tokens", "8", "--max-batch", "6", "--precision", "bf16",
                            "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json")] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return json.loads((out / "p.json").read_text()), json.loads((out / "s.json").read_text())
    (tmp_path / "b").mkdir()
    (tmp_path / "g").mkdir()
    rows, s = run(tmp_path / "b", ["--beam-size", "3", "--n-best", "2", "--length-penalty", "1"])
    assert s["config_used"]["beam_size"] == 3 and s["n_best"] == 2 and s["length_penalty"] == 1 and len(rows) == 5
    for row in rows:
        h = row["hypotheses"]
        assert len(h) == 2 and set(h[0]) == {"text", "sum_logprob", "rank_score", "finished"} and h[0]["rank_score"] >= h[1]["rank_score"]
        assert row["text"] == (h[0]["text"] or "[EMPTY]")
    rows_g, s_g = run(tmp_path / "g", [])
    assert "beam_size" not in s_g["config_used"] and all("hypotheses" not in r for r in rows_g) and "n_best" not in s_g


def test_cli_writes_every_windows_hypotheses_of_a_long_file(gpu, tmp_path):
    """A 70 s WAV (3 windows) beside a 20 s one: the long file's row lists every window's 2 best, each with its window index."""
    import json
    import os
    import subprocess
    from test_cli_gpu import _write_wav
    cli = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "whisper-rust-ort_amd", "whisper_bench")
    adir = tmp_path / "audio"
    adir.mkdir()
    _write_wav(str(adir / "a_long.wav"), np.concatenate([ms.synth_clip(1500), ms.synth_clip(1501), ms.synth_clip(1502)])[: 16000 * 70])
    _write_wav(str(adir / "b_short.wav"), ms.synth_clip(1503)[: 16000 * 20])
    r = subprocess.run([cli, "--audio-dir", str(adir), "--onnx-dir", "synthetic:base:1234", "--max-new-tokens", "8", "--max-batch", "4", "--beam-size", "2", "--n-best", "2",
                        "--out-csv", str(tmp_path / "p.csv"), "--out-json", str(tmp_path / "p.json"), "--out-summary-json", str(tmp_path / "s.json")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    rows = json.loads((tmp_path / "p.json").read_text())
    assert [x["file"] for x in rows] == ["a_long.wav", "b_short.wav"]
    long_h, short_h = rows[0]["hypotheses"], rows[1]["hypotheses"]
    assert [h["window"] for h in long_h] == [0, 0, 1, 1, 2, 2] and all(set(h) == {"window", "text", "sum_logprob", "rank_score", "finished"} for h in long_h)
    assert all(long_h[2 * w]["rank_score"] >= long_h[2 * w + 1]["rank_score"] for w in range(3))
    assert len(short_h) == 2 and "window" not in short_h[0]
