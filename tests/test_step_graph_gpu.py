"""The captured decode step across calls (wh_ctx::StepKey): one context is walked through a sequence of option states with a decode after
each, and every result is held to a fresh context that was only ever put in that state.  A value the captured step bakes in without a key
entry shows here as a stale graph on the walked context.  Tokens are compared exactly; with log-probabilities on, logprobs() (and the
no-speech probabilities) bit for bit; kept logits bit for bit.  Twelve new tokens: eleven positions replay the graph.  Run with -m gpu."""
import numpy as np
import pytest

import test_logprobs_gpu as tl
from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

NEW = 12


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def walk(n_clips):
    """The states, in order: (name, state).  A state lists every option; what it does not list is off."""
    lens = [(0, 1, 5)[i % 3] for i in range(n_clips)]
    pfx = [[20 + 3 * b + i for i in range(n)] for b, n in enumerate(lens)]
    empty = [[] for _ in range(n_clips)]
    on = dict(rules=True, lp=True)
    rep = dict(on, rep=(1.2, 2))
    return [
        ("plain", {}),
        ("rules", dict(rules=True)),
        ("rules + logprobs", on),
        ("+ repetition (1.3, 3)", dict(on, rep=(1.3, 3))),
        ("repetition (1.3, 2)", dict(on, rep=(1.3, 2))),
        ("repetition (1.2, 2)", rep),
        ("+ prefixes", dict(rep, pfx=pfx)),
        ("prefixes all empty", dict(rep, pfx=empty)),
        ("two forced tokens", dict(rep, pfx=empty, forced=[11, 13])),
        ("another eot", dict(rep, pfx=empty, eot_shift=1)),
        ("two clips", dict(rep, pfx=empty[:2], n_clips=2)),
        ("logits of rows [0, 2]", dict(rep, pfx=empty, rows=[0, 2])),
        ("logits of row [1]", dict(rep, pfx=empty, rows=[1])),
        ("everything cleared", {}),
    ]


def put(ctx, st, preset, fresh):
    """Puts ctx in state st.  A fresh context sees only the setters of what is on; the walked one also the clears of what is off."""
    _, _, tb, nots = setup(preset)
    if st.get("rules"):
        ctx.set_timestamp_rules(tb, nots, 50)
    elif not fresh:
        ctx.clear_timestamp_rules()
    if st.get("lp"):
        ctx.set_logprobs(tl.no_speech_id(preset), 0)
    elif not fresh:
        ctx.clear_logprobs()
    if st.get("rep"):
        ctx.set_repetition(*st["rep"])
    elif not fresh:
        ctx.clear_repetition()
    if st.get("pfx") is not None:
        ctx.set_prefixes(st["pfx"])
    elif not fresh:
        ctx.clear_prefixes()


def decode(ctx, st, preset, clips):
    """The state's decode: (tokens, logprobs or None, no-speech or None, kept logits or None)."""
    prompt, eot, _, _ = setup(preset)
    p = wb.DecodeParams(prompt, NEW, eot + st.get("eot_shift", 0), [eot], forced=st.get("forced"))
    toks = ctx.transcribe_batch(clips[: st.get("n_clips", len(clips))], p)
    lg = None
    if st.get("rows"):
        toks, lg = ctx.greedy_decode_resident_rows(p, st["rows"])
    lps, ns = ctx.logprobs() if st.get("lp") else (None, None)
    return [t.tolist() for t in toks], lps, ns, lg


def same(a, b, what):
    assert a[0] == b[0], what
    for x, y in zip(a[1:], b[1:]):
        assert (x is None) == (y is None), what
        if x is None:
            continue
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y), what
        else:
            assert len(x) == len(y) and all(np.array_equal(u, v) for u, v in zip(x, y)), what


@pytest.mark.parametrize("preset,seed,prec_name,n_clips", [("nano", 7, "f32", 3), ("base", 1234, "bf16", 4)])
def test_a_walked_context_decodes_like_a_fresh_one(gpu, preset, seed, prec_name, n_clips):
    model = wb.Model(f"synthetic:{preset}:{seed}", 0, wb.PRECISIONS[prec_name])
    clips = [ms.synth_clip(1700 + i) for i in range(n_clips)]
    states = walk(n_clips)
    ref = []
    for name, st in states:
        fresh = wb.Context(model, n_clips)
        put(fresh, st, preset, True)
        ref.append(decode(fresh, st, preset, clips))
        fresh.close()
    by_name = {name: r for (name, _), r in zip(states, ref)}
    # the "on" states really are other decodes: the rules move the tokens, and so does repetition (1.3, 3) on top of rules + logprobs
    assert by_name["rules"][0] != by_name["plain"][0]
    assert by_name["+ repetition (1.3, 3)"][0] != by_name["rules + logprobs"][0]
    ctx = wb.Context(model, n_clips)
    for (name, st), r in zip(states, ref):
        put(ctx, st, preset, False)
        same(decode(ctx, st, preset, clips), r, name)
    same(ref[-1], ref[0], "everything cleared is plain")
    ctx.close()


# ---- the options that came after the walk above: language detection, alignment, beam search, sampling -----------------------------------------

SEED = 20240


def walk_options(preset, n_clips):
    """The states of the second walk, in order: (name, state).  A state lists every option; what it does not list is off."""
    d = ms.PRESETS[preset]
    prompt = setup(preset)[0]
    lang_a = [prompt[1] + i for i in range(3)]
    lang_b = [prompt[1] + 5 + i for i in range(4)]
    # two heads in different layers where the preset has two layers, else two heads of one layer
    heads_a = [(0, 0), (1, 1)] if d.dec_layers >= 2 else [(0, 0), (0, 1)]
    heads_b = [(0, 1), (1, 0)] if d.dec_layers >= 2 else [(0, 1), (0, 0)]
    warm = dict(sample=[0.7] * n_clips)
    mixed = dict(rules=True, lp=True, sample=[0.5] * n_clips)
    return [
        ("plain", {}),
        ("language detection, three ids", dict(lang=lang_a)),
        ("language detection, another list", dict(lang=lang_b)),
        ("language detection cleared", {}),
        ("alignment, heads A", dict(align=heads_a)),
        ("alignment, heads B", dict(align=heads_b)),
        ("alignment, heads B, 16 new tokens", dict(align=heads_b, new=16)),   # the query side buffer grows: the captured step is dropped
        ("alignment cleared", {}),
        ("beam search K = 2", dict(beam=2)),
        ("beam search K = 3", dict(beam=3)),
        ("beam search cleared", {}),                                          # its buffers are freed while a graph was captured on them
        ("sampling T = 0.7", warm),
        ("sampling, all temperatures 0", dict(sample=[0.0] * n_clips)),       # the trivial path: the plain kernels
        ("sampling cleared", {}),
        ("rules + logprobs + sampling T = 0.5", mixed),
        ("logits of row [1]", dict(mixed, rows=[1])),
        ("logits of row [1], 20 new tokens", dict(mixed, rows=[1], new=20)),  # the parity buffer grows
        ("everything cleared", {}),
    ]


def put_options(ctx, st, preset, fresh):
    """put() for the second walk's options (the first walk's rules and log-probabilities included)."""
    put(ctx, st, preset, fresh)
    if st.get("lang"):
        ctx.set_language_detection(st["lang"], 0)
    elif not fresh:
        ctx.clear_language_detection()
    if st.get("align"):
        ctx.set_alignment(st["align"], debug_rows=[0])
    elif not fresh:
        ctx.clear_alignment()
    if st.get("beam"):
        ctx.set_beam_search(st["beam"], 1.0, -1.0, [0])
    elif not fresh:
        ctx.clear_beam_search()
    if st.get("sample"):
        ctx.set_sampling(SEED, st["sample"])
    elif not fresh:
        ctx.clear_sampling()


def decode_options(ctx, st, preset, clips):
    """The state's decode: (tokens, {getter: what it returned}) with every getter the state has on."""
    prompt, eot, _, _ = setup(preset)
    p = wb.DecodeParams(prompt, st.get("new", NEW), eot, [eot])
    toks = ctx.transcribe_batch(clips, p)
    out = {}
    if st.get("rows"):
        toks, out["logits"] = ctx.greedy_decode_resident_rows(p, st["rows"])
    if st.get("lp"):
        out["logprobs"] = ctx.logprobs()
    if st.get("lang"):
        out["languages"] = ctx.languages()
    if st.get("align"):
        out["token_frames"] = ctx.token_frames()
        out["alignment_debug"] = ctx.alignment_debug(0)
    if st.get("beam"):
        out["beams"] = ctx.beams()
        out["beam_trace"] = ctx.beam_trace(0)
    return [t.tolist() for t in toks], out


def bits(x):
    """x with every array replaced by (dtype, shape, bytes): equality is then bit for bit."""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return {k: bits(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [bits(v) for v in x]
    if isinstance(x, float):
        return np.float64(x).tobytes()
    return x


@pytest.mark.parametrize("preset,seed,prec_name,n_clips", [("nano", 7, "f32", 3), ("base", 1234, "bf16", 4)])
def test_a_context_walked_through_the_later_options_decodes_like_a_fresh_one(gpu, preset, seed, prec_name, n_clips):
    """Language detection, alignment, beam search and sampling through set / change / clear on one context (max_batch = 3 x clips, so that
    three beams fit and both sides pad their rows alike), each state held to a fresh context: tokens exactly, every getter bit for bit."""
    model = wb.Model(f"synthetic:{preset}:{seed}", 0, wb.PRECISIONS[prec_name])
    clips = [ms.synth_clip(1700 + i) for i in range(n_clips)]
    states = walk_options(preset, n_clips)
    ref = []
    for name, st in states:
        fresh = wb.Context(model, 3 * n_clips)
        put_options(fresh, st, preset, True)
        ref.append(decode_options(fresh, st, preset, clips))
        fresh.close()
    by_name = {name: r for (name, _), r in zip(states, ref)}
    # the "on" states really are other decodes: a third beam changes the n-best, and T = 0.7 moves a token
    nbest = lambda r: [[h["tokens"].tolist() for h in c] for c in r[1]["beams"]]
    assert nbest(by_name["beam search K = 3"]) != nbest(by_name["beam search K = 2"])
    assert by_name["sampling T = 0.7"][0] != by_name["plain"][0]
    assert by_name["sampling, all temperatures 0"][0] == by_name["plain"][0]
    ctx = wb.Context(model, 3 * n_clips)
    for (name, st), r in zip(states, ref):
        put_options(ctx, st, preset, False)
        got = decode_options(ctx, st, preset, clips)
        assert got[0] == r[0], name
        assert sorted(got[1]) == sorted(r[1]), name
        for k in r[1]:
            assert bits(got[1][k]) == bits(r[1][k]), (name, k)
    assert ref[-1] == ref[0], "everything cleared is plain"
    ctx.close()
