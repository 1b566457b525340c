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
