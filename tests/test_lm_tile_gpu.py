"""The LM-head tile kernels (k_lm_head_tile, k_lm_head_tile_x3; their shared epilogue is csrc/wh_lm_tile.h) held to k_lm_head on the same
clips, at the smallest shapes where the epilogue can go wrong.  WH_LM_TILE_MIN_ROWS is read at every launch decision: "1" sends any batch
to the tile kernel, "0" sends it to k_lm_head; one context per setting, everything a context does runs under its setting.  Run with -m gpu.

Shapes: nano (K = 128: exactly the four k-steps that fill the bf16 ring once; vocabulary 1024: four full column tiles) with 3 clips; micro
(vocabulary 4099: the 17th column tile is three columns wide — the nn < N guards, the bitmap words past rep_words, the last mask word) with 5
clips (m < M inside one 256-row tile) and with 260 (two row tiles, the second with four live rows).

Bounds: tokens equal, kept logits bit-identical (both kernels state the same MFMA chain and the same un-contracted epilogue expression); the
log-probabilities and the no-speech probabilities within test_logprobs_gpu.TOL, the bound that file derives for the two-pass sum of the
tile kernels against k_lm_head's online sum; -inf matches -inf.  No position is skipped."""
import numpy as np
import pytest

import repetition_ref as rr
import test_logprobs_gpu as tl
import test_timestamps_gpu as tg
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

TOL = tl.TOL
NEW = 12
CASES = [("nano", "bf16", 3), ("micro", "bf16", 5), ("micro", "f16x3", 5), ("micro", "bf16", 260), ("micro", "f16x3", 260)]
COMBOS = [(rules, lp, rep) for rules in (False, True) for lp in (False, True) for rep in (False, True)]
_CLIPS = {}


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def clip(i):
    if i not in _CLIPS:
        _CLIPS[i] = ms.synth_clip(2100 + i)
    return _CLIPS[i]


def kept_rows(nb):
    """A spread of rows with the first and the last live row of every 256-row tile."""
    edges = {r for t in range(0, nb, 256) for r in (t, min(t + 255, nb - 1))}
    return sorted(edges | set(tl.spread(nb)))


def run(monkeypatch, setting, model, preset, nb):
    """Everything one context does under WH_LM_TILE_MIN_ROWS = setting: {(rules, lp, rep, forced?): (tokens, kept logits, logprobs, no-speech)}
    and the forced cycle."""
    monkeypatch.setenv("WH_LM_TILE_MIN_ROWS", setting)
    prompt, eot, tb, nots = tg.setup(preset)
    ctx = wb.Context(model, nb)
    rows = kept_rows(nb)
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    first = ctx.transcribe_batch([clip(i % 12) for i in range(nb)], p)
    # three distinct text ids the first row generated (ids of its own choosing, so their logits are not far down)
    cycle = list(dict.fromkeys(int(x) for x in first[0][len(prompt):] if x != eot and x < tb))[:3]
    cycle = (cycle + [10, 11, 12])[:3]
    forced = (cycle * NEW)[:NEW]
    out = {}
    for rules, lp, rep in COMBOS:
        if rules:
            ctx.set_timestamp_rules(tb, nots, 50)
        else:
            ctx.clear_timestamp_rules()
        if lp:
            ctx.set_logprobs(tl.no_speech_id(preset), 0)
        else:
            ctx.clear_logprobs()
        if rep:
            ctx.set_repetition(1.3, 3)
        else:
            ctx.clear_repetition()
        for F in (None, forced):
            toks, lg = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, NEW, eot, [eot], forced=F) if F else p, rows)
            lps, ns = ctx.logprobs() if lp else (None, None)
            out[(rules, lp, rep, F is not None)] = ([t.tolist() for t in toks], [np.array(x) for x in lg], lps, ns)
    ctx.close()
    return out, forced


def close_or_both_minus_inf(a, b):
    """Largest |a - b| over the finite entries; -inf only where the other is -inf, no NaN, nothing above TOL."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape
    assert not np.isnan(a).any() and not np.isnan(b).any()
    inf = np.isneginf(a)
    assert np.array_equal(inf, np.isneginf(b))
    d = np.abs(a[~inf] - b[~inf])
    assert np.all(d <= TOL), float(d.max())
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize("preset,prec_name,nb", CASES)
def test_tile_kernel_agrees_with_k_lm_head(gpu, monkeypatch, preset, prec_name, nb):
    prompt, eot, tb, nots = tg.setup(preset)
    P = len(prompt)
    model = wb.Model(f"synthetic:{preset}:{tl.SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    tile, forced_t = run(monkeypatch, "1", model, preset, nb)
    head, forced_h = run(monkeypatch, "0", model, preset, nb)
    assert forced_t == forced_h
    worst_lp = worst_ns = 0.0
    lp_bits_differ = 0
    for key in tile:
        rules, lp, rep, is_forced = key
        t_tok, t_lg, t_lp, t_ns = tile[key]
        h_tok, h_lg, h_lp, h_ns = head[key]
        assert len(t_tok) == nb and t_tok == h_tok, key
        assert all(len(t) == P + NEW for t in t_tok), key
        assert len(t_lg) == len(h_lg) == len(kept_rows(nb))
        for j, (x, y) in enumerate(zip(t_lg, h_lg)):
            assert x.shape == (NEW, ms.PRESETS[preset].vocab) and np.array_equal(x, y), (key, kept_rows(nb)[j])
        if lp:
            assert len(t_lp) == len(h_lp) == nb and t_ns.shape == h_ns.shape == (nb,)
            for x, y in zip(t_lp, h_lp):
                assert len(x) == NEW
                worst_lp = max(worst_lp, close_or_both_minus_inf(x, y))
                lp_bits_differ += int(np.sum(np.asarray(x) != np.asarray(y)))
            assert np.all(t_ns > 0) and np.all(h_ns > 0)
            worst_ns = max(worst_ns, close_or_both_minus_inf(np.log(t_ns.astype(np.float64)), np.log(h_ns.astype(np.float64))))
    print(f"{preset} {prec_name} {nb} clips: max |d logprob| {worst_lp:.3g}, max |d log no_speech_prob| {worst_ns:.3g} over {len(tile)} decodes; "
          f"{lp_bits_differ} log-probabilities differ in some bit between the two kernels; forced cycle {forced_t[:3]}")
    # against vacuity: the rules act on a row, and the forced cycle gives the repetition pass touched ids (penalised or banned) to work on
    assert any(a != b for a, b in zip(tile[(True, False, False, False)][0], tile[(False, False, False, False)][0]))
    for ex in (None, tb):
        assert any(any(rr.touched(forced_t[:i], 1.3, 3, ex)) for i in range(NEW)), ex
    assert any(rr.banned_ids(forced_t[:i], 3) for i in range(NEW))      # (the cycle closes a trigram from its sixth token on)
