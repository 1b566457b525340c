"""wh_score_tokens (log p(given tokens | audio) in one decoder pass over all positions) held to the f32 oracle, to the float64 restatement
in tests/score_ref.py on the call's own logits, to the bf16 golden vectors and to the library's own forced token loop.  Run with -m gpu.

Bounds (the issue's): logits within the project's 1e-3 of the oracle; log-probabilities within 2e-3 of the restatement on the oracle's logits
(lp = v[t] - LSE(v), LSE 1-Lipschitz in the max norm: twice the logit tolerance); 2e-4 against the restatement on the call's own logits (the
bound of tests/test_logprobs_gpu.py); bf16 logits within 0.16 of the golden vectors, and within 0.32 of the bf16 token loop (both within 0.16
of f32).  The argmax is compared wherever the reference's top-1 margin exceeds 2e-3; at most one entry in eight may fall under it."""
import functools
import os

import numpy as np
import pytest

import score_ref as sr
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

LOGIT_TOL, LP_TOL_ORACLE, LP_TOL_SELF, MARGIN = 1e-3, 2e-3, 2e-4, 2e-3
BF16_GOLDEN, BF16_LOOP = 0.16, 0.32
SEEDS = {"nano": 7, "micro": 11, "base": 1234}
# hypothesis lengths n (T = P + n - 1 rows, P = 4): 1, 2, and either side of the self-attention kernel's edges in T — its groups of 4 rows
# (T = 16 / 17 at n = 13 / 14), its 64-row query blocks and 64-key chunks (T = 64 / 65 at n = 61 / 62, T = 128 / 129 at n = 125 / 126) — and
# the issue's 15, 16, 17, 63, 64, 65, 129, 140
LENGTHS = [1, 2, 13, 14, 15, 16, 17, 60, 61, 62, 63, 64, 65, 124, 125, 126, 129, 140]
TOKEN_SEED = 2024   # (checked on the CPU: with it the oracle alone keeps the entries under MARGIN far below one in eight)


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def setup(preset):
    """(prompt, eot): the multilingual ids for base; for the small vocabularies an EOT near the top, so that tokens below it are most of them."""
    d = ms.PRESETS[preset]
    return ([50258, 50259, 50359, 50363], 50257) if d.vocab > 50400 else ([3, 5, 7, 9], d.vocab - 303)


def draw(preset, n, seed=TOKEN_SEED):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.integers(0, setup(preset)[1], size=n).tolist()


@functools.lru_cache(maxsize=None)
def weights(preset):
    d = ms.PRESETS[preset]
    return ms.flatten_state_dict(d, ms.synth_state_dict(d, SEEDS[preset]))


@functools.lru_cache(maxsize=None)
def oracle_enc(preset, clip):
    d = ms.PRESETS[preset]
    return orc.encoder(d, weights(preset), orc.window_mel(orc.log_mel(ms.synth_clip(clip), d.n_mels), 0, 3000))


@functools.lru_cache(maxsize=None)
def oracle_logits(preset, clip, toks):
    """[len(toks)][vocab]: the oracle's logits of every entry of the hypothesis `toks` (a tuple) on clip `clip`; computed once, shared, not modified"""
    d = ms.PRESETS[preset]
    prompt, eot = setup(preset)
    _, lg = orc.decode_greedy(d, weights(preset), oracle_enc(preset, clip), prompt, len(toks), eot, forced=list(toks[:-1]), want_logits=True)
    assert lg.shape[0] == len(toks)
    lg.setflags(write=False)
    return lg


def check_against_oracle(preset, clip, toks, lp, am, logits, suppress=(), begin_suppress=(), history=None):
    """One hypothesis as in the issue's test 1 (history: a longer hypothesis `toks` is a prefix of, whose oracle run is shared).  Returns
    (entries, entries under MARGIN)."""
    ref = oracle_logits(preset, clip, tuple(history if history is not None else toks))[: len(toks)]
    assert len(lp) == len(am) == len(toks)
    if logits is not None:
        assert logits.shape == ref.shape
        np.testing.assert_allclose(logits, ref, rtol=0, atol=LOGIT_TOL)
    rlp, ram = sr.score_ref(ref, toks, suppress, begin_suppress)
    near = 0
    for i in range(len(toks)):
        if rlp[i] == -np.inf:
            assert lp[i] == -np.inf, (i, lp[i])
        else:
            assert abs(float(lp[i]) - rlp[i]) <= LP_TOL_ORACLE, (i, float(lp[i]), rlp[i])
        if sr.top1_margin(ref[i], i, suppress, begin_suppress) > MARGIN:
            assert int(am[i]) == int(ram[i]), (i, int(am[i]), int(ram[i]))
        else:
            near += 1
    return len(toks), near


def check_self(toks, lp, am, logits, suppress=(), begin_suppress=()):
    """The issue's test 2 for one hypothesis: exact argmax and 2e-4 on the call's own logits.  Returns the largest |difference|."""
    rlp, ram = sr.score_ref(logits, toks, suppress, begin_suppress)
    assert am.tolist() == ram.tolist()
    worst = 0.0
    for i in range(len(toks)):
        if rlp[i] == -np.inf:
            assert lp[i] == -np.inf, (i, lp[i])
        else:
            assert abs(float(lp[i]) - rlp[i]) <= LP_TOL_SELF, (i, float(lp[i]), rlp[i])
            worst = max(worst, abs(float(lp[i]) - rlp[i]))
    return worst


def model_of(preset, prec):
    return wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, prec)


# ---- 1. f32 against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset", ["nano", "micro"])
def test_f32_matches_the_oracle_at_every_edge(gpu, preset):
    prompt, eot = setup(preset)
    ctx = wb.Context(model_of(preset, wb.WH_PREC_F32), 160)   # 143 rows at n = 140: one hypothesis per call
    p = wb.DecodeParams(prompt, 1, eot)
    ctx.transcribe_batch([ms.synth_clip(1500)], p)
    full = draw(preset, max(LENGTHS))
    total = near = 0
    for n in LENGTHS:
        toks = full[:n]   # (prefixes of one history: the oracle runs once per distinct history)
        lp, am, lg = ctx.score_tokens(p, [toks], 1, [0])
        k, m = check_against_oracle(preset, 1500, toks, lp[0], am[0], lg[0], history=full)
        total, near = total + k, near + m
    print(f"{preset} f32: {total} entries, {near} under the {MARGIN} margin")
    assert near * 8 <= total
    ctx.close()


# ---- 2. internal consistency on every supported configuration --------------------------------------------------------------------------
CONFIGS = [   # (preset, precision, cross_es, max_batch, clips, H, lengths of the hypotheses of a clip)
    ("nano", wb.WH_PREC_F32, None, 96, 3, 2, (9, 20)),
    ("base", wb.WH_PREC_BF16, False, 128, 3, 2, (7, 24)),      # K / V planes
    ("base", wb.WH_PREC_BF16, True, 128, 3, 2, (7, 24)),       # encoder states
    ("base", wb.WH_PREC_BF16, None, 1024, 8, 1, (124,)),       # 8 x 127 = 1016 rows, WH_DEC_TILE=1: the tile GEMMs and the tile LM head
]


@pytest.mark.parametrize("preset,prec,cross_es,max_batch,ncl,H,lens", CONFIGS)
def test_outputs_follow_the_definition_on_the_calls_own_logits(gpu, monkeypatch, preset, prec, cross_es, max_batch, ncl, H, lens):
    if max_batch >= 1024:
        monkeypatch.setenv("WH_DEC_TILE", "1")
    prompt, eot = setup(preset)
    ctx = wb.Context(model_of(preset, prec), max_batch, cross_es=cross_es)
    if cross_es is not None:
        assert ctx.cross_mode == int(cross_es)
    hyps = [draw(preset, lens[j] - (b % 2 if lens[j] > 2 else 0), seed=100 + b * H + j) for b in range(ncl) for j in range(H)]
    suppress, begin = [eot, hyps[0][1] if len(hyps[0]) > 1 else 0], [hyps[-1][0]]
    p = wb.DecodeParams(prompt, 1, eot, suppress, begin)
    ctx.transcribe_batch([ms.synth_clip(1500 + b) for b in range(ncl)], p)
    sel = list(range(len(hyps))) if max_batch < 1024 else [0, len(hyps) // 2, len(hyps) - 1]
    lp, am, lg = ctx.score_tokens(p, hyps, H, sel)
    assert max(len(h) for h in hyps) + len(prompt) - 1 <= max_batch // H
    worst = 0.0
    for j, g in enumerate(sel):
        assert np.isfinite(lg[j]).all()
        worst = max(worst, check_self(hyps[g], lp[g], am[g], lg[j], suppress, begin))
    assert lp[0][1] == -np.inf if len(hyps[0]) > 1 else True
    print(f"{preset} prec {prec} cross_es {cross_es} {max_batch}-row context: max |logprob - restatement| {worst:.3g} over {sum(len(hyps[g]) for g in sel)} entries")
    ctx.close()


# ---- 3. bf16 against the golden vectors ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cross_es", [False, True])
def test_bf16_logits_match_the_golden_vectors(gpu, golden_dir, cross_es):
    g = {c: np.load(os.path.join(golden_dir, f"base_s1234_c{c}.npz")) for c in (0, 3)}
    prompt, eot = g[0]["prompt"].tolist(), int(g[0]["eot"])
    ctx = wb.Context(model_of("base", wb.WH_PREC_BF16), 64, cross_es=cross_es)
    p = wb.DecodeParams(prompt, 1, eot)
    ctx.transcribe_batch([ms.synth_clip(0), ms.synth_clip(3)], p)
    hyps = [g[c]["forced_c"].tolist() + [eot] for c in (0, 3)]
    assert all(len(h) == 24 for h in hyps)
    lp, am, lg = ctx.score_tokens(p, hyps, 1, [0, 1])
    for j, c in enumerate((0, 3)):
        err = max(float(np.abs(lg[j][i][g[c]["top_ids_c"][i]] - g[c]["top_vals_c"][i]).max()) for i in range(24))
        print(f"bf16 base clip {c} cross_es {cross_es}: max |logit - golden| over 24 entries {err:.4f}")
        assert err < BF16_GOLDEN
    ctx.close()


# ---- 4. against the library's own forced loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,prec", [("nano", wb.WH_PREC_F32), ("base", wb.WH_PREC_BF16)])
def test_agrees_with_the_forced_token_loop(gpu, preset, prec):
    prompt, eot = setup(preset)
    ctx = wb.Context(model_of(preset, prec), 128)
    suppress, begin = [eot], [11]
    p = wb.DecodeParams(prompt, 1, eot, suppress, begin)
    ncl = 3
    ctx.transcribe_batch([ms.synth_clip(1500 + b) for b in range(ncl)], p)
    hyps = [draw(preset, n, seed=300 + b) for b, n in enumerate((5, 17, 30))]
    lp, am, lg = ctx.score_tokens(p, hyps, 1, list(range(ncl)))
    worst, near, total = 0.0, 0, 0
    for b, t in enumerate(hyps):
        toks, ll = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, len(t), eot, suppress, begin, forced=t[:-1]), [b])
        assert ll[0].shape == lg[b].shape
        diff = float(np.abs(ll[0] - lg[b]).max())
        worst = max(worst, diff)
        if prec == wb.WH_PREC_F32:
            assert diff <= LOGIT_TOL, (b, diff)
            rec = toks[b][len(prompt):].tolist()
            for i in range(len(t)):
                total += 1
                if sr.top1_margin(ll[0][i], i, suppress, begin) > MARGIN:
                    assert rec[i] == int(am[b][i]), (b, i, rec[i], int(am[b][i]))
                else:
                    near += 1
        else:
            assert diff <= BF16_LOOP, (b, diff)
    print(f"{preset} prec {prec}: max |scoring logit - token-loop logit| {worst:.3g}; {near} of {total} entries under the margin")
    assert near * 8 <= max(total, 8)
    ctx.close()


# ---- 5. several hypotheses per clip and several passes ---------------------------------------------------------------------------------------
def test_hypotheses_per_clip_and_passes(gpu):
    preset, ncl, H = "nano", 5, 3
    prompt, eot = setup(preset)
    lens = [[20, 3, 11], [1, 17, 8], [16, 16, 2], [5, 19, 13], [9, 1, 20]]
    hyps = [draw(preset, lens[b][j], seed=500 + b * H + j) for b in range(ncl) for j in range(H)]
    T = len(prompt) + 20 - 1
    p = wb.DecodeParams(prompt, 1, eot)
    clips = [ms.synth_clip(1500 + b) for b in range(ncl)]
    results = []
    for max_batch in (2 * H * T + 2, ncl * H * T + 7):   # 2 clips per pass: 3 passes; everything in one pass
        ctx = wb.Context(model_of(preset, wb.WH_PREC_F32), max_batch)
        ctx.transcribe_batch(clips, p)
        lp, am, lg = ctx.score_tokens(p, hyps, H, list(range(ncl * H)))
        lp2, am2, lg2 = ctx.score_tokens(p, hyps, H, list(range(ncl * H)))
        total = near = 0
        for g, t in enumerate(hyps):
            assert lp[g].tobytes() == lp2[g].tobytes() and am[g].tolist() == am2[g].tolist() and lg[g].tobytes() == lg2[g].tobytes()
            k, m = check_against_oracle(preset, 1500 + g // H, t, lp[g], am[g], lg[g])
            total, near = total + k, near + m
        assert near * 8 <= total
        results.append((lp, am))
        ctx.close()
    for g in range(ncl * H):   # (two row layouts of the same hypotheses: the same values up to the oracle bound, twice)
        np.testing.assert_allclose(results[0][0][g], results[1][0][g], rtol=0, atol=2 * LP_TOL_ORACLE)


# ---- 6. masks ---------------------------------------------------------------------------------------------------------------------------
def test_masks(gpu):
    preset = "nano"
    prompt, eot = setup(preset)
    hyps = [draw(preset, 12, seed=600), draw(preset, 9, seed=601)]
    free = [i for i in range(100, 130) if i not in hyps[0] and i not in hyps[1]]
    hyps[1] = [free[1] if t == hyps[0][4] else t for t in hyps[1]]   # the suppressed id occurs in hypothesis 0 only ...
    hyps[1][0] = hyps[1][3] = free[0]             # ... begin_suppress's id in hypothesis 1 only, again at a later entry: allowed there
    suppress, begin = [hyps[0][4]], [hyps[1][0]]
    assert suppress[0] not in hyps[1] and begin[0] not in hyps[0]
    p = wb.DecodeParams(prompt, 1, eot, suppress, begin)
    ctx = wb.Context(model_of(preset, wb.WH_PREC_F32), 64)
    ctx.transcribe_batch([ms.synth_clip(1500), ms.synth_clip(1501)], p)
    lp, am, lg = ctx.score_tokens(p, hyps, 1, [0, 1])
    hit0 = [i for i, t in enumerate(hyps[0]) if t == suppress[0]]
    assert 4 in hit0 and all(lp[0][i] == -np.inf for i in hit0)
    assert all(np.isfinite(lp[0][i]) for i in range(12) if i not in hit0)
    assert lp[1][0] == -np.inf and np.isfinite(lp[1][1:]).all()      # entry 0 only
    assert suppress[0] not in am[0].tolist() + am[1].tolist() and am[0][0] != begin[0] and am[1][0] != begin[0]
    for g in range(2):
        check_self(hyps[g], lp[g], am[g], lg[g], suppress, begin)
    # the unmasked call differs exactly where a mask hit or moved the sum
    lp0, _, _ = ctx.score_tokens(wb.DecodeParams(prompt, 1, eot), hyps, 1)
    assert np.isfinite(lp0[0]).all() and np.isfinite(lp0[1]).all()
    ctx.close()


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("preset,prec,cross_es", [("nano", wb.WH_PREC_F32, None), ("base", wb.WH_PREC_BF16, True)])
def test_a_decode_after_scoring_returns_what_it_returned_before(gpu, preset, prec, cross_es):
    prompt, eot = setup(preset)
    nb = 64
    ctx = wb.Context(model_of(preset, prec), nb, cross_es=cross_es)
    p = wb.DecodeParams(prompt, 12, eot, [eot])
    A = [t.tolist() for t in ctx.transcribe_batch([ms.synth_clip(1500 + (b % 8)) for b in range(nb)], p)]
    before = [t.tolist() for t in ctx.greedy_decode_resident_batch(p)[0]]   # (captures the step graph the later call replays)
    assert before == A
    hyps = [a[len(prompt):len(prompt) + 8] for a in A]
    lp, am, _ = ctx.score_tokens(p, hyps, 1)
    assert all(np.isfinite(x).all() for x in lp)
    after = [t.tolist() for t in ctx.greedy_decode_resident_batch(p)[0]]
    assert after == A
    ctx.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------
def refused(ctx, code, fn):
    with pytest.raises(wb.WhisperHipError) as ei:
        fn()
    assert ei.value.code == code, (ei.value.code, str(ei.value))
    assert (ctx.lib.wh_last_error(ctx.h) or b"").decode() != ""


def test_refusals(gpu):
    import ctypes as C
    preset = "nano"
    prompt, eot = setup(preset)
    d = ms.PRESETS[preset]
    model = model_of(preset, wb.WH_PREC_F32)
    ctx = wb.Context(model, 32)
    p = wb.DecodeParams(prompt, 4, eot)
    clips = [ms.synth_clip(1500), ms.synth_clip(1501)]
    hyps = [[5, 6, 7], [8, 9]]
    ARG, STATE, UNSUPPORTED = 4, 3, 8

    def good():
        lp, am, _ = ctx.score_tokens(p, hyps, 1)
        assert [len(x) for x in lp] == [3, 2] and all(np.isfinite(x).all() for x in lp)

    refused(ctx, STATE, lambda: ctx.score_tokens(p, hyps, 1))                       # no resident states
    ctx.transcribe_batch(clips, p)
    good()

    def raw(struct_size=None, ids=None, offsets=None, n_hyp=2, H=1, cap=3, sel=(), cap_rows=3, want_logits=False, params=p):
        pc, keep = params.to_c()
        ids = np.asarray([5, 6, 7, 8, 9] if ids is None else ids, np.int64)
        offsets = np.asarray([0, 3, 5] if offsets is None else offsets, np.uint64)
        inp = wb.WhScoreInput(C.sizeof(wb.WhScoreInput) if struct_size is None else struct_size, ids.ctypes.data_as(C.POINTER(C.c_int64)),
                              offsets.ctypes.data_as(C.POINTER(C.c_size_t)), n_hyp, H)
        lp = np.zeros((max(n_hyp, 1), max(cap, 1)), np.float32)
        s = np.asarray(list(sel), np.int32)
        lg = np.zeros((max(len(s), 1), max(cap_rows, 1), d.vocab), np.float32)
        ctx._check(ctx.lib.wh_score_tokens(ctx.h, C.byref(pc), C.byref(inp), lp.ctypes.data_as(C.POINTER(C.c_float)), None, cap,
                                           s.ctypes.data_as(C.POINTER(C.c_int32)) if len(s) else None, len(s),
                                           lg.ctypes.data_as(C.POINTER(C.c_float)) if want_logits else None, cap_rows))

    raw()                                                                            # (the raw form of the good call)
    for kw in (dict(struct_size=8),                                                  # wrong struct_size
               dict(offsets=[1, 3, 5]), dict(offsets=[0, 3, 3]), dict(offsets=[0, 4, 3]),   # bad offsets (an empty hypothesis included)
               dict(ids=[5, 6, d.vocab, 8, 9]), dict(ids=[5, -1, 7, 8, 9]),          # an id outside [0, vocab)
               dict(n_hyp=1, offsets=[0, 3]), dict(H=2),                             # n_hyp != resident clips * H
               dict(params=wb.DecodeParams(prompt, 4, eot, forced=[1])),             # n_forced != 0
               dict(cap=2),                                                          # cap_tokens below the longest hypothesis
               dict(sel=[2], want_logits=True), dict(sel=[-1], want_logits=True),    # logit_hyps out of range
               dict(sel=[0], want_logits=True, cap_rows=2)):                         # cap_logits_rows too small
        refused(ctx, ARG, lambda: raw(**kw))
        good()
    long_h = list(range(d.n_text_ctx - len(prompt) + 1))
    refused(ctx, ARG, lambda: ctx.score_tokens(p, [long_h, [1]], 1))                 # P + longest > n_text_ctx
    good()
    refused(ctx, ARG, lambda: ctx.score_tokens(p, [list(range(30)), [1]], 1))        # H * T = 33 > max_batch 32
    good()
    # options set on the ctx
    tb = d.vocab - 301
    for on, off in ((lambda: ctx.set_timestamp_rules(tb, tb - 1, 50), ctx.clear_timestamp_rules),
                    (lambda: ctx.set_repetition(1.2, 0), ctx.clear_repetition),
                    (lambda: ctx.set_sampling(1, [0.5, 0.5]), ctx.clear_sampling),
                    (lambda: ctx.set_beam_search(2), ctx.clear_beam_search),
                    (lambda: ctx.set_alignment([(0, 0)]), ctx.clear_alignment),
                    (lambda: ctx.set_language_detection([20, 21], 0), ctx.clear_language_detection),
                    (lambda: ctx.set_prefixes([[4, 5], []]), ctx.clear_prefixes)):
        on()
        refused(ctx, UNSUPPORTED, lambda: ctx.score_tokens(p, hyps, 1))
        off()
        good()
    ctx.set_prefixes([[], []])                                                        # an empty prefix set is no prefix
    good()
    ctx.clear_prefixes()
    # states that belong to a prefetched batch
    hip = wb.HipRuntime()
    dp = hip.upload(0, np.stack(clips))
    try:
        ctx.transcribe_batch_device(dp, 2, p, dp, 2)
        refused(ctx, STATE, lambda: ctx.score_tokens(p, hyps, 1))
        ctx.transcribe_batch_device(dp, 2, p)
        good()
    finally:
        hip.free(dp)
    ctx.close()
    # precision modes without a rows_per_clip cross-attention kernel
    prompt, eot = setup("micro")
    p = wb.DecodeParams(prompt, 4, eot)
    for prec in (wb.WH_PREC_FP8, wb.WH_PREC_F16X3):
        c2 = wb.Context(model_of("micro", prec), 8)
        toks = c2.transcribe_batch(clips, p)
        refused(c2, UNSUPPORTED, lambda: c2.score_tokens(p, hyps, 1))
        assert [t.tolist() for t in c2.greedy_decode_resident_batch(p)[0]] == [t.tolist() for t in toks]   # the ctx stays usable
        c2.close()
