"""CPU checks of the log-probability feature: the numpy restatement against a brute-force softmax, the host library's avg_logprob,
silence rule and segment JSON, the C entries without a device, and the CLI's flags."""
import math
import os
import subprocess

import numpy as np
import pytest

import logprob_ref as lr
import timestamp_rules_ref as tr
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")

# a small vocabulary: 0..9 text, 10 = EOT, 11 = <|nospeech|>, 12 special, 13 = <|notimestamps|>, 14.. = timestamps (tb = 14)
V, EOT, NOSP, NOTS, TB = 40, 10, 11, 13, 14


def brute(x, allowed):
    """log-softmax over the allowed ids, term by term in Python floats: (argmax, its log-probability)."""
    ids = [i for i in range(len(x)) if allowed[i] and not math.isnan(x[i]) and x[i] > -math.inf]
    if not ids:
        return 0, -math.inf
    best = max(ids, key=lambda i: (x[i], -i))
    return best, -math.log(sum(math.exp(float(x[i]) - float(x[best])) for i in ids))


def test_restatement_against_brute_force_softmax():
    rng = np.random.default_rng(5)
    for trial in range(40):
        x = rng.normal(0, 4, V).astype(np.float32)
        x[rng.integers(0, V, 3)] = -np.inf
        if trial % 3 == 0:
            x[rng.integers(0, V)] = np.nan
        suppress = [int(i) for i in rng.integers(0, V, 4)]
        tok, lp, _ = lr.token_logprob(x, [1, 2], EOT, suppress)
        allowed = [i not in suppress for i in range(V)]
        bt, bl = brute(x, allowed)
        assert tok == bt and lp == pytest.approx(bl, abs=1e-12)
        # rules on: the allowed set is rule_mask, text removed when rule 5 fires
        seq = [[], [TB + 2], [TB + 2, 3], [TB + 2, 3, TB + 5, TB + 5]][trial % 4]
        tok, lp, margin = lr.token_logprob(x, seq, EOT, suppress, (), (TB, NOTS, 50))
        ok = tr.rule_mask(V, seq, TB, EOT, NOTS, 50, suppress)
        ref_tok, lse, mt = tr.apply_rules(x, seq, TB, EOT, NOTS, 50, suppress)
        if lse > mt:
            ok[:TB] = False
        bt, bl = brute(x, ok)
        assert tok == bt == ref_tok and lp == pytest.approx(bl, abs=1e-12)
        assert margin == pytest.approx(abs(lse - mt)) or not (math.isfinite(lse) or math.isfinite(mt))


def test_restatement_edge_cases():
    x = np.full(V, -np.inf, np.float32)
    assert lr.token_logprob(x, [], EOT) == (0, -math.inf, math.inf)            # nothing allowed: token 0, -inf
    x[7] = 3.0
    assert lr.token_logprob(x, [], EOT)[:2] == (7, 0.0)                        # one id: probability 1
    x[9] = 3.0
    tok, lp, _ = lr.token_logprob(x, [], EOT)
    assert tok == 7 and lp == pytest.approx(-math.log(2))                      # a tie: the lowest id, half the mass
    assert lr.token_logprob(x, [], EOT, suppress=[7])[:2] == (9, 0.0)
    y = np.zeros(V, np.float32)
    assert lr.no_speech_prob(y, NOSP) == pytest.approx(1 / V)
    y[NOSP] = np.log(V - 1)
    assert lr.no_speech_prob(y, NOSP) == pytest.approx(0.5)


def test_avg_logprob_hand_made_cases():
    lp = [-0.5, -1.5, -1.0, -3.0]
    assert wb.avg_logprob(lp, [4, 5, 6, EOT], EOT) == pytest.approx(-6.0 / 4)        # EOT emitted: its value in the sum, not in the length
    assert wb.avg_logprob(lp, [4, 5, 6, 7], EOT) == pytest.approx(-6.0 / 5)          # cut at max_new_tokens: every token counts
    assert wb.avg_logprob(lp, [4, EOT, 6, 7], EOT) == pytest.approx(-2.0 / 2)        # nothing after the first EOT
    assert wb.avg_logprob([-2.0], [EOT], EOT) == pytest.approx(-2.0)                 # EOT alone
    assert wb.avg_logprob([], [], EOT) == 0.0                                        # empty
    for toks in ([4, 5, 6, EOT], [4, 5, 6, 7], [EOT, 1, 2, 3]):
        assert wb.avg_logprob(lp, toks, EOT) == pytest.approx(lr.avg_logprob(lp, toks, EOT))


def test_segment_json_carries_the_fields_only_when_supplied():
    L = wb.load_host_library()
    gen = np.ascontiguousarray([TB, 3, 4, TB + 5, TB + 5, 6, TB + 9, EOT], np.int64)
    ll = wb.C.POINTER(wb.C.c_longlong)

    def text(call):
        n = call(None, 0)
        buf = wb.C.create_string_buffer(n + 1)
        call(buf, n + 1)
        return buf.value.decode()

    plain = text(lambda o, c: L.whh_segments_json(gen.ctypes.data_as(ll), gen.size, TB, EOT, 30.0, o, c))
    assert plain == ('[{"start": 0.000000, "end": 0.100000, "tokens": [3, 4]}, {"start": 0.100000, "end": 0.180000, "tokens": [6]}]')   # today's string
    conf = text(lambda o, c: L.whh_segments_conf_json(gen.ctypes.data_as(ll), gen.size, TB, EOT, 30.0, -0.25, 0.125, o, c))
    assert conf == ('[{"start": 0.000000, "end": 0.100000, "tokens": [3, 4], "avg_logprob": -0.25, "no_speech_prob": 0.125}, '
                    '{"start": 0.100000, "end": 0.180000, "tokens": [6], "avg_logprob": -0.25, "no_speech_prob": 0.125}]')
    segs = wb.split_segments(gen, TB, EOT, 30.0)
    assert all(set(s) == {"start", "end", "tokens"} for s in segs)
    segs = wb.split_segments(gen, TB, EOT, 30.0, -0.25, 0.125)
    assert len(segs) == 2 and all(s["avg_logprob"] == -0.25 and s["no_speech_prob"] == 0.125 for s in segs)


def test_threshold_rule_on_both_sides_of_each_threshold():
    # openai's defaults: skipped when no_speech_prob > 0.6 and avg_logprob < -1.0
    assert wb.skip_window(0.7, -1.5, 0.6, -1.0) is True
    assert wb.skip_window(0.5, -1.5, 0.6, -1.0) is False       # speech likely
    assert wb.skip_window(0.7, -0.5, 0.6, -1.0) is False       # the decoder was sure of its text
    assert wb.skip_window(0.5, -0.5, 0.6, -1.0) is False
    assert wb.skip_window(0.6, -1.5, 0.6, -1.0) is False       # strict on both sides
    assert wb.skip_window(0.7, -1.0, 0.6, -1.0) is False
    assert wb.skip_window(0.7, -math.inf, 0.6, -1.0) is True
    assert wb.skip_window(0.99, -9.0) is False                 # both off
    assert wb.skip_window(0.99, -9.0, None, -1.0) is False     # no no-speech threshold: nothing is skipped
    assert wb.skip_window(0.7, -0.1, 0.6, None) is True        # no log-probability threshold: the no-speech test alone
    for ns, lp in ((0.7, -1.5), (0.5, -1.5), (0.7, -0.5), (0.6, -1.0)):
        for a, b in ((0.6, -1.0), (None, -1.0), (0.6, None), (None, None)):
            assert wb.skip_window(ns, lp, a, b) == lr.skip_window(ns, lp, a, b)


def test_no_speech_token_of_the_multilingual_vocabulary():
    assert wb.no_speech_token() == 50362


def test_c_entries_refuse_null_without_a_device():
    lib = wb.load_library()
    o = wb.WhLogprobOpts(wb.C.sizeof(wb.WhLogprobOpts), -1, 0)
    assert lib.wh_ctx_set_logprobs(None, wb.C.byref(o)) == 4
    assert lib.wh_ctx_set_logprobs(None, None) == 4
    n = wb.C.c_size_t(0)
    buf = np.zeros(4, np.float32)
    assert lib.wh_get_logprobs(None, buf.ctypes.data_as(wb.C.POINTER(wb.C.c_float)), 4, None, 1, wb.C.byref(n)) == 4
    assert lib.wh_abi_version() == 1
    assert "wh_ctx_set_logprobs" in wb.EXPORTS and "wh_get_logprobs" in wb.EXPORTS


def test_cli_help_lists_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    for flag in ("--logprobs", "--no-speech-threshold", "--logprob-threshold"):
        assert flag in r.stdout
    assert "0.6" in r.stdout and "-1.0" in r.stdout


def test_cli_synthetic_clip_is_exported():
    x = wb.cli_synthetic_clip(1000)
    assert x.shape == (wb.WH_CLIP_SAMPLES,) and x.dtype == np.float32 and np.abs(x).max() <= 1.0 and 0.05 < x.std() < 0.5
    assert np.array_equal(x, wb.cli_synthetic_clip(1000)) and not np.array_equal(x, wb.cli_synthetic_clip(1001))
