"""The repetition controls without a device: the numpy restatement (tests/repetition_ref.py) against hand-written cases, the C struct and
the exported symbol through ctypes, and the CLI's refusal of bad values before it touches a device."""
import os
import subprocess

import numpy as np
import pytest

import logprob_ref as lr
import repetition_ref as rr
import timestamp_rules_ref as tr
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
F = np.float32


def test_penalty_on_each_kind_of_logit():
    x = np.array([2.0, -2.0, 0.0, np.nan, -np.inf, 3.0, np.inf, 1.5], F)
    p = 1.3
    y = rr.adjust(x, [0, 1, 2, 3, 4, 6, 0, 1], p, 0)
    inv = F(1.0) / F(p)
    assert y.dtype == np.float32
    assert y[0] == F(F(2.0) * inv) and y[1] == F(F(-2.0) * F(p))             # positive shrinks, negative grows away from zero
    assert y[2] == 0.0 and np.isnan(y[3]) and y[4] == -np.inf and y[6] == np.inf
    assert y[5] == x[5] and y[7] == x[7]                                     # not in the history: untouched
    assert rr.greedy(y) == 6 and rr.greedy(np.array([np.nan, np.nan], F)) == 0
    # an id twice in the history is penalised once
    assert rr.adjust(x, [0, 0, 0], p, 0)[0] == F(F(2.0) * inv)
    # the stated multiplication is within one ulp of HF's division
    v = np.linspace(0.01, 30, 997).astype(F)
    got = rr.adjust(v, list(range(v.size)), p, 0)
    assert np.all(np.abs(got.astype(np.float64) - (v / F(p)).astype(np.float64)) <= np.spacing(v / F(p)))
    # p = 1: nothing moves, bit for bit; p < 1 rewards repetition
    assert np.array_equal(rr.adjust(x, [0, 1, 5], 1.0, 0), x, equal_nan=True)
    assert rr.adjust(x, [0], 0.5, 0)[0] == 4.0 and rr.adjust(x, [1], 0.5, 0)[1] == -1.0


def test_bans_for_n_1_2_3():
    x = np.arange(10, dtype=F)
    h = [4, 5, 6, 4, 5]
    assert rr.banned_ids(h, 1) == {4, 5, 6}                                  # n = 1: every id of the history
    assert rr.banned_ids(h, 2) == {6}                                        # ... 5 -> 6 seen
    assert rr.banned_ids(h, 3) == {6}                                        # ... 4 5 -> 6 seen
    assert rr.banned_ids(h + [6], 3) == {4}                                  # 5 6 -> 4 seen
    assert rr.banned_ids([1, 2, 3], 2) == set() and rr.banned_ids([], 1) == set() and rr.banned_ids(h, 0) == set()
    y = rr.adjust(x, h, 1.0, 2)
    assert y[6] == -np.inf and np.array_equal(np.delete(y, 6), np.delete(x, 6))
    assert rr.greedy(rr.adjust(x, list(range(10)), 1.0, 1)) == 0             # everything banned: 0


def test_history_shorter_than_the_ngram():
    assert rr.banned_ids([7], 3) == set()                                    # len(h) + 1 < n
    assert rr.banned_ids([7, 7], 3) == set()                                 # long enough, but no complete earlier 3-gram
    assert rr.banned_ids([7, 7, 7], 3) == {7}
    assert rr.banned_ids([], 2) == set() and rr.banned_ids([3], 2) == set()
    assert rr.banned_ids([3, 3], 2) == {3}


def test_overlapping_matches():
    assert rr.banned_ids([1, 1, 1, 2, 1, 1], 3) == {1, 2}                    # 1 1 -> 1 (overlapping itself) and 1 1 -> 2
    assert rr.banned_ids([9, 9], 2) == {9}                                   # the match may overlap the suffix
    assert rr.banned_ids([1, 2, 1, 3, 1], 2) == {2, 3}


def test_banned_and_penalised_is_banned():
    x = np.array([1.0, 5.0, 2.0], F)
    y = rr.adjust(x, [1, 1], 1.3, 2)
    assert y[1] == -np.inf and rr.greedy(y) == 2
    pen, ban = rr.touched([1, 1], 1.3, 2)
    assert pen == {1} and ban == {1}


def test_exemption_at_and_above_timestamp_begin():
    tb = 6
    x = np.array([1, 2, 3, 4, 5, 6, 7, 8], F)
    h = [5, 6, 6, 5, 6]
    y = rr.adjust(x, h, 2.0, 2, exempt_from=tb)
    assert y[6] == x[6] and y[7] == x[7]                                     # tb itself and above: neither penalised nor banned
    assert rr.adjust(x, h, 2.0, 0, exempt_from=tb)[5] == F(3.0)              # tb - 1 is an ordinary id: penalised (6 * 0.5) ...
    assert rr.banned_ids(h, 2, tb) == {5} and rr.banned_ids(h, 2) == {5, 6}  # ... and bannable; timestamps are members of the n-grams
    assert y[5] == -np.inf                                                   # 6 -> 5 was seen: a timestamp inside the matched n-gram
    assert rr.adjust(x, [6, 7, 6], 1.0, 2, exempt_from=tb)[7] == x[7]        # 6 -> 7 was seen, but 7 is exempt
    z = rr.adjust(x, h, 2.0, 2)                                              # rules off: no id is exempt
    assert z[6] == -np.inf and z[5] == -np.inf and rr.adjust(x, h, 2.0, 0)[6] == F(3.5)


def test_composes_with_the_rules_and_the_logprob_restatements():
    """The adjusted logits go to apply_rules / token_logprob as they are: rule 5 sees the largest adjusted text logit, the log-probability
    is the log-softmax of the adjusted allowed logits."""
    tb, eot = 8, 2
    x = np.full(12, -4.0, F)
    x[5], x[6], x[10] = 6.0, 5.0, 5.5
    h = [9, 5]                                                               # a timestamp, then text id 5: timestamps from 10 on are allowed
    tok, lse, mt = tr.apply_rules(x, h, tb, eot)
    assert tok == 5 and mt == 6.0
    adj = rr.adjust(x, h, 2.0, 0, exempt_from=tb)
    tok2, lse2, mt2 = tr.apply_rules(adj, h, tb, eot)
    assert adj[5] == 3.0 and adj[10] == 5.5 and mt2 == 5.0 and lse2 == lse and mt > lse2 > mt2 and tok2 == 10   # rule 5 now decides for timestamps
    t3, lp3, _ = lr.token_logprob(adj, h, eot, (), (), None)
    ref = adj.astype(np.float64)
    assert t3 == 10 and abs(lp3 - (ref[10] - np.log(np.exp(ref).sum()))) < 1e-12
    banned = rr.adjust(x, [5, 6, 5], 1.0, 2)                                 # 5 -> 6 banned: the log-softmax leaves it out
    t4, lp4, _ = lr.token_logprob(banned, [5, 6, 5], eot)
    keep = np.delete(x.astype(np.float64), 6)
    assert t4 == 5 and abs(lp4 - (6.0 - np.log(np.exp(keep).sum()))) < 1e-12


def test_repeated_bigram_positions():
    assert rr.repeated_bigrams([1, 2, 3, 1, 2, 2, 2]) == [4, 6]
    assert rr.repeated_bigrams([1, 9, 1, 9], exempt_from=9) == []


def test_struct_layout_and_exported_symbol():
    o = wb.WhRepetitionOpts
    assert wb.C.sizeof(o) == 16
    assert (o.struct_size.offset, o.repetition_penalty.offset, o.no_repeat_ngram_size.offset) == (0, 8, 12)
    assert (o.struct_size.size, o.repetition_penalty.size, o.no_repeat_ngram_size.size) == (8, 4, 4)
    assert wb.WH_MAX_NGRAM == 32
    lib = wb.load_library()
    assert "wh_ctx_set_repetition" in wb.EXPORTS and hasattr(lib, "wh_ctx_set_repetition")
    assert lib.wh_ctx_set_repetition(None, wb.C.byref(o(wb.C.sizeof(o), 1.3, 3))) == 4     # no ctx: WH_ERR_ARG, nothing dereferenced
    assert lib.wh_ctx_set_repetition(None, None) == 4
    hdr = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    assert "#define WH_MAX_NGRAM 32" in hdr and "int wh_ctx_set_repetition(wh_ctx* c, const wh_repetition_opts* o);" in hdr


@pytest.mark.parametrize("flag,value,needle", [
    ("--repetition-penalty", "0", "--repetition-penalty"), ("--repetition-penalty", "-1.5", "--repetition-penalty"),
    ("--repetition-penalty", "nan", "--repetition-penalty"), ("--repetition-penalty", "inf", "--repetition-penalty"),
    ("--repetition-penalty", "1.3x", "--repetition-penalty"),
    ("--no-repeat-ngram-size", "-1", "--no-repeat-ngram-size"), ("--no-repeat-ngram-size", "33", "--no-repeat-ngram-size"),
    ("--no-repeat-ngram-size", "two", "--no-repeat-ngram-size"),
])
def test_cli_refuses_bad_values_before_touching_a_device(flag, value, needle):
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7", flag, value, "--print-plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and needle in r.stderr and "error:" in r.stderr, (r.returncode, r.stderr)


def test_cli_accepts_good_values_and_lists_the_flags():
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7", "--repetition-penalty", "1.3", "--no-repeat-ngram-size=32", "--print-plan"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert h.returncode == 0 and "--repetition-penalty" in h.stdout and "--no-repeat-ngram-size" in h.stdout
