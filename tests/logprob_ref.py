"""Numpy restatement (float64) of the token log-probability and the no-speech probability of Whisper's greedy loop (openai-whisper's
GreedyDecoder.update and DecodingTask._main_loop) and of avg_logprob — the references tests/test_logprobs_cpu.py and
tests/test_logprobs_gpu.py hold the library to.  Not collected as tests."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

import timestamp_rules_ref as tr


def allowed_set(logits: np.ndarray, seq: Sequence[int], eot: int, suppress: Sequence[int] = (), begin_suppress: Sequence[int] = (),
                rules: Optional[Tuple[int, int, int]] = None) -> Tuple[np.ndarray, float]:
    """Boolean [vocab] of the ids still allowed at a position whose generated history is `seq`, after the suppress masks and, with
    rules = (timestamp_begin, no_timestamps, max_initial_timestamp_index), the timestamp rules including rule 5; NaN logits are never
    allowed.  Also returns rule 5's margin |lse_ts - max_text| (inf without rules)."""
    x = np.asarray(logits, np.float64)
    margin = np.inf
    if rules is None:
        ok = np.ones(x.size, bool)
        ok[[i for i in suppress if 0 <= i < x.size]] = False
        if len(seq) == 0:
            ok[[i for i in begin_suppress if 0 <= i < x.size]] = False
    else:
        tb, no_ts, max_init = rules
        ok = tr.rule_mask(x.size, seq, tb, eot, no_ts, max_init, suppress, begin_suppress)
        _, lse, max_text = tr.apply_rules(x, seq, tb, eot, no_ts, max_init, suppress, begin_suppress)
        if lse > max_text:
            ok[:tb] = False
        if np.isfinite(lse) or np.isfinite(max_text):
            margin = abs(lse - max_text)
    ok &= ~np.isnan(x)
    return ok, float(margin)


def masked_log_softmax_max(logits: np.ndarray, ok: np.ndarray) -> Tuple[int, float]:
    """(argmax over the allowed ids with ties to the lowest id and 0 when nothing exceeds -inf, its log-probability under the softmax over
    the allowed ids; -inf when nothing is allowed)."""
    x = np.where(ok, np.asarray(logits, np.float64), -np.inf)
    best = x.max() if x.size else -np.inf
    if not best > -np.inf:
        return 0, float("-inf")
    tok = int(np.argmax(x == best))
    return tok, float(-np.log(np.exp(x[x > -np.inf] - best).sum()))


def token_logprob(logits: np.ndarray, seq: Sequence[int], eot: int, suppress: Sequence[int] = (), begin_suppress: Sequence[int] = (),
                  rules: Optional[Tuple[int, int, int]] = None) -> Tuple[int, float, float]:
    """(recorded token, its log-probability, rule 5's margin) of one position."""
    ok, margin = allowed_set(logits, seq, eot, suppress, begin_suppress, rules)
    tok, lp = masked_log_softmax_max(logits, ok)
    return tok, lp, margin


def no_speech_prob(logits: np.ndarray, no_speech: int) -> float:
    """softmax(logits)[no_speech] over the unfiltered logits (NaN left out of the sum)."""
    x = np.asarray(logits, np.float64)
    y = x[~np.isnan(x)]
    m = y.max()
    return float(np.exp(x[no_speech] - m - np.log(np.exp(y - m).sum())))


def avg_logprob(logprobs: Sequence[float], tokens: Sequence[int], eot: int) -> float:
    """openai's sum_logprobs / (len(tokens) + 1): the sum runs over the generated tokens up to and including the first EOT, the length
    counts the tokens before it."""
    s, n = 0.0, 0
    for lp, t in zip(logprobs, tokens):
        s += float(lp)
        if int(t) == eot:
            break
        n += 1
    return s / (n + 1)


def skip_window(no_speech_p: float, avg_lp: float, no_speech_threshold: Optional[float], logprob_threshold: Optional[float]) -> bool:
    """openai-whisper's silence rule: no_speech_prob > no_speech_threshold, unless avg_logprob > logprob_threshold.  A threshold that is
    None is off: without a no-speech threshold nothing is skipped; without a log-probability threshold the no-speech test decides alone."""
    if no_speech_threshold is None or not no_speech_p > no_speech_threshold:
        return False
    return logprob_threshold is None or avg_lp < logprob_threshold
