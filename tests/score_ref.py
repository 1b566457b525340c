"""Numpy restatement (float64) of wh_score_tokens' definition (include/whisper_hip.h): per entry of a hypothesis the log-probability of the
given token under the softmax over the allowed ids, and the masked argmax — the reference tests/test_score_cpu.py and
tests/test_score_gpu.py hold the library to.  Not collected as tests."""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np


def allowed(v: np.ndarray, entry: int, suppress: Sequence[int] = (), begin_suppress: Sequence[int] = ()) -> np.ndarray:
    """Boolean [vocab]: not in `suppress`, not in `begin_suppress` at entry 0, and a logit that is neither NaN nor -inf."""
    x = np.asarray(v, np.float64)
    ok = np.ones(x.size, bool)
    ok[[i for i in suppress if 0 <= i < x.size]] = False
    if entry == 0:
        ok[[i for i in begin_suppress if 0 <= i < x.size]] = False
    with np.errstate(invalid="ignore"):
        ok &= x > -np.inf   # (NaN: not greater)
    return ok


def score_ref(logits: np.ndarray, targets: Sequence[int], suppress: Sequence[int] = (), begin_suppress: Sequence[int] = ()) -> Tuple[np.ndarray, np.ndarray]:
    """logits [n][vocab] (row i = the raw logits of entry i), targets [n] -> (logprob float64 [n], argmax int64 [n]).
    logprob[i] = v[t] - (m + log(sum_allowed exp(v - m))), m the largest allowed logit; -inf if t is not allowed.  argmax[i] = the allowed id
    with the largest logit, ties to the lowest id; nothing allowed: 0 and -inf."""
    logits = np.asarray(logits)
    n = len(targets)
    assert logits.shape[0] >= n
    lp = np.full(n, -np.inf, np.float64)
    am = np.zeros(n, np.int64)
    for i, t in enumerate(targets):
        x = np.asarray(logits[i], np.float64)
        ok = allowed(x, i, suppress, begin_suppress)
        if not ok.any():
            continue
        m = x[ok].max()
        am[i] = int(np.flatnonzero(ok & (x == m))[0])
        if ok[int(t)]:
            lp[i] = (x[int(t)] - m) - np.log(np.exp(x[ok] - m).sum())
    return lp, am


def top1_margin(v: np.ndarray, entry: int, suppress: Sequence[int] = (), begin_suppress: Sequence[int] = ()) -> float:
    """Distance between the two largest allowed logits (inf with fewer than two allowed ids)."""
    x = np.asarray(v, np.float64)
    y = np.sort(x[allowed(x, entry, suppress, begin_suppress)])
    return float(y[-1] - y[-2]) if y.size >= 2 else float("inf")
