"""Numpy restatement of Whisper's timestamp rules (openai-whisper's ApplyTimestampRules, greedy) and a Python form of the segment
splitter — the references tests/test_timestamps_cpu.py and tests/test_timestamps_gpu.py hold the library to.  Not collected as tests."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

TIME_PRECISION = 0.02


def rule_mask(vocab: int, seq: Sequence[int], tb: int, eot: int, no_ts: int = -1, max_init: int = 50,
              suppress: Sequence[int] = (), begin_suppress: Sequence[int] = ()) -> np.ndarray:
    """Boolean [vocab]: True where an id survives the suppress masks and steps 1-4 at a position whose generated history is `seq`."""
    ok = np.ones(vocab, bool)
    ok[[i for i in suppress if 0 <= i < vocab]] = False
    if len(seq) == 0:
        ok[[i for i in begin_suppress if 0 <= i < vocab]] = False
    if 0 <= no_ts < vocab:                                    # 1
        ok[no_ts] = False
    last_ts = len(seq) >= 1 and seq[-1] >= tb
    pen_ts = len(seq) < 2 or seq[-2] >= tb
    if last_ts:                                               # 2
        if pen_ts:
            ok[tb:] = False
        else:
            ok[:eot] = False
    ts_hist = [t for t in seq if t >= tb]
    if ts_hist:                                               # 3
        last = ts_hist[-1] if (last_ts and not pen_ts) else ts_hist[-1] + 1
        ok[tb:last] = False
    if len(seq) == 0:                                         # 4
        ok[:tb] = False
        if max_init >= 0:
            ok[tb + max_init + 1:] = False
    return ok


def apply_rules(logits: np.ndarray, seq: Sequence[int], tb: int, eot: int, no_ts: int = -1, max_init: int = 50,
                suppress: Sequence[int] = (), begin_suppress: Sequence[int] = ()) -> Tuple[int, float, float]:
    """Steps 1-6 on one logits row: (token, lse_ts, max_text).  Step 5 compares the log-sum-exp of the surviving timestamp logits
    with the largest surviving text logit (NaN left out of both); step 6 is the argmax with strict > (lowest index on ties, NaN never
    wins, nothing above -inf: 0)."""
    x = np.asarray(logits, np.float64)
    ok = rule_mask(x.size, seq, tb, eot, no_ts, max_init, suppress, begin_suppress)
    ok &= ~np.isnan(x)
    ts = x[tb:][ok[tb:]]
    ts = ts[ts > -np.inf]
    if ts.size:
        m = ts.max()
        lse = m + np.log(np.exp(ts - m).sum())
    else:
        lse = -np.inf
    text = x[:tb][ok[:tb]]
    max_text = text.max() if text.size else -np.inf
    if lse > max_text:                                        # 5
        ok[:tb] = False
    cand = np.where(ok, x, -np.inf)                           # 6
    best = cand.max()
    tok = int(np.argmax(cand == best)) if best > -np.inf else 0
    return tok, float(lse), float(max_text)


def split_segments(generated: Sequence[int], tb: int, eot: int, duration: float) -> List[dict]:
    """openai's slicing rule over one window's generated tokens (cut at the first EOT): [{start, end, tokens (text ids)}]."""
    t = []
    for x in generated:
        if x == eot:
            break
        t.append(int(x))
    is_ts = [x >= tb for x in t]
    cuts = [i for i in range(1, len(t)) if is_ts[i - 1] and is_ts[i]]
    text = lambda a, b: [t[i] for i in range(a, b) if not is_ts[i]]
    if not cuts:
        end = duration
        stamps = [x for x in t if x >= tb]
        if stamps and stamps[-1] > tb:
            end = (stamps[-1] - tb) * TIME_PRECISION
        return [{"start": 0.0, "end": end, "tokens": text(0, len(t))}]
    if len(t) >= 2 and is_ts[-1] and not is_ts[-2]:
        cuts.append(len(t))
    out, last = [], 0
    for c in cuts:
        start = (t[last] - tb) * TIME_PRECISION if is_ts[last] else 0.0   # only the first slice can open with text
        out.append({"start": start, "end": (t[c - 1] - tb) * TIME_PRECISION, "tokens": text(last, c)})
        last = c
    if last < len(t):
        rest = text(last, len(t))
        if rest:
            start = (t[last] - tb) * TIME_PRECISION if is_ts[last] else out[-1]["end"]
            out.append({"start": start, "end": duration, "tokens": rest})
    return out


def merge_windows(windows: Sequence[List[dict]], starts: Sequence[float], overlap_s: float) -> List[dict]:
    """Long-form: window k's segments shifted by its start; in the overlap of k and k+1 a segment belongs to k if it starts before
    start(k+1) + overlap_s / 2, else to k + 1."""
    out = []
    for k, segs in enumerate(windows):
        lo = -np.inf if k == 0 else starts[k] + overlap_s / 2
        hi = starts[k + 1] + overlap_s / 2 if k + 1 < len(windows) else np.inf
        for s in segs:
            s = dict(s, start=s["start"] + starts[k], end=s["end"] + starts[k])
            if lo <= s["start"] < hi:
                out.append(s)
    return out
