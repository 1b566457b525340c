"""Numpy restatement of the repetition controls of the GPU token loop (wh_ctx_set_repetition): HF's RepetitionPenaltyLogitsProcessor with
the division stated as one float32 multiplication by 1.0f / p, then HF's NoRepeatNGramLogitsProcessor — the reference
tests/test_repetition_cpu.py and tests/test_repetition_gpu.py hold the library to.  The adjusted logits compose with
timestamp_rules_ref.apply_rules and logprob_ref.token_logprob by being passed to them.  Not collected as tests."""
from __future__ import annotations

from typing import List, Optional, Sequence, Set, Tuple

import numpy as np

NO_EXEMPT = 2 ** 31 - 1


def penalised_ids(h: Sequence[int], p: float, exempt_from: int = NO_EXEMPT) -> Set[int]:
    """The distinct non-exempt ids of the history, if the penalty is on."""
    if np.float32(p) == np.float32(1.0):
        return set()
    return {int(t) for t in h if t < exempt_from}


def banned_ids(h: Sequence[int], n: int, exempt_from: int = NO_EXEMPT) -> Set[int]:
    """Ids that would close an n-gram the history already holds: with s = the last n - 1 ids of h, every h[i + n - 1] with
    h[i : i + n - 1] == s and i + n - 1 < len(h), unless exempt.  Timestamps are ordinary members of the n-grams."""
    h = [int(t) for t in h]
    if n <= 0 or len(h) + 1 < n:
        return set()
    s = h[len(h) - (n - 1):] if n > 1 else []
    out = set()
    for i in range(len(h) - (n - 1)):
        if h[i: i + n - 1] == s and h[i + n - 1] < exempt_from:
            out.add(h[i + n - 1])
    return out


def adjust(logits_f32: np.ndarray, h: Sequence[int], p: float = 1.0, n: int = 0, exempt_from: Optional[int] = None) -> np.ndarray:
    """The adjusted float32 logits of a position whose generated history is h: v' = v > 0 ? v * inv : v * p (float32, inv = 1.0f / p computed
    once) on every distinct non-exempt id of h, then -inf on the banned ids.  exempt_from = timestamp_begin with the rules on, None: no id is exempt."""
    ex = NO_EXEMPT if exempt_from is None else int(exempt_from)
    x = np.array(logits_f32, np.float32, copy=True)
    p32 = np.float32(p)
    inv = np.float32(1.0) / p32
    with np.errstate(invalid="ignore", over="ignore"):
        for t in sorted(penalised_ids(h, p, ex)):
            v = x[t]
            x[t] = np.float32(v * inv) if v > 0 else np.float32(v * p32)
    for t in banned_ids(h, n, ex):
        x[t] = -np.inf
    return x


def touched(h: Sequence[int], p: float, n: int, exempt_from: Optional[int] = None) -> Tuple[Set[int], Set[int]]:
    ex = NO_EXEMPT if exempt_from is None else int(exempt_from)
    return penalised_ids(h, p, ex), banned_ids(h, n, ex)


def greedy(logits_f32: np.ndarray, suppress: Sequence[int] = ()) -> int:
    """Argmax over the unsuppressed ids: ties to the lowest id, NaN never wins, nothing above -inf: 0."""
    x = np.asarray(logits_f32, np.float64).copy()
    x[[i for i in suppress if 0 <= i < x.size]] = -np.inf
    x[np.isnan(x)] = -np.inf
    best = x.max()
    return int(np.argmax(x == best)) if best > -np.inf else 0


def repeated_bigrams(gen: Sequence[int], exempt_from: int = NO_EXEMPT) -> List[int]:
    """Positions i >= 1 at which (gen[i-1], gen[i]) already occurred earlier in gen and gen[i] is not exempt: the positions a no-repeat
    bigram ban would have changed."""
    seen, out = set(), []
    for i in range(1, len(gen)):
        g = (int(gen[i - 1]), int(gen[i]))
        if g in seen and g[1] < exempt_from:
            out.append(i)
        seen.add(g)
    return out
