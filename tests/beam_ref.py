"""Numpy restatement of the beam search of wh_ctx_set_beam_search (include/whisper_hip.h), after openai-whisper's
BeamSearchDecoder and MaximumLikelihoodRanker — the reference tests/test_beam_cpu.py and tests/test_beam_gpu.py hold the library to.
All arithmetic that decides something is float32, as the definition says.  Not collected as tests."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

import timestamp_rules_ref as tr

F = np.float32
NEG = F(-np.inf)


def row_logprobs(v: np.ndarray, hist: Sequence[int], eot: int, suppress: Sequence[int] = (), begin_suppress: Sequence[int] = (),
                 rules: Optional[Tuple[int, int, int]] = None) -> Tuple[Optional[np.ndarray], float]:
    """lp [vocab] float32 of one live row (-inf where an id is not allowed), or None when nothing is allowed; and rule 5's margin
    |lse_ts - max_text| (inf without rules).  rules = (timestamp_begin, no_timestamps, max_initial_timestamp_index)."""
    x = np.asarray(v, F)
    margin = np.inf
    if rules is None:
        ok = np.ones(x.size, bool)
        ok[[i for i in suppress if 0 <= i < x.size]] = False
        if len(hist) == 0:
            ok[[i for i in begin_suppress if 0 <= i < x.size]] = False
    else:
        tb, no_ts, max_init = rules
        ok = tr.rule_mask(x.size, hist, tb, eot, no_ts, max_init, suppress, begin_suppress)
    ok &= ~np.isnan(x)
    ok &= x > NEG
    if rules is not None:
        ts = x[tb:][ok[tb:]]
        lse = F(ts.max() + np.log(np.exp(ts - ts.max(), dtype=F).sum(dtype=F))) if ts.size else NEG
        text = x[:tb][ok[:tb]]
        max_text = text.max() if text.size else NEG
        if lse > max_text:                                   # rule 5
            ok[:tb] = False
        if np.isfinite(lse) or np.isfinite(max_text):
            margin = float(abs(np.float64(lse) - np.float64(max_text)))
    if not ok.any():
        return None, margin
    m = x[ok].max()
    lse = F(m + np.log(np.exp(x[ok] - m, dtype=F).sum(dtype=F)))
    lp = np.full(x.size, NEG, F)
    lp[ok] = x[ok] - lse
    return lp, margin


def _candidates(lps: Sequence[Optional[np.ndarray]], scores: Sequence[float], per_row: Optional[int]) -> List[Tuple[float, int, int, float]]:
    """(score, beam, id, lp) of every candidate, ordered by score descending, then beam, then id.  per_row: only each row's best per_row
    ids by (lp descending, id ascending) — the top-(K + 1) shortcut; None: the whole K x V list."""
    out = []
    for j, lp in enumerate(lps):
        if lp is None or not F(scores[j]) > NEG:
            continue
        ids = np.flatnonzero(lp > NEG)
        if per_row is not None and ids.size > per_row:
            ids = ids[np.lexsort((ids, -lp[ids].astype(np.float64)))[:per_row]]
        sc = (F(scores[j]) + lp[ids]).astype(F)               # one f32 addition
        out += [(float(s), j, int(i), float(lp[i])) for s, i in zip(sc, ids) if s > NEG and not np.isnan(s)]
    out.sort(key=lambda c: (-c[0], c[1], c[2]))
    return out


def walk(cands: List[Tuple[float, int, int, float]], K: int, eot: int, pool_room: int):
    """Step 4 and 5 over an ordered candidate list: (live [(parent, token, score, lp)] padded with dead beams (j, -1, -inf, 0),
    finished [(parent, score, lp)] that enter the pool, margins [one per live slot, then one per finished entry]): a decision's margin is
    the score gap to its nearest neighbour in the order among the candidates the walk looked at and the first one it did not."""
    live, fin, taken = [], [], []
    for t, (sc, j, i, lp) in enumerate(cands):
        if i == eot:
            if len(fin) < pool_room:
                fin.append((j, sc, lp))
                taken.append(("f", t))
        else:
            live.append((j, i, sc, lp))
            taken.append(("l", t))
            if len(live) == K:
                break

    def gap(t):
        g = np.inf
        if t > 0:
            g = min(g, cands[t - 1][0] - cands[t][0])
        if t + 1 < len(cands):
            g = min(g, cands[t][0] - cands[t + 1][0])
        return g

    m_live = [gap(t) for kind, t in taken if kind == "l"]
    m_fin = [gap(t) for kind, t in taken if kind == "f"]
    # an EOT candidate the walk passed while the pool was full decides nothing; fewer live beams than K: the dead slots decide nothing
    for s in range(len(live), K):
        live.append((s, -1, float("-inf"), 0.0))
        m_live.append(np.inf)
    return live, fin, m_live + m_fin


def step(logits: np.ndarray, histories: Sequence[Sequence[int]], scores: Sequence[float], eot: int, pool_room: int,
         suppress: Sequence[int] = (), begin_suppress: Sequence[int] = (), rules: Optional[Tuple[int, int, int]] = None, full: bool = False):
    """One generated position of one clip.  logits [K][V], histories / scores of the K beams.  Returns (live, finished, margins, rule5):
    as walk(), and the smallest rule-5 margin over the live rows."""
    K = len(histories)
    lps, r5 = [], np.inf
    for j in range(K):
        if not F(scores[j]) > NEG:
            lps.append(None)
            continue
        lp, mg = row_logprobs(logits[j], histories[j], eot, suppress, begin_suppress, rules)
        lps.append(lp)
        r5 = min(r5, mg)
    live, fin, margins = walk(_candidates(lps, scores, None if full else K + 1), K, eot, pool_room)
    return live, fin, margins, r5


def rank(pool: List[dict], live: List[dict], K: int, length_penalty: float) -> List[dict]:
    """The ranked hypotheses: the pool in insertion order, then live beams by descending score until K; f32 arithmetic; stable."""
    hyps = [dict(h, finished=True) for h in pool]
    if len(hyps) < K:
        alive = sorted([h for h in live if F(h["score"]) > NEG], key=lambda h: -h["score"])
        hyps += [dict(h, finished=False) for h in alive[: K - len(hyps)]]
    for h in hyps:
        n = F(max(1, len(h["tokens"]) - (1 if h["finished"] else 0)))
        s = F(h["score"])
        h["rank"] = float(s / n) if length_penalty < 0 else float(s / np.power((F(5) + n) / F(6), F(length_penalty), dtype=F))
    return sorted(hyps, key=lambda h: -h["rank"])


def search(logits_fn: Callable[[List[List[int]]], np.ndarray], K: int, patience: float, max_new_tokens: int, eot: int,
           suppress: Sequence[int] = (), begin_suppress: Sequence[int] = (), rules: Optional[Tuple[int, int, int]] = None,
           length_penalty: float = -1.0, full: bool = False) -> dict:
    """The whole loop of one clip.  logits_fn(histories) -> [K][V] logits of the next position of every beam (dead beams' rows are not
    read).  Returns {hyps (ranked), pool, live, trace: [{parents, tokens, scores, pool_size, margins, rule5}]}."""
    C = int(np.floor(F(K) * F(patience) + F(0.5)))
    hist: List[List[int]] = [[] for _ in range(K)]
    lps: List[List[float]] = [[] for _ in range(K)]
    scores = [0.0] + [float("-inf")] * (K - 1)
    pool, trace = [], []
    for g in range(max_new_tokens):
        live, fin, margins, r5 = step(np.asarray(logits_fn(hist)), hist, scores, eot, C - len(pool), suppress, begin_suppress, rules, full)
        for j, sc, lp in fin:
            pool.append({"tokens": hist[j] + [eot], "lps": lps[j] + [lp], "score": sc})
        nh = [hist[p] + [t] if t >= 0 else list(hist[s]) for s, (p, t, _, _) in enumerate(live)]
        nl = [lps[p] + [lp] if t >= 0 else list(lps[s]) for s, (p, t, _, lp) in enumerate(live)]
        hist, lps, scores = nh, nl, [c[2] for c in live]
        trace.append({"parents": [c[0] for c in live], "tokens": [c[1] for c in live], "scores": list(scores), "pool_size": len(pool),
                      "margins": margins, "rule5": r5})
        if len(pool) >= C:
            break
    live_h = [{"tokens": hist[j], "lps": lps[j], "score": scores[j]} for j in range(K)]
    return {"hyps": rank(pool, live_h, K, length_penalty), "pool": pool, "live": live_h, "trace": trace}


def delta(score: float, vmax: float, vocab: int) -> float:
    """The undecided band of a comparison of two f32 scores: 8 x the f32 spacing at max(|score|, max|v| + log V) — one rounded addition, one
    rounded subtraction and a few-ulp logf on each side of the comparison."""
    return 8.0 * float(np.spacing(F(max(abs(score), vmax + np.log(vocab)))))
