"""Numpy restatement of the temperature sampling of wh_ctx_set_sampling (include/whisper_hip.h): Philox4x32-10, the uniform
draw, the Gumbel score and one position's choice — the reference tests/test_sample_cpu.py and tests/test_sample_gpu.py hold the library to.
Also a Python form of the fallback ladder the CLI runs above the C ABI.  All arithmetic that decides something is float32, as the definition
says.  Not collected as tests."""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

import logprob_ref as lr

F = np.float32
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter: Sequence[int], key: Sequence[int]) -> Tuple[int, int, int, int]:
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) on Python integers."""
    c0, c1, c2, c3 = (int(x) & MASK for x in counter)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & MASK, p1 & MASK, ((p0 >> 32) ^ c3 ^ k1) & MASK, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_block(blocks, g, row_id, seed: int) -> np.ndarray:
    """The same, vectorised: uint32 [...][4] for counters (blocks, g, row_id low, row_id high) under the key (seed low, seed high);
    blocks, g and row_id broadcast against each other."""
    blocks, g, row_id = np.broadcast_arrays(np.asarray(blocks, np.uint64), np.asarray(g, np.uint64), np.asarray(row_id, np.uint64))
    m = np.uint64(MASK)
    c0, c1, c2, c3 = blocks & m, g & m, row_id & m, (row_id >> np.uint64(32)) & m
    k0, k1 = int(seed) & MASK, (int(seed) >> 32) & MASK
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # (32 x 32 -> 64 bits: no overflow)
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def uniform(x) -> np.ndarray:
    """u = ((x >> 9) + 0.5f) * 2^-23 in float32: exact, strictly inside (0, 1)."""
    return (((np.asarray(x, np.uint32) >> np.uint32(9)).astype(F) + F(0.5)) * F(2.0 ** -23)).astype(F)


def gumbel(u) -> np.ndarray:
    """-logf(-logf(u)) in float32."""
    u = np.asarray(u, F)
    return (-np.log(-np.log(u, dtype=F), dtype=F)).astype(F)


def draws(vocab: int, g: int, row_id: int, seed: int) -> np.ndarray:
    """The Gumbel score of every id at generated position g of the stream (seed, row_id): id i takes word i & 3 of block i >> 2."""
    x = philox_block(np.arange((vocab + 3) // 4), g, row_id, seed).reshape(-1)[:vocab]
    return gumbel(uniform(x))


def step(logits: np.ndarray, history: Sequence[int], T: float, seed: int, row_id: int, g: int, eot: int, suppress: Sequence[int] = (),
         begin_suppress: Sequence[int] = (), rules: Optional[Tuple[int, int, int]] = None) -> Tuple[int, float, float, float, float]:
    """One generated position of one row: (token, its log-probability, the margin between the best and the second-best perturbed allowed
    value, rule 5's margin, delta).  history = the row's fed tokens so far.  T == 0: plain argmax (the margin is that of the raw values).
    delta = 8 x the float32 spacing at max(1, max|z| + max|gum|): the band below which a margin is undecided.  Nothing allowed: (0, -inf,
    inf, margin5, delta)."""
    v = np.asarray(logits, F)
    ok, r5 = lr.allowed_set(v, history, eot, suppress, begin_suppress, rules)
    ok &= v > F(-np.inf)
    if not ok.any():
        return 0, float("-inf"), float("inf"), r5, 0.0
    ids = np.flatnonzero(ok)
    if T > 0:
        inv_t = F(1.0) / F(T)
        z = (v[ids] * inv_t).astype(F)
        gum = draws(v.size, g, row_id, seed)[ids]
        score = (z + gum).astype(F)
        scale = max(1.0, float(np.abs(z).max()) + float(np.abs(gum).max()))
    else:
        score = v[ids]
        scale = max(1.0, float(np.abs(score).max()))
    best = score.max()
    k = int(np.argmax(score == best))                          # ties: the lowest id
    tok = int(ids[k])
    rest = np.delete(score, k)
    margin = float(np.float64(best) - np.float64(rest.max())) if rest.size else float("inf")
    x = v[ids].astype(np.float64)
    m = x.max()
    lp = float(np.float64(v[tok]) - (m + np.log(np.exp(x - m).sum())))
    return tok, lp, margin, r5, 8.0 * float(np.spacing(F(scale)))


# ---- the fallback ladder above the C ABI (whisper_bench; host/wh_host.h) --------------------------------------------------------------------

def needs_fallback(cr: float, avg_lp: float, no_speech_prob: float, cr_thr: Optional[float], lp_thr: Optional[float], ns_thr: Optional[float]) -> bool:
    """openai-whisper's decode_with_fallback: too repetitive or too unlikely, unless the window counts as silence.  None: threshold off."""
    need = (cr_thr is not None and cr > cr_thr) or (lp_thr is not None and avg_lp < lp_thr)
    if ns_thr is not None and no_speech_prob > ns_thr:
        need = False
    return bool(need)


def ladder(n_windows: int, temperatures: Sequence[float], decode: Callable[[float, List[int]], List[Tuple[float, float, float]]],
           cr_thr: Optional[float], lp_thr: Optional[float], ns_thr: Optional[float]) -> Tuple[List[int], List[List[int]]]:
    """decode(T, rows) -> [(compression_ratio, avg_logprob, no_speech_prob)] of the listed windows.  Returns (rung index that produced
    each window's result, the windows decoded at each rung)."""
    rung_of = [0] * n_windows
    todo, log = list(range(n_windows)), []
    for r, T in enumerate(temperatures):
        if not todo:
            break
        log.append(list(todo))
        res = decode(T, todo)
        nxt = []
        for w, (cr, lp, ns) in zip(todo, res):
            rung_of[w] = r
            if needs_fallback(cr, lp, ns, cr_thr, lp_thr, ns_thr):
                nxt.append(w)
        todo = nxt
    return rung_of, log
