"""Numpy restatement of forced alignment (wh_align_tokens), wired from tests/align_ref.py:
decoder (teacher-forced over prompt ++ t[:-1]) -> probs(first_row = P - 1, n, S_b) -> pipeline -> dtw.

Row i of a hypothesis t[0 .. n) is model position P - 1 + i: the position whose logits predict t[i].  Its input token is prompt[P - 1] for
i == 0 and t[i - 1] otherwise, so the last token t[n - 1] is a target only and never enters the decoder.

Test infrastructure only: nothing here is imported by the package."""
import numpy as np

import align_ref as ar


def model_sequence(prompt, tokens):
    """The decoder's input for hypothesis `tokens`: prompt ++ tokens[:-1] (P + n - 1 positions)."""
    return [int(t) for t in prompt] + [int(t) for t in tokens[:-1]]


def rows_probs(dims, sd, enc, prompt, tokens, heads, s_b, dtype=np.float64, rnd=None):
    """P [len(heads), n, s_b] of the hypothesis's n rows."""
    _, scores = ar.decoder(dims, sd, enc, model_sequence(prompt, tokens), dtype, rnd)
    return ar.probs(scores, heads, len(prompt) - 1, len(tokens), s_b)


def forced_align(dims, sd, enc, prompt, tokens, heads, s_b, dtype=np.float64):
    """(frames int32 [n], P [len(heads), n, s_b], M [n, s_b]) of one hypothesis on encoder states enc [S, d].  n == 1: frame 0, no matrix."""
    n = len(tokens)
    if n == 1:
        return np.zeros(1, np.int32), np.zeros((len(heads), 1, s_b), dtype), np.zeros((1, s_b), dtype)
    P = rows_probs(dims, sd, enc, prompt, tokens, heads, s_b, dtype)
    M = ar.pipeline(P, dtype)
    frames, _ = ar.dtw(-M.astype(np.float32))
    return frames, P, M
