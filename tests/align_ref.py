"""Numpy restatement of the word-level timestamps (wh_ctx_set_alignment), used by the CPU and the GPU tests:

  - a teacher-forced Whisper decoder over a state dict (modelspec.synth_state_dict), in float32 or float64, that returns the logits of every
    position and the cross-attention scores q . k of every (layer, head); optionally with every matrix and contraction operand rounded
    (bf16_round), as an emulation of what bf16 arithmetic alone does to those scores;
  - the matrix pipeline: softmax over the cropped frames, per-column mean / population std over the rows, median of 7 with reflect padding,
    head average;
  - openai-whisper's dtw on x = -M in float32 (vectorised by anti-diagonals) and the frame of each row.

Test infrastructure only: nothing here is imported by the package."""
import math

import numpy as np

_erf = np.frompyfunc(math.erf, 1, 1)


def _gelu(x):
    return (0.5 * x * (1.0 + _erf(x.astype(np.float64) / math.sqrt(2.0)).astype(np.float64))).astype(x.dtype)


def _ln(x, w, b):
    mu = x.mean(axis=-1, keepdims=True)
    var = ((x - mu) ** 2).mean(axis=-1, keepdims=True)
    return (x - mu) / np.sqrt(var + x.dtype.type(1e-5)) * w + b


def _softmax(x):
    e = np.exp(x - x.max(axis=-1, keepdims=True))
    return e / e.sum(axis=-1, keepdims=True)


def bf16_round(x):
    """x rounded to the nearest bfloat16 (ties to even), returned in x's dtype."""
    x = np.asarray(x)
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return u.astype(np.uint32).view(np.float32).astype(x.dtype)


def decoder(dims, sd, enc, tokens, dtype=np.float64, rnd=None):
    """Teacher-forced decoder pass over `tokens` (model positions 0 .. T-1) on encoder states enc [S, d].  Returns (logits [T, vocab],
    scores [dec_layers, n_heads, T, S]): scores[l, h, t, s] = q_t . k_s of layer l's cross-attention, the head_dim^-0.5 factor on q.
    rnd (e.g. bf16_round): an emulation of a reduced-precision decoder — the matrices (Linear weights, token embedding) and both operands of
    every contraction pass through it, everything else (residual stream, LayerNorm, softmax, GELU, accumulation) stays in dtype."""
    R = rnd if rnd is not None else (lambda a: a)
    W = lambda n: (R(sd[n].astype(dtype)) if n.endswith("_proj.weight") or n.endswith(".fc1.weight") or n.endswith(".fc2.weight")
                   or n.endswith("embed_tokens.weight") else sd[n].astype(dtype))
    H, hd, T = dims.n_heads, dims.head_dim, len(tokens)
    enc = R(enc.astype(dtype))
    scale = dtype(hd ** -0.5)
    x = W("model.decoder.embed_tokens.weight")[np.asarray(tokens)] + W("model.decoder.embed_positions.weight")[:T]
    causal = np.triu(np.full((T, T), -np.inf, dtype), 1)
    scores = np.zeros((dims.dec_layers, H, T, enc.shape[0]), dtype)

    def heads(a):
        return a.reshape(a.shape[0], H, hd).transpose(1, 0, 2)

    for l in range(dims.dec_layers):
        p = f"model.decoder.layers.{l}"
        h = _ln(x, W(f"{p}.self_attn_layer_norm.weight"), W(f"{p}.self_attn_layer_norm.bias"))
        q = heads((R(h) @ W(f"{p}.self_attn.q_proj.weight").T + W(f"{p}.self_attn.q_proj.bias")) * scale)
        k = heads(R(h) @ W(f"{p}.self_attn.k_proj.weight").T)
        v = heads(R(h) @ W(f"{p}.self_attn.v_proj.weight").T + W(f"{p}.self_attn.v_proj.bias"))
        a = R(_softmax(R(q) @ R(k).transpose(0, 2, 1) + causal)) @ R(v)
        x = x + R(a.transpose(1, 0, 2).reshape(T, -1)) @ W(f"{p}.self_attn.out_proj.weight").T + W(f"{p}.self_attn.out_proj.bias")
        h = _ln(x, W(f"{p}.encoder_attn_layer_norm.weight"), W(f"{p}.encoder_attn_layer_norm.bias"))
        q = heads((R(h) @ W(f"{p}.encoder_attn.q_proj.weight").T + W(f"{p}.encoder_attn.q_proj.bias")) * scale)
        k = heads(enc @ W(f"{p}.encoder_attn.k_proj.weight").T)
        v = heads(enc @ W(f"{p}.encoder_attn.v_proj.weight").T + W(f"{p}.encoder_attn.v_proj.bias"))
        sc = R(q) @ R(k).transpose(0, 2, 1)
        scores[l] = sc
        a = R(_softmax(sc)) @ R(v)
        x = x + R(a.transpose(1, 0, 2).reshape(T, -1)) @ W(f"{p}.encoder_attn.out_proj.weight").T + W(f"{p}.encoder_attn.out_proj.bias")
        h = _ln(x, W(f"{p}.final_layer_norm.weight"), W(f"{p}.final_layer_norm.bias"))
        x = x + R(_gelu(R(h) @ W(f"{p}.fc1.weight").T + W(f"{p}.fc1.bias"))) @ W(f"{p}.fc2.weight").T + W(f"{p}.fc2.bias")
    x = _ln(x, W("model.decoder.layer_norm.weight"), W("model.decoder.layer_norm.bias"))
    return R(x) @ W("model.decoder.embed_tokens.weight").T, scores


def frames_of(n_samples, n_audio_ctx=1500):
    """S_b of a clip of n_samples: half its mel frames (rounded up), at least 8, at most the audio context."""
    nf = 1 + n_samples // 160
    nf = nf - 1 if nf > 1 else nf
    return min(n_audio_ctx, max(8, (nf + 1) // 2))


def probs(scores, heads, first_row, n_gen, s_b):
    """P [len(heads), n_gen, s_b]: the listed heads' rows first_row .. first_row + n_gen - 1, softmax over the first s_b frames."""
    return np.stack([_softmax(scores[l, h, first_row:first_row + n_gen, :s_b]) for l, h in heads])


def pipeline(P, dtype=np.float32):
    """Steps 3-5: W = (P - mean) / std per (head, frame) over the rows (0 where std == 0), median of 7 along the frames with reflect padding
    of 3, mean over the heads.  P [A, n, S] -> M [n, S]."""
    P = P.astype(dtype)
    mean = P.mean(axis=1, keepdims=True)
    std = P.std(axis=1, keepdims=True)
    W = np.where(std == 0, dtype(0), (P - mean) / np.where(std == 0, dtype(1), std))
    pad = np.pad(W, ((0, 0), (0, 0), (3, 3)), mode="reflect")
    win = np.lib.stride_tricks.sliding_window_view(pad, 7, axis=2)
    med = np.sort(win, axis=-1)[..., 3]
    return med.mean(axis=0).astype(dtype)


def dtw_tables(x):
    """cost [N+1, M+1] float32 and the steps (0 diagonal, 1 up, 2 left) of openai-whisper's dtw_cpu on x [N, M], by anti-diagonals."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    cost = np.full((N + 1, M + 1), np.inf, np.float32)
    cost[0, 0] = 0
    trace = np.full((N + 1, M + 1), 2, np.int8)
    trace[:, 0] = 1
    trace[0, :] = 2
    for d in range(2, N + M + 1):
        i = np.arange(max(1, d - M), min(N, d - 1) + 1)
        j = d - i
        c0, c1, c2 = cost[i - 1, j - 1], cost[i - 1, j], cost[i, j - 1]
        s0 = (c0 < c1) & (c0 < c2)
        s1 = ~s0 & (c1 < c0) & (c1 < c2)
        c = np.where(s0, c0, np.where(s1, c1, c2))
        cost[i, j] = x[i - 1, j - 1] + c
        trace[i, j] = np.where(s0, 0, np.where(s1, 1, 2))
    return cost, trace


def dtw(x):
    """frame[g] = the smallest frame on the dtw path of x [N, M] within row g (N == 1: [0]); also returns the path [(row, frame)]."""
    x = np.asarray(x, np.float32)
    N, M = x.shape
    if N == 1:
        return np.zeros(1, np.int32), [(0, 0)]
    _, trace = dtw_tables(x)
    i, j = N, M
    path = []
    frames = np.zeros(N, np.int32)
    while i > 0 or j > 0:
        if i > 0 and j > 0:
            path.append((i - 1, j - 1))
            frames[i - 1] = j - 1
        s = 2 if i == 0 else 1 if j == 0 else trace[i, j]
        if s == 0:
            i, j = i - 1, j - 1
        elif s == 1:
            i -= 1
        else:
            j -= 1
    return frames, path[::-1]
