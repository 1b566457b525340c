"""CPU checks of the word-level timestamps: the numpy restatement in tests/align_ref.py against the CPU oracle's logits and
against a brute-force dynamic time warping, its edge cases, and the host library's words_from_tokens."""
import json

import numpy as np
import pytest

import align_ref as ar
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

HEADS = {"nano": [(1, 0), (1, 1), (0, 1)], "micro": [(2, 0), (2, 1), (2, 2), (2, 3), (0, 1)]}


@pytest.fixture(scope="module", params=[("nano", 7), ("micro", 11)], ids=["nano", "micro"])
def decoded(request):
    """One oracle decode per model, shared: (preset, dims, sd, enc, tokens, oracle logits)."""
    preset, seed = request.param
    dims = ms.PRESETS[preset]
    sd = ms.synth_state_dict(dims, seed)
    w = ms.flatten_state_dict(dims, sd)
    enc = orc.encoder(dims, w, orc.window_mel(orc.log_mel(ms.synth_clip(1500), dims.n_mels), 0, 3000))
    toks, logits = orc.decode_greedy(dims, w, enc, [3, 5, 7], 24, 2, [2], want_logits=True)
    assert len(toks) == 27
    return preset, dims, sd, enc, toks, logits


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_numpy_decoder_against_the_oracle(decoded, dtype):
    """Bound 1e-4: the oracle and HF agree to about 1e-5 on these models by the project's own record; measured here 5.6e-6 to 1.7e-5."""
    preset, dims, sd, enc, toks, logits = decoded
    got, scores = ar.decoder(dims, sd, enc, list(toks[:-1]), dtype)
    d = float(np.abs(got[2:] - logits).max())
    print(f"{preset} {np.dtype(dtype).name}: max |d logit| {d:.3g}")
    assert d <= 1e-4
    assert scores.shape == (dims.dec_layers, dims.n_heads, 26, dims.n_audio_ctx)


def test_frames_of_the_pipeline(decoded):
    """frame[] is non-decreasing, starts at 0 and stays below S_b, for the full and for a cropped clip; the f32 and f64 matrices agree to
    reordering and give the same path here."""
    preset, dims, sd, enc, toks, _ = decoded
    _, scores = ar.decoder(dims, sd, enc, list(toks[:-1]), np.float64)
    for sb in (1500, 400, 8):
        P = ar.probs(scores, HEADS[preset], 2, 24, sb)
        assert P.shape == (len(HEADS[preset]), 24, sb) and abs(P.sum(-1) - 1).max() < 1e-12
        m32, m64 = ar.pipeline(P, np.float32), ar.pipeline(P, np.float64)
        assert m32.dtype == np.float32 and np.abs(m32 - m64).max() < 1e-5
        frames, path = ar.dtw(-m32)
        assert frames[0] == 0 and (np.diff(frames) >= 0).all() and frames.max() < sb
        assert path[0] == (0, 0) and path[-1] == (23, sb - 1)
        assert all(0 <= b[0] - a[0] <= 1 and 0 <= b[1] - a[1] <= 1 and a != b for a, b in zip(path, path[1:]))
        assert [min(s for g, s in path if g == r) for r in range(24)] == frames.tolist()


def test_bf16_arithmetic_alone_moves_the_probabilities():
    """Why tests/test_align_gpu.py holds the bf16 probabilities to an absolute 0.05 and not to four times what was measured on the GPU
    (0.019 - 0.023): on the synthetic whisper-base weights the cross-attention of the test's heads is near one-hot, and a numpy decoder whose
    matrices and contraction operands are rounded to bf16 — no GPU code involved — already differs from the float64 one by more than a
    quarter of that ceiling.  Figures printed; measured here: largest probability 0.73, largest score change 0.27, largest |dP| 0.034."""
    dims = ms.PRESETS["base"]
    sd = ms.synth_state_dict(dims, 1234)
    enc = orc.encoder(dims, ms.flatten_state_dict(dims, sd), orc.window_mel(orc.log_mel(ms.synth_clip(1500), dims.n_mels), 0, 3000)).astype(np.float64)
    seq = [50258, 50259, 50359] + [1000 + 37 * i for i in range(11)]
    heads = [(5, 0), (5, 7), (3, 2), (2, 4)]
    _, sc = ar.decoder(dims, sd, enc, seq, np.float64)
    _, scb = ar.decoder(dims, sd, enc, seq, np.float64, rnd=ar.bf16_round)
    P, Pb = ar.probs(sc, heads, 2, 12, 1500), ar.probs(scb, heads, 2, 12, 1500)
    d = float(np.abs(P - Pb).max())
    ds = max(float(np.abs(sc[l, h, 2:14] - scb[l, h, 2:14]).max()) for l, h in heads)
    print(f"base, bf16-rounded decoder against float64: largest probability {P.max():.3g}, max |d score| {ds:.3g}, max |dP| {d:.3g}")
    assert P.max() > 0.5 and 0.05 / 4 < d < 0.05


def brute_paths(n, m):
    """Every monotone path from (0, 0) to (n - 1, m - 1) with steps (1, 1), (1, 0), (0, 1)."""
    out = []

    def walk(i, j, acc):
        acc = acc + [(i, j)]
        if (i, j) == (n - 1, m - 1):
            out.append(acc)
            return
        if i + 1 < n and j + 1 < m:
            walk(i + 1, j + 1, acc)
        if i + 1 < n:
            walk(i + 1, j, acc)
        if j + 1 < m:
            walk(i, j + 1, acc)

    walk(0, 0, [])
    return out


def test_dtw_against_brute_force():
    paths = brute_paths(5, 9)
    assert len(paths) == 3649   # the Delannoy number D(4, 8)
    rng = np.random.default_rng(3)
    for trial in range(20):
        x = rng.permutation(45).astype(np.float32).reshape(5, 9) + rng.uniform(0, 0.5, (5, 9)).astype(np.float32)   # distinct entries
        assert len(set(x.ravel().tolist())) == 45
        costs = sorted((sum(float(x[i, j]) for i, j in p), k) for k, p in enumerate(paths))
        frames, path = ar.dtw(x)
        got = sum(float(x[i, j]) for i, j in path)
        assert abs(got - costs[0][0]) <= 1e-4 * max(1.0, abs(costs[0][0]))
        if costs[1][0] - costs[0][0] > 1e-3:
            assert path == paths[costs[0][1]]
        assert frames.tolist() == [min(j for i, j in path if i == r) for r in range(5)]


def test_one_row_and_zero_std_columns():
    frames, path = ar.dtw(-np.ones((1, 12), np.float32))
    assert frames.tolist() == [0] and path == [(0, 0)]
    rng = np.random.default_rng(4)
    P = rng.uniform(0, 1, (2, 6, 16)).astype(np.float32)
    P[:, :, 5] = 0.0      # a frame no row attends to
    P[0, :, 9] = 0.25     # a constant column of one head
    for dt in (np.float32, np.float64):
        M = ar.pipeline(P, dt)
        assert np.isfinite(M).all()
    # every column constant: every std is 0, so W, its medians and M are exactly 0 (no 0 / 0)
    assert (ar.pipeline(np.zeros((1, 4, 10), np.float32)) == 0).all()
    assert (ar.pipeline(np.full((3, 5, 8), 0.125, np.float32), np.float64) == 0).all()
    # a head whose columns are all constant adds nothing: the mean over the heads is the other head's medians, halved
    two = np.stack([P[1], np.full((6, 16), 0.5, np.float32)])
    assert np.allclose(ar.pipeline(two, np.float64), ar.pipeline(P[1:2], np.float64) / 2, atol=1e-12)


def test_words_from_tokens(tmp_path):
    """openai-whisper's split on spaces through the host C API: a word begins at a piece with a leading space, a piece that ends inside a
    UTF-8 sequence stays with the next one, timestamps and EOT are dropped; starts from the frames, ends from the next kept row."""
    tj = {"model": {"vocab": {"Hello": 0, "Ġworld": 1, "!": 2, "Ã": 3, "©": 4, "Ġcaf": 5}},
          "added_tokens": [{"id": 6, "content": "<|endoftext|>", "special": True}] + [{"id": 7 + i, "content": f"<|{i * 0.02:.2f}|>", "special": True} for i in range(4)]}
    p = tmp_path / "tokenizer.json"
    p.write_text(json.dumps(tj))
    #        <|0.00|> Hello  _world  !   <|0.04|> _caf  0xC3  0xA9  EOT
    toks = [7,        0,     1,      2,  9,       5,    3,    4,    6]
    frames = [0,      10,    40,     55, 60,      100,  120,  121,  140]
    words = wb.words_from_tokens(toks, frames, 7, 6, 30.0, 0.0, str(p))
    assert [w["word"] for w in words] == ["Hello", " world!", " café"]
    assert [w["start"] for w in words] == [0.2, 0.8, 2.0]
    assert [w["end"] for w in words] == [0.8, 2.0, 30.0]
    shifted = wb.words_from_tokens(toks, frames, 7, 6, 30.0, 25.0, str(p))
    assert [w["start"] for w in shifted] == [25.2, 25.8, 27.0] and shifted[-1]["end"] == 55.0
    # without a tokenizer the pieces are those of the "[TOKENS:a b c]" text, one word per id
    words = wb.words_from_tokens([900, 11, 12, 2], [0, 5, 9, 12], 800, 2, 1.0)
    assert "".join(w["word"] for w in words) == "[TOKENS:11 12]"
    assert [w["start"] for w in words] == [0.1, 0.18] and [w["end"] for w in words] == [0.18, 1.0]
    assert wb.words_from_tokens([2], [0], 800, 2, 1.0) == []
