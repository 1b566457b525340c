"""CPU checks of forced alignment (wh_align_tokens): the exported symbol and its declaration, the refusal without a ctx, the
binding's argument packing, and the numpy reference (tests/forced_align_ref.py) on nano in float64.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_ref as ar
import forced_align_ref as fr
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADS = [(1, 0), (1, 1), (0, 1)]
PROMPT = [3, 5, 7, 9]


def test_symbol_is_declared_listed_and_exported():
    header = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    m = re.search(r"int wh_align_tokens\(([^;]*)\);", header)
    assert m, "wh_align_tokens is not declared in include/whisper_hip.h"
    args = [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["c", "p", "in", "heads", "frames_out", "n_frames_out", "logprob_out", "cap_tokens"]
    assert "wh_align_tokens" in wb.EXPORTS
    lib = wb.load_library()
    assert hasattr(lib, "wh_align_tokens")
    assert lib.wh_abi_version() == 1


def test_null_ctx_is_an_argument_error():
    lib = wb.load_library()
    assert lib.wh_align_tokens(None, None, None, None, None, None, None, 0) == 4   # WH_ERR_ARG, nothing dereferenced


def test_binding_packs_hypotheses_heads_and_debug_hypotheses():
    inp, opts, lens, cap, keep = wb.align_pack([[5, 6, 7], [8], [9, 10], [11]], [(1, 0), (0, 1)], hyps_per_clip=2, debug_hyps=[3, 0])
    assert lens == [3, 1, 2, 1] and cap == 3
    assert inp.struct_size == C.sizeof(wb.WhScoreInput) and inp.n_hyp == 4 and inp.hyps_per_clip == 2
    assert [inp.ids[i] for i in range(7)] == [5, 6, 7, 8, 9, 10, 11] and [inp.offsets[i] for i in range(5)] == [0, 3, 4, 6, 7]
    assert opts.struct_size == C.sizeof(wb.WhAlignmentOpts) and opts.n_heads == 2 and opts.n_debug_rows == 2
    assert [opts.heads[i] for i in range(4)] == [1, 0, 0, 1] and [opts.debug_rows[i] for i in range(2)] == [3, 0]
    inp, opts, lens, cap, keep = wb.align_pack([[4]], [(0, 0)])
    assert cap == 1 and opts.n_debug_rows == 0 and not opts.debug_rows and inp.hyps_per_clip == 1


@pytest.fixture(scope="module")
def nano():
    dims = ms.PRESETS["nano"]
    sd = ms.synth_state_dict(dims, 7)
    w = ms.flatten_state_dict(dims, sd)
    enc = orc.encoder(dims, w, orc.window_mel(orc.log_mel(ms.synth_clip(1500), dims.n_mels), 0, 3000)).astype(np.float64)
    tokens = [10 + (i * 5) % 23 for i in range(23)] + [2]   # 24 ids, the last one an EOT that is a target only
    return dims, sd, enc, tokens


@pytest.mark.parametrize("s_b", [1500, 8])
def test_reference_frames_and_rows(nano, s_b):
    dims, sd, enc, tokens = nano
    frames, P, M = fr.forced_align(dims, sd, enc, PROMPT, tokens, HEADS, s_b)
    n = len(tokens)
    assert frames.shape == (n,) and P.shape == (len(HEADS), n, s_b) and M.shape == (n, s_b)
    assert frames[0] == 0 and (np.diff(frames) >= 0).all() and frames.max() < s_b
    assert abs(P.sum(axis=-1) - 1).max() < 1e-12
    # "row i predicts t[i]": the rows are rows P - 1 .. P - 1 + n - 1 of a decoder run over prompt ++ t[:-1] — its last n rows, and the
    # run has exactly P + n - 1 positions, so t[n - 1] never enters it
    seq = PROMPT + tokens[:-1]
    assert fr.model_sequence(PROMPT, tokens) == seq and len(seq) == len(PROMPT) + n - 1
    _, scores = ar.decoder(dims, sd, enc, seq, np.float64)
    assert scores.shape[2] == len(PROMPT) - 1 + n
    want = ar.probs(scores, HEADS, len(PROMPT) - 1, n, s_b)
    assert np.array_equal(P, want)
    assert np.array_equal(P[:, -1], np.stack([ar._softmax(scores[l, h, -1:, :s_b])[0] for l, h in HEADS]))
    # one position earlier would take the last prompt-only row in and leave the row that predicts t[n - 1] out
    assert not np.array_equal(P, ar.probs(scores, HEADS, len(PROMPT) - 2, n, s_b))
    # changing the last token changes nothing; changing the one before it changes the last row only
    other = tokens[:-1] + [(tokens[-1] + 1) % dims.vocab]
    assert np.array_equal(fr.rows_probs(dims, sd, enc, PROMPT, other, HEADS, s_b), P)
    other = tokens[:-2] + [(tokens[-2] + 1) % dims.vocab, tokens[-1]]
    P2 = fr.rows_probs(dims, sd, enc, PROMPT, other, HEADS, s_b)
    assert np.array_equal(P2[:, :-1], P[:, :-1]) and not np.array_equal(P2[:, -1], P[:, -1])


def test_one_token_gives_frame_0(nano):
    dims, sd, enc, tokens = nano
    frames, P, M = fr.forced_align(dims, sd, enc, PROMPT, tokens[:1], HEADS, 1500)
    assert frames.tolist() == [0] and P.shape == (3, 1, 1500) and M.shape == (1, 1500)
