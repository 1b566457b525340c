"""CPU checks of the scoring entry's reference (tests/score_ref.py), of the binding's struct mirror and hypothesis packing, and of the exported
symbol.  No GPU."""
import ctypes as C

import numpy as np

import score_ref as sr
from whisper_rust_ort_amd import binding as wb

NAN, INF = float("nan"), float("inf")


def test_masked_target_is_minus_inf_and_begin_suppress_hits_entry_0_only():
    v = np.array([[1.0, 2.0, 3.0, 0.5]] * 3, np.float32)
    # id 2 suppressed everywhere, id 1 at entry 0 only
    lp, am = sr.score_ref(v, [2, 1, 1], suppress=[2], begin_suppress=[1])
    assert lp[0] == -INF                       # a suppressed target
    assert am.tolist() == [0, 1, 1]            # entry 0: {0, 3} allowed; later: {0, 1, 3}
    lp0, _ = sr.score_ref(v, [1, 1, 1], suppress=[2], begin_suppress=[1])
    assert lp0[0] == -INF and np.isfinite(lp0[1]) and lp0[1] == lp0[2]
    x = np.array([1.0, 2.0, 0.5])
    np.testing.assert_allclose(lp0[1], 2.0 - (2.0 + np.log(np.exp(x - 2.0).sum())), rtol=0, atol=1e-12)
    # entry 0 sums over {0, 3} only
    lp3, _ = sr.score_ref(v, [3], suppress=[2], begin_suppress=[1])
    np.testing.assert_allclose(lp3[0], 0.5 - (1.0 + np.log(1.0 + np.exp(-0.5))), rtol=0, atol=1e-12)


def test_ties_go_to_the_lowest_id():
    v = np.array([[0.0, 5.0, 5.0, 5.0, 1.0]], np.float32)
    _, am = sr.score_ref(v, [0])
    assert am.tolist() == [1]
    _, am = sr.score_ref(v, [0], suppress=[1])
    assert am.tolist() == [2]


def test_nan_and_minus_inf_never_win_and_are_left_out_of_the_sum():
    v = np.array([[NAN, 1.0, -INF, 2.0, NAN]], np.float32)
    lp, am = sr.score_ref(v, [3])
    assert am.tolist() == [3]
    np.testing.assert_allclose(lp[0], -np.log(1.0 + np.exp(-1.0)), rtol=0, atol=1e-12)
    assert sr.score_ref(v, [0])[0][0] == -INF and sr.score_ref(v, [2])[0][0] == -INF   # a NaN / -inf target is not allowed
    assert sr.top1_margin(v[0], 0) == 1.0


def test_nothing_allowed_gives_0_and_minus_inf():
    v = np.array([[NAN, -INF, 3.0]], np.float32)
    lp, am = sr.score_ref(v, [2], suppress=[2])
    assert am.tolist() == [0] and lp[0] == -INF
    lp, am = sr.score_ref(np.full((2, 4), -INF, np.float32), [1, 2])
    assert am.tolist() == [0, 0] and (lp == -INF).all()


def test_struct_mirror_layout_and_size():
    o = wb.WhScoreInput
    assert C.sizeof(o) == 40
    assert (o.struct_size.offset, o.ids.offset, o.offsets.offset, o.n_hyp.offset, o.hyps_per_clip.offset) == (0, 8, 16, 24, 32)
    assert all(f.size == 8 for f in (o.struct_size, o.ids, o.offsets, o.n_hyp, o.hyps_per_clip))


def test_ragged_hypotheses_are_packed_back_to_back():
    ids, off = wb.pack_hypotheses([[5, 6, 7], [8], [9, 10]])
    assert ids.dtype == np.int64 and off.dtype == np.uint64 and off.itemsize == C.sizeof(C.c_size_t)
    assert ids.tolist() == [5, 6, 7, 8, 9, 10] and off.tolist() == [0, 3, 4, 6]
    ids, off = wb.pack_hypotheses([])
    assert ids.size == 0 and off.tolist() == [0]


def test_symbol_is_exported_and_refuses_without_a_ctx():
    lib = wb.load_library()
    assert hasattr(lib, "wh_score_tokens")
    assert lib.wh_score_tokens(None, None, None, None, None, 0, None, 0, None, 0) == 4   # no ctx: WH_ERR_ARG, nothing dereferenced
