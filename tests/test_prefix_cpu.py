"""Per-clip prompt prefixes, the parts that need no GPU: the host's prefix rule against its Python restatement, the binding's struct and
argument packing, and the agreement of the header with the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import prefix_ref as pr
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_build_prefix(history, sot_prev, n_text_ctx):
    H = wb.load_host_library()
    H.whh_build_prefix.argtypes = [C.POINTER(C.c_longlong), C.c_size_t, C.c_longlong, C.c_int, C.POINTER(C.c_longlong), C.c_size_t]
    H.whh_build_prefix.restype = C.c_size_t
    h = (C.c_longlong * max(1, len(history)))(*history)
    out = (C.c_longlong * (n_text_ctx + 4))()
    n = H.whh_build_prefix(h, len(history), sot_prev, n_text_ctx, out, n_text_ctx + 4)
    return [int(out[i]) for i in range(n)]


@pytest.mark.parametrize("n_text_ctx", [448, 16])
def test_host_prefix_rule_equals_the_restatement(n_text_ctx):
    keep = n_text_ctx // 2 - 1
    rng = np.random.default_rng(3)
    for n in (0, 1, keep - 1, keep, keep + 1, 3 * keep + 5):   # empty, one id, exactly n_text_ctx/2 - 1 ids, longer
        hist = [int(t) for t in rng.integers(0, 50000, n)]
        got = host_build_prefix(hist, 50361, n_text_ctx)
        assert got == pr.build_prev_prefix(hist, 50361, n_text_ctx), n
        assert len(got) == (0 if n == 0 else 1 + min(n, keep))
        if n:
            assert got[0] == 50361 and got[-1] == hist[-1] and got[1:] == hist[-min(n, keep):]


def test_fallback_special_tokens_know_startofprev():
    hdr = open(os.path.join(ROOT, "whisper-rust-ort_amd", "host", "wh_host.h")).read()
    fields = re.search(r"struct WhisperSpecial \{ int64_t ([^;]+); \};", hdr).group(1)
    assert [f.strip() for f in fields.split(",")][-1] == "sot_prev"
    assert "s.sot_prev = 50361;" in hdr and '"<|startofprev|>"' in hdr


def test_header_and_binding_agree_on_the_prefix_entry():
    hdr = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    declared = set(re.findall(r"\b(wh_[a-z_0-9]+)\s*\(", hdr))
    assert "wh_ctx_set_prefixes" in declared & set(wb.EXPORTS)
    assert declared == set(wb.EXPORTS)
    assert int(re.search(r"#define WH_PREFIX_FIRST_WINDOW (\d+)", hdr).group(1)) == wb.WH_PREFIX_FIRST_WINDOW == 0
    assert int(re.search(r"#define WH_PREFIX_ALL_WINDOWS\s+(\d+)", hdr).group(1)) == wb.WH_PREFIX_ALL_WINDOWS == 1
    assert int(re.search(r"#define WH_ABI_VERSION (\d+)", hdr).group(1)) == 1
    # the struct the binding passes has the header's layout: size_t, pointer, pointer, size_t, int32 (+ padding)
    assert C.sizeof(wb.WhPrefixOpts) == 40
    assert [wb.WhPrefixOpts.ids.offset, wb.WhPrefixOpts.offsets.offset, wb.WhPrefixOpts.n_clips.offset, wb.WhPrefixOpts.longform_scope.offset] == [8, 16, 24, 32]
    lib = wb.load_library()
    assert hasattr(lib, "wh_ctx_set_prefixes") and lib.wh_ctx_set_prefixes(None, None) == 4


def test_prefix_packing():
    ids, off = wb.pack_prefixes([[], [5, 6, 7], [], [9], []])
    assert ids.dtype == np.int64 and off.dtype == np.uint64 and off.itemsize == C.sizeof(C.c_size_t)
    assert ids.tolist() == [5, 6, 7, 9] and off.tolist() == [0, 0, 3, 3, 4, 4]
    ids, off = wb.pack_prefixes([[], []])
    assert ids.size == 0 and off.tolist() == [0, 0, 0]
    ids, off = wb.pack_prefixes([list(range(140))])
    assert ids.tolist() == list(range(140)) and off.tolist() == [0, 140]


def test_shared_inputs_are_what_the_gpu_tests_describe():
    pre = pr.prefixes(1024)
    assert [len(p) for p in pre] == list(pr.LENS) and max(pr.LENS) == 140
    assert all(10 <= t < 1024 - 400 for p in pre for t in p)
    assert [140 - n for n in pr.LENS] == [140, 139, 77, 76, 75, 11, 0]
