"""Language detection, the parts that need no GPU: the float64 restatement (tests/language_ref.py) on hand-made vectors, the host's
language table, the CLI's --language auto surface, and the agreement of the header with the binding."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import language_ref as lg
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")


def test_reference_probabilities_in_list_order():
    v = np.zeros(10)
    v[[2, 5, 7]] = [1.0, 3.0, 2.0]
    best, p = lg.detect(v, [7, 2, 5])
    e = np.exp(np.array([2.0, 1.0, 3.0]) - 3.0)
    assert best == 5 and np.allclose(p, e / e.sum(), rtol=0, atol=1e-15) and abs(p.sum() - 1) < 1e-15
    assert lg.detect(v, [2])[0] == 2 and lg.detect(v, [2])[1].tolist() == [1.0]   # one language: certain
    # ids outside the list play no part, however large their logits
    v[9] = 100.0
    assert lg.detect(v, [7, 2, 5])[0] == 5


def test_reference_ties_go_to_the_lowest_id_not_the_lowest_position():
    v = np.full(10, -1.0)
    v[[8, 3, 6]] = 4.0
    best, p = lg.detect(v, [8, 6, 3, 1])
    assert best == 3
    assert np.allclose(p[:3], p[0]) and p[3] < p[0]
    assert lg.detect([0.0, -0.0], [1, 0])[0] == 0   # +0 and -0 compare equal


def test_reference_nan_is_left_out_and_never_wins():
    v = np.array([0.0, np.nan, 2.0, np.nan, 1.0])
    best, p = lg.detect(v, [3, 4, 1, 2])
    assert best == 2 and p[0] == 0 and p[2] == 0
    e = np.exp(np.array([1.0, 2.0]) - 2.0)
    assert np.allclose([p[1], p[3]], e / e.sum())
    assert abs(p.sum() - 1) < 1e-15


def test_reference_nothing_finite_picks_the_lowest_id_with_zero_probabilities():
    for row in ([np.nan] * 4, [np.nan, -np.inf, -np.inf, np.nan], [-np.inf] * 4):
        best, p = lg.detect(np.array(row), [3, 1, 2])
        assert best == 1 and p.tolist() == [0.0, 0.0, 0.0]
    # -inf beside a finite logit is an ordinary zero
    best, p = lg.detect(np.array([-np.inf, 0.5, np.nan]), [0, 2, 1])
    assert best == 1 and p.tolist() == [0.0, 0.0, 1.0]
    # +inf: the limit
    best, p = lg.detect(np.array([np.inf, 0.5, np.inf]), [2, 1, 0])
    assert best == 0 and p.tolist() == [0.5, 0.0, 0.5]


def test_pick_ids_finds_a_pair_that_flips():
    rng = np.random.default_rng(0)
    L = rng.normal(scale=0.05, size=(4, 400))
    L[:, 10] += 8
    L[:, 20] += 8
    L[:2, 10] += 1
    L[2:, 20] += 1
    ids, gap = lg.pick_ids(L, 7)
    assert len(ids) == len(set(ids)) == 7 and ids[-2:] == [20, 10] and gap > 0
    assert {lg.detect(L[b], ids)[0] for b in range(4)} == {10, 20}


def test_host_language_table():
    codes, ids = wb.language_table(51865)
    assert len(codes) == len(ids) == 99 and len(set(codes)) == 99
    assert ids == list(range(50259, 50259 + 99))
    assert ids[codes.index("en")] == 50259 and ids[codes.index("hi")] == 50276 and codes[-1] == "su"
    codes3, ids3 = wb.language_table(51866)
    assert len(codes3) == 100 and codes3[:99] == codes and codes3[-1] == "yue" and ids3[-1] == 50358
    # what the fallback table of special_tokens knows today stays what it was
    H = wb.load_host_library()
    H.whh_special_tokens.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_longlong)]
    out = (C.c_longlong * 5)()
    for code in ("en", "hi"):
        assert H.whh_special_tokens(code.encode(), b"transcribe", b"", out) == 0 and out[2] == ids[codes.index(code)]
    assert H.whh_special_tokens(b"auto", b"transcribe", b"", out) == 0 and out[0] == 50258 and out[3] == 50359   # the placeholder prompt


def test_small_vocabulary_is_refused_with_a_clear_message():
    for vocab in (1024, 4099, 50357):
        with pytest.raises(ValueError) as ei:
            wb.language_table(vocab)
        msg = str(ei.value)
        assert "--language auto" in msg and "tokenizer.json" in msg and str(vocab) in msg and "50259" in msg


def test_language_table_from_a_tokenizer(tmp_path):
    import json
    added = [{"id": 7, "content": "<|startoftranscript|>", "special": True}, {"id": 12, "content": "<|de|>", "special": True},
             {"id": 9, "content": "<|en|>", "special": True}, {"id": 30, "content": "<|yue|>", "special": True},
             {"id": 5000, "content": "<|fr|>", "special": True}, {"id": 11, "content": "<|0.00|>", "special": True}]
    path = tmp_path / "tokenizer.json"
    path.write_text(json.dumps({"model": {"vocab": {"a": 0}}, "added_tokens": added}))
    codes, ids = wb.language_table(1024, str(path))    # <|fr|> lies outside this vocabulary; the order is the standard list's
    assert codes == ["en", "de", "yue"] and ids == [9, 12, 30]


def test_cli_help_names_language_auto():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--language en|auto" in r.stdout and "--language auto " in r.stdout


def test_header_and_binding_agree_on_the_new_entries():
    hdr = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    declared = set(re.findall(r"\b(wh_[a-z_0-9]+)\s*\(", hdr))
    assert {"wh_ctx_set_language_detection", "wh_get_languages"} <= declared & set(wb.EXPORTS)
    assert int(re.search(r"#define WH_MAX_LANGUAGES (\d+)", hdr).group(1)) == wb.WH_MAX_LANGUAGES == 128
    lib = wb.load_library()
    assert hasattr(lib, "wh_ctx_set_language_detection") and hasattr(lib, "wh_get_languages")
    # the struct the binding passes has the header's layout: size_t, pointer, size_t, int32 (+ padding)
    assert C.sizeof(wb.WhLanguageOpts) == 32 and wb.WhLanguageOpts.sot_index.offset == 24
    assert lib.wh_get_languages(None, None, None, 0, None) == 4 and lib.wh_ctx_set_language_detection(None, None) == 4
