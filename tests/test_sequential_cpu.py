"""CPU checks of sequential long-form's host logic (host/wh_host.h seek_advance and run_sequential through the shims of libwh_host.so) against
the Python restatement tests/seq_ref.py, and of the new symbols.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import seq_ref
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TB, EOT, SOT_PREV = 1000, 900, 901      # ids below TB other than EOT are text; TB + k is the timestamp k * 0.02 s


def T(k):
    return TB + k


def check_rule(gen, seg_frames=3000):
    got = wb.seek_advance(gen, TB, EOT, seg_frames)
    segs, adv = seq_ref.seek_advance(gen, TB, EOT, seg_frames)
    assert got["advance"] == adv, gen
    assert got["segments"] == segs, gen        # times compared as the doubles they are
    return got


# ---- the seek rule, by hand ------------------------------------------------------------------------------------------------------------------

def test_pairs_and_trailing_text():
    got = check_rule([T(0), 5, 6, T(100), T(100), 7, T(250), T(250), 8, 9])
    assert got["advance"] == 500                                   # the last pair closes at 5.0 s: 250 * 2 frames
    assert [(s["start"], s["end"]) for s in got["segments"]] == [(0.0, 2.0), (2.0, 5.0)]
    assert got["segments"][1]["ids"] == [T(100), 7, T(250)]        # timestamps included; the trailing 8 9 are no segment


def test_single_timestamp_ending():
    got = check_rule([T(0), 5, T(100), T(100), 7, 8, T(400)], seg_frames=2500)
    assert got["advance"] == 2500                                  # single_end: the whole window
    assert [(s["start"], s["end"]) for s in got["segments"]] == [(0.0, 2.0), (2.0, 8.0)]


def test_no_timestamps_at_all():
    got = check_rule([5, 6, 7], seg_frames=1234)
    assert got["advance"] == 1234 and got["segments"] == [{"start": 0.0, "end": 12.34, "ids": [5, 6, 7]}]
    got = check_rule([T(0), 5, 6, T(70)], seg_frames=3000)         # no pair, a last timestamp above tb: the segment ends there
    assert got["advance"] == 3000 and got["segments"][0]["end"] == 70 * 0.02


def test_one_trailing_timestamp_at_tb():
    got = check_rule([5, 6, T(0)], seg_frames=800)
    assert got["advance"] == 800 and got["segments"] == [{"start": 0.0, "end": 8.0, "ids": [5, 6, T(0)]}]


def test_zero_length_and_textless_segments_are_dropped():
    got = check_rule([T(10), 5, T(10), T(10), T(20), T(20), 6, T(30), T(30)])
    # [T10 5 T10] has start == end; [T10 T20] has no text; [T20 6 T30] stays
    assert [s["ids"] for s in got["segments"]] == [[T(20), 6, T(30)]] and got["advance"] == 60
    assert check_rule([T(0), T(0)])["segments"] == []
    assert check_rule([])["segments"] == [] and check_rule([EOT])["advance"] == 3000


def test_zero_advance_becomes_the_whole_window():
    got = check_rule([T(0), T(0), 5, 6], seg_frames=3000)          # a closing pair at <|0.00|>
    assert got["advance"] == 3000 and got["segments"] == []
    assert check_rule([T(0), T(0)], seg_frames=17)["advance"] == 17


def test_advance_beyond_seg_frames_at_a_files_end():
    got = check_rule([T(0), 5, T(600), T(600)], seg_frames=400)    # the model stamps 12 s into a 4 s remainder
    assert got["advance"] == 1200 and got["segments"][0]["end"] == 12.0


def test_eot_in_the_middle():
    got = check_rule([T(0), 5, T(50), T(50), EOT, 6, T(90), T(90)])
    assert got["advance"] == 100 and len(got["segments"]) == 1


def test_seek_rule_on_random_sequences():
    rng = np.random.default_rng(20)
    for _ in range(4000):
        n = int(rng.integers(0, 14))
        kinds = rng.integers(0, 10, n)
        stamps = np.sort(rng.integers(0, 40, n)) if rng.integers(0, 2) else rng.integers(0, 40, n)
        gen = [int(EOT) if k == 0 else T(int(s)) if k < 5 else int(rng.integers(1, 800)) for k, s in zip(kinds, stamps)]
        check_rule(gen, seg_frames=int(rng.integers(1, 3001)))


# ---- the loop, scripted ----------------------------------------------------------------------------------------------------------------------

CFG = dict(tb=TB, eot=EOT, sot_prev=SOT_PREV, n_text_ctx=448, n_prompt=3, max_new_tokens=32)


def win(tokens, avg_logprob=-0.3, no_speech_prob=0.1, temperature=0.0):
    return {"tokens": tokens, "avg_logprob": avg_logprob, "no_speech_prob": no_speech_prob, "temperature": temperature}


def both(frames, script, **kw):
    cfg = dict(CFG, **kw)
    got = wb.run_sequential_scripted(frames, script, **cfg)
    want = seq_ref.run_sequential(frames, seq_ref.scripted_step(script), **cfg)
    assert got["steps"] == want["steps"]
    for f, (g, w) in enumerate(zip(got["files"], want["files"])):
        assert g["segments"] == w["segments"], f
        assert len(g["windows"]) == len(w["windows"]), f
        for k, (a, b) in enumerate(zip(g["windows"], w["windows"])):
            assert a == b, (f, k)
    return got


PAIR = [T(0), 5, 6, T(500), T(500), 7]            # advances 10 s
FULL = [T(0), 8, 9, T(700)]                       # no pair: the whole window


def test_three_files_finish_at_different_steps():
    got = both([6500, 3100, 400], [[win(PAIR), win(FULL)], [win(FULL)], [win(PAIR)]])
    assert got["steps"][0] == [0, 1, 2] and got["steps"][1] == [0, 1] and got["steps"][-1] == [0]      # rows compact as files finish
    assert [w["seek"] for w in got["files"][0]["windows"]] == [0, 1000, 4000]
    assert [w["seg_frames"] for w in got["files"][0]["windows"]] == [3000, 3000, 2500]
    assert got["files"][2]["windows"][0]["advance"] == 1000                                            # beyond its 400 frames: the file ends
    assert got["files"][0]["segments"][1]["start"] == 10.0                                             # shifted by the window's seek
    assert got["files"][0]["windows"][1]["prefix"] == [SOT_PREV, T(0), 5, 6, T(500)]                   # the first window's kept segment


def test_skipped_window():
    script = [[win(PAIR), win(PAIR, avg_logprob=-2.0, no_speech_prob=0.9), win(PAIR)]]
    got = both([2500], script, no_speech_threshold=0.6, logprob_threshold=-1.0)
    w = got["files"][0]["windows"]
    assert [x["skipped"] for x in w] == [False, True]
    assert w[1]["advance"] == 1500 and len(got["files"][0]["segments"]) == 1
    got = both([5000], script, no_speech_threshold=0.6, logprob_threshold=-1.0)
    w = got["files"][0]["windows"]
    assert w[2]["prefix"] == w[1]["prefix"]                                                            # a skipped window leaves the history alone


def test_temperature_resets_the_prompt_above_one_half_only():
    script = [[win(PAIR, temperature=0.6), win(PAIR, temperature=0.4), win(PAIR)]]
    w = both([3000], script)["files"][0]["windows"]
    assert w[1]["prefix"] == []                                                                        # 0.6 > 0.5: the next window starts clean
    assert w[2]["prefix"] == [SOT_PREV, T(0), 5, 6, T(500)]                                            # 0.4: only window 1's text, window 0's is cut off


def test_conditioning_off_keeps_the_initial_prompt_for_the_first_window_only():
    w = both([3000], [[win(PAIR)]], condition_on_previous_text=False, initial_prompt=[11, 12])["files"][0]["windows"]
    assert w[0]["prefix"] == [SOT_PREV, 11, 12] and all(x["prefix"] == [] for x in w[1:])


def test_initial_prompt_heads_the_history():
    w = both([2000], [[win(PAIR)]], initial_prompt=[11, 12, 13])["files"][0]["windows"]
    assert w[0]["prefix"] == [SOT_PREV, 11, 12, 13]
    assert w[1]["prefix"] == [SOT_PREV, 11, 12, 13, T(0), 5, 6, T(500)]


def test_history_longer_than_half_the_text_context():
    long_seg = [T(0)] + list(range(1, 150)) + [T(500), T(500)]
    w = both([3000], [[win(long_seg)]], max_new_tokens=160)["files"][0]["windows"]
    assert len(w[1]["prefix"]) == 152 and len(w[2]["prefix"]) == 224                                   # 1 + 151 ids, then 1 + (448 / 2 - 1)
    assert w[2]["prefix"][0] == SOT_PREV and w[2]["prefix"][-1] == T(500)


def test_prefix_trimmed_against_a_large_max_new_tokens():
    long_seg = [T(0)] + list(range(1, 150)) + [T(500), T(500)]
    w = both([3000], [[win(long_seg)]], max_new_tokens=400)["files"][0]["windows"]
    assert len(w[1]["prefix"]) == 448 - 3 - 400 and w[1]["prefix"][0] == SOT_PREV and w[1]["prefix"][-1] == T(500)
    w = both([3000], [[win(long_seg)]], max_new_tokens=444)["files"][0]["windows"]
    assert w[1]["prefix"] == []                                                                        # room for <|startofprev|> alone: no prefix


def test_terminates_under_the_zero_advance_script():
    got = both([7000, 100], [[win([T(0), T(0), 5])], [win([T(0), T(0)])]])
    assert [w["advance"] for w in got["files"][0]["windows"]] == [3000, 3000, 1000]
    assert len(got["files"][1]["windows"]) == 1 and got["files"][0]["segments"] == []


# ---- the CLI's refusals, before any device is touched ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra,word", [(["--language", "auto"], "--language auto"), (["--overlap-s", "5"], "--overlap-s"), (["--beam-size", "2"], "--beam-size"),
                                        (["--condition-on-previous-text", "2"], "0 or 1"), (["--sequential-max-audio-s", "0"], "above 0")])
def test_cli_refuses_what_sequential_cannot_do(extra, word):
    import subprocess
    cli = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
    r = subprocess.run([cli, "--sequential", "--onnx-dir", "synthetic:nano:1"] + extra, capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and word in r.stderr, r.stderr


# ---- the symbols --------------------------------------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported():
    host = wb.load_host_library()
    for name in ("whh_seek_advance", "whh_run_sequential"):
        assert hasattr(host, name)
    hdr = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    for name in ("wh_files_load", "wh_files_load_raw", "wh_transcribe_windows", "wh_files_window_mel"):
        assert re.search(r"\bint %s\(wh_ctx\*" % name, hdr), name
    L = wb.load_library()
    for name in ("wh_files_load", "wh_files_load_raw", "wh_transcribe_windows", "wh_files_window_mel"):
        assert hasattr(L, name)
    for name in ("files_load", "files_load_raw", "transcribe_windows", "files_window_mel"):
        assert callable(getattr(wb.Context, name))
