"""CPU checks of the timestamp feature: known answers of the numpy restatement of the rules, the host library's segment splitter
against its Python form, the SRT / VTT text byte for byte, and the CLI's flags."""
import os
import subprocess

import numpy as np
import pytest

import timestamp_rules_ref as tr
from whisper_rust_ort_amd import binding as wb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")

# a small vocabulary: 0..9 text, 10 = EOT, 11..12 specials, 13 = <|notimestamps|>, 14.. = timestamps (tb = 14)
V, EOT, NOTS, TB = 40, 10, 13, 14


def row(**vals):
    x = np.full(V, -5.0, np.float32)
    for k, v in vals.items():
        x[int(k[1:])] = v
    return x


def pick(x, seq, max_init=50, **kw):
    return tr.apply_rules(x, seq, TB, EOT, NOTS, max_init, **kw)[0]


def test_pair_forbids_timestamps_and_keeps_text():
    x = row(t3=1.0, t20=9.0)
    assert pick(x, [TB, 5, 16, 16]) == 3          # after a pair: no timestamp, text wins
    assert pick(x, [TB, 5, 16]) == 20             # after a single one a timestamp is allowed


def test_single_timestamp_forbids_text_below_eot():
    x = row(t3=9.0, t10=1.0, t15=-20.0, t30=-20.0)
    assert pick(x, [TB, 5, 20]) == EOT            # ids < EOT suppressed, EOT allowed
    x = row(t3=9.0, t10=-30.0, t25=2.0)
    assert pick(x, [TB, 5, 20]) == 25             # ... or a timestamp at or above the last


def test_last_timestamp_versus_plus_one():
    x = row(t20=9.0, t21=8.0)
    assert pick(x, [TB, 5, 20]) == 20             # single ending: timestamps below T suppressed, T itself allowed
    x = row(t3=-30.0, t20=9.0, t21=8.0)
    assert pick(x, [TB, 20, 5]) == 21             # text ending: below T + 1 suppressed


def test_first_token_bound():
    x = row(t3=50.0, t30=10.0, t16=1.0)
    assert pick(x, [], max_init=5) == 16          # first token is a timestamp within tb + 5
    assert pick(x, [], max_init=-1) == 30         # no bound
    assert pick(x, [], max_init=16) == 30


def test_step_five_fires_and_not():
    x = row(t3=1.0, **{f"t{i}": 0.0 for i in range(20, 26)})   # lse of six 0.0 logits = log 6 = 1.79 > 1.0
    assert pick(x, [TB, 5]) == 20
    x = row(t3=2.0, **{f"t{i}": 0.0 for i in range(20, 26)})   # 1.79 < 2.0: the argmax over both
    assert pick(x, [TB, 5]) == 3


def test_notimestamps_suppressed():
    x = row(t13=100.0, t3=1.0)
    assert pick(x, [TB, 5, 6]) == 3


def test_all_suppressed_is_zero_and_ties_take_the_lowest_id():
    x = row(t3=1.0)
    assert pick(x, [TB, 5], suppress=list(range(V))) == 0
    x = row(t4=2.0, t7=2.0)
    assert pick(x, [TB, 5, 16, 16]) == 4
    x = row(t3=-40.0, t21=3.0, t22=3.0)
    assert pick(x, [TB, 5, 20]) == 21


def test_nan_never_wins_and_is_left_out_of_the_sum():
    x = row(t3=1.0, t5=np.nan, t20=np.nan, t21=0.5)
    tok, lse, mt = tr.apply_rules(x, [TB, 5], TB, EOT, NOTS, 50)
    assert tok == 3 and np.isclose(lse, np.log(np.exp(0.5) + (V - TB - 3) * np.exp(-5.0)))   # tb itself is below T + 1
    assert mt == 1.0


def crafted_sequences():
    return [
        [], [EOT], [TB, EOT], [TB, 3, 4, 20, 20, 5, 6, 30, EOT], [TB, 3, 20], [TB, 3, 20, 20, 5, 6], [3, 4, 5],
        [3, 4, 25, EOT, 9, 9], [TB, TB], [TB, 3, 20, 20, 30, 30, 5, 40], [TB, 20, 3], [20, 3, 4],
    ]


def test_cpp_splitter_equals_python_form():
    rng = np.random.Generator(np.random.PCG64(5))
    seqs = crafted_sequences()
    for _ in range(300):
        n = int(rng.integers(0, 30))
        seqs.append(rng.choice(np.r_[np.arange(0, 10), np.arange(TB, V), [EOT]], size=n).tolist())
    for s in seqs:
        got = wb.split_segments(s, TB, EOT, 30.0)
        ref = tr.split_segments(s, TB, EOT, 30.0)
        assert len(got) == len(ref), s
        for g, r in zip(got, ref):
            assert g["tokens"] == r["tokens"] and abs(g["start"] - r["start"]) < 1e-6 and abs(g["end"] - r["end"]) < 1e-6, (s, got, ref)


def test_splitter_ending_cases():
    assert tr.split_segments([TB, 3, 20, 20, 5, 30], TB, EOT, 30.0) == [
        {"start": 0.0, "end": 6 * 0.02, "tokens": [3]}, {"start": 6 * 0.02, "end": 16 * 0.02, "tokens": [5]}]          # single ending closes
    segs = tr.split_segments([TB, 3, 20, 20, 5, 6], TB, EOT, 12.5)
    assert segs[-1] == {"start": 6 * 0.02, "end": 12.5, "tokens": [5, 6]}                                              # open text: to duration
    assert tr.split_segments([3, 4, 25], TB, EOT, 30.0) == [{"start": 0.0, "end": 11 * 0.02, "tokens": [3, 4]}]     # no pair
    assert tr.split_segments([3, 4], TB, EOT, 7.0) == [{"start": 0.0, "end": 7.0, "tokens": [3, 4]}]
    # text before the first pair: that slice starts at 0, never at a negative time
    assert tr.split_segments([3, TB + 6, TB + 7, 4], TB, EOT, 9.0) == [
        {"start": 0.0, "end": 6 * 0.02, "tokens": [3]}, {"start": 7 * 0.02, "end": 9.0, "tokens": [4]}]
    assert wb.split_segments([3, TB + 6, TB + 7, 4], TB, EOT, 9.0)[0]["start"] == 0.0


def test_splitter_times_lie_in_the_window():
    rng = np.random.Generator(np.random.PCG64(13))
    for _ in range(300):
        s = rng.choice(np.r_[np.arange(0, 10), np.arange(TB, V), [EOT]], size=int(rng.integers(0, 30))).tolist()
        for g in wb.split_segments(s, TB, EOT, 30.0):
            assert 0.0 <= g["start"] and 0.0 <= g["end"] <= 30.0, (s, g)


def test_longform_merge_equals_python_form():
    rng = np.random.Generator(np.random.PCG64(9))
    for _ in range(50):
        k = int(rng.integers(1, 5))
        windows = [[TB] + rng.choice(np.r_[np.arange(0, 10), np.arange(TB, V)], size=int(rng.integers(0, 20))).tolist() for _ in range(k)]
        starts = [25.0 * i for i in range(k)]
        durs = [30.0] * (k - 1) + [float(rng.uniform(1, 30))]
        got = wb.longform_segments(windows, starts, durs, 5.0, TB, EOT)
        ref = tr.merge_windows([tr.split_segments(w, TB, EOT, d) for w, d in zip(windows, durs)], starts, 5.0)
        assert [g["tokens"] for g in got] == [r["tokens"] for r in ref]
        assert np.allclose([g["start"] for g in got], [r["start"] for r in ref], atol=1e-6)
        assert np.allclose([g["end"] for g in got], [r["end"] for r in ref], atol=1e-6)
    # a segment of window 1 starting inside the first half of the overlap belongs to window 0
    got = wb.longform_segments([[TB, 3, TB + 100, TB + 100, 4, TB + 500], [TB, 5, TB + 50, TB + 150, 6, TB + 200]], [0.0, 25.0], [30.0, 10.0], 5.0,
                               TB, EOT)
    assert [g["tokens"] for g in got] == [[3], [4], [6]]
    assert np.isclose(got[2]["start"], 28.0) and np.isclose(got[2]["end"], 29.0)


def test_srt_and_vtt_text():
    cues = [(0.0, 1.5, "hello"), (3723.4565, 3725.0004, "x y"), (36000.0, 36000.02, "late")]
    assert wb.srt(cues) == ("1\n00:00:00,000 --> 00:00:01,500\nhello\n\n"
                            "2\n01:02:03,457 --> 01:02:05,000\nx y\n\n"
                            "3\n10:00:00,000 --> 10:00:00,020\nlate\n\n")
    assert wb.vtt(cues) == ("WEBVTT\n\n"
                            "1\n00:00:00.000 --> 00:00:01.500\nhello\n\n"
                            "2\n01:02:03.457 --> 01:02:05.000\nx y\n\n"
                            "3\n10:00:00.000 --> 10:00:00.020\nlate\n\n")
    assert wb.srt([]) == "" and wb.vtt([]) == "WEBVTT\n\n"


def test_cli_help_lists_the_timestamp_flags():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=30).stdout
    for flag in ("--timestamp-rules", "--write-srt", "--write-vtt", "--timestamps"):
        assert flag in out, flag


def test_rules_struct_and_entry_are_exported():
    lib = wb.load_library()
    assert hasattr(lib, "wh_ctx_set_timestamp_rules")
    assert wb.C.sizeof(wb.WhTimestampRules) == 32
