"""CPU checks of the beam search: the numpy restatement in tests/beam_ref.py on hand-built logit tables with known answers,
against greedy decoding on the numpy decoder, the top-(K + 1)-per-row shortcut against the walk over the whole K x V list, and the ABI."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import align_ref as ar
import beam_ref as br
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EOT = 2
NINF = float("-inf")


def table(rows):
    """logits [K][V] whose row softmaxes are the given probabilities (log p: lp == the table, lse == 0)."""
    return np.log(np.asarray(rows, np.float64)).astype(np.float32)


def test_eot_enters_the_pool_mid_walk():
    """K = 2, both beams live.  Order: (0, 5) .6*.5, (1, EOT) .4*.7, (0, 6) .6*.3 ... -> the EOT of beam 1 is finished between the two live picks."""
    lg = table([[.05, .05, .1, .0001, .0001, .5, .2998], [.05, .05, .7, .05, .05, .05, .05]])
    sc = [float(np.log(np.float32(.6))), float(np.log(np.float32(.4)))]
    live, fin, margins, _ = br.step(lg, [[9], [8]], sc, EOT, 2)
    assert [(p, t) for p, t, _, _ in live] == [(0, 5), (0, 6)]
    assert [j for j, _, _ in fin] == [1]
    assert abs(fin[0][1] - np.log(.4 * .7)) < 1e-6 and abs(live[0][2] - np.log(.6 * .5)) < 1e-6
    assert len(margins) == 3 and min(margins) > 0.05   # log(.6 * .3) against log(.4 * .7)


def test_patience_two_keeps_collecting():
    """K = 2, patience 2 -> C = 4: a search whose every position offers EOT second runs until the pool holds 4."""
    def fn(h):
        return table([[.1, .1, .3, .4, .1]] * 2)
    r = br.search(fn, 2, 2.0, 24, EOT)
    assert len(r["pool"]) == 4 and r["trace"][-1]["pool_size"] == 4
    r1 = br.search(fn, 2, 1.0, 24, EOT)
    assert len(r1["pool"]) == 2 and len(r1["trace"]) < len(r["trace"])
    assert all(h["tokens"][-1] == EOT for h in r["pool"])


def test_dead_beams():
    """All but two ids suppressed: position 0 yields two candidates for K = 3 -> the third beam is dead, keeps its own index as parent, and
    none of its candidates is ever taken."""
    lg = np.zeros((3, 6), np.float32)
    live, fin, _, _ = br.step(lg, [[], [], []], [0.0, NINF, NINF], EOT, 3, suppress=[0, 1, 2, 3])
    assert [(p, t) for p, t, _, _ in live] == [(0, 4), (0, 5), (2, -1)] and live[2][2] == NINF and not fin
    lg[2, 4] = 100.0   # the dead beam's logits do not matter
    live2, _, _, _ = br.step(lg, [[4], [5], []], [live[0][2], live[1][2], NINF], EOT, 3, suppress=[0, 1, 2, 3])
    assert [(p, t) for p, t, _, _ in live2] == [(0, 4), (0, 5), (1, 4)]   # four candidates from the two live beams: the dead slot is filled again
    # nothing allowed at all: every beam dies
    live3, fin3, _, _ = br.step(lg, [[4], [5], []], [0.0, -1.0, NINF], EOT, 3, suppress=list(range(6)))
    assert [t for _, t, _, _ in live3] == [-1, -1, -1] and not fin3


def test_len_zero_ranks_without_dividing_by_zero():
    """EOT first: the hypothesis [EOT] has len 0 -> counted as 1."""
    def fn(h):
        return table([[.05, .05, .8, .1]])
    r = br.search(fn, 1, 1.0, 4, 3)        # eot = 3 is never best: a live beam of 4 tokens
    assert not r["hyps"][0]["finished"] and len(r["hyps"][0]["tokens"]) == 4
    r = br.search(fn, 1, 1.0, 4, EOT)      # K = 1: the best candidate is EOT at position 0
    h = r["hyps"][0]
    assert h["finished"] and h["tokens"] == [EOT] and np.isfinite(h["rank"]) and abs(h["rank"] - np.log(np.float32(.8))) < 1e-6
    for lpn in (0.0, 1.0):
        assert np.isfinite(br.rank([{"tokens": [EOT], "lps": [0.0], "score": -1.0}], [], 1, lpn)[0]["rank"])


def test_tie_order():
    """Equal scores: the lower beam first, then the lower id; the margins of tied decisions are 0."""
    lg = np.zeros((2, 5), np.float32)
    live, _, margins, _ = br.step(lg, [[7], [7]], [-1.0, -1.0], 9, 2)
    assert [(p, t) for p, t, _, _ in live] == [(0, 0), (0, 1)] and margins == [0.0, 0.0]
    lg[1, 3] = 1e-3
    live, _, _, _ = br.step(lg, [[7], [7]], [-1.0, -1.0], 9, 2)
    assert (live[0][0], live[0][1]) == (1, 3)


def test_ranking_and_length_penalty():
    pool = [{"tokens": [5, 6, 7, EOT], "lps": [0] * 4, "score": -3.0}, {"tokens": [5, EOT], "lps": [0] * 2, "score": -1.5}]
    live = [{"tokens": [5, 6], "lps": [0, 0], "score": -0.5}, {"tokens": [1, 1], "lps": [0, 0], "score": NINF}]
    r = br.rank(pool, live, 3, -1.0)
    assert [h["score"] for h in r] == [-0.5, -3.0, -1.5] and [h["finished"] for h in r] == [False, True, True]
    assert abs(r[1]["rank"] + 1.0) < 1e-6 and abs(r[2]["rank"] + 1.5) < 1e-6
    r0 = br.rank(pool, live, 3, 0.0)       # penalty 0: the raw scores
    assert [h["score"] for h in r0] == [-0.5, -1.5, -3.0]
    r1 = br.rank(pool, live, 2, 1.0)       # pool already holds K: no live beam added
    assert len(r1) == 2 and abs(r1[0]["rank"] - (-1.5 / 1.0)) < 1e-6 and abs(r1[1]["rank"] - (-3.0 / (8.0 / 6.0))) < 1e-6


@pytest.fixture(scope="module")
def nano():
    dims = ms.PRESETS["nano"]
    sd = ms.synth_state_dict(dims, 7)
    w = ms.flatten_state_dict(dims, sd)
    enc = orc.encoder(dims, w, orc.window_mel(orc.log_mel(ms.synth_clip(1500), dims.n_mels), 0, 3000))
    return dims, sd, w, enc


def test_k1_equals_greedy_on_the_numpy_decoder(nano):
    dims, sd, w, enc = nano
    prompt = [3, 5, 7]
    toks, _ = orc.decode_greedy(dims, w, enc, prompt, 12, EOT, [EOT], want_logits=True)
    greedy = [int(t) for t in toks[len(prompt):]]

    def fn(hists):
        return np.stack([ar.decoder(dims, sd, enc, prompt + h, np.float32)[0][-1] for h in hists])
    r = br.search(fn, 1, 1.0, 12, EOT, suppress=[EOT])
    assert r["hyps"][0]["tokens"] == greedy
    assert all(t["parents"] == [0] for t in r["trace"])


@pytest.mark.parametrize("K,rules", [(1, None), (3, None), (5, None), (8, None), (4, (40, 39, 3))])
def test_top_k_plus_one_per_row_is_the_full_walk(K, rules):
    rng = np.random.default_rng(100 + K)
    V = 64
    for trial in range(40):
        lg = rng.standard_normal((K, V)).astype(np.float32) * 3
        lg[:, EOT] += rng.uniform(0, 6)                         # EOT near the top now and then
        if trial % 3 == 0:
            lg[rng.integers(K), rng.integers(V, size=5)] = np.nan
        if trial % 4 == 0:
            lg = np.round(lg)                                   # ties
        scores = (-rng.uniform(0, 3, K)).astype(np.float32).tolist()
        for j in range(K):
            if j and rng.uniform() < 0.2:
                scores[j] = NINF
        hists = [[int(t) for t in rng.integers(3, V - 1, size=trial % 4)] for _ in range(K)]
        room = int(rng.integers(0, 4))
        a = br.step(lg, hists, scores, EOT, room, suppress=[0], begin_suppress=[EOT], rules=rules, full=False)
        b = br.step(lg, hists, scores, EOT, room, suppress=[0], begin_suppress=[EOT], rules=rules, full=True)
        assert a[0] == b[0] and a[1] == b[1], (trial, a[:2], b[:2])


def test_header_and_library_export_the_beam_symbols():
    lib = wb.load_library()
    hdr = open(os.path.join(ROOT, "include", "whisper_hip.h")).read()
    for name in ("wh_ctx_set_beam_search", "wh_get_beams", "wh_get_beam_trace"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in wb.EXPORTS and hasattr(lib, name)
    for macro, val in (("WH_MAX_BEAMS", 8), ("WH_MAX_BEAM_CANDIDATES", 16), ("WH_MAX_BEAM_TRACE_CLIPS", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, val), hdr) and getattr(wb, macro) == val
    assert C.sizeof(wb.WhBeamOpts) == 40
    # NULL handles are refused, nothing is dereferenced
    assert lib.wh_ctx_set_beam_search(None, None) == 4
    assert lib.wh_get_beams(None, None, 0, None, None, None, None, 0, None, 0, None) == 4
    assert lib.wh_get_beam_trace(None, 0, None, None, None, None, 0, None) == 4


CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")


@pytest.mark.parametrize("flags,needle", [
    (["--beam-size", "0"], "--beam-size"), (["--beam-size", "9"], "--beam-size"), (["--beam-size", "five"], "--beam-size"),
    (["--beam-size", "2", "--patience", "0"], "--patience"), (["--beam-size", "2", "--patience", "nan"], "--patience"),
    (["--beam-size", "8", "--patience", "2.2"], "--patience"), (["--beam-size", "2", "--length-penalty", "nan"], "--length-penalty"),
    (["--beam-size", "2", "--n-best", "0"], "--n-best"), (["--n-best", "2"], "--n-best"),
    (["--beam-size", "4", "--max-batch", "3"], "--max-batch"),
    (["--beam-size", "2", "--repetition-penalty", "1.3"], "--repetition-penalty"), (["--beam-size", "2", "--word-timestamps"], "--word-timestamps"),
    (["--beam-size", "2", "--prompt-ids", "5,6"], "--prompt-ids"), (["--beam-size", "2", "--precision", "fp8"], "--precision"),
])
def test_cli_refuses_bad_beam_flags_before_touching_a_device(flags, needle):
    import subprocess
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7"] + flags + ["--print-plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and needle in r.stderr and "error:" in r.stderr, (r.returncode, r.stderr)


def test_cli_accepts_the_beam_flags_and_plans_the_batches():
    import json
    import subprocess
    r = subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7", "--beam-size", "5", "--patience=2", "--length-penalty", "1", "--n-best", "3", "--max-batch", "16",
                        "--print-plan"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    plan = json.loads(r.stdout)
    assert plan["beam_size"] == 5 and plan["n_best"] == 3 and plan["files_per_batch"] == 3 and plan["patience"] == 2 and plan["length_penalty"] == 1
    # --beam-size 1 is the greedy path: the plan of a command line without the flag
    a = subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7", "--beam-size", "1", "--print-plan"], capture_output=True, text=True, timeout=60)
    b = subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7", "--print-plan"], capture_output=True, text=True, timeout=60)
    assert a.returncode == 0 and a.stdout == b.stdout and "beam_size" not in b.stdout
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert all(f in h.stdout for f in ("--beam-size", "--patience", "--length-penalty", "--n-best"))


def test_config_used_gains_beam_size_only_from_two_beams_on():
    """Through the summary emitter whisper_bench calls (reference_summary): without --beam-size, and with --beam-size 1, the text is the
    greedy one byte for byte (tests/test_host_cpu.py holds that text to the reference's archived file); from two beams on config_used
    gains beam_size and nothing else moves.  results_table reads the key when it is there."""
    import importlib.util
    import json
    L = C.CDLL(os.path.join(ROOT, "whisper-rust-ort_amd", "libwh_host.so"))
    L.whh_summary_json.argtypes = [C.POINTER(C.c_double), C.c_size_t, C.c_char_p, C.POINTER(C.c_longlong), C.c_uint, C.c_char_p, C.c_size_t]
    L.whh_summary_json.restype = C.c_size_t

    def summary(beam):
        lists = (C.c_double * 6)(2.0, 0.1, 0.2, 1.5, 0.1, 0.07)
        strs = b"openai/whisper-base\0synthetic:base:1\0en\0transcribe\0\0SEQUENTIAL\0ENABLE_ALL\0"
        ints = (C.c_longlong * 3)(1, 1, 128)
        buf = C.create_string_buffer(1 << 16)
        n = L.whh_summary_json(lists, 1, strs, ints, 2 | 4 | 8 | (beam << 4), buf, len(buf))
        return buf.raw[:n].decode()
    greedy = summary(0)
    assert summary(1) == greedy and "beam_size" not in greedy
    j0, j5 = json.loads(greedy), json.loads(summary(5))
    assert j5["config_used"].pop("beam_size") == 5 and j5 == j0
    spec = importlib.util.spec_from_file_location("results_table", os.path.join(ROOT, "whisper-rust-ort_amd", "results_table.py"))
    rt = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rt)
    assert rt.beam_of(j0) == 1 and rt.beam_of(json.loads(summary(5))) == 5


@pytest.fixture(scope="module")
def cap_models():
    """The two CPU-sized models of tests/test_beam_gpu.py with the encoder states of the clips its cases use (1500 .. 1502)."""
    out = {}
    for preset, seed in (("nano", 7), ("micro", 11)):
        dims = ms.PRESETS[preset]
        sd = ms.synth_state_dict(dims, seed)
        w = ms.flatten_state_dict(dims, sd)
        out[preset] = (dims, sd, [orc.encoder(dims, w, orc.window_mel(orc.log_mel(ms.synth_clip(1500 + i), dims.n_mels), 0, 3000)) for i in range(3)])
    return out


# the nano / micro cases of tests/test_beam_gpu.py: (preset, K, patience, rules, EOT suppressed, begin_suppress)
CAP_CASES = [("nano", 1, 1.0, False, True, [5]), ("nano", 2, 1.0, False, True, [5]), ("nano", 5, 1.0, False, True, [5]), ("nano", 8, 1.0, False, True, [5]),
             ("micro", 5, 1.0, True, True, []), ("micro", 5, 2.0, False, False, [])]


@pytest.mark.parametrize("preset,K,patience,rules_on,sup_eot,begin", CAP_CASES, ids=[f"{c[0]}-K{c[1]}-p{c[2]:g}-{'rules' if c[3] else 'plain'}" for c in CAP_CASES])
def test_reference_stays_under_the_undecided_cap(cap_models, preset, K, patience, rules_on, sup_eot, begin):
    """The seeds, clips, beam sizes and 24 positions tests/test_beam_gpu.py uses for nano and micro: on the numpy decoder's f32 logits the
    decisions whose margin is below delta (or whose position's rule-5 margin is below 1e-4) are at most 2 % per case — the cap that file
    holds a GPU run to.  (The base and large-v3 cases have no CPU-sized decoder; their GPU runs are held to the cap directly.)"""
    dims, sd, encs = cap_models[preset]
    prompt, tb = [3, 5, 7], dims.vocab - 301
    rules = (tb, tb - 1, 50) if rules_on else None
    n = und = 0
    for enc in encs:
        vmax = [0.0]

        def fn(hists):
            live = {tuple(h) for h in hists}                       # (equal histories: one decoder pass)
            lg = {h: ar.decoder(dims, sd, enc, prompt + list(h), np.float32)[0][-1] for h in live}
            out = np.stack([lg[tuple(h)] for h in hists])
            vmax[0] = float(np.abs(out).max())
            return out
        r = br.search(fn, K, patience, 24, EOT, suppress=[EOT] if sup_eot else [], begin_suppress=begin, rules=rules)
        for t in r["trace"]:
            for s, m in zip(t["scores"], t["margins"]):
                n += 1
                und += m < br.delta(s if np.isfinite(s) else 0.0, vmax[0], dims.vocab) or t["rule5"] < 1e-4
    print(f"{preset} K={K} patience={patience:g} rules={rules_on}: {n} decisions, {und} undecided")
    assert n >= 24 * 3 and und <= 0.02 * n
