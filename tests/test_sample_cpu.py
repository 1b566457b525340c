"""CPU checks of the temperature sampling's reference (tests/sample_ref.py) and of the host logic of the temperature ladder (host/wh_host.h
through the shims of libwh_host.so, and whisper_bench's flags).  No GPU."""
import ctypes as C
import json
import os
import subprocess
import zlib

import numpy as np
import pytest

import sample_ref as sr
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
F = np.float32
NAN = float("nan")


# ---- Philox4x32-10 and the draw ----------------------------------------------------------------------------------------------------------------

KAT = [   # Random123's known answers for philox4x32 with 10 rounds: (counter, key, output)
    ([0, 0, 0, 0], [0, 0], [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
    ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
    ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0], [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]),
]


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox_known_answers(ctr, key, want):
    assert list(sr.philox4x32_10(ctr, key)) == want
    seed, row = key[0] | (key[1] << 32), ctr[2] | (ctr[3] << 32)
    assert sr.philox_block([ctr[0]], ctr[1], row, seed)[0].tolist() == want          # the vectorised form, counters and key laid out as the definition says


def test_vectorised_philox_is_the_scalar_one():
    rng = np.random.default_rng(3)
    for _ in range(20):
        c0, g = int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 448))
        row, seed = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 63))
        want = sr.philox4x32_10([c0, g, row & sr.MASK, row >> 32], [seed & sr.MASK, seed >> 32])
        assert sr.philox_block([c0], g, row, seed)[0].tolist() == list(want)


def test_uniform_is_exact_and_strictly_inside_the_unit_interval():
    u = sr.uniform([0, 0xFFFFFFFF, 0x1FF, 0x200])
    assert u.dtype == F and 0.0 < u.min() and u.max() < 1.0
    assert u[0] == F(2.0 ** -24) and u[1] == F(1.0 - 2.0 ** -24) and u[2] == u[0] and u[3] == F(1.5 * 2.0 ** -23)
    assert float(u[1]) == (float(0xFFFFFFFF >> 9) + 0.5) * 2.0 ** -23                # no rounding: the f32 value is the real number
    g = sr.gumbel(u)
    assert np.isfinite(g).all() and g[0] < 0 < g[1]
    # why 23 bits and not 24: (x >> 8) + 0.5f is not representable above 2^23, and the largest draws would round to u = 1 (gum = +inf)
    assert F(0xFFFFFFFF >> 8) + F(0.5) == F(2 ** 24)


CHI2_BOUND = 24.32   # the 0.999 quantile of chi-square with 7 degrees of freedom; measured: T = 0.5 -> 5.71, T = 1 -> 4.90 (deterministic)


@pytest.mark.parametrize("T", [0.5, 1.0])
def test_reference_draws_follow_softmax_of_v_over_t(T):
    """8 allowed ids of a 12-id vocabulary, 20,000 row ids, one seed: the observed frequencies against softmax(v / T)."""
    V, n, seed, g = 12, 20000, 20240607, 3
    v = np.array([0.3, -1.0, 2.0, 0.5, 9.0, 1.2, -0.4, 0.0, 9.0, 1.7, 0.9, -2.0], F)
    suppress = [4, 8, 1, 11]
    ids = np.array([i for i in range(V) if i not in suppress])
    x = sr.philox_block(np.arange(3)[None, :], g, np.arange(n)[:, None], seed).reshape(n, 12)
    score = (v[None, :] * (F(1.0) / F(T))).astype(F) + sr.gumbel(sr.uniform(x))
    tok = ids[np.argmax(score[:, ids], axis=1)]
    for r in range(100):   # the vectorised form above is what step() computes
        assert sr.step(v, [0], T, seed, r, g, 99, suppress)[0] == tok[r]
    p = np.exp(v[ids].astype(np.float64) / T)
    p /= p.sum()
    obs = np.array([(tok == i).sum() for i in ids], np.float64)
    chi2 = float(((obs - n * p) ** 2 / (n * p)).sum())
    print(f"T={T}: chi-square {chi2:.2f} (bound {CHI2_BOUND})")
    assert chi2 < CHI2_BOUND


def test_step_masks_rules_and_logprob():
    v = np.array([1.0, 5.0, np.nan, 2.0, -np.inf, 3.0], F)
    tok, lp, margin, r5, delta = sr.step(v, [], 0.0, 1, 0, 0, eot=99, suppress=[1])
    ok = [0, 3, 5]
    assert tok == 5 and margin == 1.0 and r5 == np.inf
    assert abs(lp - (3.0 - np.log(np.exp(v[ok].astype(np.float64)).sum()))) < 1e-12
    assert sr.step(v, [], 1.0, 1, 0, 0, eot=99, suppress=[0, 1, 3, 5])[:2] == (0, float("-inf"))     # nothing allowed
    # T > 0: the token is always an allowed one, and the same (seed, row id, position) draws the same token
    for r in range(50):
        a = sr.step(v, [], 1.0, 7, r, 2, eot=99, suppress=[1])
        assert a[0] in ok and a == sr.step(v, [], 1.0, 7, r, 2, eot=99, suppress=[1])
    assert len({sr.step(v, [], 1.0, 7, r, 2, eot=99, suppress=[1])[0] for r in range(50)}) > 1


def test_reference_is_decided_on_the_oracle_logits():
    """The undecided band on real logits: the oracle's nano logits of 24 positions, 20 random streams each at T = 1 and T = 0.2 — at most 2 % of
    the positions may have a perturbed margin below delta (measured: 0 of 960)."""
    from oracle import oracle as orc
    dims = ms.PRESETS["nano"]
    w = ms.flatten_state_dict(dims, ms.synth_state_dict(dims, 7))
    mel = orc.window_mel(orc.log_mel(ms.synth_clip(1500), 80), 0, 3000)
    _, logits = orc.decode_greedy(dims, w, orc.encoder(dims, w, mel), [3, 5, 7], 24, 2, [2], want_logits=True)
    n = und = 0
    for T in (1.0, 0.2):
        for r in range(20):
            for g in range(len(logits)):
                _, _, margin, _, delta = sr.step(logits[g], [0] * g, T, 11, r, g, 2, [2])
                n += 1
                und += margin < delta
    print(f"{n} positions, {und} undecided")
    assert n == 960 and und <= 0.02 * n


# ---- the host logic of the ladder -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def host():
    L = C.CDLL(os.path.join(ROOT, "whisper-rust-ort_amd", "libwh_host.so"))
    L.whh_compression_ratio.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_char_p, C.c_size_t]
    L.whh_compression_ratio.restype = C.c_double
    L.whh_zlib_version.argtypes = [C.c_char_p, C.c_size_t]
    L.whh_zlib_version.restype = C.c_size_t
    L.whh_needs_fallback.argtypes = [C.c_double] * 6
    L.whh_run_ladder.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_double), C.c_double, C.c_double, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_ubyte)]
    L.whh_run_ladder.restype = None
    L.whh_parse_temperatures.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_size_t, C.c_char_p, C.c_size_t]
    L.whh_parse_temperatures.restype = C.c_long
    L.whh_ladder_row_json.argtypes = [C.c_char_p, C.c_char_p, C.c_double, C.c_double, C.c_int, C.c_char_p, C.c_size_t]
    L.whh_ladder_row_json.restype = C.c_size_t
    L.whh_ladder_config_json.argtypes = [C.POINTER(C.c_float), C.c_size_t, C.c_char_p, C.c_size_t]
    L.whh_ladder_config_json.restype = C.c_size_t
    return L


def cr_of(host, data: bytes):
    n, err = C.c_size_t(0), C.create_string_buffer(256)
    cr = host.whh_compression_ratio(data, len(data), C.byref(n), err, 256)
    assert not np.isnan(cr), err.value
    return cr, int(n.value)


def test_compression_ratio_is_openai_whispers(host):
    rep = ("the same thing again and again " * 40).encode()
    rng = np.random.default_rng(5)
    rnd = bytes(rng.integers(33, 127, 200, dtype=np.uint8).tolist())
    assert len(rnd) == 200
    ver = C.create_string_buffer(64)
    assert host.whh_zlib_version(ver, 64) > 0
    same = ver.value.decode() == zlib.ZLIB_RUNTIME_VERSION
    for data, test in ((rep, lambda c: c > 5.0), (rnd, lambda c: c < 1.5), ("żółć — ¿qué? " .encode() * 9, lambda c: c > 1.0)):
        cr, n = cr_of(host, data)
        py = len(data) / len(zlib.compress(data))
        assert test(cr) and test(py), (cr, py)
        assert (cr > 2.4) == (py > 2.4)                       # the decision at openai-whisper's threshold
        if same:
            assert n == len(zlib.compress(data)) and cr == py
    assert cr_of(host, b"")[0] == 0.0


def test_needs_fallback(host):
    f = lambda *a: bool(host.whh_needs_fallback(*a))
    for args in [(3.0, -0.5, 0.1, 2.4, -1.0, 0.6), (2.0, -1.5, 0.1, 2.4, -1.0, 0.6), (2.0, -0.5, 0.1, 2.4, -1.0, 0.6), (3.0, -1.5, 0.9, 2.4, -1.0, 0.6),
                 (3.0, -1.5, 0.9, 2.4, -1.0, NAN), (3.0, -0.5, 0.1, NAN, -1.0, 0.6), (2.0, -1.5, 0.1, 2.4, NAN, 0.6), (9.0, -9.0, 0.0, NAN, NAN, NAN),
                 (2.4, -1.0, 0.6, 2.4, -1.0, 0.6), (float("inf"), float("-inf"), 0.0, 2.4, -1.0, 0.6)]:
        none = lambda x: None if np.isnan(x) else x
        assert f(*args) == sr.needs_fallback(args[0], args[1], args[2], none(args[3]), none(args[4]), none(args[5])), args
    assert f(3.0, -0.5, 0.1, 2.4, -1.0, 0.6) and f(2.0, -1.5, 0.1, 2.4, -1.0, 0.6) and not f(2.0, -0.5, 0.1, 2.4, -1.0, 0.6)
    assert not f(3.0, -1.5, 0.9, 2.4, -1.0, 0.6)             # silence stops the ladder
    assert f(3.0, -1.5, 0.9, 2.4, -1.0, NAN)                 # ... unless its threshold is off


def test_ladder_driver_against_a_scripted_decoder(host):
    """Four rungs, six windows.  Window 0 passes at once; 1 fails on its log-probability once; 2 fails on its compression ratio twice; 3 fails
    at every rung (the last result stands); 4 fails but counts as silence (never decoded again); 5 fails, then turns silent at rung 1."""
    n, R = 6, 4
    good, bad_lp, bad_cr, silent = (1.5, -0.3, 0.1), (1.5, -2.0, 0.1), (4.0, -0.3, 0.1), (4.0, -2.0, 0.9)
    script = np.zeros((R, n, 3))
    script[:, 0] = good
    script[:, 1] = [bad_lp, good, good, good]
    script[:, 2] = [bad_cr, bad_cr, good, good]
    script[:, 3] = [bad_lp, bad_cr, bad_lp, bad_cr]
    script[:, 4] = silent
    script[:, 5] = [bad_lp, silent, good, good]
    rung_of = (C.c_int * n)()
    dec = np.zeros((R, n), np.uint8)
    host.whh_run_ladder(n, R, script.ctypes.data_as(C.POINTER(C.c_double)), 2.4, -1.0, 0.6, rung_of, dec.ctypes.data_as(C.POINTER(C.c_ubyte)))
    assert list(rung_of) == [0, 1, 2, 3, 0, 1]
    assert dec.tolist() == [[1, 1, 1, 1, 1, 1], [0, 1, 1, 1, 0, 1], [0, 0, 1, 1, 0, 0], [0, 0, 0, 1, 0, 0]]
    want_rung, want_log = sr.ladder(n, [0.0, 0.2, 0.4, 0.6], lambda T, rows: [tuple(script[[0.0, 0.2, 0.4, 0.6].index(T), w]) for w in rows], 2.4, -1.0, 0.6)
    assert want_rung == list(rung_of) and want_log == [np.flatnonzero(d).tolist() for d in dec]
    # thresholds off: one rung, whatever the scores
    host.whh_run_ladder(n, R, script.ctypes.data_as(C.POINTER(C.c_double)), NAN, NAN, NAN, rung_of, dec.ctypes.data_as(C.POINTER(C.c_ubyte)))
    assert list(rung_of) == [0] * n and dec[1:].sum() == 0


def test_temperature_parsing(host):
    out, err = (C.c_float * 8)(), C.create_string_buffer(256)
    assert host.whh_parse_temperatures(b"0,0.2,0.4,0.6,0.8,1.0", out, 8, err, 256) == 6
    assert [F(x) for x in out[:6]] == [F(0), F(0.2), F(0.4), F(0.6), F(0.8), F(1.0)]
    assert host.whh_parse_temperatures(b" 0.5 ", out, 8, err, 256) == 1 and out[0] == 0.5
    for bad in (b"", b"0,,1", b"-0.1", b"nan", b"inf", b"0.2x", b"0,"):
        assert host.whh_parse_temperatures(bad, out, 8, err, 256) == -1 and b"--temperature" in err.value, bad


def test_json_keys_appear_only_with_a_ladder(host):
    buf = C.create_string_buffer(4096)
    host.whh_ladder_row_json(b"a.wav", b"hello", 0.0, 0.0, 0, buf, 4096)
    plain = json.loads(buf.value)
    assert set(plain[0]) == {"file", "duration_s", "end_to_end_s", "rtf", "text"}
    host.whh_ladder_row_json(b"a.wav", b"hello", 0.2, 1.25, 1, buf, 4096)
    row = json.loads(buf.value)[0]
    assert row["temperature"] == 0.2 and row["compression_ratio"] == 1.25 and '"temperature": 0.2,' in buf.value.decode()
    host.whh_ladder_config_json(None, 0, buf, 4096)
    base = buf.value
    assert "temperature" not in json.loads(base)
    t = (C.c_float * 3)(0.0, 0.2, 1.0)
    host.whh_ladder_config_json(t, 3, buf, 4096)
    cfg = json.loads(buf.value)
    assert cfg.pop("temperature") == [0, 0.2, 1] and cfg == json.loads(base)


def plan(flags):
    return subprocess.run([CLI, "--onnx-dir", "synthetic:nano:7"] + flags + ["--print-plan"], capture_output=True, text=True, timeout=60)


def test_cli_flags():
    r = plan(["--temperature", "0,0.2,1.0", "--compression-ratio-threshold", "2.4", "--logprob-threshold=-1", "--seed", "77"])
    assert r.returncode == 0, r.stderr
    p = json.loads(r.stdout)
    assert p["temperature"] == [0, 0.2, 1] and p["compression_ratio_threshold"] == 2.4 and p["seed"] == 77 and p["pipelined"] is False
    # the default ladder is no ladder: the plan of a command line without the flag
    a, b = plan(["--temperature", "0"]), plan([])
    assert a.returncode == 0 and a.stdout == b.stdout and "temperature" not in b.stdout
    for flags, needle in [(["--temperature", "0,-1"], "--temperature"), (["--temperature", "x"], "--temperature"), (["--temperature", ""], "--temperature"),
                          (["--compression-ratio-threshold", "2.4"], "needs a --temperature ladder"),
                          (["--temperature", "0,1", "--beam-size", "2"], "--beam-size"), (["--temperature", "0.5", "--no-repeat-ngram-size", "3"], "--no-repeat-ngram-size"),
                          (["--temperature", "0,1", "--word-timestamps"], "--word-timestamps"), (["--temperature", "0,1", "--compression-ratio-threshold", "z"], "not a number")]:
        r = plan(flags)
        assert r.returncode != 0 and needle in r.stderr and "error:" in r.stderr, (flags, r.stderr)
    h = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert "--temperature" in h.stdout and "--compression-ratio-threshold" in h.stdout and "unpipelined" in h.stdout


def test_the_entry_is_exported_and_refuses_null():
    lib = wb.load_library()
    assert "wh_ctx_set_sampling" in wb.EXPORTS and hasattr(lib, "wh_ctx_set_sampling")
    assert lib.wh_ctx_set_sampling(None, None) == 4
    assert C.sizeof(wb.WhSamplingOpts) == 48
