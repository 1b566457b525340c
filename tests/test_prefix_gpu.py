"""Per-clip prompt prefixes in the GPU token loop (wh_ctx_set_prefixes).

The reference of almost every test here is the library itself on code this feature does not touch: with prefixes off, a call whose prompt
is prefix ++ prompt decodes a row exactly as the prefixed call must.  Every row of a prefixed batch is compared bit for bit with the
explicit call of its own prefix.  Shared inputs: tests/prefix_ref.py (lengths 0, 1, 63, 64, 65, 129, 140: the run passes local positions
64 and 128 of the self-attention kernel and the V prefetch groups of 32 and 64 rows)."""
import functools
import json
import os
import subprocess
import wave

import numpy as np
import pytest

import prefix_ref as pr
from test_timestamps_gpu import setup
from oracle import oracle as orc
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
SEEDS = {"nano": 7, "micro": 11, "base": 1234}
NEW = pr.NEW


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def make(preset, prec_name, nb):
    model = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, wb.PRECISIONS[prec_name])
    return model, wb.Context(model, nb)


def batch(preset, nb, which=None):
    """(clips, the seven prefixes, each row's prefix index): row i has length LENS[i % 7] unless `which` lists the indices."""
    pre = pr.prefixes(ms.PRESETS[preset].vocab)
    idx = [which[i] if which else i % 7 for i in range(nb)]
    return [ms.synth_clip(1500 + i % 16) for i in range(nb)], pre, idx


def gen(t, P):
    return [int(x) for x in t[P:]]


# (preset, precision, clips, prefix index of each row or None for i % 7, compared rows, distinct lengths among them)
EXPLICIT = [
    ("nano", "f32", 3, (0, 3, 6), (0, 1, 2), 3),          # partial row tile; lengths 0, 64, 140 (three rows: three lengths)
    ("micro", "f16x3", 16, None, tuple(range(16)), 7),
    ("base", "bf16", 64, None, tuple(range(14)) + (31, 63), 7),
    ("base", "fp8", 64, None, tuple(range(14)) + (31, 63), 7),
]


@pytest.mark.parametrize("preset,prec_name,nb,which,rows,n_len", EXPLICIT)
def test_prefixed_rows_equal_the_explicit_prompt_bit_for_bit(gpu, preset, prec_name, nb, which, rows, n_len):
    """One prefixed batch (free-running, and with a forced history F = row 0's free-running tokens) against one un-prefixed call per
    distinct prefix with prompt = prefix ++ prompt on the same resident clips: the rows that own the prefix have identical generated
    tokens and np.array_equal logits.  (The 3-clip configuration has three rows, so three lengths; the others compare all seven.)"""
    prompt, eot, tb, nots = setup(preset)
    P = len(prompt)
    model, ctx = make(preset, prec_name, nb)
    clips, pre, idx = batch(preset, nb, which)
    ctx.set_prefixes([pre[k] for k in idx])
    free = ctx.transcribe_batch(clips, wb.DecodeParams(prompt, NEW, eot, [eot]))
    assert all(len(t) == P + NEW and t[:P].tolist() == prompt for t in free)      # the prefix is not echoed
    F = gen(free[0], P)
    forced_t, forced_l = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, NEW, eot, [eot], forced=F), list(rows))
    ctx.clear_prefixes()
    lens = set()
    for k in sorted(set(idx)):
        own = [r for r in rows if idx[r] == k]
        if not own:
            continue
        lens.add(len(pre[k]))
        full = pre[k] + prompt
        ex_t, ex_l = ctx.greedy_decode_resident_rows(wb.DecodeParams(full, NEW, eot, [eot], forced=F), own)
        ex_free, _ = ctx.greedy_decode_resident_batch(wb.DecodeParams(full, NEW, eot, [eot]))
        for j, r in enumerate(own):
            assert gen(ex_t[r], len(full)) == gen(forced_t[r], P), (k, r)
            assert ex_l[j].shape == (NEW, model.dims.vocab)
            assert np.array_equal(ex_l[j], forced_l[rows.index(r)]), (k, r, float(np.abs(ex_l[j] - forced_l[rows.index(r)]).max()))
            assert gen(ex_free[r], len(full)) == gen(free[r], P), (k, r)
    assert len(lens) == n_len and (n_len >= 5 or nb < 5)
    ctx.close()


@functools.lru_cache(maxsize=None)
def oracle_runs(preset):
    """The f32 oracle on clip 1500: its own un-prefixed 8 greedy tokens F, then the logits of prefix ++ prompt under F for every length."""
    prompt, eot, tb, nots = setup(preset)
    dims = ms.PRESETS[preset]
    w = ms.flatten_state_dict(dims, ms.synth_state_dict(dims, SEEDS[preset]))
    enc = orc.encoder(dims, w, orc.window_mel(orc.log_mel(ms.synth_clip(1500), dims.n_mels), 0, 3000))
    toks, _ = orc.decode_greedy(dims, w, enc, prompt, NEW, eot, [eot])
    F = gen(toks, len(prompt))
    out = []
    for p in pr.prefixes(dims.vocab):
        _, lg = orc.decode_greedy(dims, w, enc, p + prompt, NEW, eot, [eot], forced=F, want_logits=True)
        out.append(np.asarray(lg, np.float32)[:NEW].copy())
    return F, out


@pytest.mark.parametrize("preset,prec_name", [("nano", "f32"), ("micro", "f16x3")])
def test_prefixed_rows_agree_with_the_f32_oracle(gpu, preset, prec_name):
    """Seven copies of clip 1500, one per length, under the oracle's own un-prefixed history F: logits within the project's 1e-3 of
    orc.decode_greedy(prefix ++ prompt, forced=F), tokens equal wherever the oracle's top-1 margin exceeds 2e-3; at most one step in
    eight may fall under that margin (the oracle has none with these inputs: smallest margin 1.2e-2 nano, 3.9e-3 micro).  A prefix moves
    the logits by 2.5 - 4.4, so a build that ignores the prefix or mis-places positions cannot pass."""
    prompt, eot, tb, nots = setup(preset)
    P = len(prompt)
    F, ref = oracle_runs(preset)
    model, ctx = make(preset, prec_name, 7)
    pre = pr.prefixes(model.dims.vocab)
    ctx.set_prefixes(pre)
    ctx.transcribe_batch([ms.synth_clip(1500)] * 7, wb.DecodeParams(prompt, NEW, eot, [eot]))
    toks, lg = ctx.greedy_decode_resident_rows(wb.DecodeParams(prompt, NEW, eot, [eot], forced=F), list(range(7)))
    for k in range(7):
        err = float(np.abs(lg[k] - ref[k]).max())
        moved = float(np.abs(ref[k] - ref[0]).max())
        x = ref[k].astype(np.float64).copy()
        x[:, eot] = -np.inf
        s = np.sort(x, axis=1)
        margin = s[:, -1] - s[:, -2]
        print(f"{preset} {prec_name} length {len(pre[k])}: max |gpu - oracle| {err:.3g}, prefix moves the logits by {moved:.3g}, "
              f"smallest top-1 margin {margin.min():.3g}")
        assert err < 1e-3, (k, err)
        assert k == 0 or moved > 1.0
        assert (margin <= 2e-3).sum() <= NEW // 8
        got = gen(toks[k], P)
        for i in range(NEW):
            if margin[i] > 2e-3:
                assert got[i] == int(np.argmax(x[i])), (k, i)
    ctx.close()


@pytest.mark.parametrize("preset,prec_name,nb,which", [("base", "bf16", 64, None), ("nano", "f32", 3, (0, 3, 6))])
def test_nothing_else_moves(gpu, preset, prec_name, nb, which):
    prompt, eot, tb, nots = setup(preset)
    model, ctx = make(preset, prec_name, nb)
    clips, pre, idx = batch(preset, nb, which)
    rows = sorted({0, 1, nb // 2, nb - 1})
    p = wb.DecodeParams(prompt, NEW, eot, [eot])

    def run():
        t = ctx.transcribe_batch(clips, p)
        t2, lg = ctx.greedy_decode_resident_rows(p, rows)
        assert [a.tolist() for a in t] == [a.tolist() for a in t2]
        return [a.tolist() for a in t], lg

    def same(a, b):
        return a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))

    before = run()                                     # before any setter
    ctx.set_prefixes([[] for _ in range(nb)])          # set, but all empty
    assert same(run(), before)
    ctx.set_prefixes([pre[k] for k in idx])
    on = run()
    assert not same(on, before)
    ctx.clear_prefixes()
    assert same(run(), before)
    ctx.set_prefixes([pre[k] for k in idx])
    assert same(run(), on)
    ctx.clear_prefixes()
    assert same(run(), before)
    ctx.close()


def test_with_rules_logprobs_and_the_probe(gpu):
    """Timestamp rules + token log-probabilities + the no-speech probe at sot_index 0 with prefixes on: tokens, token_logprobs and
    no_speech_prob equal, bit for bit per row, the explicit-prompt calls with the same settings (where the probe's sot_index is n_b)."""
    prompt, eot, tb, nots = setup("base")
    P, nb = len(prompt), 64
    ns = nots - 1
    model, ctx = make("base", "bf16", nb)
    clips, pre, idx = batch("base", nb)
    assert all(t != nots for p in pre for t in p)     # (the explicit calls below carry the prefix in their prompt, where the rules check it)
    ctx.set_timestamp_rules(tb, nots, 50)
    ctx.set_logprobs(ns, 0)
    ctx.set_prefixes([pre[k] for k in idx])
    p = wb.DecodeParams(prompt, NEW, eot, [])
    toks = ctx.transcribe_batch(clips, p)
    lps, nsp = ctx.logprobs()
    assert all(int(t[P]) >= tb for t in toks) and len(lps) == nb and nsp is not None
    ctx.clear_prefixes()
    for k in range(7):
        full = pre[k] + prompt
        ctx.set_logprobs(ns, len(pre[k]))
        ex, _ = ctx.greedy_decode_resident_batch(wb.DecodeParams(full, NEW, eot, []))
        ex_lp, ex_ns = ctx.logprobs()
        for r in range(k, nb, 7):
            assert gen(ex[r], len(full)) == gen(toks[r], P), (k, r)
            assert np.array_equal(ex_lp[r], lps[r]) and len(lps[r]) == len(toks[r]) - P, (k, r)
            assert ex_ns[r] == nsp[r], (k, r)
    assert len({float(x) for x in nsp[:7]}) > 1       # the probe reads the prefixed row
    ctx.close()


@pytest.mark.parametrize("max_batch", [2, 4])
def test_longform_scopes(gpu, max_batch):
    prompt, eot, tb, nots = setup("nano")
    P = len(prompt)
    model, ctx = make("nano", "f32", max_batch)
    pre = pr.prefixes(model.dims.vocab)[5]              # 129 ids
    pcm = np.concatenate([ms.synth_clip(40), ms.synth_clip(41), ms.synth_clip(42)[:200000]])   # 72.5 s: three windows
    params = wb.DecodeParams(prompt, NEW, eot, [eot])
    full = wb.DecodeParams(pre + prompt, NEW, eot, [eot])
    offs = wb.longform_plan(pcm.size)
    assert len(offs) == 3
    plain = ctx.transcribe_longform(pcm, params)
    ctx.set_prefixes([pre])
    first = ctx.transcribe_longform(pcm, params)
    ctx.set_prefixes([pre], all_windows=True)
    every = ctx.transcribe_longform(pcm, params)
    ctx.clear_prefixes()
    mel_full = ctx.whisper_log_mel(pcm)
    for w, off in enumerate(offs):
        ctx.run_encoder(orc.window_mel(mel_full, off // 160, 3000), want_output=False)
        alone, _ = ctx.greedy_decode_with_past(params)
        explicit, _ = ctx.greedy_decode_with_past(full)
        assert plain[w].tolist() == alone.tolist()
        assert gen(explicit, len(pre) + P) != gen(alone, P)
        assert first[w].tolist() == (prompt + gen(explicit, len(pre) + P) if w == 0 else alone.tolist()), w
        assert every[w].tolist() == prompt + gen(explicit, len(pre) + P), w
    ctx.set_prefixes([pre, pre])                        # long-form takes one prefix
    with pytest.raises(wb.WhisperHipError) as ei:
        ctx.transcribe_longform(pcm, params)
    assert ei.value.code == 4
    ctx.close()


def test_refusals_leave_the_context_usable(gpu):
    prompt, eot, tb, nots = setup("nano")
    P = len(prompt)
    model, ctx = make("nano", "f32", 2)
    vocab, tctx = model.dims.vocab, model.dims.n_text_ctx
    clips = [ms.synth_clip(0), ms.synth_clip(1)]
    p = wb.DecodeParams(prompt, NEW, eot, [eot])
    pre = pr.prefixes(vocab)
    plain = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    ctx.set_prefixes([pre[1], pre[4]])
    good = [t.tolist() for t in ctx.transcribe_batch(clips, p)]
    assert good != plain

    def setter(ids, offsets, n_clips, scope=0, size=None):
        a = np.ascontiguousarray(ids, np.int64)
        o = np.ascontiguousarray(offsets, np.uint64)
        opts = wb.WhPrefixOpts(wb.C.sizeof(wb.WhPrefixOpts) if size is None else size, a.ctypes.data_as(wb.C.POINTER(wb.C.c_int64)),
                               o.ctypes.data_as(wb.C.POINTER(wb.C.c_size_t)), n_clips, scope)
        return ctx.lib.wh_ctx_set_prefixes(ctx.h, wb.C.byref(opts))

    for bad in (dict(size=wb.C.sizeof(wb.WhPrefixOpts) - 8), dict(n_clips=0), dict(n_clips=3, offsets=[0, 1, 2, 2]), dict(offsets=[1, 1, 2]),
                dict(offsets=[0, 2, 1]), dict(ids=[11, vocab]), dict(ids=[-1, 12]), dict(scope=2)):
        args = dict(ids=[11, 12], offsets=[0, 1, 2], n_clips=2)
        args.update(bad)
        assert setter(**args) == 4, bad
        assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == good, bad      # the setting in force is unchanged
    with pytest.raises(wb.WhisperHipError) as ei:                                       # two prefixes, one clip
        ctx.transcribe_batch(clips[:1], p)
    assert ei.value.code == 4
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == good
    # Nmax + P + NEW = n_text_ctx runs, n_text_ctx + 1 is refused
    room = tctx - P - NEW
    rng = np.random.default_rng(9)
    longest = [int(t) for t in rng.integers(10, vocab - 400, room + 1)]
    ctx.set_prefixes([longest[:room], []])
    fits = ctx.transcribe_batch(clips, p)
    assert all(len(t) == P + NEW for t in fits) and fits[1].tolist() == plain[1]
    ctx.clear_prefixes()
    ex, _ = ctx.greedy_decode_resident_batch(wb.DecodeParams(longest[:room] + prompt, NEW, eot, [eot]))
    assert gen(ex[0], room + P) == gen(fits[0], P)
    ctx.set_prefixes([longest, []])
    with pytest.raises(wb.WhisperHipError) as ei:
        ctx.transcribe_batch(clips, p)
    assert ei.value.code == 4 and str(tctx) in str(ei.value)
    # language detection: refused with a non-empty prefix (code 8, with advice), runs with all-empty ones
    ctx.set_prefixes([pre[1], []])
    ctx.set_language_detection([20, 21, 22], 0)
    with pytest.raises(wb.WhisperHipError) as ei:
        ctx.transcribe_batch(clips, p)
    assert ei.value.code == 8 and "un-prefixed" in str(ei.value)
    ctx.set_prefixes([[], []])
    det = ctx.transcribe_batch(clips, p)
    ids, probs = ctx.languages()
    assert all(int(t[1]) == int(i) for t, i in zip(det, ids)) and set(ids.tolist()) <= {20, 21, 22}
    ctx.clear_language_detection()
    ctx.clear_prefixes()
    assert [t.tolist() for t in ctx.transcribe_batch(clips, p)] == plain
    ctx.close()


def _write_wav(path, pcm):
    x = np.clip(np.round(pcm * 32767.0), -32768, 32767).astype(np.int16)
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000); w.writeframes(x.tobytes())
    return x.astype(np.float32) / np.float32(32768)


def _model_dir(mdir, dims, seed, special):
    """config.json + model.safetensors + generation_config.json + a tokenizer.json in which ordinary id i detokenises to " t<i>", so the CLI's
    text spells out the ids the GPU produced."""
    sd = ms.synth_state_dict(dims, seed)
    hdr, blobs, off = {}, [], 0
    for name, arr in sd.items():
        b = arr.astype("<f4").tobytes()
        hdr[name] = {"dtype": "F32", "shape": list(arr.shape), "data_offsets": [off, off + len(b)]}
        blobs.append(b)
        off += len(b)
    hj = json.dumps(hdr).encode()
    (mdir / "model.safetensors").write_bytes(len(hj).to_bytes(8, "little") + hj + b"".join(blobs))
    (mdir / "config.json").write_text(json.dumps({
        "num_mel_bins": 80, "d_model": dims.d_model, "encoder_attention_heads": dims.n_heads, "decoder_attention_heads": dims.n_heads,
        "encoder_layers": dims.enc_layers, "decoder_layers": dims.dec_layers, "encoder_ffn_dim": dims.ffn, "decoder_ffn_dim": dims.ffn,
        "vocab_size": dims.vocab, "max_source_positions": 1500, "max_target_positions": 448}))
    (mdir / "generation_config.json").write_text(json.dumps({"suppress_tokens": [], "begin_suppress_tokens": []}))
    vocab = {f"Ġt{i}": i for i in range(dims.vocab) if i not in special.values()}
    (mdir / "tokenizer.json").write_text(json.dumps({"model": {"vocab": vocab}, "added_tokens": [
        {"id": i, "content": name, "special": True} for name, i in special.items()]}))


def test_cli_prompt_flags(gpu, tmp_path):
    """Four one-window files, three with ids files (1, 64 and 140 ids; the CLI puts <|startofprev|> in front) and one without: every file's
    text spells the tokens of the binding's explicit-prompt call; without the flags the output is what it was."""
    dims = ms.PRESETS["nano"]
    special = {"<|endoftext|>": 2, "<|startoftranscript|>": 3, "<|en|>": 5, "<|transcribe|>": 7, "<|notimestamps|>": 9, "<|startofprev|>": 4}
    adir, mdir, pdir = tmp_path / "audio", tmp_path / "model", tmp_path / "prompts"
    for d in (adir, mdir, pdir):
        d.mkdir()
    _model_dir(mdir, dims, 7, special)
    names = ["a.wav", "b.wav", "c.wav", "d.wav"]
    pcm = [_write_wav(str(adir / n), ms.synth_clip(80 + i)[: 200000 + 40000 * i]) for i, n in enumerate(names)]
    rng = np.random.default_rng(6)
    hist = {"a": [int(t) for t in rng.integers(10, 600, 1)], "b": [int(t) for t in rng.integers(10, 600, 64)],
            "c": [int(t) for t in rng.integers(10, 600, 140)]}
    (pdir / "a.txt").write_text(",".join(map(str, hist["a"])))
    (pdir / "b.txt").write_text(" ".join(map(str, hist["b"])) + "\n")
    (pdir / "c.txt").write_text(",\n".join(map(str, hist["c"])))
    prompt, eot = [3, 5, 7, 9], 2

    def run(out, *extra):
        r = subprocess.run([CLI, "--audio-dir", str(adir), "--onnx-dir", str(mdir), "--max-new-tokens", "6", "--precision", "f32", "--max-batch", "4",
                            "--out-csv", str(out / "p.csv"), "--out-json", str(out / "p.json"), "--out-summary-json", str(out / "s.json"), *extra],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        return json.loads((out / "p.json").read_text()), (out / "p.csv").read_text()

    rows, _ = run(tmp_path / "with", "--prompt-ids-dir", str(pdir))
    base_rows, base_csv = run(tmp_path / "without")
    model = wb.Model(str(mdir), 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 1)

    def text_of(prefix, x):
        full = prefix + prompt
        g = gen(ctx.transcribe_batch([x], wb.DecodeParams(full, 6, eot))[0], len(full))
        if g and g[-1] == eot:
            g.pop()
        return "".join(f" t{t}" for t in g).strip()

    assert [r["file"] for r in rows] == names
    differ = 0
    for row, base, n, x in zip(rows, base_rows, names, pcm):
        h = hist.get(n[0], [])
        prefix = pr.build_prev_prefix(h, 4, dims.n_text_ctx)
        assert row["prompt_tokens"] == len(prefix) == (len(h) + 1 if h else 0)
        assert row["text"] == text_of(prefix, x), n
        assert "prompt_tokens" not in base and base["text"] == text_of([], x), n
        differ += row["text"] != base["text"]
    assert differ >= 2 and rows[3]["text"] == base_rows[3]["text"]
    # the same ids for every file; a file of the directory still wins
    rows2, _ = run(tmp_path / "both", "--prompt-ids", ",".join(map(str, hist["b"])), "--prompt-ids-dir", str(pdir))
    assert [r["prompt_tokens"] for r in rows2] == [2, 65, 141, 65] and rows2[3]["text"] == text_of([4] + hist["b"], pcm[3])
    assert [r["text"] for r in rows2[:3]] == [r["text"] for r in rows[:3]]
    ctx.close()
    r = subprocess.run([CLI, "--audio-dir", str(adir), "--onnx-dir", str(mdir), "--language", "auto", "--prompt-ids", "11"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--language auto" in r.stderr and "--prompt-ids" in r.stderr
