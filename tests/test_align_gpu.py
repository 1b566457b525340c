"""Word-level timestamps on the GPU (wh_ctx_set_alignment), held to the numpy restatement in tests/align_ref.py.  Run with -m gpu.

Every case checks the same ladder on its debug rows:
  (a) exact: align_ref.dtw(-matrix) on the RETURNED matrix equals token_frames() of that row, element for element (the DTW is a chain of single
      f32 additions and comparisons: no tolerance);
  (b) the returned matrix against the pipeline (column statistics, median of 7, head mean) run on the RETURNED probs: with
      e = max |pipeline_f32(probs) - pipeline_f64(probs)| — reference against reference, the size of f32 reordering on these very inputs —
      max |matrix - pipeline_f64(probs)| <= 8 e (another summation tree over at most 448 rows and the head mean; the median passes errors
      through one to one);
  (c) the returned probs against the numpy decoder, teacher-forced on the tokens the GPU fed, on float64 encoder states.  f32 mode: the bound
      is 16 x max |P_numpy32 - P_numpy64| on the same inputs, encoder states from the CPU oracle.  bf16: BF16_PROBS_TOL (see there), against the
      numpy decoder on the encoder states of wh_encode on the same model and precision (DESIGN.md §5l has the measurements)."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import align_ref as ar
from oracle import oracle as orc
from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
SEEDS = {"nano": 7, "micro": 11, "base": 1234}
NANO_HEADS = [(1, 0), (1, 1), (0, 1)]
BASE_HEADS = [(5, 0), (5, 7), (3, 2), (2, 4)]
# bf16, ladder (c).  Measured on an MI355X on cases 3 and 4 below (encoder states from wh_encode, so only the decoder differs): see the figures
# in DESIGN.md section 5l.  4 x the largest of them exceeds 0.05, the ceiling the feature's specification puts on this constant, so the cause
# was looked for: the synthetic whisper-base weights (q / k projections x 2.5) give near one-hot cross-attention (largest probability 0.73 on
# these heads), and bf16 arithmetic in the decoder upstream of the scores moves a score by up to 0.27 — a numpy decoder with bf16-rounded
# weights and matmul operands (align_ref.decoder(rnd=bf16_round), no GPU code involved; tests/test_align_cpu.py reproduces it) differs from the
# float64 one by 0.034 on the same probabilities.  The score kernels
# themselves are exact to f32 rounding (cases 1, 2, 5) and a clip alone agrees with its batch row bit for bit.  The constant is therefore the
# ceiling itself, not 4 x the measurement: a margin of about 2 over the figures measured.
BF16_PROBS_TOL = 0.05


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


_sd = {}


def state_dict(preset):
    if preset not in _sd:
        dims = ms.PRESETS[preset]
        sd = ms.synth_state_dict(dims, SEEDS[preset])
        _sd[preset] = (dims, sd, ms.flatten_state_dict(dims, sd))
    return _sd[preset]


def oracle_states(preset, pcm):
    dims, _, w = state_dict(preset)
    return orc.encoder(dims, w, orc.window_mel(orc.log_mel(pcm, dims.n_mels), 0, 3000)).astype(np.float64)


def ladder(dbg, preset, heads, k, frames, sb, prompt, fed, enc64, bf16, prefix=(), label=""):
    """(a)-(c) on debug row k, dbg = its (probs, matrix) or the context to ask; fed = the tokens the row fed at its generated positions (its
    own, or the forced ones).  Returns the figures."""
    dims, sd, _ = state_dict(preset)
    probs, matrix = dbg if isinstance(dbg, tuple) else dbg.alignment_debug(k)
    n = len(frames)
    assert probs.shape == (len(heads), n, sb) and matrix.shape == (n, sb), (probs.shape, matrix.shape, n, sb)
    ref_frames, _ = ar.dtw(-matrix)
    assert np.array_equal(ref_frames, frames), (label, ref_frames, frames)                      # (a)
    assert frames[0] == 0 and (np.diff(frames) >= 0).all() and frames.max() < sb, (label, frames)
    if n == 1:
        return 0.0, 0.0, 0.0, 0.0
    assert abs(probs.sum(axis=-1) - 1).max() < 1e-5
    m64 = ar.pipeline(probs, np.float64)
    e = float(np.abs(ar.pipeline(probs, np.float32) - m64).max())
    dm = float(np.abs(matrix - m64).max())
    seq = list(prefix) + list(prompt) + [int(t) for t in fed[: n - 1]]
    first = len(prefix) + len(prompt) - 1
    _, sc64 = ar.decoder(dims, sd, enc64, seq, np.float64)
    p64 = ar.probs(sc64, heads, first, n, sb)
    if bf16:
        bound = BF16_PROBS_TOL
    else:
        _, sc32 = ar.decoder(dims, sd, enc64, seq, np.float32)
        bound = 16 * float(np.abs(ar.probs(sc32, heads, first, n, sb) - p64).max())
    dp = float(np.abs(probs - p64).max())
    print(f"{label} row {k}: n_gen {n}, S_b {sb}, distinct frames {len(set(frames.tolist()))}; (b) |matrix - pipe64| {dm:.3g} vs 8e = {8 * e:.3g}; "
          f"(c) |probs - numpy64| {dp:.3g} vs bound {bound:.3g}")
    assert dm <= 8 * e, (label, k, dm, e)                                                        # (b)
    if not bf16:   # (bf16: the caller asserts on the largest figure of the case, after every row has printed its own)
        assert dp <= bound, (label, k, dp, bound)                                                # (c)
    return dm, e, dp, bound


def test_score_kernels_against_host_restatement(gpu):
    """tools/align_check: the three score kernels on random operands against a double-precision restatement with the very operands they read,
    within 5e-5 on the probabilities (derived there) — tight enough to see a split query that lost its lo limb, which the model-level bf16
    bound below cannot."""
    exe = os.path.join(ROOT, "tools", "align_check")
    assert os.path.exists(exe), f"{exe} missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and r.stdout.count(" ok") == 3, r.stdout + r.stderr


NANO_SAMPLES = (480000, 128000, 2400)


@pytest.fixture(scope="module")
def nano(gpu):
    """Case 1's context, clips and oracle encoder states, shared by the cases that run on it."""
    prompt, eot, tb, nots = setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 3)
    clips = [ms.synth_clip(1500 + i)[:n] for i, n in enumerate(NANO_SAMPLES)]
    enc = [oracle_states("nano", c) for c in clips]
    yield ctx, clips, enc, prompt, eot, tb, nots
    ctx.close()


def test_f32_three_frame_counts_two_layers(nano):
    """Case 1: the float kernel, S_b = 1500 / 400 / 8 in one batch, heads of two layers, every row a debug row."""
    ctx, clips, enc, prompt, eot, tb, nots = nano
    ctx.set_alignment(NANO_HEADS, debug_rows=[0, 1, 2])
    p = wb.DecodeParams(prompt, 24, eot, [eot])
    toks = ctx.transcribe_batch(clips, p)
    frames, nf = ctx.token_frames()
    assert nf.tolist() == [1500, 400, 8] == [ar.frames_of(n) for n in NANO_SAMPLES]
    for b in range(3):
        gen = toks[b][len(prompt):]
        assert len(gen) == 24 and len(frames[b]) == 24
        ladder(ctx, "nano", NANO_HEADS, b, frames[b], int(nf[b]), prompt, gen, enc[b], False, label="case 1")
    ctx.clear_alignment()


def test_f32_full_text_context(nano):
    """Case 2: max_new_tokens = 445 on one clip — the full text context, the LDS diagonals of the DTW at their largest."""
    ctx, clips, enc, prompt, eot, tb, nots = nano
    ctx.set_alignment(NANO_HEADS, debug_rows=[0])
    p = wb.DecodeParams(prompt, 445, eot, [eot])
    toks = ctx.transcribe_batch(clips[:1], p)
    frames, nf = ctx.token_frames()
    assert len(frames) == 1 and len(frames[0]) == 445 and nf[0] == 1500
    ladder(ctx, "nano", NANO_HEADS, 0, frames[0], 1500, prompt, toks[0][len(prompt):], enc[0], False, label="case 2")
    ctx.clear_alignment()


def gpu_states(ctx, clip):
    """Encoder states of one clip from wh_encode on this context (so that only the decoder differs from the numpy restatement)."""
    return ctx.run_encoder(ctx.whisper_log_mel(clip), want_output=True).astype(np.float64)


@pytest.mark.parametrize("cross_es,nb", [(False, 2), (True, 3)])
def test_bf16_base(gpu, cross_es, nb):
    """Cases 3 and 4: whisper-base in bf16 on the projected K / V (the bf16 K/V kernel) and on the encoder states (dk = 512, the es_rows
    pitch); in the encoder-state form each clip decoded alone agrees with its batch row within the bf16 constant."""
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, nb, cross_es=cross_es)
    assert ctx.cross_mode == (1 if cross_es else 0)
    clips = [ms.synth_clip(1500 + i) for i in range(nb)]
    ctx.set_alignment(BASE_HEADS, debug_rows=list(range(nb)))
    p = wb.DecodeParams(prompt, 12, eot, [eot])
    toks = ctx.transcribe_batch(clips, p)
    frames, nf = ctx.token_frames()
    dbg = [ctx.alignment_debug(b) for b in range(nb)]
    worst = 0.0
    for b in range(nb):
        gen = toks[b][len(prompt):]
        states = gpu_states(ctx, clips[b])   # (the context now holds this one clip's encoder states)
        if cross_es:   # the clip alone (wh_encode + wh_decode_greedy, fed the batch row's tokens) against its batch row
            ctx.set_alignment(BASE_HEADS, debug_rows=[0])
            ctx.greedy_decode_with_past(wb.DecodeParams(prompt, 12, eot, [eot], forced=[int(t) for t in gen]))
            alone = ctx.alignment_debug(0)[0]
            d = float(np.abs(alone - dbg[b][0]).max())
            print(f"case 4 clip {b}: alone against its batch row, max |d probs| {d:.3g}")
            assert d <= BF16_PROBS_TOL
        _, _, dp, _ = ladder(dbg[b], "base", BASE_HEADS, b, frames[b], int(nf[b]), prompt, gen, states, True, label=f"case {4 if cross_es else 3}")
        worst = max(worst, dp)
    print(f"bf16 {'encoder-state' if cross_es else 'K/V'} form: largest |probs - numpy64| {worst:.3g}")
    assert worst <= BF16_PROBS_TOL, worst                                                        # (c)
    ctx.close()


def test_composition_prefixes_rules_logprobs_forced(nano):
    """Case 5: per-clip prefixes of 0, 2 and 5 ids (the rows wait for each other), timestamp rules and log-probabilities on, a forced
    history; then a call with max_new_tokens = 1."""
    ctx, clips, enc, prompt, eot, tb, nots = nano
    prefixes = [[], [20, 21], [30, 31, 32, 33, 34]]
    ctx.set_prefixes(prefixes)
    ctx.set_timestamp_rules(tb, nots, 50)
    ctx.set_logprobs()
    ctx.set_alignment(NANO_HEADS, debug_rows=[0, 1, 2])
    forced = [10 + (i * 5) % 23 for i in range(24)]
    try:
        p = wb.DecodeParams(prompt, 24, eot, [eot], forced=forced)
        toks = ctx.transcribe_batch(clips, p)
        frames, nf = ctx.token_frames()
        for b in range(3):
            assert len(frames[b]) == len(toks[b]) - len(prompt) == 24
            ladder(ctx, "nano", NANO_HEADS, b, frames[b], int(nf[b]), prompt, forced, enc[b], False, prefix=prefixes[b], label="case 5 forced")
        p = wb.DecodeParams(prompt, 24, eot, [eot])
        toks = ctx.transcribe_batch(clips, p)
        frames, nf = ctx.token_frames()
        for b in range(3):
            gen = toks[b][len(prompt):]
            assert len(frames[b]) == len(gen)
            ladder(ctx, "nano", NANO_HEADS, b, frames[b], int(nf[b]), prompt, gen, enc[b], False, prefix=prefixes[b], label="case 5 free")
        p1 = wb.DecodeParams(prompt, 1, eot, [eot])
        toks = ctx.transcribe_batch(clips, p1)
        frames, nf = ctx.token_frames()
        for b in range(3):
            assert len(toks[b]) == len(prompt) + 1 and frames[b].tolist() == [0] and nf[b] == ar.frames_of(NANO_SAMPLES[b])
            probs, matrix = ctx.alignment_debug(b)
            assert probs.shape == (3, 1, int(nf[b])) and matrix.shape == (1, int(nf[b]))
    finally:
        ctx.clear_prefixes()
        ctx.clear_timestamp_rules()
        ctx.clear_logprobs()
        ctx.clear_alignment()


def test_off_is_off(nano):
    """Case 6: tokens, logits and log-probabilities are bit-identical with the option set and cleared; the getter refuses after a call
    without it; a second call with it set replays the captured step."""
    ctx, clips, enc, prompt, eot, tb, nots = nano
    ctx.set_logprobs()
    p = wb.DecodeParams(prompt, 24, eot, [eot])
    try:
        ctx.transcribe_batch(clips, p)
        t0, l0 = ctx.greedy_decode_resident_batch(p, want_logits=True)
        lp0 = ctx.logprobs()[0]
        n = C.c_size_t(0)
        assert ctx.lib.wh_get_token_frames(ctx.h, None, 0, None, 0, C.byref(n)) == 3   # WH_ERR_STATE
        ctx.set_alignment(NANO_HEADS, debug_rows=[0, 1, 2])
        f = []
        for _ in range(2):
            t1, l1 = ctx.greedy_decode_resident_batch(p, want_logits=True)
            lp1 = ctx.logprobs()[0]
            f.append(ctx.token_frames()[0])
            for b in range(3):
                assert np.array_equal(t0[b], t1[b]) and np.array_equal(l0[b], l1[b]) and np.array_equal(lp0[b], lp1[b])
        assert all(np.array_equal(a, b) for a, b in zip(f[0], f[1]))
        ctx.clear_alignment()
        t2, l2 = ctx.greedy_decode_resident_batch(p, want_logits=True)
        for b in range(3):
            assert np.array_equal(t0[b], t2[b]) and np.array_equal(l0[b], l2[b])
        assert ctx.lib.wh_get_token_frames(ctx.h, None, 0, None, 0, C.byref(n)) == 3
    finally:
        ctx.clear_logprobs()
        ctx.clear_alignment()


def test_refusals(nano):
    """Case 7: every WH_ERR_ARG case of the setter (the context unchanged), the debug row outside the batch, and WH_ERR_UNSUPPORTED for the
    fp8 and the f16x3 mode at decode time with the context usable afterwards."""
    ctx, clips, enc, prompt, eot, tb, nots = nano
    i32p = C.POINTER(C.c_int32)

    def raw(heads, n_heads=None, debug=(), n_debug=None, size=None):
        h = np.ascontiguousarray(heads, np.int32).reshape(-1)
        d = np.ascontiguousarray(list(debug), np.int32)
        o = wb.WhAlignmentOpts(C.sizeof(wb.WhAlignmentOpts) if size is None else size, h.ctypes.data_as(i32p), len(h) // 2 if n_heads is None else n_heads,
                               d.ctypes.data_as(i32p) if d.size else None, d.size if n_debug is None else n_debug)
        return ctx.lib.wh_ctx_set_alignment(ctx.h, C.byref(o))

    ctx.set_alignment(NANO_HEADS)
    p = wb.DecodeParams(prompt, 6, eot, [eot])
    ctx.transcribe_batch(clips, p)
    before = ctx.token_frames()[0]
    ARG = 4
    assert raw(NANO_HEADS, size=C.sizeof(wb.WhAlignmentOpts) + 8) == ARG
    assert raw(NANO_HEADS, n_heads=0) == ARG
    assert raw([(0, 0)] * 33) == ARG
    assert raw([(2, 0)]) == ARG and raw([(-1, 0)]) == ARG          # layer outside the model (nano: 2 layers)
    assert raw([(0, 2)]) == ARG and raw([(0, -1)]) == ARG          # head outside the model (nano: 2 heads)
    assert raw([(1, 0), (0, 1), (1, 0)]) == ARG                    # a pair listed twice
    assert raw(NANO_HEADS, debug=list(range(9))) == ARG
    assert raw(NANO_HEADS, debug=[-1]) == ARG
    ctx.transcribe_batch(clips, p)                                 # the list in force is still the first one
    assert all(np.array_equal(a, b) for a, b in zip(before, ctx.token_frames()[0]))
    ctx.set_alignment(NANO_HEADS, debug_rows=[3])                  # a debug row outside a batch of 3
    with pytest.raises(wb.WhisperHipError) as ei:
        ctx.transcribe_batch(clips, p)
    assert ei.value.code == ARG
    ctx.clear_alignment()
    ctx.transcribe_batch(clips, p)
    for preset, prec in (("micro", wb.WH_PREC_FP8), ("micro", wb.WH_PREC_F16X3)):
        pr, e2, _, _ = setup(preset)
        m = wb.Model(f"synthetic:{preset}:{SEEDS[preset]}", 0, prec)
        c2 = wb.Context(m, 1)
        pp = wb.DecodeParams(pr, 4, e2, [e2])
        ref = c2.transcribe_batch(clips[:1], pp)
        c2.set_alignment([(1, 0)])
        with pytest.raises(wb.WhisperHipError) as ei:
            c2.transcribe_batch(clips[:1], pp)
        assert ei.value.code == 8   # WH_ERR_UNSUPPORTED
        c2.clear_alignment()
        assert np.array_equal(c2.transcribe_batch(clips[:1], pp)[0], ref[0])
        c2.close()


def test_longform_windows(nano):
    """Case 8: a 70 s file — frames for every window, each window's frame count from its valid length."""
    ctx, clips, enc, prompt, eot, tb, nots = nano
    pcm = np.concatenate([ms.synth_clip(1600), ms.synth_clip(1601), ms.synth_clip(1602)[:160000]])
    assert pcm.size == 70 * 16000
    ctx.set_alignment(NANO_HEADS)
    try:
        p = wb.DecodeParams(prompt, 8, eot, [eot])
        toks = ctx.transcribe_longform(pcm, p, 30.0, 5.0)
        offs = wb.longform_plan(pcm.size, 30.0, 5.0)
        frames, nf = ctx.token_frames()
        assert len(toks) == len(offs) == len(frames) == 3
        n_mel = 1 + pcm.size // 160 - 1
        for w, off in enumerate(offs):
            valid = min(3000, n_mel - off // 160)
            assert nf[w] == min(1500, max(8, (valid + 1) // 2)), (w, nf[w], valid)
            assert len(frames[w]) == len(toks[w]) - len(prompt)
            assert frames[w][0] == 0 and (np.diff(frames[w]) >= 0).all() and frames[w].max() < nf[w]
        assert nf[2] < 1500
    finally:
        ctx.clear_alignment()


def test_cli_word_timestamps(gpu, tmp_path):
    """Case 9: whisper_bench --word-timestamps on four synthetic clips."""
    out = tmp_path / "rows.json"
    cmd = [CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "4", "--max-batch", "4", "--word-timestamps", "--max-new-tokens", "16",
           "--out-json", str(out), "--out-csv", str(tmp_path / "rows.csv"), "--out-summary-json", str(tmp_path / "summary.json")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = json.loads(out.read_text())
    assert len(rows) == 4
    for row in rows:
        assert "words" in row and "token_times" in row
        words = row["words"]
        if row["text"] == "[EMPTY]":   # (a window that ended at once: no text, no words)
            assert words == []
            continue
        assert words and "".join(w["word"] for w in words) == row["text"]
        starts = [w["start"] for w in words]
        assert all(w["start"] <= w["end"] for w in words)
        assert all(a <= b for a, b in zip(starts, starts[1:]))
        assert all(0 <= w["start"] <= row["duration_s"] and w["end"] <= row["duration_s"] for w in words)
