"""Forced alignment on the GPU (wh_align_tokens): the frame of every token of a given transcript from one decoder pass over all
its positions, held to the numpy restatement (tests/align_ref.py wired by tests/forced_align_ref.py).  Run with -m gpu.

The ladder is that of tests/test_align_gpu.py, with its constants, on every debug hypothesis:
  (a) exact: align_ref.dtw(-matrix) on the RETURNED matrix equals the returned frames;
  (b) |matrix - pipeline_f64(probs)| <= 8 e on the RETURNED probs, e = max |pipeline_f32 - pipeline_f64| on these very inputs;
  (c) the returned probs against the numpy decoder teacher-forced on prompt ++ t[:-1], rows P - 1 .. P - 1 + n - 1.  f32: 16 x
      max |P_numpy32 - P_numpy64|, encoder states from the CPU oracle.  bf16: BF16_PROBS_TOL = 0.05, encoder states from wh_encode.
Measured on an MI355X (DESIGN.md §5v has the table): see the figures each case prints."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import align_ref as ar
from test_align_gpu import BASE_HEADS, BF16_PROBS_TOL, NANO_HEADS, NANO_SAMPLES, gpu_states, ladder, oracle_states
from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")
ARG, STATE, UNSUPPORTED = 4, 3, 8


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def ids(n, k=0):
    """n transcript ids below the small vocabularies' timestamp block, none of them the EOT (2)."""
    return [10 + ((i + k) * 5) % 23 for i in range(n)]


def test_gather_kernel_against_host_loop(gpu):
    """tools/align_gather_check: k_align_gather on random operands (bf16 and f32 sources, dk 64 and 512, ragged lengths 1, 2, 17, Lmax, P = 1
    and 4) against a host loop; every element the definition does not name still holds the sentinel."""
    exe = os.path.join(ROOT, "tools", "align_gather_check")
    assert os.path.exists(exe), f"{exe} missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout and r.stdout.count(" ok") == 8, r.stdout + r.stderr


@pytest.fixture(scope="module")
def nano(gpu):
    """A nano f32 context of 96 rows with the three clips of test_align_gpu's case 1 resident, and their oracle encoder states."""
    prompt, eot, tb, nots = setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 96)
    clips = [ms.synth_clip(1500 + i)[:n] for i, n in enumerate(NANO_SAMPLES)]
    enc = [oracle_states("nano", c) for c in clips]
    ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 1, eot, [eot]))
    yield ctx, clips, enc, prompt, eot
    ctx.close()


def resident(ctx, clips, prompt, eot):
    ctx.transcribe_batch(clips, wb.DecodeParams(prompt, 1, eot, [eot]))


def test_f32_three_frame_counts_ragged_lengths(nano):
    """Case 1: S_b = 1500 / 400 / 8, hypotheses of 24, 7 and 2 ids in one call, heads of two layers, every hypothesis a debug row."""
    ctx, clips, enc, prompt, eot = nano
    resident(ctx, clips, prompt, eot)
    hyps = [ids(24), ids(7, 3), ids(2, 9)]
    frames, nf, lp = ctx.align_tokens(wb.DecodeParams(prompt, 1, eot), hyps, NANO_HEADS, debug_hyps=[0, 1, 2])
    assert lp is None
    assert nf.tolist() == [1500, 400, 8] == [ar.frames_of(n) for n in NANO_SAMPLES]
    for g in range(3):
        assert len(frames[g]) == len(hyps[g])
        ladder(ctx, "nano", NANO_HEADS, g, frames[g], int(nf[g]), prompt, hyps[g], enc[g], False, label="forced case 1")
    n = C.c_size_t(0)
    assert ctx.lib.wh_get_token_frames(ctx.h, None, 0, None, 0, C.byref(n)) == STATE   # the decode getters have nothing after this call


def test_generating_loop_against_forced_pass(nano):
    """Case 2: a greedy decode with wh_ctx_set_alignment on, then the forced pass on the tokens it generated — the same rows from two routes.
    Each route lies within the ladder-(c) bound of the same float64 probabilities, so they lie within twice that of each other.  The option
    stays set on the ctx during the forced call (it is ignored) and the decode repeated afterwards returns what it returned before."""
    ctx, clips, enc, prompt, eot = nano
    ctx.set_alignment(NANO_HEADS, debug_rows=[0, 1, 2])
    try:
        p = wb.DecodeParams(prompt, 24, eot, [eot])
        toks = ctx.transcribe_batch(clips, p)
        loop_frames, loop_nf = ctx.token_frames()
        loop = [ctx.alignment_debug(b) for b in range(3)]
        gen = [[int(t) for t in toks[b][len(prompt):]] for b in range(3)]
        assert all(len(g) == 24 for g in gen)
        frames, nf, _ = ctx.align_tokens(p, gen, NANO_HEADS, debug_hyps=[0, 1, 2])
        assert nf.tolist() == loop_nf.tolist()
        differ = 0
        for b in range(3):
            forced = ctx.alignment_debug(b)
            _, _, _, bound = ladder(forced, "nano", NANO_HEADS, b, frames[b], int(nf[b]), prompt, gen[b], enc[b], False, label="forced case 2")
            d = float(np.abs(forced[0] - loop[b][0]).max())
            differ += int((frames[b] != loop_frames[b]).sum())
            print(f"forced case 2 clip {b}: max |P_forced - P_loop| {d:.3g} vs 2 x bound = {2 * bound:.3g}")
            assert d <= 2 * bound, (b, d, bound)
        print(f"forced case 2: {differ} of {3 * 24} frames differ between the generating loop and the forced pass")
        toks2 = ctx.transcribe_batch(clips, p)
        frames2, _ = ctx.token_frames()
        for b in range(3):
            assert np.array_equal(toks[b], toks2[b]) and np.array_equal(loop_frames[b], frames2[b])
    finally:
        ctx.clear_alignment()


def test_hypotheses_per_clip_and_passes(nano):
    """Case 3: H = 2 on two clips, the same 63 ids everywhere (T = 65, a clip's hypotheses take 130 rows): on a context of 258 rows one
    clip fits per pass, on one of 262 both do.  The two sizes are chosen on the same side of every context-wide switch: the number of key
    ranges the K/V cross-attention splits a clip into is a property of the context (256 / max_batch, at least 1: one range for both), and
    two contexts that differ in it differ in the last bit of everything behind layer 0's cross-attention, whatever entry runs — so only the
    pass layout differs between the two, which is what the case is about."""
    _, clips, enc, prompt, eot = nano
    H, t = 2, ids(63)
    T = len(prompt) + len(t) - 1
    small, big = wb.Context(nano[0].model, 2 * H * T - 2), wb.Context(nano[0].model, 2 * H * T + 2)
    assert (2 * H * T - 2) // (H * T) == 1 and (2 * H * T + 2) // (H * T) == 2 and 2 * H * T - 2 > 256
    p = wb.DecodeParams(prompt, 1, eot)
    hyps = [t] * 4
    out = []
    for ctx in (small, small, big):
        resident(ctx, clips[:2], prompt, eot)
        frames, nf, _ = ctx.align_tokens(p, hyps, NANO_HEADS, hyps_per_clip=H, debug_hyps=[0, 1, 2, 3])
        assert nf.tolist() == [1500, 1500, 400, 400]
        out.append((frames, [ctx.alignment_debug(k) for k in range(4)]))
    small.close()
    big.close()
    frames, dbg = out[0]
    for b in range(2):
        ladder(dbg[2 * b], "nano", NANO_HEADS, 2 * b, frames[2 * b], (1500, 400)[b], prompt, t, enc[b], False, label="forced case 3")
        assert dbg[2 * b][0].tobytes() == dbg[2 * b + 1][0].tobytes() and dbg[2 * b][1].tobytes() == dbg[2 * b + 1][1].tobytes()
        assert np.array_equal(frames[2 * b], frames[2 * b + 1])
    assert dbg[0][0].shape != dbg[2][0].shape and not np.array_equal(dbg[0][0][:, :, :400], dbg[2][0])   # another clip's keys
    for k in range(4):   # the call repeated; the same call in one pass on the larger context
        assert np.array_equal(out[1][0][k], frames[k]) and out[1][1][k][0].tobytes() == dbg[k][0].tobytes() and out[1][1][k][1].tobytes() == dbg[k][1].tobytes()
        assert np.array_equal(out[2][0][k], frames[k]) and out[2][1][k][0].tobytes() == dbg[k][0].tobytes()


def test_f32_full_text_context(gpu):
    """Case 4: a transcript of n_text_ctx - P ids (the greedy tokens with EOT suppressed) on a context of max_batch = n_text_ctx rows."""
    prompt, eot, tb, nots = setup("nano")
    tc = ms.PRESETS["nano"].n_text_ctx
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, tc)
    clip = ms.synth_clip(1500)
    n = tc - len(prompt)
    toks = ctx.transcribe_batch([clip], wb.DecodeParams(prompt, n, eot, [eot]))
    t = [int(x) for x in toks[0][len(prompt):]]
    assert len(t) == n
    frames, nf, _ = ctx.align_tokens(wb.DecodeParams(prompt, 1, eot, [eot]), [t], NANO_HEADS, debug_hyps=[0])
    assert len(frames[0]) == n and nf[0] == 1500
    ladder(ctx, "nano", NANO_HEADS, 0, frames[0], 1500, prompt, t, oracle_states("nano", clip), False, label="forced case 4")
    ctx.close()


def test_one_token_hypotheses(nano):
    """Case 5: n_h == 1 among longer hypotheses gives frame 0; a call of one-token hypotheses alone returns zeros."""
    ctx, clips, enc, prompt, eot = nano
    resident(ctx, clips, prompt, eot)
    p = wb.DecodeParams(prompt, 1, eot)
    hyps = [ids(9), [17], ids(5, 2)]
    frames, nf, _ = ctx.align_tokens(p, hyps, NANO_HEADS, debug_hyps=[0, 1])
    assert frames[1].tolist() == [0] and len(frames[0]) == 9 and len(frames[2]) == 5
    ladder(ctx, "nano", NANO_HEADS, 0, frames[0], 1500, prompt, hyps[0], enc[0], False, label="forced case 5")
    probs, matrix = ctx.alignment_debug(1)
    assert probs.shape == (3, 1, 400) and matrix.shape == (1, 400) and not probs.any()
    frames, nf, lp = ctx.align_tokens(p, [[11], [12], [13]], NANO_HEADS, debug_hyps=[2], want_logprobs=True)
    assert [f.tolist() for f in frames] == [[0], [0], [0]] and nf.tolist() == [1500, 400, 8]
    assert ctx.alignment_debug(0)[0].shape == (3, 1, 8)
    want, _, _ = ctx.score_tokens(p, [[11], [12], [13]])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lp, want))


@pytest.mark.parametrize("cross_es,nb", [(False, 2), (True, 3)])
def test_bf16_base(gpu, cross_es, nb):
    """Case 6: whisper-base in bf16 on the projected K / V (bf16 queries, dk 64) and on the encoder states (f32 expanded queries, dk 512);
    12 ids, four heads of three layers.  max_batch 32 holds two clips of T = 14 rows: the encoder-state case's three clips take two passes."""
    prompt, eot, tb, nots = setup("base")
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, 32, cross_es=cross_es)
    assert ctx.cross_mode == (1 if cross_es else 0)
    clips = [ms.synth_clip(1500 + i) for i in range(nb)]
    p = wb.DecodeParams(prompt, 12, eot, [eot])
    toks = ctx.transcribe_batch(clips, p)
    hyps = [[int(t) for t in toks[b][len(prompt):]] for b in range(nb)]
    assert all(len(h) == 12 for h in hyps) and (len(prompt) + 11) * 2 <= 32 < (len(prompt) + 11) * 3
    frames, nf, _ = ctx.align_tokens(p, hyps, BASE_HEADS, debug_hyps=list(range(nb)))
    dbg = [ctx.alignment_debug(b) for b in range(nb)]
    worst = 0.0
    for b in range(nb):
        states = gpu_states(ctx, clips[b])   # (the context now holds this one clip's encoder states)
        _, _, dp, _ = ladder(dbg[b], "base", BASE_HEADS, b, frames[b], int(nf[b]), prompt, hyps[b], states, True, label=f"forced case 6 {'es' if cross_es else 'kv'}")
        worst = max(worst, dp)
    print(f"forced bf16 {'encoder-state' if cross_es else 'K/V'} form: largest |probs - numpy64| {worst:.3g}")
    assert worst <= BF16_PROBS_TOL, worst                                                        # (c)
    ctx.close()


def test_logprobs_are_the_scoring_pass(gpu):
    """Case 7: want_logprobs equals score_tokens bit for bit; without it a fresh context needs no logits scratch and still scores afterwards."""
    prompt, eot, tb, nots = setup("nano")
    model = wb.Model("synthetic:nano:7", 0, wb.WH_PREC_F32)
    ctx = wb.Context(model, 64)
    clips = [ms.synth_clip(1500), ms.synth_clip(1501)[:128000]]
    p = wb.DecodeParams(prompt, 1, eot, [eot], [12])
    ctx.transcribe_batch(clips, p)
    hyps = [ids(20), ids(6, 4)]
    f0, _, lp0 = ctx.align_tokens(p, hyps, NANO_HEADS)
    assert lp0 is None
    want, _, _ = ctx.score_tokens(p, hyps)
    f1, _, lp1 = ctx.align_tokens(p, hyps, NANO_HEADS, want_logprobs=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(lp1, want))
    assert all(np.array_equal(a, b) for a, b in zip(f0, f1))
    assert lp1[0][0] != 0 and np.isfinite(lp1[1][1:]).all()
    ctx.close()


def test_refusals(nano):
    """Case 8: every refusal, before anything is launched; a decode afterwards returns what it returned before."""
    ctx, clips, enc, prompt, eot = nano
    p = wb.DecodeParams(prompt, 6, eot, [eot])
    before = ctx.transcribe_batch(clips, p)
    hyps = [ids(5), ids(4, 1), ids(3, 2)]
    i32p = C.POINTER(C.c_int32)

    def raw(hyps=hyps, heads=NANO_HEADS, H=1, debug=(), params=p, frames=True, cap=None, null_heads=False, size=None, n_heads=None, n_hyp=None, in_size=None,
            first_off=None):
        pc, keep = params.to_c()
        inp, opts, lens, cp, keep2 = wb.align_pack(hyps, heads, H, debug)
        if size is not None:
            opts.struct_size = size
        if n_heads is not None:
            opts.n_heads = n_heads
        if n_hyp is not None:
            inp.n_hyp = n_hyp
        if in_size is not None:
            inp.struct_size = in_size
        if first_off is not None:
            keep2[1][0] = first_off
        cap = cp if cap is None else cap
        fr = np.zeros((len(hyps), max(cap, cp)), np.int32)
        return ctx.lib.wh_align_tokens(ctx.h, C.byref(pc), C.byref(inp), None if null_heads else C.byref(opts), fr.ctypes.data_as(i32p) if frames else None, None,
                                       None, cap)

    assert raw() == 0
    # the head list's own errors
    assert raw(null_heads=True) == ARG
    assert raw(size=C.sizeof(wb.WhAlignmentOpts) + 8) == ARG
    assert raw(n_heads=0) == ARG and raw(heads=[(0, 0)] * 33) == ARG
    assert raw(heads=[(2, 0)]) == ARG and raw(heads=[(-1, 0)]) == ARG and raw(heads=[(0, 2)]) == ARG and raw(heads=[(0, -1)]) == ARG
    assert raw(heads=[(1, 0), (0, 1), (1, 0)]) == ARG
    assert raw(debug=list(range(9))) == ARG and raw(debug=[-1]) == ARG
    assert raw(debug=[3]) == ARG                                    # a debug hypothesis >= n_hyp
    assert raw(cap=4) == ARG and raw(frames=False) == ARG
    # what the scoring entry refuses, with its codes
    assert raw(in_size=8) == ARG and raw(n_hyp=2) == ARG and raw(hyps=hyps + [ids(2)]) == ARG and raw(first_off=1) == ARG
    assert raw(hyps=[ids(5), [], ids(3)]) == ARG                    # offsets not strictly increasing
    assert raw(hyps=[ids(5), [10 ** 6], ids(3)]) == ARG             # an id outside the vocabulary
    assert raw(params=wb.DecodeParams(prompt, 6, eot, [eot], forced=[11])) == ARG
    tc = ms.PRESETS["nano"].n_text_ctx
    assert raw(hyps=[ids(tc - len(prompt) + 1), ids(4), ids(3)]) == ARG          # P + longest > n_text_ctx
    assert raw(hyps=[ids(97), ids(4), ids(3)]) == ARG               # H * T > max_batch (96)
    assert raw(hyps=[ids(5)] * 6, H=2) == 0 and raw(hyps=[ids(5)] * 6, H=3) == ARG
    for setter, clear in ((lambda: ctx.set_timestamp_rules(ms.PRESETS["nano"].vocab - 301), ctx.clear_timestamp_rules), (lambda: ctx.set_repetition(1.2, 0), ctx.clear_repetition),
                          (lambda: ctx.set_beam_search(2), ctx.clear_beam_search), (lambda: ctx.set_prefixes([[20], [], []]), ctx.clear_prefixes)):
        setter()
        try:
            assert raw() == UNSUPPORTED
        finally:
            clear()
    ctx.set_alignment([(0, 0)])                                     # alignment on the ctx: ignored by this entry
    assert raw() == 0
    ctx.clear_alignment()
    after = ctx.transcribe_batch(clips, p)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    fresh = wb.Context(ctx.model, 32)                               # no resident states
    pc, keep = p.to_c()
    inp, opts, lens, cp, keep2 = wb.align_pack([ids(3)], NANO_HEADS)
    fr = np.zeros((1, 3), np.int32)
    assert fresh.lib.wh_align_tokens(fresh.h, C.byref(pc), C.byref(inp), C.byref(opts), fr.ctypes.data_as(i32p), None, None, 3) == STATE
    fresh.close()
    for prec in (wb.WH_PREC_FP8, wb.WH_PREC_F16X3):
        pr, e2, _, _ = setup("micro")
        c2 = wb.Context(wb.Model("synthetic:micro:11", 0, prec), 32)
        pp = wb.DecodeParams(pr, 4, e2, [e2])
        ref = c2.transcribe_batch(clips[:1], pp)
        with pytest.raises(wb.WhisperHipError) as ei:
            c2.align_tokens(pp, [ids(4)], [(1, 0)])
        assert ei.value.code == UNSUPPORTED
        assert np.array_equal(c2.transcribe_batch(clips[:1], pp)[0], ref[0])
        c2.close()


def test_cli_align_ids_dir(gpu, tmp_path):
    """Case 9: whisper_bench --align-ids-dir on four synthetic clips, the ids files written from the binding's greedy tokens."""
    common = [CLI, "--onnx-dir", "synthetic:base:1234", "--synthetic-clips", "4", "--max-batch", "4", "--max-new-tokens", "16",
              "--out-csv", str(tmp_path / "rows.csv"), "--out-summary-json", str(tmp_path / "summary.json")]
    # the ids files: the greedy tokens of the same model on the CLI's synthetic clips, through the binding (EOT included where it was hit)
    prompt, eot, tb, nots = setup("base")
    ctx = wb.Context(wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16), 4)
    toks = ctx.transcribe_batch([wb.cli_synthetic_clip(1000 + i) for i in range(4)], wb.DecodeParams(prompt, 16, eot))
    ctx.close()
    ids_dir = tmp_path / "ids"
    ids_dir.mkdir()
    for i, t in enumerate(toks):
        (ids_dir / f"clip_{i:04d}.txt").write_text(" ".join(str(int(x)) for x in t[len(prompt):]) + "\n")
    out = tmp_path / "aligned.json"
    r = subprocess.run(common + ["--out-json", str(out), "--align-ids-dir", str(ids_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    aligned = json.loads(out.read_text())
    assert len(aligned) == 4
    for i, row in enumerate(aligned):
        assert row["aligned"] is True and "words" in row and "token_times" in row and "avg_logprob" in row
        assert len(row["token_times"]) == len(toks[i]) - len(prompt)
        words = row["words"]
        if row["text"] == "[EMPTY]":
            assert words == []
            continue
        assert words and "".join(w["word"] for w in words) == row["text"]
        starts = [w["start"] for w in words]
        assert all(w["start"] <= w["end"] for w in words)
        assert all(a <= b for a, b in zip(starts, starts[1:]))
        assert all(0 <= w["start"] <= row["duration_s"] and w["end"] <= row["duration_s"] for w in words)
    stem = "clip_0002"
    (ids_dir / f"{stem}.txt").unlink()
    r = subprocess.run(common + ["--out-json", str(out), "--align-ids-dir", str(ids_dir)], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and f"{stem}.txt" in r.stderr, (r.returncode, r.stderr[-2000:])
