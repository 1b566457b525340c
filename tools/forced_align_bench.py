"""Cost of forced alignment (wh_align_tokens): bf16 whisper-base (synthetic weights) in the encoder-state form, six alignment
heads of three layers, on a 2048-row context with the encoder states of 15 clips resident.  Alternating in one process, 2 warm-up + 5 timed
rounds, the HIP-event time of the call (wh_get_timings decode_s), min-max:
  (a)  wh_align_tokens on 15 clips x 128 tokens (15 x 131 = 1965 rows, one pass), with and without logprob_out;
  (s)  wh_score_tokens on the same input, on a second context of the same model (the scoring entry refuses a ctx with alignment set);
  (b)  the same frames through the only route the parent commit has: the forced token loop with wh_ctx_set_alignment on, one call per
       transcript (the loop takes one history per call), and its best case, one call with a shared history.
Then the split of (a) into gather and the three post-pass kernels on a third context created under WH_ALIGN_TIMING=1 (its events make the host
wait per chunk, so it is not the context the totals come from), and one clip x 445 tokens alone, the shape one workgroup per (head, hypothesis)
of the score kernel bounds.  Writes profiles/forced_align_bench.json (--out) and prints it.

    python tools/forced_align_bench.py [--steps 5] [--warmup 2]
    python tools/forced_align_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # records bench.py's result lines of both trees in --out
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402
from repetition_bench import bench_lines  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359, 50363], 50257
HEADS = [(5, 0), (5, 7), (4, 1), (4, 5), (3, 2), (3, 6)]


def stats(xs):
    return {"all": [float(x) for x in xs], "median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forced_align_bench.json"))
    ap.add_argument("--bench-lines", nargs=2, metavar=("THIS", "PARENT"), help="record bench.py's result lines of this tree and of the parent commit in --out")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines:
        old["headline_vs_parent"] = bench_lines(*a.bench_lines)
        old["headline_vs_parent"]["command"] = "python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR, the two trees alternating in one visit, parent first"
        json.dump(old, open(a.out, "w"), indent=1)
        print(json.dumps(old))
        return
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.rows, cross_es=True)       # (a), (b): alignment stays set on it, so the captured step is captured once
    ctx_s = wb.Context(model, a.rows, cross_es=True)     # (s)
    os.environ["WH_ALIGN_TIMING"] = "1"
    ctx_t = wb.Context(model, a.rows, cross_es=True)     # the split
    del os.environ["WH_ALIGN_TIMING"]
    ctx_t.lib.wh_debug_forced_align_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.stack([ms.synth_clip(3000 + i) for i in range(15)])))
    rng = np.random.Generator(np.random.PCG64(5))
    p1 = wb.DecodeParams(PROMPT, 1, EOT, [EOT])
    out = {"rows": a.rows, "precision": "bf16", "preset": "base", "cross_mode": ctx.cross_mode, "heads": HEADS, "steps": a.steps, "warmup": a.warmup}

    def split(c, params, hyps, want):
        c.align_tokens(params, hyps, HEADS, want_logprobs=want)
        total = c.timings()["decode_s"] * 1e3
        ms4 = (C.c_double * 4)()
        c._check(c.lib.wh_debug_forced_align_times(c.h, ms4))
        post = ms4[1] + ms4[2] + ms4[3]
        return {"call_ms_with_timing_events": total, "k_align_gather_ms_all_layers": ms4[0], "k_align_scores_ms": ms4[1], "k_align_filter_ms": ms4[2],
                "k_align_dtw_ms": ms4[3], "post_pass_ms": post, "pass_ms": total - post - ms4[0]}
    try:
        for c in (ctx, ctx_s, ctx_t):
            c.transcribe_batch_device(d_pcm, 15, p1)
        ctx.set_alignment(HEADS)
        texts = [rng.integers(0, EOT, size=128).tolist() for _ in range(15)]
        forced = [wb.DecodeParams(PROMPT, 128, EOT, [EOT], forced=t[:-1]) for t in texts]

        def ev(c, fn):
            fn()
            return c.timings()["decode_s"]

        def run_b():
            t = 0.0
            for b in range(15):
                ctx.greedy_decode_resident_batch(forced[b])
                t += ctx.timings()["decode_s"]
            return t
        runs = {
            "a_align_15x128_with_logprobs": lambda: ev(ctx, lambda: ctx.align_tokens(p1, texts, HEADS, want_logprobs=True)),
            "a_align_15x128_frames_only": lambda: ev(ctx, lambda: ctx.align_tokens(p1, texts, HEADS)),
            "s_score_15x128": lambda: ev(ctx_s, lambda: ctx_s.score_tokens(p1, texts, 1)),
            "b_forced_loop_alignment_15_calls": run_b,
            "b_forced_loop_alignment_shared_history": lambda: ev(ctx, lambda: ctx.greedy_decode_resident_batch(forced[0])),
        }
        res = {k: [] for k in runs}
        for i in range(a.warmup + a.steps):
            for k, fn in runs.items():
                t = fn()
                if i >= a.warmup:
                    res[k].append(t)
        for k in runs:
            out[k] = {"decode_s": stats(res[k])}
        med = lambda k: out[k]["decode_s"]["median"]   # noqa: E731
        out["b_15_calls_over_a_with_logprobs"] = med("b_forced_loop_alignment_15_calls") / med("a_align_15x128_with_logprobs")
        out["b_shared_history_over_a_with_logprobs"] = med("b_forced_loop_alignment_shared_history") / med("a_align_15x128_with_logprobs")
        out["a_with_logprobs_minus_score_ms"] = (med("a_align_15x128_with_logprobs") - med("s_score_15x128")) * 1e3
        out["split_15x128_with_logprobs"] = split(ctx_t, p1, texts, True)
        out["split_15x128_frames_only"] = split(ctx_t, p1, texts, False)
        # ---- one clip x 445 tokens (P = 3: 447 rows) ----
        p3 = wb.DecodeParams(PROMPT[:3], 1, EOT, [EOT])
        long = [rng.integers(0, EOT, size=445).tolist()]
        for c in (ctx, ctx_t):
            c.transcribe_batch_device(d_pcm, 1, p3)
        r = []
        for i in range(a.warmup + a.steps):
            t = ev(ctx, lambda: ctx.align_tokens(p3, long, HEADS, want_logprobs=True))
            if i >= a.warmup:
                r.append(t)
        out["one_clip_x_445"] = {"decode_s": stats(r), "split": split(ctx_t, p3, long, True)}
    finally:
        hip.free(d_pcm)
    if "headline_vs_parent" in old:
        out["headline_vs_parent"] = old["headline_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
