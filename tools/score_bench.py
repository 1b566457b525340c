"""Cost of scoring given transcripts (wh_score_tokens): bf16 whisper-base (synthetic weights) on a 2048-row context with the
encoder states resident.  Alternating in one process:
  (a) wh_score_tokens on 15 clips x 1 hypothesis x 128 tokens (15 x 131 = 1965 rows, one pass);
  (b) the same texts through the forced token loop: 15 calls of wh_decode_greedy_rows, since the loop takes one history per call;
  (c) one forced loop over the 15 clips with a single shared history, the loop's best case;
then, on 409 resident clips, (d) wh_score_tokens on 409 clips x 5 hypotheses x 24 tokens (28 passes of 15 clips).
Per call: host wall time and the HIP-event decode time (wh_get_timings).  Then one run of (a) and of (d) with the kernel groups bracketed by events
(wh_profile_enable) and the two scoring kernels timed on their own (WH_SCORE_TIMING=1, read through wh_debug_score_times).  Writes
profiles/score_bench.json (--out) and prints it.

    python tools/score_bench.py [--steps 5] [--warmup 2]
    # the regression against the parent commit is bench.py's own headline, run alternately on both trees in one session:
    python tools/score_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # records both series in --out (no threshold)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["WH_SCORE_TIMING"] = "1"
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402
from repetition_bench import bench_lines  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359, 50363], 50257


def stats(xs):
    return {"all": [float(x) for x in xs], "median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_bench.json"))
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
    ctx = wb.Context(model, a.rows)
    ctx.lib.wh_debug_score_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    hip = wb.HipRuntime()
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(16)])
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (26, 1))[:409]))
    rng = np.random.Generator(np.random.PCG64(5))
    p1 = wb.DecodeParams(PROMPT, 1, EOT, [EOT])
    out = {"rows": a.rows, "precision": "bf16", "preset": "base", "cross_mode": ctx.cross_mode, "steps": a.steps, "warmup": a.warmup}

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        return time.perf_counter() - t0, ctx.timings()["decode_s"]

    def kernel_groups(fn):
        ctx.profile_enable(True)
        fn()
        ms2 = (C.c_double * 2)()
        ctx._check(ctx.lib.wh_debug_score_times(ctx.h, ms2))
        pg = ctx.profile_get()
        ctx.profile_enable(False)
        return {"groups": pg, "k_score_self_attn_ms_all_layers": ms2[0], "k_score_finish_ms": ms2[1], "decode_s": ctx.timings()["decode_s"]}
    try:
        # ---- 15 resident clips: (a), (b), (c) alternating ----
        ctx.transcribe_batch_device(d_pcm, 15, p1)
        texts = [rng.integers(0, EOT, size=128).tolist() for _ in range(15)]
        forced = [wb.DecodeParams(PROMPT, 128, EOT, [EOT], forced=t[:-1]) for t in texts]

        def run_a():
            ctx.score_tokens(p1, texts, 1)

        def run_b():
            for b in range(15):
                ctx.decode_resident_rows_raw(forced[b], [b])

        def run_c():
            ctx.decode_resident_rows_raw(forced[0], [0])
        runs = {"a_score_15x1x128": run_a, "b_forced_loop_15_calls": run_b, "c_forced_loop_shared_history": run_c}
        res = {k: {"wall_s": [], "decode_s": []} for k in runs}
        for i in range(a.warmup + a.steps):
            for k, fn in runs.items():
                if k.startswith("b_"):   # the sum of its 15 calls' event times
                    t0, ev = time.perf_counter(), 0.0
                    for b in range(15):
                        ctx.decode_resident_rows_raw(forced[b], [b])
                        ev += ctx.timings()["decode_s"]
                    w = time.perf_counter() - t0
                else:
                    w, ev = timed(fn)
                if i >= a.warmup:
                    res[k]["wall_s"].append(w)
                    res[k]["decode_s"].append(ev)
        for k in runs:
            out[k] = {"wall_s": stats(res[k]["wall_s"]), "decode_s": stats(res[k]["decode_s"])}
        out["a_score_15x1x128"]["rows"] = 15 * (len(PROMPT) + 128 - 1)
        out["a_score_15x1x128"]["kernels"] = kernel_groups(run_a)
        out["c_over_a_decode_s"] = out["c_forced_loop_shared_history"]["decode_s"]["median"] / out["a_score_15x1x128"]["decode_s"]["median"]
        out["b_over_a_decode_s"] = out["b_forced_loop_15_calls"]["decode_s"]["median"] / out["a_score_15x1x128"]["decode_s"]["median"]
        # ---- 409 resident clips: (d) ----
        ctx.transcribe_batch_device(d_pcm, 409, p1)
        hyps = [rng.integers(0, EOT, size=24).tolist() for _ in range(409 * 5)]

        def run_d():
            ctx.score_tokens(p1, hyps, 5)
        rd = {"wall_s": [], "decode_s": []}
        for i in range(a.warmup + a.steps):
            w, ev = timed(run_d)
            if i >= a.warmup:
                rd["wall_s"].append(w)
                rd["decode_s"].append(ev)
        out["d_score_409x5x24"] = {"wall_s": stats(rd["wall_s"]), "decode_s": stats(rd["decode_s"]), "passes": -(-409 // (a.rows // (5 * (len(PROMPT) + 24 - 1)))),
                                   "kernels": kernel_groups(run_d)}
    finally:
        hip.free(d_pcm)
    if "headline_vs_parent" in old:
        out["headline_vs_parent"] = old["headline_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
