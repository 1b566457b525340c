"""Cost of language detection in the token loop: bf16 whisper-base (synthetic weights) at 2048 resident clips through
wh_transcribe_batch_device, the same clips with detection off and on (the 99 ids of the multilingual block, sot_index 0), EOT suppressed so
both modes decode every position; the two modes alternate step by step.  Writes profiles/lang_detect_bench.json (--out) and prints it.

    python tools/lang_detect_bench.py [--clips 2048] [--steps 4] [--warmup 1]
    # the kernels' own times, from a profiler run of its own (every position launched eagerly, no graph replay under the profiler):
    WH_NO_GRAPH=1 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/lang_detect_bench.py --trace-child
    python tools/lang_detect_bench.py --kernel-stats DIR/.../*_kernel_stats.csv     # merges the per-launch times into the JSON

The condition the design is held to: the language head and its finish together take no longer than ONE launch of the LM head at the same
rows — what detection through the existing LM head under a complement mask would cost."""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359], 50257
LANG_IDS = list(range(50259, 50259 + 99))


def kernel_stats(path):
    """Per-launch microseconds of the language head, the language finish and the LM head from a rocprofv3 kernel-stats CSV."""
    want = {"language_head": "k_lang_head", "language_finish": "k_lang_finish", "lm_head": "k_lm_head"}
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for key, pat in want.items():
                if pat in row["Name"]:
                    e = out.setdefault(key, {"kernel": row["Name"][:120], "calls": 0, "total_ns": 0.0})
                    e["calls"] += int(row["Calls"])
                    e["total_ns"] += float(row["TotalDurationNs"])
    for e in out.values():
        e["us_per_launch"] = e.pop("total_ns") / max(1, e["calls"]) / 1e3
    if {"language_head", "language_finish", "lm_head"} <= set(out):
        out["head_plus_finish_us"] = out["language_head"]["us_per_launch"] + out["language_finish"]["us_per_launch"]
        out["within_one_lm_head_launch"] = out["head_plus_finish_us"] <= out["lm_head"]["us_per_launch"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lang_detect_bench.json"))
    ap.add_argument("--trace-child", action="store_true", help="a few short detection-on steps and nothing else: the program to run under the profiler")
    ap.add_argument("--kernel-stats", help="merge the per-launch kernel times of this rocprofv3 kernel-stats CSV into --out")
    a = ap.parse_args()
    if a.kernel_stats:
        out = json.load(open(a.out)) if os.path.exists(a.out) else {}
        out["kernels"] = kernel_stats(a.kernel_stats)
        json.dump(out, open(a.out, "w"), indent=1)
        print(json.dumps(out))
        return
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.clips)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (a.clips // 64 + 1, 1))[: a.clips]))
    try:
        if a.trace_child:
            ctx.set_language_detection(LANG_IDS, 0)
            for _ in range(3):
                ctx.transcribe_batch_device(d_pcm, a.clips, wb.DecodeParams(PROMPT, 8, EOT, [EOT]))
            return
        p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT, [EOT])
        res = {"off": {"decode_s": [], "step_s": []}, "on": {"decode_s": [], "step_s": []}}
        toks = {}
        for i in range(a.warmup + a.steps):
            for mode in ("off", "on"):
                if mode == "on":
                    ctx.set_language_detection(LANG_IDS, 0)
                else:
                    ctx.clear_language_detection()
                t0 = time.perf_counter()
                toks[mode] = ctx.transcribe_batch_device(d_pcm, a.clips, p)   # (ends in a stream synchronise)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    res[mode]["decode_s"].append(ctx.timings()["decode_s"])
                    res[mode]["step_s"].append(t1 - t0)
        langs, probs = ctx.languages()
        assert langs.shape == (a.clips,) and abs(float(probs.sum(1).min()) - 1) < 1e-4 and abs(float(probs.sum(1).max()) - 1) < 1e-4
        assert all(int(t[1]) == int(g) for t, g in zip(toks["on"], langs))
    finally:
        hip.free(d_pcm)
    out = {"clips": a.clips, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base", "n_lang": len(LANG_IDS),
           "languages_detected": sorted({int(g) for g in langs})}
    for mode in ("off", "on"):
        out[mode] = {**res[mode], "decode_s_median": float(np.median(res[mode]["decode_s"])), "step_s_median": float(np.median(res[mode]["step_s"]))}
    out["step_on_minus_off_s"] = out["on"]["step_s_median"] - out["off"]["step_s_median"]
    out["step_spread_off_s"] = float(np.max(res["off"]["step_s"]) - np.min(res["off"]["step_s"]))
    if os.path.exists(a.out):
        old = json.load(open(a.out))
        if "kernels" in old:
            out["kernels"] = old["kernels"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
