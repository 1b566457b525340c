"""Cost of the word-level timestamps (wh_ctx_set_alignment): bf16 whisper-base (synthetic weights) at 2048 resident clips
through wh_transcribe_batch_device, 128 tokens, EOT suppressed so every row decodes every position, 6 alignment heads.  The option is turned
off and on alternately, step by step, in one process.  Reports the step and decode times of both, the three post-pass kernels' times
(HIP events around each launch: WH_ALIGN_TIMING=1, read through wh_debug_align_times) and the per-position copy's time (what is left of the
decode-time difference after the post-pass, per decoder position).  Writes profiles/align_bench.json (--out) and prints it.

    python tools/align_bench.py [--clips 2048] [--steps 3] [--warmup 1]
    # the option-off regression against the parent commit is bench.py's own headline, run alternately on both trees in one session:
    python tools/align_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # records both series in --out (no threshold)
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
os.environ["WH_ALIGN_TIMING"] = "1"
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402
from repetition_bench import bench_lines  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359], 50257
HEADS = [(5, 0), (5, 3), (4, 1), (4, 6), (3, 2), (3, 7)]
KERNELS = ("scores_ms", "filter_ms", "dtw_ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.json"))
    ap.add_argument("--bench-lines", nargs=2, metavar=("THIS", "PARENT"), help="record bench.py's result lines of this tree and of the parent commit in --out")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines:
        old["option_off_vs_parent"] = bench_lines(*a.bench_lines)
        old["option_off_vs_parent"]["command"] = "python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR, the two trees alternating (two visits)"
        json.dump(old, open(a.out, "w"), indent=1)
        print(json.dumps(old))
        return
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.clips)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (a.clips // 64 + 1, 1))[: a.clips]))
    p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT, [EOT])
    ctx.lib.wh_debug_align_times.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    res = {m: {"decode_s": [], "step_s": []} for m in ("off", "on")}
    kern = {k: [] for k in KERNELS}
    toks = {}
    try:
        for i in range(a.warmup + a.steps):
            for mode in ("off", "on"):
                if mode == "on":
                    ctx.set_alignment(HEADS)
                else:
                    ctx.clear_alignment()
                t0 = time.perf_counter()
                toks[mode] = ctx.transcribe_batch_device(d_pcm, a.clips, p)   # (ends in a stream synchronise)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    res[mode]["decode_s"].append(ctx.timings()["decode_s"])
                    res[mode]["step_s"].append(t1 - t0)
                    if mode == "on":
                        ms3 = (C.c_double * 3)()
                        ctx._check(ctx.lib.wh_debug_align_times(ctx.h, ms3))
                        for k, v in zip(KERNELS, ms3):
                            kern[k].append(float(v))
        frames, nf = ctx.token_frames()
    finally:
        hip.free(d_pcm)
    positions = len(PROMPT) + a.max_new_tokens - 1
    out = {"clips": a.clips, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base", "heads": len(HEADS), "positions": positions,
           "cross_mode": ctx.cross_mode, "tokens_identical": all(np.array_equal(x, y) for x, y in zip(toks["off"], toks["on"]))}
    for mode in ("off", "on"):
        out[mode] = {**res[mode], "decode_s_median": float(np.median(res[mode]["decode_s"])), "step_s_median": float(np.median(res[mode]["step_s"]))}
    out["kernels"] = {k: float(np.median(v)) for k, v in kern.items()}
    post_s = sum(out["kernels"].values()) * 1e-3
    d_decode = out["on"]["decode_s_median"] - out["off"]["decode_s_median"]
    out["post_pass_s"] = post_s
    out["on_minus_off_decode_s"] = d_decode
    out["share_of_step"] = (out["on"]["step_s_median"] - out["off"]["step_s_median"]) / out["on"]["step_s_median"]
    out["copy_per_position_us"] = (d_decode - post_s) / positions * 1e6
    out["step_spread_off_s"] = float(np.max(res["off"]["step_s"]) - np.min(res["off"]["step_s"]))
    out["distinct_frames_row0"] = int(len(set(frames[0].tolist())))
    if "option_off_vs_parent" in old:
        out["option_off_vs_parent"] = old["option_off_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
