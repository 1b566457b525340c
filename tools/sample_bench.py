"""Cost of temperature sampling (wh_ctx_set_sampling): bf16 whisper-base (synthetic weights) on a 2048-row context through
wh_transcribe_batch_device, 128 tokens, EOT suppressed so every active row decodes every position.  Three configurations alternate step by
step in one process: greedy (the option cleared), sampling at T = 1 on all rows, sampling at T = 1 with 10 % of the rows active (what a rung of
the ladder costs without compacting the batch to the failing rows).  Then one pass per sampling configuration with every position launched
eagerly and k_sample_select timed with HIP events (WH_SAMPLE_TIMING=1, read through wh_debug_sample_times).  Writes profiles/sample_bench.json
(--out) and prints it.

    python tools/sample_bench.py [--rows 2048] [--steps 3] [--warmup 1]
    # the option-off regression against the parent commit is bench.py's own headline, run alternately on both trees in one session:
    python tools/sample_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # records both series in --out (no threshold)
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
os.environ["WH_SAMPLE_TIMING"] = "1"
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402
from repetition_bench import bench_lines  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359], 50257
HBM_TBPS = 8.0   # MI355X peak HBM3E bandwidth


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample_bench.json"))
    ap.add_argument("--bench-lines", nargs=2, metavar=("THIS", "PARENT"), help="record bench.py's result lines of this tree and of the parent commit in --out")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines:
        old["option_off_vs_parent"] = bench_lines(*a.bench_lines)
        old["option_off_vs_parent"]["command"] = "python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR, the two trees alternating in one visit"
        json.dump(old, open(a.out, "w"), indent=1)
        print(json.dumps(old))
        return
    n = a.rows
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, n)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (n // 64 + 1, 1))[:n]))
    p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT, [EOT])
    ctx.lib.wh_debug_sample_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    tenth = [1 if i % 10 == 0 else 0 for i in range(n)]
    configs = {"greedy": None, "sample_all": [1] * n, "sample_tenth": tenth}
    res = {m: {"decode_s": [], "step_s": []} for m in configs}

    def run(mode):
        act = configs[mode]
        if act is None:
            ctx.clear_sampling()
        else:
            ctx.set_sampling(20240607, [1.0] * n, act)
        t0 = time.perf_counter()
        ctx.transcribe_batch_device(d_pcm, n, p)   # (ends in a stream synchronise)
        return time.perf_counter() - t0
    try:
        for i in range(a.warmup + a.steps):
            for mode in configs:
                dt = run(mode)
                if i >= a.warmup:
                    res[mode]["decode_s"].append(ctx.timings()["decode_s"])
                    res[mode]["step_s"].append(dt)
        positions = len(PROMPT) + a.max_new_tokens - 1
        vocab = model.dims.vocab
        out = {"rows": n, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base", "positions": positions, "cross_mode": ctx.cross_mode,
               "scratch_bytes_per_pass": n * vocab * 4}
        for mode in configs:
            out[mode] = {**res[mode], "active_rows": n if configs[mode] is None else int(sum(configs[mode])),
                         "decode_s_median": float(np.median(res[mode]["decode_s"])), "step_s_median": float(np.median(res[mode]["step_s"]))}
            out[mode]["decode_ms_per_position"] = out[mode]["decode_s_median"] / positions * 1e3
        # every position launched eagerly, k_sample_select between two events
        for mode in ("sample_all", "sample_tenth"):
            ctx.profile_enable(["dec_other"])
            run(mode)
            ms1, npos = C.c_double(0), C.c_long(0)
            ctx._check(ctx.lib.wh_debug_sample_times(ctx.h, C.byref(ms1), C.byref(npos)))
            ctx.profile_enable(False)
            us = ms1.value / max(1, npos.value) * 1e3
            active = out[mode]["active_rows"]
            out[mode]["k_sample_select_us_per_position"] = us
            out[mode]["positions_timed"] = int(npos.value)
            # two passes over the active rows' logits; against one pass at the HBM rate
            out[mode]["k_sample_select_tbps_two_passes"] = 2 * active * vocab * 4 / us * 1e-6
            out[mode]["one_pass_at_hbm_rate_us"] = active * vocab * 4 / (HBM_TBPS * 1e6)
    finally:
        hip.free(d_pcm)
    out["sample_all_over_greedy"] = out["sample_all"]["decode_s_median"] / out["greedy"]["decode_s_median"]
    out["sample_tenth_over_greedy"] = out["sample_tenth"]["decode_s_median"] / out["greedy"]["decode_s_median"]
    if "option_off_vs_parent" in old:
        out["option_off_vs_parent"] = old["option_off_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
