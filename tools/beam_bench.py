"""Cost of beam search (wh_ctx_set_beam_search): bf16 whisper-base (synthetic weights) on a 2048-row context through
wh_transcribe_batch_device, 128 tokens, EOT suppressed so every row decodes every position.  Three configurations alternate step by step in
one process: greedy on 2048 clips, greedy on 409 clips, beam_size 5 on 409 clips (2045 rows).  Then one pass per configuration with every
position launched eagerly and timed (wh_profile_enable): the cross-attention kernel's time per launch, and — WH_BEAM_TIMING=1, read through
wh_debug_beam_times — k_beam_select and k_beam_reorder per position.  Writes profiles/beam_bench.json (--out) and prints it.

    python tools/beam_bench.py [--rows 2048] [--beam-size 5] [--steps 3] [--warmup 1]
    # the option-off regression against the parent commit is bench.py's own headline, run alternately on both trees in one session:
    python tools/beam_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # records both series in --out (no threshold)
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
os.environ["WH_BEAM_TIMING"] = "1"
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402
from repetition_bench import bench_lines  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359], 50257


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--beam-size", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    ap.add_argument("--bench-lines", nargs=2, metavar=("THIS", "PARENT"), help="record bench.py's result lines of this tree and of the parent commit in --out")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines:
        old["option_off_vs_parent"] = bench_lines(*a.bench_lines)
        old["option_off_vs_parent"]["command"] = "python bench.py --gpus 1 --steps 3 --warmup 1 --dump-outputs DIR, the two trees alternating in one visit"
        json.dump(old, open(a.out, "w"), indent=1)
        print(json.dumps(old))
        return
    K, n_beam = a.beam_size, a.rows // a.beam_size
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.rows)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (a.rows // 64 + 1, 1))[: a.rows]))
    p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT, [EOT])
    ctx.lib.wh_debug_beam_times.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_long)]
    configs = {"greedy_all": (a.rows, 0), "greedy_clips": (n_beam, 0), "beam": (n_beam, K)}
    res = {m: {"decode_s": [], "step_s": []} for m in configs}

    def run(mode):
        n, k = configs[mode]
        if k:
            ctx.set_beam_search(k, 1.0, -1.0)
        else:
            ctx.clear_beam_search()
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
        out = {"rows": a.rows, "beam_size": K, "clips_with_beams": n_beam, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base",
               "positions": positions, "cross_mode": ctx.cross_mode}
        for mode in configs:
            out[mode] = {**res[mode], "clips": configs[mode][0], "decode_s_median": float(np.median(res[mode]["decode_s"])),
                         "step_s_median": float(np.median(res[mode]["step_s"]))}
            out[mode]["decode_ms_per_position"] = out[mode]["decode_s_median"] / positions * 1e3
        # every position launched eagerly and timed: the cross-attention launches, and the two beam kernels
        d = model.dims
        state_bytes = d.n_audio_ctx * d.d_model * 2
        for mode in configs:
            ctx.profile_enable(["dec_cross_attn"])
            run(mode)
            g = ctx.profile_get()["dec_cross_attn"]
            us = g["ms"] / max(1, g["launches"]) * 1e3
            n, k = configs[mode]
            rows = n * max(1, k)
            out[mode]["cross_attn_us_per_launch"] = us
            # the rate if every row read its states from memory, and the rate counting each clip's states once
            out[mode]["cross_attn_tbps_per_row"] = rows * state_bytes / us * 1e-6
            out[mode]["cross_attn_tbps_per_clip"] = n * state_bytes / us * 1e-6
            if k:
                ms2, npos = (C.c_double * 2)(), C.c_long(0)
                ctx._check(ctx.lib.wh_debug_beam_times(ctx.h, ms2, C.byref(npos)))
                out["kernels"] = {"positions_timed": int(npos.value), "k_beam_select_us_per_position": ms2[0] / max(1, npos.value) * 1e3,
                                  "k_beam_reorder_us_per_position": ms2[1] / max(1, npos.value) * 1e3}
            ctx.profile_enable(False)
    finally:
        hip.free(d_pcm)
    out["beam_over_greedy_same_clips"] = out["beam"]["decode_s_median"] / out["greedy_clips"]["decode_s_median"]
    out["beam_over_greedy_same_rows"] = out["beam"]["decode_s_median"] / out["greedy_all"]["decode_s_median"]
    if "option_off_vs_parent" in old:
        out["option_off_vs_parent"] = old["option_off_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
