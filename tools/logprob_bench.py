"""Cost of the token log-probabilities in the token loop: bf16 whisper-base (synthetic weights) at 2048 resident clips through
wh_transcribe_batch_device, the same clips with log-probabilities off and on, EOT suppressed so both runs decode every position.  Prints one
JSON line with decode_s per step of each mode (median of --steps after --warmup).  --probe adds the no-speech probe to the `on` mode,
--rules runs both modes with Whisper's timestamp rules.

    python tools/logprob_bench.py [--clips 2048] [--steps 3] [--warmup 1] [--mode both|off|on] [--probe] [--rules]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--mode", choices=("both", "off", "on"), default="both")
    ap.add_argument("--probe", action="store_true", help="the `on` mode also runs the no-speech probe (id 50362 at prompt position 0)")
    ap.add_argument("--rules", action="store_true", help="both modes with the timestamp rules on")
    a = ap.parse_args()
    prompt, eot, tb, nots, no_speech = [50258, 50259, 50359], 50257, 50364, 50363, 50362
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.clips)
    if a.rules:
        ctx.set_timestamp_rules(tb, nots, 50)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (a.clips // 64 + 1, 1))[: a.clips]))
    p = wb.DecodeParams(prompt, a.max_new_tokens, eot, [eot])
    out = {"clips": a.clips, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base", "probe": a.probe, "timestamp_rules": a.rules}
    try:
        for mode in (("off", "on") if a.mode == "both" else (a.mode,)):
            if mode == "on":
                ctx.set_logprobs(no_speech if a.probe else -1, 0)
            else:
                ctx.clear_logprobs()
            dec, wall = [], []
            for i in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                toks = ctx.transcribe_batch_device(d_pcm, a.clips, p)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    dec.append(ctx.timings()["decode_s"])
                    wall.append(t1 - t0)
            assert all(len(t) == len(prompt) + a.max_new_tokens for t in toks)
            if mode == "on":
                lps, ns = ctx.logprobs()
                assert len(lps) == a.clips and all(len(l) == a.max_new_tokens and np.all(l <= 0) for l in lps) and (ns is not None) == a.probe
            out[mode] = {"decode_s": dec, "decode_s_median": float(np.median(dec)), "step_s_median": float(np.median(wall))}
    finally:
        hip.free(d_pcm)
    if "on" in out and "off" in out:
        out["decode_on_over_off"] = out["on"]["decode_s_median"] / out["off"]["decode_s_median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
