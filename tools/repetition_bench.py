"""Cost of the repetition controls in the token loop (wh_ctx_set_repetition): bf16 whisper-base (synthetic weights) at 2048
resident clips through wh_transcribe_batch_device, 128 tokens, EOT suppressed so every mode decodes every position.  Modes, alternating
step by step: option off; {1.3, 0} (penalty only); {1.0, 3} (ban only); {1.3, 3}.  Writes profiles/repetition_bench.json (--out) and prints it.

    python tools/repetition_bench.py [--clips 2048] [--steps 3] [--warmup 1]
    # the option-off regression against the parent commit is bench.py's own headline, run alternately on both trees in one session:
    python tools/repetition_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # records both series in --out (no threshold)
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

PROMPT, EOT = [50258, 50259, 50359], 50257
MODES = {"off": None, "penalty_1.3": (1.3, 0), "ngram_3": (1.0, 3), "penalty_1.3_ngram_3": (1.3, 3)}


def bench_lines(this_path, parent_path):
    """bench.py result lines (one JSON object per line) of this tree and of the parent commit, run alternately in one session: both
    series as they are, and the parent's own run-to-run spread beside them."""
    def steps(path):
        return [json.loads(line) for line in map(str.strip, open(path)) if line.startswith("{")]
    a, b = steps(this_path), steps(parent_path)
    k = "ms_per_step"   # (lower is better)
    res = {"metric": k, "command": "python bench.py --gpus 1 --steps 5 --warmup 2, the two trees alternating", "this": [j.get(k) for j in a], "parent": [j.get(k) for j in b]}
    if a and b:
        pa = [float(x) for x in res["parent"]]
        res["parent_spread"] = [min(pa), max(pa)]
        res["this_median"] = float(np.median([float(x) for x in res["this"]]))
        res["parent_median"] = float(np.median(pa))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "repetition_bench.json"))
    ap.add_argument("--bench-lines", nargs=2, metavar=("THIS", "PARENT"), help="record bench.py's result lines of this tree and of the parent commit in --out")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines:
        old["option_off_vs_parent"] = bench_lines(*a.bench_lines)
        json.dump(old, open(a.out, "w"), indent=1)
        print(json.dumps(old))
        return
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.clips)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (a.clips // 64 + 1, 1))[: a.clips]))
    p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT, [EOT])
    res = {m: {"decode_s": [], "step_s": []} for m in MODES}
    toks = {}
    try:
        for i in range(a.warmup + a.steps):
            for mode, opt in MODES.items():
                if opt is None:
                    ctx.clear_repetition()
                else:
                    ctx.set_repetition(*opt)
                t0 = time.perf_counter()
                toks[mode] = ctx.transcribe_batch_device(d_pcm, a.clips, p)   # (ends in a stream synchronise)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    res[mode]["decode_s"].append(ctx.timings()["decode_s"])
                    res[mode]["step_s"].append(t1 - t0)
    finally:
        hip.free(d_pcm)
    P = len(PROMPT)
    bigrams = lambda t: sum(1 for j in range(P + 1, len(t)) if (int(t[j - 1]), int(t[j])) in {(int(t[k - 1]), int(t[k])) for k in range(P + 1, j)})
    out = {"clips": a.clips, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base", "positions": P + a.max_new_tokens - 1}
    for mode in MODES:
        out[mode] = {**res[mode], "decode_s_median": float(np.median(res[mode]["decode_s"])), "step_s_median": float(np.median(res[mode]["step_s"])),
                     "repeated_bigrams_per_row": float(np.mean([bigrams(t) for t in toks[mode][:64]]))}
        out[mode]["minus_off_s"] = out[mode]["step_s_median"] - float(np.median(res["off"]["step_s"]))
        out[mode]["decode_per_position_s"] = out[mode]["decode_s_median"] / out["positions"]
    out["step_spread_off_s"] = float(np.max(res["off"]["step_s"]) - np.min(res["off"]["step_s"]))
    if "option_off_vs_parent" in old:
        out["option_off_vs_parent"] = old["option_off_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
