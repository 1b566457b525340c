"""Cost of per-clip prompt prefixes in the token loop (wh_ctx_set_prefixes): bf16 whisper-base (synthetic weights) at 2048
resident clips through wh_transcribe_batch_device, EOT suppressed so every mode decodes every position.  Modes, alternating step by step:
prefixes off; every clip with a prefix of 0, 32 and 224 ids; a ragged batch whose lengths cycle through 0, 1, 63, 64, 65, 129, 140.
Writes profiles/prefix_bench.json (--out) and prints it.

    python tools/prefix_bench.py [--clips 2048] [--steps 2] [--warmup 1]
    # the prefixes-off regression against the parent commit is bench.py's own headline, run alternately on both trees in one session:
    python tools/prefix_bench.py --bench-lines THIS.jsonl PARENT.jsonl     # merges the two trees' bench.py result lines into --out

The per-position cost (step(224) - step(0)) / 224 is the number a later one-pass prompt prefill is judged against."""
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
LENS = (0, 1, 63, 64, 65, 129, 140)


def bench_lines(this_path, parent_path):
    """bench.py result lines (one JSON object per line) of this tree and of the parent commit, run alternately in one session."""
    def steps(path):
        out = []
        for line in open(path):
            line = line.strip()
            if line.startswith("{"):
                j = json.loads(line)
                out.append(j)
        return out
    a, b = steps(this_path), steps(parent_path)
    k = "ms_per_step"   # (lower is better)
    res = {"metric": k, "command": "python bench.py --gpus 1 --steps 5 --warmup 2, the two trees alternating", "this": [j.get(k) for j in a], "parent": [j.get(k) for j in b]}
    if a and b:
        pa = [float(x) for x in res["parent"]]
        th = [float(x) for x in res["this"]]
        res["parent_spread"] = [min(pa), max(pa)]
        res["this_median"] = float(np.median(th))
        res["parent_median"] = float(np.median(pa))
        res["this_median_within_parent_spread"] = min(pa) <= res["this_median"] <= max(pa)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-new-tokens", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefix_bench.json"))
    ap.add_argument("--bench-lines", nargs=2, metavar=("THIS", "PARENT"), help="merge bench.py's result lines of this tree and of the parent commit into --out")
    a = ap.parse_args()
    old = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.bench_lines:
        old["prefixes_off_vs_parent"] = bench_lines(*a.bench_lines)
        json.dump(old, open(a.out, "w"), indent=1)
        print(json.dumps(old))
        return
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.clips)
    uniq = np.stack([ms.synth_clip(3000 + i) for i in range(64)])
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(uniq, (a.clips // 64 + 1, 1))[: a.clips]))
    rng = np.random.default_rng(5)
    ids = [int(t) for t in rng.integers(10, model.dims.vocab - 2000, 224)]
    modes = {"off": None, "len0": [[]] * a.clips, "len32": [ids[:32]] * a.clips, "len224": [ids] * a.clips,
             "ragged": [ids[: LENS[i % 7]] for i in range(a.clips)]}
    p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT, [EOT])
    res = {m: {"decode_s": [], "step_s": []} for m in modes}
    toks = {}
    try:
        for i in range(a.warmup + a.steps):
            for mode, pre in modes.items():
                if pre is None:
                    ctx.clear_prefixes()
                else:
                    ctx.set_prefixes(pre)
                t0 = time.perf_counter()
                toks[mode] = ctx.transcribe_batch_device(d_pcm, a.clips, p)   # (ends in a stream synchronise)
                t1 = time.perf_counter()
                if i >= a.warmup:
                    res[mode]["decode_s"].append(ctx.timings()["decode_s"])
                    res[mode]["step_s"].append(t1 - t0)
    finally:
        hip.free(d_pcm)
    assert all(x.tolist() == y.tolist() for x, y in zip(toks["off"], toks["len0"]))
    assert all(toks["ragged"][i].tolist() == toks["off"][i].tolist() for i in range(0, a.clips, 7))   # the rows with an empty prefix
    out = {"clips": a.clips, "max_new_tokens": a.max_new_tokens, "precision": "bf16", "preset": "base", "positions_without_prefix": len(PROMPT) + a.max_new_tokens - 1}
    for mode in modes:
        out[mode] = {**res[mode], "decode_s_median": float(np.median(res[mode]["decode_s"])), "step_s_median": float(np.median(res[mode]["step_s"]))}
    out["step_spread_off_s"] = float(np.max(res["off"]["step_s"]) - np.min(res["off"]["step_s"]))
    out["len0_minus_off_s"] = out["len0"]["step_s_median"] - out["off"]["step_s_median"]
    out["per_prefix_position_s"] = {"from_32": (out["len32"]["decode_s_median"] - out["len0"]["decode_s_median"]) / 32,
                                    "from_224": (out["len224"]["decode_s_median"] - out["len0"]["decode_s_median"]) / 224}
    out["per_generated_position_s"] = out["off"]["decode_s_median"] / out["positions_without_prefix"]
    out["ragged_minus_off_s"] = out["ragged"]["step_s_median"] - out["off"]["step_s_median"]
    if "prefixes_off_vs_parent" in old:
        out["prefixes_off_vs_parent"] = old["prefixes_off_vs_parent"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
