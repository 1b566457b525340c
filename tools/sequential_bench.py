"""Cost of sequential long-form (wh_files_load / wh_transcribe_windows).  Records, with no threshold, for whisper-base bf16 and a
set of --files synthetic files of --minutes minutes each:

  sequential   the lockstep loop (tests/seq_ref.py run_sequential driven over Context.transcribe_windows, each row's text so far as its
               prefix): the load of the file set, windows decoded, steps, wall clock, x real time, windows per second, and per step the rows,
               the window-cut kernel's time beside the encoder's and the token loop's, and the longest prefix of the step;
  fixed        the same files one after the other through wh_transcribe_longform (30 s windows every 25 s): windows, wall clock, x real time,
               windows per second.

The synthetic model's logits are flat, so where its timestamps fall — and with them the advances and the number of windows — is arbitrary:
windows per second compares the two paths, x real time does not.

    python tools/sequential_bench.py [--files 32] [--minutes 4] [--max-new-tokens 32]

Writes profiles/sequential_bench.json (--out) and prints it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import seq_ref  # noqa: E402
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402

PROMPT, EOT, TB, NOTS, SOT_PREV = [50258, 50259, 50359], 50257, 50364, 50363, 50361


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "sum": float(np.sum(v)), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=32)
    ap.add_argument("--minutes", type=float, default=4.0)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sequential_bench.json"))
    a = ap.parse_args()
    n = int(a.minutes * 60 * 16000)
    clips = [ms.synth_clip(5000 + k) for k in range(8)]
    files = [np.resize(np.concatenate(clips[k % 8:] + clips[:k % 8]), n + 1600 * k).astype(np.float32) for k in range(a.files)]   # lengths differ a little: the files finish at different steps
    audio_s = sum(f.size for f in files) / 16000.0
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.files)
    ctx.set_timestamp_rules(TB, NOTS, 50)
    p = wb.DecodeParams(PROMPT, a.max_new_tokens, EOT)
    out = {"preset": "base", "precision": "bf16", "files": a.files, "minutes_per_file": a.minutes, "audio_s": audio_s, "max_new_tokens": a.max_new_tokens,
           "mel_store_bytes": int(sum(80 * 4 * ((wb.load_library().wh_mel_frames(f.size) + 15) // 16 * 16) for f in files))}
    ctx.transcribe_longform(files[0][:800000], p)       # warm both paths' kernels
    res = {}
    for run in range(2):                                # the second run is the one kept
        steps = []
        t0 = time.perf_counter()
        frames = ctx.files_load(files)
        load_s = time.perf_counter() - t0
        load_kernel_s = ctx.timings()["preprocess_s"]

        def step(rows):
            ctx.set_prefixes([r["prefix"] for r in rows])
            ts = time.perf_counter()
            toks = ctx.transcribe_windows([(r["file"], r["seek"]) for r in rows], p)
            tm = ctx.timings()
            steps.append({"rows": len(rows), "call_s": time.perf_counter() - ts, "window_cut_s": tm["preprocess_s"], "encode_s": tm["encode_s"], "decode_s": tm["decode_s"],
                          "longest_prefix": max(len(r["prefix"]) for r in rows),
                          "positions": max(len(r["prefix"]) for r in rows) + len(PROMPT) + a.max_new_tokens - 1})
            return [{"tokens": t[len(PROMPT):].tolist()} for t in toks]

        r = seq_ref.run_sequential(frames, step, TB, EOT, SOT_PREV, 448, len(PROMPT), a.max_new_tokens)
        wall = time.perf_counter() - t0
        ctx.clear_prefixes()
        windows = sum(len(f["windows"]) for f in r["files"])
        adv = [w["advance"] for f in r["files"] for w in f["windows"]]
        res = {"files_load_s": load_s, "files_load_kernels_s": load_kernel_s, "windows": windows, "steps": len(steps), "wall_s": wall, "x_real_time": audio_s / wall,
               "windows_per_s": windows / wall, "advance_frames": stats(adv), "full_window_advances": int(sum(1 for f in r["files"] for w in f["windows"] if w["advance"] == w["seg_frames"])),
               "rows_per_step": stats([s["rows"] for s in steps]), "step_call_s": stats([s["call_s"] for s in steps]),
               "window_cut_us_per_step": stats([s["window_cut_s"] * 1e6 for s in steps]), "encoder_ms_per_step": stats([s["encode_s"] * 1e3 for s in steps]),
               "token_loop_ms_per_step": stats([s["decode_s"] * 1e3 for s in steps]), "longest_prefix_per_step": stats([s["longest_prefix"] for s in steps]),
               "decoder_positions_per_step": stats([s["positions"] for s in steps]),
               "full_rows_steps": [s for s in steps if s["rows"] == a.files][:3]}
    out["sequential"] = res
    for run in range(2):
        t0 = time.perf_counter()
        windows, enc, dec = 0, 0.0, 0.0
        for f in files:
            windows += len(ctx.transcribe_longform(f, p, 30.0, 5.0))
            tm = ctx.timings()
            enc += tm["encode_s"]
            dec += tm["decode_s"]
        wall = time.perf_counter() - t0
        out["fixed"] = {"windows": windows, "wall_s": wall, "x_real_time": audio_s / wall, "windows_per_s": windows / wall, "encode_s": enc, "decode_s": dec,
                        "windows_per_call": windows / len(files)}
    ctx.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
