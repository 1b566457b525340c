"""Cost of the raw-audio ingest (wh_transcribe_batch_raw*, whisper_bench --gpu-ingest).  Records, with no threshold:

  kernel   the ingest kernel at --clips clips x 30 s for 16 kHz mono S16 and 48 kHz stereo S16: one wh_transcribe_batch_raw call stages the
           batch, then wh_debug_ingest_times launches the conversion again between HIP events (warm; median, min and max of --reps launches),
           beside the log-mel kernels' time of the same process (wh_transcribe_batch_device under wh_profile_enable) and the bytes per second
           the launch time implies (raw bytes read once + f32 rows written) against the 8 TB/s of HBM;
  host     samples per second of one load_audio_16k_mono thread (libwh_host.so's whh_load_wav) on a 30 s 48 kHz stereo S16 file;
  cli      whisper_bench over --files thirty-second 48 kHz stereo S16 WAVs with and without --gpu-ingest, same build, same files, --runs runs
           each alternating, every wall clock kept.  The files are hard links to 8 distinct contents (copies where links are refused): the
           loaders read every file from the page cache either way.

    python tools/ingest_bench.py [--clips 2048] [--files 2048] [--runs 3] [--skip-cli]

Writes profiles/ingest_bench.json (--out) and prints it."""
import argparse
import ctypes as C
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import audio_ref as ar  # noqa: E402
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402

PROMPT, EOT = [50258, 50259, 50359, 50363], 50257
HBM_BYTES_PER_S = 8.0e12
CLI = os.path.join(ROOT, "whisper-rust-ort_amd", "whisper_bench")


def s16_clip(k, channels, rate):
    n = 30 * rate
    src = np.resize(ms.synth_clip(3000 + k), n).astype(np.float32)
    chans = np.stack([src * np.float32(1.0 - 0.3 * c) for c in range(channels)], axis=1)
    return np.clip(np.round(chans * 32767.0), -32768, 32767).astype(np.int16)


def stats(v):
    v = [float(x) for x in v]
    return {"median": float(np.median(v)), "min": min(v), "max": max(v), "n": len(v)}


def kernel_times(a):
    model = wb.Model("synthetic:base:1234", 0, wb.WH_PREC_BF16)
    ctx = wb.Context(model, a.clips)
    ctx.lib.wh_debug_ingest_times.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_float)]
    p = wb.DecodeParams(PROMPT, 1, EOT)
    out = {}
    for name, ch, rate in (("s16_mono_16k", 1, 16000), ("s16_stereo_48k", 2, 48000)):
        x = s16_clip(0, ch, rate)
        clips = [(x, rate)] * a.clips            # one host array, a.clips descriptors: every clip is copied to its own staging offset
        t0 = time.perf_counter()
        ctx.transcribe_batch_raw(clips, p)
        call_s = time.perf_counter() - t0
        tm = ctx.timings()
        us = (C.c_float * (a.reps + 5))()
        ctx._check(ctx.lib.wh_debug_ingest_times(ctx.h, a.reps + 5, us))
        warm = list(us)[5:]
        raw_bytes, out_bytes = a.clips * x.nbytes, a.clips * 480000 * 4
        med = float(np.median(warm))
        out[name] = {"ingest_us": stats(warm), "raw_bytes": raw_bytes, "pcm_bytes_written": out_bytes,
                     "implied_bytes_per_s": (raw_bytes + out_bytes) / (med * 1e-6), "share_of_hbm_roof": (raw_bytes + out_bytes) / (med * 1e-6) / HBM_BYTES_PER_S,
                     "staging_call_s": call_s, "staging_call_h2d_s": tm["h2d_s"], "staging_call_preprocess_s": tm["preprocess_s"],
                     "f32_h2d_bytes_of_the_host_path": out_bytes}
    # the log-mel kernels of the same process, PCM resident
    hip = wb.HipRuntime()
    d_pcm = hip.upload(0, np.ascontiguousarray(np.tile(ms.synth_clip(3000), (a.clips, 1))))
    mel = []
    try:
        ctx.profile_enable(["mel"])
        for i in range(6):
            ctx.transcribe_batch_device(d_pcm, a.clips, p)
            if i:
                mel.append(ctx.profile_get()["mel"]["ms"] * 1e3)
        ctx.profile_enable(False)
    finally:
        hip.free(d_pcm)
    out["log_mel_us"] = stats(mel)
    for name in ("s16_mono_16k", "s16_stereo_48k"):
        out[name]["ingest_over_log_mel"] = out[name]["ingest_us"]["median"] / out["log_mel_us"]["median"]
    ctx.close()
    return out


def host_loader_rate(tmp):
    H = C.CDLL(os.path.join(ROOT, "whisper-rust-ort_amd", "libwh_host.so"))
    H.whh_load_wav.argtypes = [C.c_char_p, C.POINTER(C.c_float), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_double)]
    path = os.path.join(tmp, "rate.wav")
    ar.write_wav(path, s16_clip(1, 2, 48000), 48000)
    buf = np.zeros(480000, np.float32)
    n, dur = C.c_size_t(), C.c_double()
    ts = []
    for i in range(9):
        t0 = time.perf_counter()
        rc = H.whh_load_wav(path.encode(), buf.ctypes.data_as(C.POINTER(C.c_float)), buf.size, C.byref(n), C.byref(dur))
        ts.append(time.perf_counter() - t0)
        assert rc == 0 and n.value == 480000
    ts = ts[1:]
    med = float(np.median(ts))
    return {"file": "30 s, 48 kHz, stereo, S16", "load_s": stats(ts), "source_frames_per_s": 1440000 / med, "output_samples_per_s": 480000 / med,
            "x_real_time_one_thread": 30.0 / med}


def cli_runs(a, tmp):
    adir = os.path.join(tmp, "audio")
    os.makedirs(adir)
    t0 = time.perf_counter()
    linked = True
    for k in range(8):
        ar.write_wav(os.path.join(adir, f"clip_{k:04d}.wav"), s16_clip(10 + k, 2, 48000), 48000)
    for k in range(8, a.files):
        src, dst = os.path.join(adir, f"clip_{k % 8:04d}.wav"), os.path.join(adir, f"clip_{k:04d}.wav")
        try:
            os.link(src, dst)
        except OSError:
            linked = False
            shutil.copyfile(src, dst)
    write_s = time.perf_counter() - t0
    res = {"host": [], "gpu_ingest": []}
    texts = {}
    for run in range(a.runs):
        for tag, flags in (("host", []), ("gpu_ingest", ["--gpu-ingest"])):
            out = os.path.join(tmp, f"{tag}_{run}")
            t0 = time.perf_counter()
            r = subprocess.run([CLI, "--audio-dir", adir, "--onnx-dir", "synthetic:base:1234", "--precision", "bf16", "--max-batch", str(a.files),
                                "--max-new-tokens", str(a.max_new_tokens), "--out-csv", os.path.join(out, "p.csv"), "--out-json", os.path.join(out, "p.json"),
                                "--out-summary-json", os.path.join(out, "s.json")] + flags, capture_output=True, text=True, timeout=900)
            wall = time.perf_counter() - t0
            if r.returncode != 0:
                raise RuntimeError(r.stderr[-2000:])
            s = json.load(open(os.path.join(out, "s.json")))
            res[tag].append({"process_wall_s": wall, "file_loop_wall_s": s["gpu"]["wall_s"], "throughput_rtfx": s["gpu"]["throughput_rtfx"],
                             "gpu_busy_s": s["gpu"]["gpu_busy_s"], "load_s_median": s["breakdown_s"]["load_s"]["median"]})
            texts[tag] = [x["text"] for x in json.load(open(os.path.join(out, "p.json")))]
            shutil.rmtree(out)
    return {"files": a.files, "max_batch": a.files, "max_new_tokens": a.max_new_tokens, "hard_links": linked, "write_files_s": write_s,
            "bytes_per_file": 44 + 1440000 * 4, "runs": res, "texts_identical": texts["host"] == texts["gpu_ingest"],
            "file_loop_wall_s_median": {k: float(np.median([x["file_loop_wall_s"] for x in v])) for k, v in res.items()},
            "h2d_bytes_per_file": {"host": 480000 * 4, "gpu_ingest": 1440000 * 4}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=2048)
    ap.add_argument("--files", type=int, default=2048)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--max-new-tokens", type=int, default=32)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_bench.json"))
    a = ap.parse_args()
    out = {"clips": a.clips, "preset": "base", "precision": "bf16"}
    tmp = tempfile.mkdtemp(prefix="ingest_bench_")
    try:
        out["host_loader"] = host_loader_rate(tmp)
        out["kernel"] = kernel_times(a)
        if not a.skip_cli:
            out["cli"] = cli_runs(a, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
