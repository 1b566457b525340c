"""Builds libwhisper_hip.so (gfx950) in-tree with hipcc.  Used by __graft_entry__.build()."""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libwhisper_hip.so")
# the slowest first, so that the pool starts them first: wh_lm_head.hip (the 96 k_lm_head instantiations) bounds a clean build
SOURCES = ["wh_lm_head.hip", "wh_dec_gemm.hip", "wh_mel.hip", "wh_ingest.hip", "wh_gemm.hip", "wh_gemm8.hip", "wh_gemm8x.hip", "wh_gemm8_mx.hip", "wh_mlp.hip", "wh_attn.hip", "wh_dec_attn.hip", "wh_dec_tile.hip", "wh_cross_es.hip", "wh_cross_es8.hip", "wh_cross_es3.hip", "wh_fp8.hip", "wh_align.hip", "wh_beam.hip", "wh_sample.hip", "wh_score.hip", "wh_model.cpp", "wh_ctx.cpp", "wh_options.cpp", "wh_encode_host.cpp", "wh_decode_host.cpp", "wh_score_host.cpp", "wh_api.cpp"]
HEADERS = ["wh_common.h", "wh_es_common.h", "wh_dec_epilogue.h", "wh_kernels.h", "wh_lm_tile.h", "wh_internal.h", "wh_host_shared.h", "wh_step.h", "wh_ingest_desc.h", "wh_json.h", "../../include/whisper_hip.h"]
# -amdgpu-mfma-vgpr-form: MFMA accumulators live in VGPRs (gfx950's register file is unified).  With the default
# heuristic the attention kernel kept its score and output tiles in AGPRs and spent 160 of ~400 VALU instructions
# per key tile on v_accvgpr_read/write copies around the softmax.
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-pthread", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result",
         "-mllvm", "-amdgpu-mfma-vgpr-form=1", "-x", "hip"]


# wh_attn.hip: the softmax maxima never see a NaN that matters (a NaN score poisons its row either way); without
# this every fmaxf operand is canonicalised first (v_max_f32 x, x, x), which doubles the max instructions of a loop
# that is VALU-bound.  Infinities keep their meaning (-inf masks the tail keys).
EXTRA_FLAGS = {"wh_attn.hip": ["-fno-honor-nans"], "wh_cross_es.hip": ["-fno-honor-nans"], "wh_cross_es8.hip": ["-fno-honor-nans"], "wh_cross_es3.hip": ["-fno-honor-nans"]}   # (the same for the running maxima of wh_cross_es.hip)


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(verbose: bool = False, force: bool = False) -> str:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]

    def compile_one(src: str) -> str:
        s = os.path.join(CSRC, src)
        o = os.path.join(objdir, src + ".o")
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc] + FLAGS + EXTRA_FLAGS.get(src, []) + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
        return o

    with ThreadPoolExecutor(max_workers=min(6, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    if force or _stale(OUT, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", OUT] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    build_host(verbose, force)
    build_tools(verbose, force)
    return OUT


TOOLS = os.path.join(HERE, "..", "tools")


def build_tools(verbose: bool = False, force: bool = False) -> None:
    """Device-side check binaries the GPU tests run (tests/test_fp8_gpu.py, tests/test_hip_parity.py): the MX MFMA layout probe, the MX GEMM /
    LayerNorm kernels, the one-launch feed-forward block (k_enc_mlp) the alignment score kernels (tests/test_align_gpu.py) and the forced pass's query gather (tests/test_forced_align_gpu.py) against host restatements.  They include the library's kernel source directly."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for name, kernel_src in (("mx_mfma_check", "wh_gemm8_mx.hip"), ("mx_gemm_check", "wh_gemm8_mx.hip"), ("mlp_check", "wh_mlp.hip"), ("es16_check", "wh_cross_es.hip"), ("es8_check", "wh_cross_es8.hip"), ("es3_check", "wh_cross_es3.hip"), ("align_check", "wh_align.hip"), ("align_gather_check", "wh_align.hip")):
        src, exe = os.path.join(TOOLS, name + ".hip"), os.path.join(TOOLS, name)
        deps = [src, os.path.join(CSRC, kernel_src), os.path.join(CSRC, "wh_common.h"), os.path.join(CSRC, "wh_es_common.h"), os.path.join(CSRC, "wh_dec_epilogue.h"), os.path.join(CSRC, "wh_kernels.h")]
        if force or _stale(exe, deps):
            # the kernel source's own extra flags: a tool checks the kernel binary that ships
            cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-amdgpu-mfma-vgpr-form=1"] + EXTRA_FLAGS.get(kernel_src, []) + ["-w", "-I", CSRC, src, "-o", exe]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)
    # tools/dec_gemm_check (tests/test_hip_parity.py) calls the library's own launchers instead (wh_dec_gemm.hip, wh_dec_tile.hip): it links
    # libwhisper_hip.so, so it checks the kernels of whichever library it is built against; tools/enc_check (tests/test_hip_parity.py, tests/test_enc_check_cpu.py) does the same for
    # the encoder side: k_gemm8 / k_ln_stats, k_gemm8x, k_gemm, k_enc_attn, k_layernorm; tools/dec_attn_check (tests/test_hip_parity.py,
    # tests/test_dec_attn_check_cpu.py) for the decoder's attention: k_dec_self_attn, k_dec_cross_attn, k_dec_cross_attn_cg (wh_dec_attn.hip), k_kv_quant,
    # k_dec_cross_attn8 (wh_fp8.hip); tools/lm_check (tests/test_hip_parity.py, tests/test_lm_check_cpu.py) for the end of a decode step: k_lm_head,
    # k_argmax_finish, k_nospeech_finish, k_lang_head, k_lang_finish, k_dec_embed (wh_lm_head.hip) and the LM-head tile kernels (wh_gemm8.hip, wh_gemm8x.hip)
    for name in ("dec_gemm_check", "enc_check", "dec_attn_check", "lm_check"):
        src, exe = os.path.join(TOOLS, name + ".cpp"), os.path.join(TOOLS, name)
        if force or _stale(exe, [src, OUT, os.path.join(CSRC, "wh_kernels.h")]):
            cmd = [hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-w", src, "-o", exe, "-L" + HERE, "-lwhisper_hip", "-Wl,-rpath,$ORIGIN/../whisper-rust-ort_amd"]
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.check_call(cmd)


HOST = os.path.join(HERE, "host")
HOST_SO = os.path.join(HERE, "libwh_host.so")
CLI = os.path.join(HERE, "whisper_bench")


def build_host(verbose: bool = False, force: bool = False) -> None:
    """The host side above the C ABI (C++, because the reference's host is compiled Rust and Rust is
    not in this image): the CLI `whisper_bench` and `libwh_host.so` (host helpers for the tests)."""
    gxx = os.environ.get("CXX", "g++")
    # the temperature ladder's compression_ratio calls zlib, which the host code loads by its soname at the first use (dlopen("libz.so.1"):
    # the development symlink libz.so is not needed to link).  Python's own zlib module depends on the same soname.
    import ctypes
    try:
        ctypes.CDLL("libz.so.1")
    except OSError as e:
        raise RuntimeError(f"libz.so.1 is missing: whisper_bench --temperature and libwh_host.so's compression_ratio need zlib ({e})") from e
    hdr =[os.path.join(HOST, "wh_host.h"), os.path.join(HOST, "wh_unicode_lower.h"), os.path.join(CSRC, "wh_json.h"), os.path.join(HERE, "..", "include", "whisper_hip.h")]
    src = os.path.join(HOST, "wh_host_capi.cpp")
    if force or _stale(HOST_SO, [src] + hdr):
        cmd = [gxx, "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", HOST_SO, src, "-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    src = os.path.join(HOST, "whisper_bench.cpp")
    if force or _stale(CLI, [src, OUT] + hdr):
        cmd = [gxx, "-O2", "-std=c++17", "-Wall", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", CLI, src, "-L" + HERE, "-lwhisper_hip",
               "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib", "-L/opt/rocm/lib", "-lamdhip64", "-ldl"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)


if __name__ == "__main__":
    print(build(verbose=True, force="--force" in sys.argv))
