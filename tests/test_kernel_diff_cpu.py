"""tools/kernel_diff.py on three builds of a ten-line kernel file (cross-compiled for gfx950, no GPU): the same source compiled twice is
"all identical"; with one constant changed and a kernel added, exactly the changed kernel differs and the added one is only in NEW."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "kernel_diff.py")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SRC = """#include <hip/hip_runtime.h>
namespace {
__global__ void k_scale(float* x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] *= %s;
}
__global__ void k_fill(int* x, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) x[i] = 7;
}
%s}
void launch(float* x, int* y, int n) { hipLaunchKernelGGL(k_scale, dim3(1), dim3(64), 0, 0, x, n); hipLaunchKernelGGL(k_fill, dim3(1), dim3(64), 0, 0, y, n); %s}
"""
ADDED = "__global__ void k_added(int* x) { x[threadIdx.x] = 1; }\n"


@pytest.fixture(scope="module")
def objs(tmp_path_factory):
    d = tmp_path_factory.mktemp("kernel_diff")
    out = {}
    for name, text in (("a", SRC % ("3.0f", "", "")), ("b", SRC % ("3.0f", "", "")),
                       ("c", SRC % ("5.0f", ADDED, "hipLaunchKernelGGL(k_added, dim3(1), dim3(64), 0, 0, y); "))):
        src, obj = d / (name + ".hip"), d / (name + ".o")
        src.write_text(text)
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-c", str(src), "-o", str(obj)], check=True, timeout=300)
        out[name] = str(obj)
    return out


def run(old, new):
    r = subprocess.run([sys.executable, TOOL, old, new], capture_output=True, text=True, timeout=120)
    print(r.stdout, r.stderr)
    return r


def test_same_source_twice_is_identical(objs):
    r = run(objs["a"], objs["b"])
    assert r.returncode == 0
    assert "identical: 2  differing: 0  only in OLD: 0  only in NEW: 0" in r.stdout
    assert r.stdout.rstrip().endswith("all identical")


def test_changed_and_added_kernels_are_named(objs):
    r = run(objs["a"], objs["c"])
    assert r.returncode != 0
    lines = r.stdout.splitlines()
    assert "identical: 1  differing: 1  only in OLD: 0  only in NEW: 1" in lines
    named = [ln for ln in lines if ln.startswith(("differs", "only in"))]
    assert len(named) == 2
    assert named[0].startswith("differs (code)") and "k_scale" in named[0]
    assert named[1].startswith("only in NEW:") and "k_added" in named[1]
    assert "all identical" not in r.stdout
    # and the other way round: the added kernel is then only in OLD
    r = run(objs["c"], objs["a"])
    assert r.returncode != 0
    assert "identical: 1  differing: 1  only in OLD: 1  only in NEW: 0" in r.stdout.splitlines()
