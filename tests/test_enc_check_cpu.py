"""tools/enc_check --selftest on the host (no GPU, no HIP call): the bounds the encoder kernel check applies are shown to hold for the contract
carried out in the kernels' working precision, and to bite — every listed defect must exceed them on at least one element."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFECTS = [
    # GEMM
    "the last k-step dropped",
    "bias indexed by row instead of column",
    "the last 4-column group not written",
    "m_per ignored in the row addressing",
    "the consumer using the neighbouring row's {mean, rstd}",
    "a stats partial missing its last column",
    # attention
    "the padded keys of the last tile unmasked",
    "the rescale factor omitted where the maximum rises",
    "keys 4..7 and 16..19 exchanged in V^T only",
    "one lane group's share of the row sum left out",
    # LayerNorm
    "variance as E[x^2] - mean^2 in f32 on the mean-25 rows",
    "the second row of a pair written to the first row's place",
]


def test_enc_check_selftest():
    exe = os.path.join(ROOT, "tools", "enc_check")
    assert os.path.exists(exe), f"{exe} missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    clean = [ln for ln in lines if " clean: " in ln]
    assert {ln.split()[1] for ln in clean} == {"gemm", "attention", "layernorm"}, r.stdout
    assert "MISMATCH" not in r.stdout and "NOT CAUGHT" not in r.stdout, r.stdout
    assert all(ln.rstrip().endswith("ok") for ln in clean), r.stdout
    for d in DEFECTS:
        hit = [ln for ln in lines if " defect: " in ln and d in ln]
        assert len(hit) == 1 and hit[0].rstrip().endswith("caught"), (d, r.stdout)
    assert lines[-1] == "selftest passed", r.stdout
