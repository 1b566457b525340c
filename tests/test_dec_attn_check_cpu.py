"""tools/dec_attn_check --selftest on the host (no GPU, no HIP call): the bounds the decoder attention check applies are shown to hold for the
contracts carried out in the kernels' working precision and order of streams, and to bite — every listed defect must exceed them, or fail an
exact condition (append, guard, amax, codes), on at least one element."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFECTS = [
    # self-attention
    "1 the current key left out",
    "2 one cache row too many read (j <= pos)",
    "3 prefixes: adv ignored",
    "4 a masked V row multiplied in, not selected out",
    "5 the append at the local row",
    # cross-attention
    "6 the clamped tail key counted",
    "7 waves merged without exp(m - M)",
    "8 the denominator from the neighbouring head",
    "9 an empty wave's -inf not skipped",
    "10 _cg: the odd-parity stream dropped",
    "11 beam: kvb = b",
    "12 the slab indexed with pitch B instead of mpad",
    # fp8
    "13 fp8: K's scale not applied",
    "14 fp8: V's scale from head 0",
    "15 fp8: amax off by one row at a workgroup boundary",
]


def test_dec_attn_check_selftest():
    exe = os.path.join(ROOT, "tools", "dec_attn_check")
    assert os.path.exists(exe), f"{exe} missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    clean = [ln for ln in lines if " clean: " in ln]
    assert {ln.split()[1] for ln in clean} == {"self", "cross", "cross8"}, r.stdout
    assert "MISMATCH" not in r.stdout and "NOT CAUGHT" not in r.stdout and "DIFFERENT" not in r.stdout, r.stdout
    assert all(ln.rstrip().endswith("ok") for ln in clean), r.stdout
    for d in DEFECTS:
        hit = [ln for ln in lines if " defect: " in ln and " " + d + "  " in ln]
        assert len(hit) == 1 and hit[0].rstrip().endswith("caught"), (d, r.stdout)
    assert any(ln.startswith("selftest worst err/bound of the emulation: self ") for ln in lines), r.stdout
    assert lines[-1] == "selftest passed", r.stdout
