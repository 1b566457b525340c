"""tools/lm_check --selftest on the host (no GPU, no HIP call): the bounds and exact conditions the LM-head / finish / language / embedding check
applies are shown to hold for the contracts carried out in the kernels' working precision and partial layout, and to bite — every listed defect
must exceed a bound or fail an exact condition on at least one case of the check's own list."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFECTS = [
    # the LM heads
    "1 gen 0 reads mask_base",
    "2 a tie kept by the higher index",
    "3 the nn < N guard dropped, so the clamped last weight row is counted again",
    "4 a suppressed id enters the sum of exp",
    "5 a tile that straddles ts_begin treated as text-only",
    "6 ts_hi taken as exclusive",
    "7 text below text_lo in the LP sum",
    "8 a touched id left in the partials",
    "9 the rep_side row pitch is 32 * rep_words instead of N",
    "10 lane-group sums added without rescaling to the row maximum",
    "11 a logits_sel of -1 stored to slot 0",
    "12 partials at pitch M instead of x_mpad",
    "13 LayerNorm statistics of the neighbouring row",
    # the finish kernels
    "14 finish: a tie between partials goes to the later one",
    "15 finish: partials past 2048 dropped",
    "16 rule 5 on the timestamp maximum instead of its log-sum-exp",
    "17 LP under rule 5 includes the text sum",
    "18 a positive logit multiplied by p",
    "19 a duplicated history id merged twice",
    "20 bans not cleared with the penalty off",
    "21 a done row records its token",
    "22 a forced EOT sets done",
    "23 no-speech: a -inf partial yields NaN",
    # language, embedding
    "24 language: a tie goes to the lowest list position",
    "25 language: src_row ignored",
    "26 embed PFX: position pos - off not clamped at 0",
    "27 the fused next embedding differs from k_dec_embed in the sum order",
    # the chain of both kernels on their own state
    "28 chain: the finish leaves the row state of the previous position",
]
GROUPS = ["head", "tile", "finish", "lang", "embed"]


def test_lm_check_selftest():
    exe = os.path.join(ROOT, "tools", "lm_check")
    assert os.path.exists(exe), f"{exe} missing: __graft_entry__.build() compiles it"
    r = subprocess.run([exe, "--selftest"], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert "MISMATCH" not in r.stdout and "NOT CAUGHT" not in r.stdout, r.stdout
    clean = [ln for ln in lines if ln.startswith("selftest ") and " clean: " in ln]
    assert [ln.split()[1] for ln in clean] == GROUPS, r.stdout
    for ln in clean:
        assert ln.rstrip().endswith("ok"), ln
        assert float(ln.split("err/bound")[1].split()[0]) < 1.0, ln   # the emulation stays inside every bound
    for d in DEFECTS:
        hit = [ln for ln in lines if " defect: " + d + "  " in ln]
        assert len(hit) == 1 and hit[0].rstrip().endswith("caught"), (d, r.stdout)
    assert any(ln.startswith("selftest worst err/bound of the emulation: head ") for ln in lines), r.stdout
    assert lines[-1] == "selftest passed", r.stdout
