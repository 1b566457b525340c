"""The decoder self-attention's cache addressing: the V prefetch loads live rows only (the chunk-major K cache measured there was
not adopted).  Only addresses changed, so every result is the bit pattern it was:

  * tools/dec_attn_check self prints, per case, the hashes of out, kc and vc; they must be the lines profiles/dec_attn_check.txt records, which
    predate the change;
  * tools/dec_attn_check reorder: k_beam_reorder moves the caches the way the kernel that reads them expects;
  * end to end, a decode whose positions cross 64 and 128, plainly and with per-clip prefixes of 0 / 3 / 66 ids, on a used and on a fresh context."""
import os
import subprocess

import pytest

import prefix_ref as pr
from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "dec_attn_check")
RECORD = os.path.join(ROOT, "profiles", "dec_attn_check.txt")


@pytest.fixture(scope="module")
def gpu():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return 0


def run_group(group):
    assert os.path.exists(EXE), f"{EXE} missing: __graft_entry__.build() compiles it"
    r = subprocess.run([EXE, group], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "MISMATCH" not in r.stdout, r.stdout + r.stderr
    return r.stdout.splitlines()


def self_lines(lines):
    return [ln.rstrip() for ln in lines if ln.startswith("k_dec_self_attn") or ln.startswith("worst err/bound self")]


def test_self_lines_are_the_recorded_ones(gpu):
    """Every case of the self group — positions around each boundary in bf16, f32 and f16x3, the prefixed rows, the chain — prints the line the
    record holds: err/bound, guard, append and the three hashes."""
    with open(RECORD) as f:
        want = self_lines(f.read().splitlines())
    got = self_lines(run_group("self"))
    assert len(want) == 3 * (14 + 3 + 2 * 4) + 70 + 36 + 1, len(want)
    assert got == want, [(g, w) for g, w in zip(got, want) if g != w][:4]


def test_beam_reorder_then_self_attention(gpu):
    """k_beam_reorder alone: after it the self-attention leaves the out, kc and vc of a launch on caches permuted on the host."""
    lines = [ln for ln in run_group("reorder") if ln.startswith("reorder ")]
    assert len(lines) == 2 * 4 * 2, lines                        # bf16 and f32, g 1 / 64 / 65 / 130, the host's and the device's launch
    assert sum(ln.endswith("hashes equal") for ln in lines) == 8, lines
    assert all(" ok" in ln for ln in lines), lines


NEW = 140


@pytest.mark.parametrize("prec_name", ["bf16", "f32"])
def test_decode_across_64_and_128(gpu, prec_name):
    """micro, 4 clips, 140 new tokens.  A context decodes plainly, with per-clip prefixes of 0 / 3 / 66 ids (prefix_ref.build_prev_prefix of a
    history of 0 / 2 / 65 ids), and plainly again; a fresh context decodes with the prefixes first.  The same call gives the same tokens on
    both, whatever the caches held before, and every prefixed row is the row of the un-prefixed call whose prompt is prefix ++ prompt."""
    prompt, eot, tb, nots = setup("micro")
    dims = ms.PRESETS["micro"]
    P = len(prompt)
    hist = pr.prefixes(dims.vocab)[4]
    pre = [pr.build_prev_prefix(hist[:n], nots - 1, dims.n_text_ctx) for n in (0, 2, 65, 2)]
    assert [len(p) for p in pre] == [0, 3, 66, 3]
    clips = [ms.synth_clip(1500 + i) for i in range(4)]
    params = wb.DecodeParams(prompt, NEW, eot, [eot])

    def context():
        model = wb.Model("synthetic:micro:11", 0, wb.PRECISIONS[prec_name])
        return wb.Context(model, 4)

    def prefixed(ctx):
        ctx.set_prefixes(pre)
        out = ctx.transcribe_batch(clips, params)
        ctx.clear_prefixes()
        return [t.tolist() for t in out]

    a = context()
    plain = [t.tolist() for t in a.transcribe_batch(clips, params)]
    assert all(len(t) == P + NEW for t in plain)
    pref = prefixed(a)
    assert [t.tolist() for t in a.transcribe_batch(clips, params)] == plain
    b = context()
    assert prefixed(b) == pref
    assert [t.tolist() for t in b.transcribe_batch(clips, params)] == plain
    assert pref[0] == plain[0]                                   # an empty prefix
    for k in (1, 2):                                             # rows 1 and 3 share the prefix of 3 ids
        full = pre[k] + prompt
        ex, _ = b.greedy_decode_resident_batch(wb.DecodeParams(full, NEW, eot, [eot]))
        for r in (1, 3) if k == 1 else (2,):
            assert ex[r].tolist()[len(full):] == pref[r][P:], (k, r)
    a.close()
    b.close()
