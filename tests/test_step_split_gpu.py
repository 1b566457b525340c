"""The split token loop: a generated position runs the decoder layers of two row ranges of the batch as two branches.  A row
must compute what it computes in the one chain, so every comparison here is exact: tokens equal, kept logit rows bit for bit — split against
unsplit on the same context, with the captured graph and launched eagerly (WH_NO_GRAPH), on a fresh and on a used context, on the encoder
states and on the projected K / V.  whisper-base dims, synthetic weights, twelve new tokens (eleven positions run the split step).

Batches: 2 rows split 1 + 1, 7 rows split 4 + 3 (no multiple of anything), 65 rows split 64 + 1 (a row-group boundary of the decode GEMMs;
more than 64 rows also takes k_dec_gemm_wide).  The contexts hold 96 clips, so the slab pitch (128) covers the second range's row groups.
Run with -m gpu."""
import numpy as np
import pytest

from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

NEW = 12
MAX_BATCH = 96
SEED = 20240


@pytest.fixture(scope="module")
def model():
    if wb.device_count() < 1:
        pytest.fail("no MI355X visible: the GPU suite has no fallback")
    return wb.Model("synthetic:base:1234", 0, wb.PRECISIONS["bf16"])


@pytest.fixture(scope="module")
def clips():
    return [ms.synth_clip(1900 + i) for i in range(65)]


def params(new=NEW):
    prompt, eot, _, _ = setup("base")
    return wb.DecodeParams(prompt, new, eot, [eot])   # EOT suppressed: every row runs every position


def kept_rows(n, r0):
    """The rows whose logits are compared: the ends of both ranges."""
    return sorted({0, max(r0 - 1, 0), min(r0, n - 1), n - 1})


def resident(ctx, n, r0):
    """One decode of the resident clips: (tokens, kept logit rows as bytes, the split it ran with)."""
    toks, lg = ctx.greedy_decode_resident_rows(params(), kept_rows(n, r0))
    return [t.tolist() for t in toks], [np.ascontiguousarray(x).tobytes() for x in lg], ctx.step_split


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
@pytest.mark.parametrize("cross_es", [True, False], ids=["encoder_states", "kv"])
@pytest.mark.parametrize("n,r0", [(2, 1), (7, 4), (65, 64)])
def test_split_step_equals_the_one_chain(model, clips, monkeypatch, n, r0, cross_es, no_graph):
    if no_graph:
        monkeypatch.setenv("WH_NO_GRAPH", "1")   # read when the context is created
    ctx = wb.Context(model, MAX_BATCH, cross_es=cross_es)
    assert ctx.cross_mode == (1 if cross_es else 0)
    ctx.debug_set_step_split(r0)
    fresh = [t.tolist() for t in ctx.transcribe_batch(clips[:n], params())]   # the first decode of the context runs split
    assert ctx.step_split == r0
    assert all(len(t) == len(params().prompt) + NEW for t in fresh)
    used = resident(ctx, n, r0)
    assert used[2] == r0 and used[0] == fresh
    ctx.debug_set_step_split(0)
    one = resident(ctx, n, r0)                   # the same context, one chain: the step is captured again under the other key
    assert one[2] == 0
    assert one[0] == used[0]
    assert one[1] == used[1]
    ctx.debug_set_step_split(r0)
    again = resident(ctx, n, r0)
    assert again == used
    ctx.close()
    plain = wb.Context(model, MAX_BATCH, cross_es=cross_es)   # ... and a context that never heard of the hook
    assert [t.tolist() for t in plain.transcribe_batch(clips[:n], params())] == fresh
    assert plain.step_split == 0
    plain.close()


def test_the_step_is_keyed_on_the_split(model, clips):
    """One context walked through split sizes, the hook off in between: every call reports its split and returns the same bits."""
    n = 7
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    ctx.transcribe_batch(clips[:n], params())
    assert ctx.step_split == 0
    ref = resident(ctx, n, 4)
    for r0 in (4, 0, 3, 6, 0, 1, 4):
        ctx.debug_set_step_split(r0)
        got = resident(ctx, n, 4)
        assert got[2] == r0, r0
        assert got[:2] == ref[:2], r0
    for r0 in (7, 9):   # no second range: one chain
        ctx.debug_set_step_split(r0)
        assert resident(ctx, n, 4) == ref
    ctx.close()


def test_one_row_runs_one_chain(model, clips):
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    ctx.debug_set_step_split(1)
    a = [t.tolist() for t in ctx.transcribe_batch(clips[:1], params())]
    assert ctx.step_split == 0
    ctx.debug_set_step_split(0)
    assert [t.tolist() for t in ctx.transcribe_batch(clips[:1], params())] == a
    ctx.close()


def option_result(ctx, opt, clips4):
    p = params()
    toks = [t.tolist() for t in ctx.transcribe_batch(clips4, p)]
    if opt == "beam":
        extra = [[(h["tokens"].tolist(), np.float32(h["sum_logprob"]).tobytes()) for h in c] for c in ctx.beams()]
    elif opt == "align":
        frames, n_frames = ctx.token_frames()
        extra = ([f.tolist() for f in frames], n_frames.tolist())
    else:
        extra = None
    return toks, extra, ctx.step_split


@pytest.mark.parametrize("opt", ["beam", "sample", "align", "prefix"])
def test_other_keys_run_one_chain(model, clips, opt):
    """Beam search, sampling, alignment copies and non-empty per-clip prefixes fall back to the one chain: the call reports no split and
    returns what a context without the hook returns."""
    n = 4

    def put(ctx):
        if opt == "beam":
            ctx.set_beam_search(2, 1.0, -1.0, [0])
        elif opt == "sample":
            ctx.set_sampling(SEED, [0.7] * n)
        elif opt == "align":
            ctx.set_alignment([(0, 0), (1, 1)], debug_rows=[0])
        else:
            ctx.set_prefixes([[20 + 3 * b + i for i in range((0, 1, 5, 2)[b])] for b in range(n)])

    ref_ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    put(ref_ctx)
    ref = option_result(ref_ctx, opt, clips[:n])
    ref_ctx.close()
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    ctx.debug_set_step_split(2)
    ctx.transcribe_batch(clips[:n], params())
    assert ctx.step_split == 2          # the plain key splits here ...
    put(ctx)
    got = option_result(ctx, opt, clips[:n])
    assert got[2] == 0                  # ... and this one does not
    assert got == ref
    ctx.close()


def test_rules_logprobs_and_repetition_stay_split(model, clips):
    """What only acts behind the layers — timestamp rules, log-probabilities, repetition controls — runs split and returns the one chain's bits."""
    n, r0 = 7, 4
    _, _, tb, nots = setup("base")
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    ctx.set_timestamp_rules(tb, nots, 50)
    ctx.set_logprobs(-1, 0)
    ctx.set_repetition(1.3, 3)
    out = []
    for split in (r0, 0):
        ctx.debug_set_step_split(split)
        toks = [t.tolist() for t in ctx.transcribe_batch(clips[:n], params())]
        assert ctx.step_split == split
        lps, _ = ctx.logprobs()
        out.append((toks, [np.asarray(x, np.float32).tobytes() for x in lps]))
    assert out[0] == out[1]
    ctx.close()
