"""The free-running halves of the token loop: the two row ranges of a split call run whole positions — layers, LM head, finish —
each on its own stream with its own device-side position, ordered by two events per position and joined only where the host needs the whole
batch.  A row must compute what it computes in the one chain, so every comparison here is exact: token rows and token counts equal to the one
chain's on the same context — free against joined against one chain, with the captured graphs and launched eagerly (WH_NO_GRAPH), on a fresh
and on a used context, on the encoder states and on the projected K / V.  whisper-base dims, synthetic weights, EOT suppressed.

Twenty new tokens: the loop's nineteen positions pass one poll of the done flags, which is one join and one resume.  Batches as in
test_step_split_gpu.py: 2 rows (1 + 1), 7 rows (4 + 3), 65 rows (64 + 1) on contexts of 96 clips (slab pitch 128).  The LM-head tile kernel
takes 256 rows and more: a 520-clip context (pitch 576) runs 256 + 256 (both ranges on k_lm_head_tile) and 512 + 8 (k_lm_head_tile and
k_lm_head, whose partial counts differ).  Run with -m gpu."""
import numpy as np
import pytest

from test_timestamps_gpu import setup
from whisper_rust_ort_amd import binding as wb
from whisper_rust_ort_amd import modelspec as ms

pytestmark = pytest.mark.gpu

NEW = 20
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


def hook(ctx, r0, free):
    ctx.debug_set_step_split(r0)
    ctx.debug_set_step_free(free)


def resident(ctx, new=NEW):
    """One decode of the resident clips: (token rows — their lengths are the token counts —, step_split, step_free)."""
    toks, _ = ctx.greedy_decode_resident_batch(params(new))
    return [t.tolist() for t in toks], ctx.step_split, ctx.step_free


@pytest.mark.parametrize("no_graph", [False, True], ids=["graph", "no_graph"])
@pytest.mark.parametrize("cross_es", [True, False], ids=["encoder_states", "kv"])
@pytest.mark.parametrize("n,r0", [(2, 1), (7, 4), (65, 64)])
def test_free_halves_equal_the_joined_split_and_the_one_chain(model, clips, monkeypatch, n, r0, cross_es, no_graph):
    if no_graph:
        monkeypatch.setenv("WH_NO_GRAPH", "1")   # read when the context is created
    ctx = wb.Context(model, MAX_BATCH, cross_es=cross_es)
    assert ctx.cross_mode == (1 if cross_es else 0)
    hook(ctx, r0, True)
    fresh = [t.tolist() for t in ctx.transcribe_batch(clips[:n], params())]   # the first decode of the context runs free
    assert (ctx.step_split, ctx.step_free) == (r0, 1)
    assert all(len(t) == len(params().prompt) + NEW for t in fresh)
    hook(ctx, r0, False)
    assert resident(ctx) == (fresh, r0, 0)       # the joined two-branch step
    hook(ctx, 0, False)
    assert resident(ctx) == (fresh, 0, 0)        # the one chain: it moves element 0 of the counters alone
    hook(ctx, r0, True)
    assert resident(ctx) == (fresh, r0, 1)       # free again on the used context: the second range's counter and ticket are re-armed
    hook(ctx, 0, True)
    assert resident(ctx) == (fresh, 0, 0)        # no split: nothing to run free
    ctx.close()
    plain = wb.Context(model, MAX_BATCH, cross_es=cross_es)   # ... and a context that never heard of the hooks
    assert [t.tolist() for t in plain.transcribe_batch(clips[:n], params())] == fresh
    assert (plain.step_split, plain.step_free) == (0, 0)
    plain.close()


def test_ranges_on_the_lm_head_tile_kernel(model, clips):
    """512 rows as 256 + 256: both ranges' LM heads are k_lm_head_tile launches; 520 rows as 512 + 8: the first range's is, the second's is a
    k_lm_head launch with another partial count.  Rows are independent, so eight clips repeated serve."""
    new = 12
    ctx = wb.Context(model, 520)
    assert ctx.cross_mode == 1
    batch = [clips[i % 8] for i in range(520)]
    for n, r0 in ((512, 256), (520, 512)):
        hook(ctx, r0, True)
        free = [t.tolist() for t in ctx.transcribe_batch(batch[:n], params(new))]
        assert (ctx.step_split, ctx.step_free) == (r0, 1)
        assert all(len(t) == len(params().prompt) + new for t in free)
        hook(ctx, 0, False)
        assert resident(ctx, new) == (free, 0, 0)
        assert free[8:] == [free[i % 8] for i in range(8, n)]
    ctx.close()


def option_result(ctx, opt, some_clips):
    toks = [t.tolist() for t in ctx.transcribe_batch(some_clips, params())]
    if opt == "beam":
        extra = [[(h["tokens"].tolist(), np.float32(h["sum_logprob"]).tobytes()) for h in c] for c in ctx.beams()]
    elif opt == "align":
        frames, n_frames = ctx.token_frames()
        extra = ([f.tolist() for f in frames], n_frames.tolist())
    elif opt == "logprobs":
        extra = [np.asarray(x, np.float32).tobytes() for x in ctx.logprobs()[0]]
    else:
        extra = None
    return toks, extra


@pytest.mark.parametrize("opt,split", [("rules", 2), ("logprobs", 2), ("repetition", 2), ("beam", 0), ("sample", 0), ("align", 0), ("prefix", 0)])
def test_other_keys_do_not_run_free(model, clips, opt, split):
    """Timestamp rules, log-probabilities and repetition controls carry per-row buffers that do not follow a range: with both hooks on they run
    the joined split.  Beam search, sampling, alignment copies and non-empty prefixes run one chain, as without the free hook.  Every call
    returns what a context without the hooks returns."""
    n = 4
    _, _, tb, nots = setup("base")

    def put(ctx):
        if opt == "rules":
            ctx.set_timestamp_rules(tb, nots, 50)
        elif opt == "logprobs":
            ctx.set_logprobs(-1, 0)
        elif opt == "repetition":
            ctx.set_repetition(1.3, 3)
        elif opt == "beam":
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
    assert (ref_ctx.step_split, ref_ctx.step_free) == (0, 0)
    ref_ctx.close()
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    hook(ctx, 2, True)
    ctx.transcribe_batch(clips[:n], params())
    assert (ctx.step_split, ctx.step_free) == (2, 1)       # the plain key runs free here ...
    put(ctx)
    got = option_result(ctx, opt, clips[:n])
    assert (ctx.step_split, ctx.step_free) == (split, 0)   # ... and this one does not
    assert got == ref
    ctx.close()


def test_kept_logit_rows_do_not_run_free(model, clips):
    n, r0 = 7, 4
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    ctx.transcribe_batch(clips[:n], params())
    out = []
    for split, free in ((r0, True), (0, False)):
        hook(ctx, split, free)
        toks, lg = ctx.greedy_decode_resident_rows(params(), [0, r0 - 1, r0, n - 1])
        assert (ctx.step_split, ctx.step_free) == (split, 0)
        out.append(([t.tolist() for t in toks], [np.ascontiguousarray(x).tobytes() for x in lg]))
    assert out[0] == out[1]
    ctx.close()


def test_event_timed_positions_join_and_resume(model, clips):
    """Sampled live timing: every fourth position runs eagerly as the one chain on the whole batch, on element 0 of the counters — a join, a
    whole-batch position, the counter's copy and a resume each time, and once more where the done flags are polled."""
    n, r0 = 7, 4
    ctx = wb.Context(model, MAX_BATCH, cross_es=True)
    hook(ctx, r0, True)
    ref = [t.tolist() for t in ctx.transcribe_batch(clips[:n], params())]
    assert (ctx.step_split, ctx.step_free) == (r0, 1)
    ctx.profile_enable(["dec_cross_attn"], stride=4)
    assert resident(ctx) == (ref, r0, 1)
    assert ctx.profile_get()["dec_cross_attn"]["launches"] > 0
    ctx.profile_enable(False)
    assert resident(ctx) == (ref, r0, 1)
    hook(ctx, 0, False)
    assert resident(ctx) == (ref, 0, 0)
    ctx.close()
