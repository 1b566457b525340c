"""Kernel launches per option state: a nano-f32 context with three clips is put through the states of both walks of
tests/test_step_graph_gpu.py with event timing on for every kernel group (every position is then launched eagerly), and the launches
each state's decode calls made are printed per group.  Two builds of the library launch the same kernels when their outputs are the same
line for line (profiles/ctx_options_launches.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import test_step_graph_gpu as sg  # noqa: E402
from whisper_rust_ort_amd import binding as wb  # noqa: E402
from whisper_rust_ort_amd import modelspec as ms  # noqa: E402

PRESET, SEED, N_CLIPS = "nano", 7, 3


def counted(ctx, acc):
    """The two decode entries the walks use, each adding its call's launches to acc."""
    def wrap(fn):
        def call(*a, **k):
            out = fn(*a, **k)
            for g, v in ctx.profile_get().items():
                acc[g] = acc.get(g, 0) + v["launches"]
            return out
        return call
    ctx.transcribe_batch = wrap(ctx.transcribe_batch)
    ctx.greedy_decode_resident_rows = wrap(ctx.greedy_decode_resident_rows)


def main():
    model = wb.Model(f"synthetic:{PRESET}:{SEED}", 0, wb.PRECISIONS["f32"])
    clips = [ms.synth_clip(1700 + i) for i in range(N_CLIPS)]
    walks = (("walk", N_CLIPS, sg.walk(N_CLIPS), sg.put, sg.decode),
             ("walk_options", 3 * N_CLIPS, sg.walk_options(PRESET, N_CLIPS), sg.put_options, sg.decode_options))
    for title, max_batch, states, put, decode in walks:
        ctx = wb.Context(model, max_batch)
        ctx.profile_enable()
        acc = {}
        counted(ctx, acc)
        for name, st in states:
            acc.clear()
            put(ctx, st, PRESET, False)
            decode(ctx, st, PRESET, clips)
            print(f"{title} | {name} | " + " ".join(f"{g}={acc[g]}" for g in wb.KG_NAMES), flush=True)
        ctx.close()


if __name__ == "__main__":
    main()
