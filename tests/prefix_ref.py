"""Per-clip prompt prefixes: the shared inputs of tests/test_prefix_gpu.py and the Python restatement of the host's
prefix rule (openai-whisper decoding.py _get_initial_tokens) that tests/test_prefix_cpu.py holds whh_build_prefix against."""
import numpy as np

# the smallest lengths that cross the self-attention kernel's boundaries: lane ownership at keys 64 and 128, the strided tail from
# key 128, the V prefetch groups of 32 rows (f32) and 64 rows (bf16); row i of a batch has length LENS[i % 7]
LENS = (0, 1, 63, 64, 65, 129, 140)
NEW = 8


def prefixes(vocab: int):
    """One prefix per length of LENS, drawn in that order from one generator."""
    rng = np.random.default_rng(5)
    return [[int(t) for t in rng.integers(10, vocab - 400, n)] for n in LENS]


def build_prev_prefix(history, sot_prev: int, n_text_ctx: int):
    """[<|startofprev|>] ++ the last n_text_ctx // 2 - 1 ids of the history; no history, no prefix."""
    history = [int(t) for t in history]
    if not history:
        return []
    keep = n_text_ctx // 2 - 1
    return [int(sot_prev)] + (history[-keep:] if keep > 0 else [])
