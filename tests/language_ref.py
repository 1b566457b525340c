"""Language detection (wh_ctx_set_language_detection) restated in float64 on one position's logits: what the language finish kernel
computes from the language head's output, written without regard to speed."""
import numpy as np


def detect(logits, ids):
    """(chosen id, probs in list order) of one row.  logits: the unfiltered logits [vocab] of the position; ids: the listed token ids.

    NaN logits are left out (probability 0, never chosen); the chosen id is the listed id with the largest logit, ties to the lowest id
    (not the lowest list position); nothing finite (every listed logit NaN or -inf): the lowest listed id and all probabilities 0."""
    ids = [int(i) for i in ids]
    v = np.asarray(logits, np.float64)[ids]
    ok = ~np.isnan(v)
    if not ok.any() or v[ok].max() == -np.inf:
        return min(ids), np.zeros(len(ids), np.float64)
    m = v[ok].max()
    best = min(i for i, x, k in zip(ids, v, ok) if k and x == m)
    if m == np.inf:   # the limit: the +inf entries share the mass
        e = np.where(ok & (v == np.inf), 1.0, 0.0)
    else:
        e = np.where(ok, np.exp(np.where(ok, v, m) - m), 0.0)
    return best, e / e.sum()


def pick_ids(L, n_lang, pool=300):
    """The id list the GPU tests detect among, built from reference logits L [clips][vocab] (hash-seeded weights put one id on top for
    every clip, so the real language block would test nothing): among the `pool` ids of highest mean logit the pair whose order flips
    between clips with the largest worst-case gap, then n_lang - 2 fillers of smallest max-over-clips logit; returned unsorted, the
    fillers first and the higher id of the pair before the lower.  Also returns that worst-case gap."""
    L = np.asarray(L, np.float64)
    top = np.argsort(L.mean(0))[-pool:]
    D = L[:, top][:, :, None] - L[:, top][:, None, :]
    flips = (D > 0).any(0) & (D < 0).any(0)
    gap = np.where(flips, np.abs(D).min(0), -1.0)
    a, b = np.unravel_index(np.argmax(gap), gap.shape)
    assert n_lang >= 2 and gap[a, b] > 0, "no pair of ids changes order between the clips"
    pair = sorted((int(top[a]), int(top[b])), reverse=True)
    fill = [int(i) for i in np.argsort(L.max(0)) if int(i) not in pair][: n_lang - 2]
    return fill + pair, float(gap[a, b])
