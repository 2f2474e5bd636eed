"""Numpy restatements for the heat-map score ranks (csrc/percentile.hip), written from their definitions: the two
counts by comparing every query with every reference value, and both percentile formulas from the counts in the order of operations
of scipy 1.15 (``rankdata(x, 'average') / len(x) * 100``, wsi_core/wsi_utils.py:124-127; ``percentileofscore(ref, q)`` with kind
'rank', vis_utils/heatmap_utils.py:22-24).  tests/test_heatmap_scores_host.py holds them against scipy itself; the GPU tests compare
the kernel with them bit for bit.  ``sample_rois_ref`` restates wsi_core/wsi_utils.py:102-158 with these ranks.
"""
import numpy as np

RANKDATA, OF_SCORE = 0, 1


def counts(q, ref, chunk=2048):
    """(less, leq) int64 [len(q)]: #{ref < q[i]} and #{ref <= q[i]}, by brute force in chunks of queries."""
    q = np.asarray(q, dtype=np.float64).reshape(-1)
    ref = np.asarray(ref, dtype=np.float64).reshape(-1)
    less = np.zeros(len(q), dtype=np.int64)
    leq = np.zeros(len(q), dtype=np.int64)
    for a in range(0, len(q), chunk):
        qq = q[a:a + chunk, None]
        less[a:a + chunk] = (ref[None] < qq).sum(1)
        leq[a:a + chunk] = (ref[None] <= qq).sum(1)
    return less, leq


def pct_from_counts(less, leq, nref, mode):
    less = np.asarray(less, dtype=np.int64)
    leq = np.asarray(leq, dtype=np.int64)
    if mode == RANKDATA:
        return (0.5 * (less + leq + 1)) / nref * 100
    return (less + leq + (less < leq)) * (50.0 / nref)


def percentiles(q, ref, mode):
    less, leq = counts(q, ref)
    return pct_from_counts(less, leq, np.asarray(ref).size, mode)


def score2percentile_loop_f32(scores, ref):
    """The reference's loop (vis_utils/heatmap_utils.py:73-77): a float32 column, each entry replaced by its percentile."""
    a = np.array(scores, dtype=np.float32).reshape(-1, 1)
    ref = np.asarray(ref)
    for i in range(len(a)):
        a[i] = percentiles(a[i], ref, OF_SCORE)
    return a


def sample_rois_ref(scores, coords, k=5, mode="range_sample", seed=1, score_start=0.45, score_end=0.55, top_left=None, bot_right=None):
    """wsi_core/wsi_utils.py:137-158 with sample_indices (:102-115), top_k (:117-122) and screen_coords (:129-135) written out."""
    if len(scores.shape) == 2:
        scores = scores.flatten()
    scores = percentiles(scores, scores, RANKDATA)
    if top_left is not None and bot_right is not None:
        mask = np.logical_and(np.all(coords >= np.array(top_left), axis=1), np.all(coords <= np.array(bot_right), axis=1))
        scores = scores[mask]
        coords = coords[mask]
    if mode == "range_sample":
        np.random.seed(seed)
        window = np.logical_and(scores >= score_start, scores <= score_end)
        indices = np.where(window)[0]
        if len(indices) < 1:
            sampled_ids = -1
        else:
            sampled_ids = np.random.choice(indices, min(k, len(indices)), replace=False)
    elif mode == "topk":
        sampled_ids = scores.argsort()[::-1][:k]
    elif mode == "reverse_topk":
        sampled_ids = scores.argsort()[:k]
    else:
        raise NotImplementedError
    return {"sampled_coords": coords[sampled_ids], "sampled_scores": scores[sampled_ids]}


def tie_set():
    """Seven values with ties among them, both signs of zero and both infinities."""
    return np.array([-np.inf, -1.5, -0.0, 0.0, 2.0 ** -1060, 3.25, np.inf])


def case(nq, nref, seed, ties):
    """(q, ref) float64: random, or drawn from the tie set (ref then holds -0.0, +0.0 and both infinities for nref >= 4)."""
    rng = np.random.default_rng(seed)
    if not ties:
        return rng.standard_normal(nq), rng.standard_normal(nref)
    t = tie_set()
    ref = t[rng.integers(0, len(t), nref)]
    must = np.array([-0.0, 0.0, np.inf, -np.inf])[:min(4, nref)]
    ref[rng.permutation(nref)[:len(must)]] = must
    q = t[rng.integers(0, len(t), nq)]
    return q, ref
