"""The DRAS-MIL sampling procedure (eval.py --sampling; utils/eval_utils.py:182-565 summary_sampling, helpers in
utils/sampling_utils.py:11-187) restated in numpy for the tests: what the reference's functions compute, written from their
behaviour.  ``oracle/`` holds the model oracles; this file is to ``hipt_abmil_atec23_amd/sampling.py`` what
``tests/resnet_ref.py`` is to the ResNet extractor.  tests/test_sampling_host.py pins it to tests/golden/dras_*.npz, which
the reference's own functions and sklearn wrote (tests/golden/make_golden_sampling.py).

kNN: brute force in exact integers (spatial) / float64 (textural), rows ordered by ascending (squared distance, index) -- the
order the HIP kernel defines; sklearn's order among equal distances is whatever its tree walk gives.
"""
import math
import random

import numpy as np

INITIAL_WEIGHT = 0.0001   # eval_utils.py:349


def _ordered(d2, k):
    order = np.lexsort((np.arange(d2.shape[0]), d2))[:k]   # by d2, ties by index
    return order, d2[order]


def knn_spatial(coords, q_idx, k):
    """ids int64 [S, k], dist float64 [S, k] (sqrt of the exact integer), d2 int64 [S, k]."""
    c = np.asarray(coords).astype(np.int64)
    if k > len(c):
        raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {len(c)}, n_neighbors = {k}")
    ids, d2s = [], []
    for q in np.asarray(q_idx).reshape(-1):
        d = c - c[q]
        o, v = _ordered(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1], k)
        ids.append(o)
        d2s.append(v)
    ids, d2s = np.asarray(ids, dtype=np.int64), np.asarray(d2s, dtype=np.int64)
    return ids, np.sqrt(d2s.astype(np.float64)), d2s


def knn_textural(X, q_idx, k, extra=1):
    """float64 brute force.  ids [S, k], dist [S, k] (sqrt), and d2 float64 [S, min(k + extra, N)]: the sorted squared distances
    with ``extra`` more ranks, so that a caller can see how far rank k-1 is from rank k."""
    x = np.asarray(X, dtype=np.float64)
    if k > len(x):
        raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {len(x)}, n_neighbors = {k}")
    ids, d2s = [], []
    for q in np.asarray(q_idx).reshape(-1):
        d = x - x[q]
        o, v = _ordered(np.einsum("nd,nd->n", d, d), min(k + extra, len(x)))
        ids.append(o[:k])
        d2s.append(v)
    ids, d2s = np.asarray(ids, dtype=np.int64), np.asarray(d2s)
    return ids, np.sqrt(d2s[:, :k]), d2s


def textural_gamma(D):
    """Relative error bound (first order) of an fp32 sum of D non-negative terms, each the square of a rounded difference:
    2 roundings per term (difference, square: 2 * 2^-24 relative) + D - 1 additions, whatever their order."""
    return (D + 2) * 2.0 ** -24


def textural_excused(d2_sorted, k, gamma):
    """[S, k] bool: positions whose float64 squared distance is NOT separated from both neighbouring ranks by more than
    2 * gamma relative; there an fp32 kernel may legitimately return either index."""
    d = np.asarray(d2_sorted)
    S = d.shape[0]
    pad = np.concatenate([np.full((S, 1), -np.inf), d, np.full((S, max(0, k + 1 - d.shape[1])), np.inf)], axis=1)
    here, below, above = pad[:, 1:k + 1], pad[:, 0:k], pad[:, 2:k + 2]
    tol = 2 * gamma * here
    return ~((here - below > tol) & (above - here > tol))


def update_sampling_weights(sampling_weights, attention_scores, all_sample_idxs, indices, neighbors, power=0.15, normalise=True,
                            sampling_update="max", repeats_allowed=False):
    """One round's weight update on a float64 copy of ``sampling_weights``.  Row i of ``indices[:, :neighbors]`` hands
    attention_scores[i] to its targets: 'max' keeps the largest, 'average' folds new = (new + s) / 2 in ascending (i, column)
    from the first positive value, 'newest' computes a value the weights never see.  The values go through ``** power``;
    'max' raises weights below them, 'average' overwrites where they are positive.  Sampled indices get weight 0."""
    assert sampling_update in ("max", "newest", "average", "none")
    w = np.array(sampling_weights, dtype=np.float64)
    s = np.asarray(attention_scores, dtype=np.float64)
    idx = np.asarray(indices)[:, :neighbors] if len(indices) else np.zeros((0, 0), dtype=np.int64)
    new = np.zeros(len(w))
    if sampling_update == "max":
        for i in range(idx.shape[0]):
            for j in idx[i]:
                if not (new[j] > 0 and s[i] <= new[j]):
                    new[j] = s[i]
        new = np.power(new, power)
        m = new > w
        w[m] = new[m]
    elif sampling_update == "average":
        for i in range(idx.shape[0]):
            for j in idx[i]:
                new[j] = (new[j] + s[i]) / 2 if new[j] > 0 else s[i]
        new = np.power(new, power)
        m = new > 0
        w[m] = new[m]
    if not repeats_allowed:
        w[np.asarray(all_sample_idxs, dtype=np.int64)] = 0
    if normalise:
        w = w / sum(w)
    return w


def generate_sample_idxs(idxs_length, previous_samples, sampling_weights, samples_per_iteration, num_random, grid=False, coords=None):
    """The reference's draw, on the global ``np.random`` / ``random`` state.  grid=False: ``samples_per_iteration - num_random``
    indices by ``np.random.choice(p=sampling_weights, replace=False)``, then ``num_random`` by ``random.sample`` from the indices
    in neither ``previous_samples`` nor the weighted draw; the random ones come first in the result.  grid=True: one index from
    every occupied cell of an int(sqrt(samples))-way split of the coordinates' bounding box, filled up uniformly."""
    if grid:
        assert len(coords) > 0
        xs = [float(c[0]) for c in coords]
        ys = [float(c[1]) for c in coords]
        n = int(math.sqrt(samples_per_iteration))
        xb = np.linspace(min(xs), max(xs) + 0.00001, n + 1)
        yb = np.linspace(min(ys), max(ys) + 0.00001, n + 1)
        cells = [[] for _ in range((n + 1) * (n + 1))]
        for ci, (x, y) in enumerate(zip(xs, ys)):
            xi = int(np.searchsorted(xb, x, side="right")) - 1
            yi = int(np.searchsorted(yb, y, side="right")) - 1
            cells[(n + 1) * xi + yi].append(ci)
        out = []
        for cell in cells:
            if cell:
                out = out + list(np.random.choice(cell, size=1, replace=False))
        if len(out) < samples_per_iteration:
            out = out + list(np.random.choice(range(0, len(coords)), size=samples_per_iteration - len(out), replace=False))
        return out
    available = set(range(idxs_length))
    weighted, uniform = [], []
    n_weighted = int(samples_per_iteration - num_random)
    if n_weighted > 0:
        weighted = list(np.random.choice(range(idxs_length), p=sampling_weights, size=n_weighted, replace=False))
        available = available - set(list(previous_samples) + weighted)
    if num_random > 0:
        uniform = random.sample(list(available), num_random)
    return uniform + weighted


def softmax_row(a):
    a = np.asarray(a, dtype=np.float32).reshape(-1)
    e = np.exp(a - a.max())
    return (e / e.sum()).astype(np.float32)


def dras_eval_slide(model_fn, coords, cfg, data, knn_fn=None):
    """The per-slide body of summary_sampling (eval_utils.py:290-509) for features held in memory.  ``model_fn(rows) ->
    (logits, Y_prob, Y_hat, A_raw[1, n])`` (numpy); ``cfg``: an object with the reference's flag names.  ``knn_fn(X, idxs, k)
    -> ids`` defaults to the brute force above.  Returns a dict like the product's."""
    n = len(coords)
    spatial = cfg.sampling_type == "spatial"
    X = np.asarray(coords) if spatial else np.asarray(data)
    if knn_fn is None:
        knn_fn = (lambda X_, q, k: knn_spatial(X_, q, k)[0]) if spatial else (lambda X_, q, k: knn_textural(X_, q, k)[0])
    spi = cfg.samples_per_iteration
    mode = "average" if cfg.sampling_average else "max"
    total = spi if cfg.fully_random else spi * cfg.resampling_iterations + cfg.final_sample_size
    if cfg.fully_random or total >= n:
        if total >= n:
            idxs, rows = list(range(n)), data
        else:
            idxs = generate_sample_idxs(n, [], [], spi, num_random=spi, grid=cfg.initial_grid_sample, coords=coords)
            rows = data[idxs]
        logits, prob, yhat, a_raw = model_fn(rows)
        return dict(logits=logits, Y_prob=prob, Y_hat=yhat, A_raw=a_raw, sample_idxs=idxs, all_sample_idxs=idxs, weights=None,
                    round_Y_prob=[prob])
    idxs = generate_sample_idxs(n, [], [], spi, num_random=spi, grid=cfg.initial_grid_sample, coords=coords)
    all_idxs = list(idxs)
    w = np.full(n, INITIAL_WEIGHT)
    logits, prob, yhat, a_raw = model_fn(data[idxs])
    scores = softmax_row(a_raw)
    raw = list(np.asarray(a_raw).reshape(-1))
    probs = [prob]
    best_idx, best_raw = list(idxs), list(raw)
    if not cfg.use_all_samples and spi > cfg.retain_best_samples:
        o = list(np.argsort(raw))[::-1][:cfg.retain_best_samples]
        best_idx, best_raw = [idxs[i] for i in o], [raw[i] for i in o]
    ids = knn_fn(X, idxs, cfg.sampling_neighbors)
    frac, neighbors = cfg.sampling_random, cfg.sampling_neighbors
    for _ in range(cfg.resampling_iterations - 1):
        frac = frac - cfg.sampling_random_delta if frac > cfg.sampling_random_delta else 0
        num_random = int(spi * frac)
        w = update_sampling_weights(w, scores, all_idxs, ids, neighbors, power=cfg.weight_smoothing, normalise=False, sampling_update=mode)
        idxs = generate_sample_idxs(n, all_idxs, w / sum(w), spi, num_random)
        ids = knn_fn(X, idxs, cfg.sampling_neighbors)
        all_idxs = all_idxs + idxs
        logits, prob, yhat, a_raw = model_fn(data[idxs])
        scores = softmax_row(a_raw)[-spi:]
        raw = list(np.asarray(a_raw).reshape(-1))
        if not cfg.use_all_samples:
            comb_raw, comb_idx = raw + best_raw, idxs + best_idx
            if len(comb_idx) > cfg.retain_best_samples:
                o = list(np.argsort(comb_raw))[::-1][:cfg.retain_best_samples]
                comb_idx, comb_raw = [comb_idx[i] for i in o], [comb_raw[i] for i in o]
            best_idx, best_raw = comb_idx, comb_raw
        probs.append(prob)
        neighbors = neighbors - cfg.sampling_neighbors_delta
    w = update_sampling_weights(w, scores, all_idxs, ids, neighbors, power=cfg.weight_smoothing, normalise=False, sampling_update=mode)
    if cfg.use_all_samples:
        idxs = generate_sample_idxs(n, all_idxs, w / sum(w), cfg.final_sample_size, num_random=0)
        idxs = idxs + all_idxs
        all_idxs = idxs
    else:
        idxs = generate_sample_idxs(n, all_idxs, w / sum(w), int(cfg.final_sample_size - len(best_idx)), num_random=0)
        all_idxs = all_idxs + idxs
        idxs = idxs + best_idx
    logits, prob, yhat, a_raw = model_fn(data[idxs])
    probs.append(prob)
    return dict(logits=logits, Y_prob=prob, Y_hat=yhat, A_raw=a_raw, sample_idxs=idxs, all_sample_idxs=all_idxs, weights=w,
                round_Y_prob=probs)


# ----------------------------------------------------------------------------------------------------------------------------
# Fixtures shared by the golden generator and the tests (integer-hash inputs, hipt_abmil_atec23_amd.synth)
# ----------------------------------------------------------------------------------------------------------------------------
TEXTURAL_CASES = ((5000, 192, 31), (3000, 1024, 32), (777, 384, 33))   # (N, D, seed)
UPDATE_CASES = (("max", 8), ("max", 5), ("newest", 8), ("average", 8), ("average", 5))   # (mode, neighbors)


def spatial_fixture(duplicates=False):
    """A 60 x 50 grid of stride-256 patch coordinates with 20 % of the points removed by hash, offset to ~10^5 (squared
    distances ~10^10: beyond fp32).  ``duplicates``: the first 40 points are appended again (identical points, higher index)."""
    from hipt_abmil_atec23_amd import synth
    gx, gy = np.meshgrid(np.arange(60), np.arange(50), indexing="ij")
    c = np.stack([gx.ravel(), gy.ravel()], axis=1).astype(np.int64) * 256 + np.array([100352, 98304])
    keep = synth.hash_u32_np(len(c), 41) % 5 != 0
    c = c[keep]
    if duplicates:
        c = np.concatenate([c, c[:40]])
    return c


def textural_fixture(n, d, seed, isotropic=False):
    """Hashed uniform fp32 features.  Default: feature j is scaled by 1 / (1 + j)^2 (a decaying spectrum, as extracted
    features have), which keeps neighbouring distances apart: at most 1 % of the positions are near-ties in the sense of
    ``textural_excused``.  ``isotropic``: every feature uniform on [-1, 1); distances then concentrate (the relative gap between
    neighbouring ranks falls below the fp32 bound at 1-40 % of the positions for these sizes, whatever the seed), so that
    fixture checks distances at every rank, and indices only where the ranks are apart."""
    from hipt_abmil_atec23_amd import synth
    x = synth.hash_uniform_np((n, d), seed)
    if isotropic:
        return x
    return x * (np.float32(1) / (np.float32(1) + np.arange(d, dtype=np.float32)) ** 2)


def query_fixture(n, s, seed=51):
    """s distinct row indices by hash."""
    from hipt_abmil_atec23_amd import synth
    order = np.argsort(synth.hash_u32_np(n, seed), kind="stable")
    return order[:s].astype(np.int64)


def update_fixture(n=500, s=12, k=8):
    """weights with history, scores (one exactly 0), neighbour lists over only 60 targets (so targets repeat, many with
    three or more contributions of different scores: the 'average' fold depends on their order), and the sampled indices."""
    from hipt_abmil_atec23_amd import synth
    w = np.full(n, INITIAL_WEIGHT)
    touched = synth.hash_u32_np(40, 61) % n
    w[touched] = np.abs(synth.hash_uniform_np((40,), 62)).astype(np.float64) * 0.9
    scores = (np.abs(synth.hash_uniform_np((s,), 63)) * 0.3).astype(np.float32)
    scores[3] = 0.0
    ids = (synth.hash_u32_np(s * k, 64) % 60).astype(np.int64).reshape(s, k) * 7
    sampled = [int(i) for i in (synth.hash_u32_np(30, 65) % n)]
    return w, scores, ids, sampled
