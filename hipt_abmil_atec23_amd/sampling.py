"""DRAS-MIL attention-guided sampling inference (the reference's ``eval.py --sampling``: utils/eval_utils.py:182-565
``summary_sampling``, helpers in utils/sampling_utils.py:11-187) on the HIP library.

A slide is classified from a few hundred instances chosen over several rounds: each round runs the aggregator on a small
sample, spreads the sample's attention scores to the k nearest neighbours of every sampled instance (in coordinate space,
``sampling_type="spatial"``, or in feature space, ``"textural"``), turns them into sampling weights and draws the next sample.

Device work: the k nearest neighbours (``hipt_knn``: brute force, no tree is fitted) and the weight update
(``hipt_sampling_update``) are HIP kernels; the aggregator is the package's ``CLAM_SB``; gathering the sampled rows is a torch
index op.  Host work, by design: the draws (:func:`generate_sample_idxs`), which use the global ``np.random`` / ``random``
state exactly as the reference does, so a seed set by a reference script draws what it drew there.  One round costs one
device-to-host copy (the weights and their sum, for the draw) and no other synchronisation.
"""
from __future__ import annotations

import math
import random
from dataclasses import dataclass, fields

import numpy as np
import torch

from . import _native as N
from . import functional as Fn

INITIAL_WEIGHT = 0.0001   # eval_utils.py:349
_KINDS = {"spatial": N.KNN_SPATIAL, "textural": N.KNN_TEXTURAL}
_MODES = {"max": N.SAMPLING_MAX, "newest": N.SAMPLING_NEWEST, "none": N.SAMPLING_NEWEST, "average": N.SAMPLING_AVERAGE}
MAX_K, MAX_QUERIES, MAX_POINTS, MAX_DIM = 64, 4096, 1 << 20, 2048


@dataclass
class SamplingConfig:
    """The reference's sampling flags with their defaults (eval.py:63-82)."""
    samples_per_iteration: int = 100
    resampling_iterations: int = 10
    sampling_random: float = 0.2
    sampling_random_delta: float = 0.02
    sampling_neighbors: int = 20
    sampling_neighbors_delta: int = 0
    sampling_type: str = "spatial"
    use_all_samples: bool = False
    final_sample_size: int = 100
    retain_best_samples: int = 100
    initial_grid_sample: bool = False
    sampling_average: bool = False
    weight_smoothing: float = 0.15
    fully_random: bool = False

    def __post_init__(self):
        if self.sampling_type not in _KINDS:
            raise ValueError(f"sampling_type must be 'spatial' or 'textural', got {self.sampling_type!r}")
        if self.samples_per_iteration < 1 or self.resampling_iterations < 1 or self.final_sample_size < 0:
            raise ValueError("samples_per_iteration and resampling_iterations must be >= 1, final_sample_size >= 0")
        if not 1 <= self.sampling_neighbors <= MAX_K:
            raise ValueError(f"sampling_neighbors must be in 1..{MAX_K} (the reference's search space tops out at 64, eval.py:183)")
        if self.sampling_neighbors - self.sampling_neighbors_delta * (self.resampling_iterations - 1) < 0 or self.sampling_neighbors_delta < 0:
            raise ValueError("sampling_neighbors_delta would shrink the neighbourhood below zero before the last round")
        if self.samples_per_iteration > MAX_QUERIES:
            raise ValueError(f"samples_per_iteration must be <= {MAX_QUERIES}")
        if not self.weight_smoothing > 0:
            raise ValueError("weight_smoothing (the exponent of the attention scores) must be positive")

    @classmethod
    def from_args(cls, args) -> "SamplingConfig":
        """From an argparse namespace of the reference's eval.py; flags it lacks keep their defaults."""
        return cls(**{f.name: getattr(args, f.name) for f in fields(cls) if hasattr(args, f.name)})


# ------------------------------------------------------------------------------------------------------------------------------
# kNN
# ------------------------------------------------------------------------------------------------------------------------------
def prepare_points(X, kind: str = "spatial", device=None) -> torch.Tensor:
    """The point set as the kernel reads it, on the device: ``spatial`` -- integer ``coords [N, 2]`` (int32 or int64 as the
    sidecar holds them) checked against +-2^30 and narrowed to int32; ``textural`` -- fp32 ``[N, D]``, D a multiple of 4 up to
    2048.  One upload per slide; :func:`knn` accepts the result as is."""
    if kind not in _KINDS:
        raise ValueError(f"kind must be 'spatial' or 'textural', got {kind!r}")
    t = torch.as_tensor(X)
    if device is not None:
        t = t.to(device)
    N.require_cuda(t, "sampling.knn")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[0] > MAX_POINTS:
        raise ValueError(f"knn: expected [N, D] points with 1 <= N <= 2^20, got {tuple(t.shape)}")
    if kind == "spatial":
        if t.shape[1] != 2 or t.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"knn: spatial points are int32 / int64 [N, 2] coordinates, got {t.dtype} {tuple(t.shape)}")
        if t.dtype == torch.int64:
            if int(t.abs().max()) > (1 << 30):
                raise ValueError("knn: coordinates outside +-2^30")
            t = t.to(torch.int32)
        elif int(t.abs().max()) > (1 << 30):
            raise ValueError("knn: coordinates outside +-2^30")
        return t.contiguous()
    if not t.dtype.is_floating_point or t.shape[1] % 4 or t.shape[1] > MAX_DIM:
        raise ValueError(f"knn: textural points are floating-point [N, D], D a multiple of 4 up to {MAX_DIM}, got {t.dtype} {tuple(t.shape)}")
    return t.detach().float().contiguous()


def _knn(Xp: torch.Tensor, kind: str, q: torch.Tensor, k: int):
    n, d = Xp.shape
    s = q.shape[0]
    if k > n:
        raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {n}, n_neighbors = {k}")   # sklearn's words
    if not 1 <= k <= MAX_K or not 1 <= s <= MAX_QUERIES:
        raise ValueError(f"knn: k={k} must be in 1..{MAX_K} and the number of queries {s} in 1..{MAX_QUERIES}")
    dev = Xp.device
    ids = torch.empty((s, k), dtype=torch.int64, device=dev)
    dist = torch.empty((s, k), dtype=torch.float64 if kind == "spatial" else torch.float32, device=dev)
    st = N.stream_ptr(dev)
    ws = Fn.workspace(dev, N.lib().hipt_knn_workspace_bytes(n, s, k), ("knn", st.value))
    N.call("hipt_knn", N.ptr(Xp), _KINDS[kind], n, d, N.ptr(q), s, k, N.ptr(ids), N.ptr(dist), N.ptr(ws), ws.numel(), st)
    return dist, ids


def knn(X, query_idx, k: int, kind: str = "spatial"):
    """``(dist [S, k], ids int64 [S, k])``: the k nearest rows of ``X`` to each of its rows ``query_idx``, every row in
    ascending (distance, index) order -- what ``NearestNeighbors(n_neighbors=k).fit(X).kneighbors(X[query_idx])`` returns, with
    the order among equal distances defined (sklearn's is not).  ``spatial``: exact integer arithmetic, ``dist`` float64;
    ``textural``: fp32 sum of squared differences, ``dist`` fp32.  ``k > N`` raises as sklearn does."""
    Xp = prepare_points(X, kind)
    q = torch.as_tensor(query_idx, dtype=torch.int64).reshape(-1)
    if q.numel() == 0:
        raise ValueError("knn: no queries")
    if int(q.min()) < 0 or int(q.max()) >= Xp.shape[0]:
        raise IndexError(f"knn: query index outside 0..{Xp.shape[0] - 1}")
    return _knn(Xp, kind, q.to(Xp.device).contiguous(), int(k))


# ------------------------------------------------------------------------------------------------------------------------------
# weight update
# ------------------------------------------------------------------------------------------------------------------------------
def _update(weights, scores, all_sampled, ids, neighbors, power, mode, sum_out):
    dev = weights.device
    n = weights.shape[0]
    s = scores.shape[0]
    if ids.shape[0] != s:
        raise ValueError(f"update_sampling_weights: {s} scores for {ids.shape[0]} neighbour lists")
    if not 0 <= neighbors <= ids.shape[1]:
        raise ValueError(f"update_sampling_weights: neighbors={neighbors} outside the lists' width {ids.shape[1]}")
    st = N.stream_ptr(dev)
    ws = Fn.workspace(dev, N.lib().hipt_sampling_update_workspace_bytes(n), ("sampling_update", st.value))
    N.call("hipt_sampling_update", N.ptr(weights), n, N.ptr(scores), s, N.ptr(ids), ids.shape[1], int(neighbors),
           N.ptr(all_sampled), all_sampled.shape[0], float(power), mode, N.ptr(sum_out), N.ptr(ws), ws.numel(), st)


def update_sampling_weights(weights, scores, all_sampled, ids, neighbors, power=0.15, sampling_update="max", return_sum=False):
    """One round of the reference's ``update_sampling_weights(..., normalise=False, repeats_allowed=False)``
    (sampling_utils.py:66-187) on device tensors, IN PLACE on ``weights`` (float64 ``[N]``), which is returned.

    ``scores`` fp32 ``[S]`` >= 0: the softmaxed attention of the round's sample; ``ids`` int64 ``[S, K]``: their neighbour lists,
    of which the first ``neighbors`` columns count; ``all_sampled`` int64: every index drawn so far (weight 0 afterwards).
    ``max``: a weight rises to the largest ``score ** power`` that reaches it.  ``average``: the reference's running pairwise
    mean ``(new + s) / 2`` over the contributions in ascending sample order, ``** power``, overwriting.  ``newest``: the
    reference assigns the newest score to a scratch array and never uses it (sampling_utils.py:174-177), so -- reproduced
    here -- only the zeroing of sampled indices happens.  ``return_sum``: also the float64 ``[1]`` sum of the new weights."""
    if sampling_update not in _MODES:
        raise ValueError(f"sampling_update must be one of {sorted(_MODES)}, got {sampling_update!r}")
    N.require_cuda(weights, "update_sampling_weights")
    if weights.dtype != torch.float64 or weights.dim() != 1 or not weights.is_contiguous():
        raise ValueError("update_sampling_weights: weights must be a contiguous float64 [N] device tensor (updated in place)")
    if not power > 0:
        raise ValueError("update_sampling_weights: power must be positive")
    dev = weights.device
    scores = torch.as_tensor(scores).to(dev).detach().float().reshape(-1).contiguous()
    ids = torch.as_tensor(ids).to(dev).to(torch.int64)
    ids = ids.reshape(scores.shape[0], -1).contiguous()
    all_sampled = torch.as_tensor(all_sampled, dtype=torch.int64).to(dev).reshape(-1).contiguous()
    N.same_device("update_sampling_weights", dev, scores, ids, all_sampled)
    total = torch.empty(1, dtype=torch.float64, device=dev)
    _update(weights, scores, all_sampled, ids, int(neighbors), power, _MODES[sampling_update], total)
    return (weights, total) if return_sum else weights


def update_sampling_weights_np(sampling_weights, attention_scores, all_sample_idxs, indices, neighbors, power=0.15, normalise=True,
                               sampling_update="max", repeats_allowed=False, device="cuda"):
    """The reference's signature and argument kinds (numpy arrays, lists, CPU or device tensors), a float64 numpy array back:
    what ``dropin.install(sampling=True)`` binds as ``utils.sampling_utils.update_sampling_weights``."""
    w = torch.as_tensor(np.array(sampling_weights, dtype=np.float64)).to(device)
    s = attention_scores.detach().float() if torch.is_tensor(attention_scores) else torch.as_tensor(np.asarray(attention_scores, dtype=np.float32))
    sampled = [] if repeats_allowed else [int(i) for i in all_sample_idxs]
    ids = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    w, total = update_sampling_weights(w, s, sampled, ids, neighbors, power, sampling_update, return_sum=True)
    out = w.cpu().numpy()
    return out / float(total) if normalise else out


# ------------------------------------------------------------------------------------------------------------------------------
# the draw (host)
# ------------------------------------------------------------------------------------------------------------------------------
def _scalar(v):
    return v.item() if hasattr(v, "item") else v


def generate_sample_idxs(idxs_length, previous_samples, sampling_weights, samples_per_iteration, num_random, grid=False, coords=None):
    """The reference's draw (sampling_utils.py:11-48) with its signature, on the global ``np.random`` / ``random`` state.

    ``grid=False``: ``samples_per_iteration - num_random`` indices by ``np.random.choice(p=sampling_weights, replace=False)``,
    then ``num_random`` indices by ``random.sample`` from those neither in ``previous_samples`` nor just drawn; the uniform ones
    come first in the returned list.  ``grid=True``: one index from every occupied cell of an ``int(sqrt(samples))``-way split
    of the coordinates' bounding box, filled up with a uniform draw."""
    if grid:
        assert len(coords) > 0
        xs = [_scalar(c[0]) for c in coords]
        ys = [_scalar(c[1]) for c in coords]
        splits = int(math.sqrt(samples_per_iteration))
        x_borders = np.linspace(min(xs), max(xs) + 0.00001, splits + 1)
        y_borders = np.linspace(min(ys), max(ys) + 0.00001, splits + 1)
        cells = [[] for _ in range((splits + 1) * (splits + 1))]
        xi = np.searchsorted(x_borders, np.asarray(xs), side="right") - 1   # the last border <= x
        yi = np.searchsorted(y_borders, np.asarray(ys), side="right") - 1
        for coord_idx in range(len(xs)):
            cells[(splits + 1) * int(xi[coord_idx]) + int(yi[coord_idx])].append(coord_idx)
        sample_idxs = []
        for cell in cells:
            if len(cell) > 0:
                sample_idxs = sample_idxs + list(np.random.choice(cell, size=1, replace=False))
        if len(sample_idxs) < samples_per_iteration:
            sample_idxs = sample_idxs + list(np.random.choice(range(0, len(coords)), size=samples_per_iteration - len(sample_idxs), replace=False))
        return sample_idxs
    available = set(range(idxs_length))
    weighted, uniform = [], []
    if int(samples_per_iteration - num_random) > 0:
        weighted = list(np.random.choice(range(idxs_length), p=sampling_weights, size=int(samples_per_iteration - num_random), replace=False))
        available = available - set(list(previous_samples) + weighted)
    if num_random > 0:
        uniform = random.sample(list(available), num_random)
    return uniform + weighted


# ------------------------------------------------------------------------------------------------------------------------------
# the per-slide loop
# ------------------------------------------------------------------------------------------------------------------------------
def resnet_patch_features(model, patches_u8):
    """A ``feature_fn`` for :func:`dras_eval_slide` (the ``--eval_features`` route, eval_utils.py:263-279,350-358): ``patches_u8``
    is the slide's resident uint8 patch tensor (``[N, 3, H, W]`` or ``[N, H, W, 3]``); only the rows asked for go through
    ``model`` (a ``ResNet_Baseline``), which normalises them on the device."""
    if patches_u8.dtype != torch.uint8 or patches_u8.dim() != 4:
        raise ValueError(f"resnet_patch_features: expected a uint8 [N, 3, H, W] / [N, H, W, 3] tensor, got {patches_u8.dtype} {tuple(patches_u8.shape)}")
    N.require_cuda(patches_u8, "resnet_patch_features")

    def feature_fn(idxs):
        with torch.no_grad():
            return model(patches_u8[torch.as_tensor(idxs, dtype=torch.int64, device=patches_u8.device)])
    return feature_fn


def _py(idxs):
    return [int(i) for i in idxs]


def dras_eval_slide(model, coords, cfg: SamplingConfig, data=None, feature_fn=None, trace=False) -> dict:
    """One slide through the reference's sampling loop (eval_utils.py:290-509): the initial sample, ``resampling_iterations - 1``
    rounds, the final sample (with the ``retain_best_samples`` book-keeping or the ``use_all_samples`` variant), and the
    ``fully_random`` / "slide smaller than the sample budget" short-cuts.

    ``model``: a ``CLAM_SB`` on a HIP device.  ``coords``: the slide's integer ``[N, 2]`` coordinates.  Exactly one of ``data``
    (``[N, D]`` device features, as ``load_bag`` returns them) and ``feature_fn(idxs) -> [n, D]`` (the ``--eval_features`` route:
    only what is sampled is ever extracted, each index once; spatial only, as in the reference).

    Returns ``logits, Y_prob, Y_hat, A_raw`` of the final call, its ``sample_idxs``, ``all_sample_idxs``, the final ``weights``
    (float64 numpy, None on the short-cuts) and ``round_Y_prob``.  ``trace=True`` adds ``trace``: ``calls`` (per aggregator call
    the indices, ``A_raw``, ``logits``, ``Y_hat``) and ``updates`` (per weight update: the scores and neighbour lists it saw, the
    prefix width, the indices zeroed, the weights before and after, their device sum, the host RNG states before the draw,
    the draw's arguments and its result) plus ``initial`` (RNG states before the first draw)."""
    if (data is None) == (feature_fn is None):
        raise ValueError("dras_eval_slide: give exactly one of data and feature_fn")
    spatial = cfg.sampling_type == "spatial"
    if feature_fn is not None and not spatial:
        raise ValueError("dras_eval_slide: the feature_fn (--eval_features) route is spatial only, as in the reference")
    dev = data.device if data is not None else next(model.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(f"dras_eval_slide: model / data are on {dev}; this package runs only on a HIP device")
    coords_np = coords.cpu().numpy() if torch.is_tensor(coords) else np.asarray(coords)
    n = len(coords_np)
    if data is not None and data.shape[0] != n:
        raise ValueError(f"dras_eval_slide: {data.shape[0]} feature rows for {n} coordinates")
    spi, iters = cfg.samples_per_iteration, cfg.resampling_iterations
    mode = _MODES["average" if cfg.sampling_average else "max"]
    total = spi if cfg.fully_random else spi * iters + cfg.final_sample_size
    tr = {"calls": [], "updates": [], "initial": None} if trace else None

    feats, where = [], {}   # feature_fn route: every extracted row is kept, so no index is extracted twice

    def rows_of(idxs, idx_dev):
        if data is not None:
            return data[idx_dev]
        fresh = [i for i in idxs if i not in where]
        if fresh:
            f = feature_fn(fresh)
            base = sum(t.shape[0] for t in feats)
            for p, i in enumerate(fresh):
                where[i] = base + p
            feats.append(f)
        allf = feats[0] if len(feats) == 1 else torch.cat(feats)
        if len(feats) > 1:
            feats[:] = [allf]
        return allf[torch.as_tensor([where[i] for i in idxs], dtype=torch.int64, device=allf.device)]

    def run(idxs, idx_dev=None, rows=None):
        if rows is None:
            if idx_dev is None:
                idx_dev = torch.as_tensor(idxs, dtype=torch.int64).to(dev)
            rows = rows_of(idxs, idx_dev)
        with torch.no_grad():
            logits, Y_prob, Y_hat, A_raw, _ = model(rows)
        if trace:
            tr["calls"].append({"idxs": list(idxs), "A_raw": A_raw, "logits": logits, "Y_hat": Y_hat})
        return logits, Y_prob, Y_hat, A_raw

    def states():
        return {"np": np.random.get_state(), "py": random.getstate()}

    # ---- short-cuts (eval_utils.py:294-344) ----
    if cfg.fully_random or total >= n:
        if trace:
            tr["initial"] = states()
        if total >= n:
            if data is not None:
                idxs = list(range(n))
                out = run(idxs, rows=data)
            else:   # the reference extracts the whole slide in a shuffled order (:298)
                idxs = _py(generate_sample_idxs(n, [], [], n, num_random=n, grid=False, coords=coords_np))
                out = run(idxs)
        else:
            idxs = _py(generate_sample_idxs(n, [], [], spi, num_random=spi, grid=cfg.initial_grid_sample, coords=coords_np))
            out = run(idxs)
        res = dict(logits=out[0], Y_prob=out[1], Y_hat=out[2], A_raw=out[3], sample_idxs=idxs, all_sample_idxs=idxs, weights=None,
                   round_Y_prob=[out[1]])
        if trace:
            res["trace"] = tr
        return res

    # ---- one upload of the point set, one workspace (the reference fits a ball tree twice, :285 and :390) ----
    kind = cfg.sampling_type
    Xp = prepare_points(coords_np if spatial else data, kind, device=dev)
    k = cfg.sampling_neighbors
    if k > n:
        raise ValueError(f"Expected n_neighbors <= n_samples, but n_samples = {n}, n_neighbors = {k}")
    wbuf = torch.full((n + 1,), INITIAL_WEIGHT, dtype=torch.float64, device=dev)   # [n] weights + their sum: one copy per round
    weights, wsum = wbuf[:n], wbuf[n:]
    all_dev = torch.empty(spi * iters + cfg.final_sample_size, dtype=torch.int64, device=dev)
    host_w = np.full(n, INITIAL_WEIGHT)

    # ---- initial sample (:347-391) ----
    if trace:
        tr["initial"] = states()
    sample_idxs = _py(generate_sample_idxs(n, [], [], spi, num_random=spi, grid=cfg.initial_grid_sample, coords=coords_np))
    all_sample_idxs = list(sample_idxs)
    idx_dev = all_dev[:len(sample_idxs)]
    idx_dev.copy_(torch.as_tensor(sample_idxs, dtype=torch.int64))
    n_all = len(sample_idxs)
    logits, Y_prob, Y_hat, A_raw = run(sample_idxs, idx_dev)
    scores = torch.softmax(A_raw, dim=1)[0]
    round_probs = [Y_prob]
    keep_best = not cfg.use_all_samples
    if keep_best:   # the best retain_best_samples by raw attention, kept on the device (the reference sorts host lists, :369-376)
        best_idx, best_raw = idx_dev, A_raw[0]
        if spi > cfg.retain_best_samples:
            o = torch.argsort(best_raw, stable=True).flip(0)[:cfg.retain_best_samples]
            best_idx, best_raw = best_idx[o], best_raw[o]
    _, ids = _knn(Xp, kind, idx_dev, k)

    def update_and_draw(n_draw, num_random, neighbors):
        nonlocal host_w
        before = host_w
        _update(weights, scores, all_dev[:n_all], ids, neighbors, cfg.weight_smoothing, mode, wsum)
        h = wbuf.cpu().numpy()   # the round's one synchronisation
        host_w, s = h[:n], float(h[n])
        st = states() if trace else None
        drawn = _py(generate_sample_idxs(n, all_sample_idxs, host_w / s, n_draw, num_random)) if n_draw > 0 else []
        if trace:
            tr["updates"].append({"scores": scores, "ids": ids, "neighbors": neighbors, "all_sampled": list(all_sample_idxs),
                                  "weights_before": before, "weights": host_w, "sum": s, "rng": st,
                                  "n_draw": n_draw, "num_random": num_random, "drawn": list(drawn)})
        return drawn

    # ---- subsequent rounds (:393-457) ----
    frac, neighbors = cfg.sampling_random, k
    for _ in range(iters - 1):
        frac = frac - cfg.sampling_random_delta if frac > cfg.sampling_random_delta else 0
        num_random = int(spi * frac)
        sample_idxs = update_and_draw(spi, num_random, neighbors)
        idx_dev = all_dev[n_all:n_all + len(sample_idxs)]
        idx_dev.copy_(torch.as_tensor(sample_idxs, dtype=torch.int64))
        n_all += len(sample_idxs)
        all_sample_idxs = all_sample_idxs + sample_idxs
        _, ids = _knn(Xp, kind, idx_dev, k)
        logits, Y_prob, Y_hat, A_raw = run(sample_idxs, idx_dev)
        scores = torch.softmax(A_raw, dim=1)[0][-spi:]
        if keep_best:
            best_raw, best_idx = torch.cat((A_raw[0], best_raw)), torch.cat((idx_dev, best_idx))
            if best_idx.shape[0] > cfg.retain_best_samples:
                o = torch.argsort(best_raw, stable=True).flip(0)[:cfg.retain_best_samples]
                best_idx, best_raw = best_idx[o], best_raw[o]
        round_probs.append(Y_prob)
        neighbors = neighbors - cfg.sampling_neighbors_delta

    # ---- final sample (:459-483) ----
    if cfg.use_all_samples:
        drawn = update_and_draw(cfg.final_sample_size, 0, neighbors)
        sample_idxs = drawn + all_sample_idxs
        all_sample_idxs = sample_idxs
        final_dev = None
    else:
        n_best = int(best_idx.shape[0])
        drawn = update_and_draw(int(cfg.final_sample_size - n_best), 0, neighbors)
        all_sample_idxs = all_sample_idxs + drawn
        final_dev = torch.cat((torch.as_tensor(drawn, dtype=torch.int64).to(dev), best_idx))
        sample_idxs = drawn + _py(best_idx.cpu().tolist())
    logits, Y_prob, Y_hat, A_raw = run(sample_idxs, final_dev)
    round_probs.append(Y_prob)
    final_w = host_w.copy()
    final_w[np.asarray(drawn, dtype=np.int64)] = 0   # what the reference's next update would do: every sampled index ends at 0
    res = dict(logits=logits, Y_prob=Y_prob, Y_hat=Y_hat, A_raw=A_raw, sample_idxs=sample_idxs, all_sample_idxs=all_sample_idxs,
               weights=final_w, round_Y_prob=round_probs)
    if trace:
        res["trace"] = tr
    return res
