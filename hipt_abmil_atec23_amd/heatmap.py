"""Attention heat-maps (the reference's ``WholeSlideImage.visHeatmap``, wsi_core/WholeSlideImage.py:508-696) on the HIP library.

The reference turns per-patch attention scores into an image with two Python loops over numpy slices (:598-610 accumulate a
score and a counter per pixel, :647-674 colour and paint patch by patch) and a block loop that blends with the slide (:699-739).
Here the pixel work is ``hipt_heatmap_overlay`` / ``hipt_heatmap_render`` (csrc/heatmap.hip): every pixel gathers
its covering patches from per-tile lists in ascending patch index, so the float64 overlay is bit for bit numpy's, and the mask,
the colour lookup and the blend happen in the same pass.

Host work, by design: scaling the coordinates (float64 ``ceil``, as numpy), the threshold, the 258-entry colour table from
matplotlib, and everything that touches the slide (``vis_heatmap``: level choice, bounding-box screening, one ``read_region`` for
the canvas, the tissue mask, PIL's final ``resize``).  ``blur=True`` is not supported (cv2's fixed-point uint8 Gaussian cannot be
reproduced without cv2).

The scores in front of the picture rank on the device too: ``hipt_score_counts`` (csrc/percentile.hip) counts, for
every score, the reference values below it and those not above it, and forms the percentile in the reference's order of operations.
``to_percentiles`` of a device tensor (``rankdata / len * 100``), ``score2percentile`` (``percentileofscore`` against the block
map's scores, vectorised), ``sample_rois`` and ``compute_from_batches`` (the loop body of ``compute_from_patches``) are built on it.
Numpy scores handed to ``render_heatmap`` / ``heatmap_overlay`` are still ranked by numpy on their way to the device.

Inputs may be numpy arrays (copied to the device, result returned as numpy) or torch tensors already on the device (result
returned as a tensor; nothing is copied to the host, with ``convert_to_percentiles`` or without).  With device tensors the one thing that needs the VALUES -- refusing
negative coordinates and non-finite scores -- costs one synchronisation, which is left out while the stream is being captured
into a graph; the kernels clip such patches at the canvas edge and read nothing out of bounds either way.
"""
from __future__ import annotations

import math

import numpy as np

from . import _frontend as F
from . import _native as N

LUT_ENTRIES = N.HEATMAP_LUT_ENTRIES


# ------------------------------------------------------------------------------------------------------------------------------
# host side: what the device gets
# ------------------------------------------------------------------------------------------------------------------------------
def colour_table(cmap="coolwarm") -> np.ndarray:
    """uint8 [258, 3]: ``(cmap(i) * 255)[:3].astype(uint8)`` for the colormap's 256 entries, then its under and over colours.
    ``cmap(v)`` of a float v is entry ``trunc(v * 256)`` of it (256 -> 255; below 0 under, above 256 over): matplotlib's own
    lookup, which is what the kernel does with the overlay."""
    if isinstance(cmap, str):
        import matplotlib
        if cmap not in matplotlib.colormaps:
            raise ValueError(f"heatmap: {cmap!r} is not a matplotlib colormap")
        cmap = matplotlib.colormaps[cmap]
    if getattr(cmap, "N", 256) != 256:
        raise ValueError(f"heatmap: colormap {getattr(cmap, 'name', cmap)!r} has {cmap.N} entries, the kernel's table has 256")
    rgba = cmap(np.concatenate([np.arange(256), [-1, 256]]))
    return np.ascontiguousarray((rgba * 255)[:, :3].astype(np.uint8))


def table_index(overlay) -> np.ndarray:
    """The kernel's row of ``colour_table`` for overlay values: t = overlay * 256; t < 0 -> 256 (under), t == 256 -> 255,
    t > 256 -> 257 (over), else trunc(t)."""
    t = np.asarray(overlay, dtype=np.float64) * 256
    inner = np.trunc(np.clip(t, 0, 255)).astype(np.int64)
    return np.where(t < 0, 256, np.where(t == 256, 255, np.where(t > 256, 257, inner)))


def to_percentiles(scores):
    """``scipy.stats.rankdata(scores, 'average') / len(scores) * 100`` (wsi_core/wsi_utils.py:124-127): in numpy for numpy
    scores; a device tensor is ranked on the device (``hipt_score_counts``) and a float64 device tensor comes back, the same bits."""
    if F.is_tensor(scores):
        F.check_no_nan("to_percentiles", scores=scores)
        s = _as_f64(scores, F.resolve_device("heatmap", None, (scores,)))
        return _counts_call(s, s, N.PCT_RANKDATA, pct=True)[2]
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    n = len(s)
    if n == 0:
        return s.copy()
    order = np.argsort(s, kind="stable")
    ss = s[order]
    first = np.ones(n, dtype=bool)
    first[1:] = ss[1:] != ss[:-1]
    starts = np.flatnonzero(first)
    ends = np.append(starts[1:], n)
    group = np.cumsum(first) - 1
    rank = np.empty(n, dtype=np.float64)
    rank[order] = (0.5 * (starts + ends + 1))[group]   # the mean of the 1-based positions starts + 1 .. ends
    return rank / n * 100


def scaled_geometry(coords, patch_size, scale):
    """``(xy int64 [N, 2], pw, ph)``: ``ceil(coords * scale)`` and ``ceil(patch_size * scale)`` in float64, as
    WholeSlideImage.py:576-577 computes them."""
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
    ps = np.ceil(np.broadcast_to(np.asarray(patch_size), (2,)) * sc).astype(np.int64)
    xy = np.ceil(np.asarray(coords) * sc).astype(np.int64)
    return xy, int(ps[0]), int(ps[1])


def threshold_of(n: int, binarize: bool, thresh: float) -> float:
    if not binarize:
        return 0.0
    if thresh < 0:
        return 1.0 / n if n else 0.0
    return float(thresh)


def patch_values(scores, *, binarize=False, thresh=0.5, convert_to_percentiles=False):
    """``(v float64 [N], paint uint8 [N])`` of numpy scores: what a patch adds to the pixels it covers, and whether it may
    paint them (``s >= threshold``; WholeSlideImage.py:584-606,651-653).  The caller's array is left as it is."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if convert_to_percentiles:
        s = to_percentiles(s)
    s = s / 100
    keep = s >= threshold_of(len(s), binarize, thresh)
    v = np.where(keep, 1.0 if binarize else s, 0.0)
    return v, keep.astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------------------
# argument checks (all before any native call)
# ------------------------------------------------------------------------------------------------------------------------------
def _check_geometry(scores, coords, patch_size, scale, region_size):
    """Shapes, dtypes and sizes; returns ``(N, w, h)``."""
    if scores.ndim not in (1, 2):   # (a 2-D array is flattened, as the reference does)
        raise ValueError(f"heatmap: scores must be a vector [N] (or [N, 1]), got {tuple(scores.shape)}")
    n = int(np.prod(tuple(scores.shape)))
    if coords.ndim != 2 or tuple(coords.shape) != (n, 2):
        raise ValueError(f"heatmap: coords must be [{n}, 2] for {n} scores, got {tuple(coords.shape)}")
    kind = str(coords.dtype)
    if "int" not in kind:
        raise ValueError(f"heatmap: coords must be integers, got {kind}")
    try:
        w, h = (int(v) for v in region_size)
        sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
        ps = np.broadcast_to(np.asarray(patch_size, dtype=np.float64), (2,))
    except (TypeError, ValueError) as e:
        raise ValueError(f"heatmap: region_size must be (w, h), patch_size and scale a number or a pair: {e}") from None
    if not (np.isfinite(sc).all() and (sc > 0).all() and np.isfinite(ps).all() and (ps > 0).all()):
        raise ValueError(f"heatmap: patch_size {patch_size} and scale {scale} must be positive and finite")
    if not (1 <= w <= N.HEATMAP_MAX_DIM and 1 <= h <= N.HEATMAP_MAX_DIM):
        raise ValueError(f"heatmap: region_size {region_size} outside 1..{N.HEATMAP_MAX_DIM} per side")
    if np.ceil(ps * sc).max() >= 2 ** 31:
        raise ValueError(f"heatmap: scaled patch size {np.ceil(ps * sc)} does not fit int32")
    return n, w, h


def _check_values(xy_min, xy_max, scores_finite):
    if xy_min < 0:
        raise ValueError("heatmap: negative coordinates (coords are relative to the region's top-left corner; the reference's "
                         "slices would wrap around)")
    if xy_max >= 2 ** 31:
        raise ValueError("heatmap: scaled coordinates do not fit int32")
    if not scores_finite:
        raise ValueError("heatmap: scores contain NaN or infinity")


# ------------------------------------------------------------------------------------------------------------------------------
# score ranks on the device (csrc/percentile.hip)
# ------------------------------------------------------------------------------------------------------------------------------
def _check_one_device(what, arrays):
    devs = sorted({str(a.device) for a in arrays if F.is_tensor(a)})
    if len(devs) > 1:
        raise ValueError(f"{what}: scores and reference scores are on different devices ({', '.join(devs)})")


def _as_f64(a, dev):
    """A flat, contiguous float64 tensor on ``dev`` (float32 scores widen exactly, as numpy's comparison promotes them)."""
    import torch
    t = a if F.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    return t.detach().to(dev, torch.float64).reshape(-1).contiguous()


def _counts_call(q, ref, mode, *, counts=False, pct=False):
    """``(less, leq, pct)`` of flat float64 device tensors ``q`` against ``ref``; what was not asked for is None."""
    import torch
    dev, nq = q.device, q.numel()
    less = torch.empty(nq, dtype=torch.int32, device=dev) if counts else None
    leq = torch.empty(nq, dtype=torch.int32, device=dev) if counts else None
    out = torch.empty(nq, dtype=torch.float64, device=dev) if pct else None
    if nq:
        with torch.cuda.device(dev):
            N.call("hipt_score_counts", N.ptr(q), nq, N.ptr(ref), ref.numel(), mode, N.ptr(less), N.ptr(leq), N.ptr(out),
                   N.stream_ptr(dev))
    return less, leq, out


def _check_score_args(what, scores, ref_scores):
    """The argument checks of ``score_counts`` / ``score2percentile``, all before any native call; returns the device."""
    nref = int(np.prod(tuple(ref_scores.shape)))
    if nref == 0:
        raise ValueError(f"{what}: ref_scores is empty (there is nothing to rank against)")
    if nref >= 2 ** 31:
        raise ValueError(f"{what}: {nref} reference scores; the counts are int32")
    _check_one_device(what, (scores, ref_scores))
    F.check_no_nan(what, scores=scores, ref_scores=ref_scores)
    return F.resolve_device("heatmap", None, (scores, ref_scores))


def score_counts(q, ref):
    """``(less, leq)``, int32 ``[len(q)]``: how many values of ``ref`` are smaller than each ``q[i]``, and how many are smaller or
    equal (IEEE comparisons in float64).  Numpy in, numpy out; device tensors in, tensors out."""
    q, ref = F.as_array(q), F.as_array(ref)
    dev = _check_score_args("score_counts", q, ref)
    less, leq, _ = _counts_call(_as_f64(q, dev), _as_f64(ref, dev), N.PCT_OF_SCORE, counts=True)
    if F.is_tensor(q):
        return less, leq
    return less.cpu().numpy(), leq.cpu().numpy()


def _torch_dtype(dtype):
    import torch
    if dtype is None or isinstance(dtype, torch.dtype):
        return dtype
    return getattr(torch, np.dtype(dtype).name)


def score2percentile(scores, ref_scores, out_dtype=None):
    """``scipy.stats.percentileofscore(ref_scores, s)`` (kind 'rank') for every ``s`` of ``scores`` at once: what the reference's
    ``score2percentile`` (vis_utils/heatmap_utils.py:22-24) gives score by score, in the shape of ``scores``.  float64, or
    ``out_dtype`` (``torch.float32`` reproduces the reference's storage, which assigns into a float32 array).  ``scores`` as a
    numpy array: a numpy array comes back (copied from the device, not recomputed); as a device tensor: a tensor.  ``ref_scores``
    may be either kind."""
    scores, ref_scores = F.as_array(scores), F.as_array(ref_scores)
    dev = _check_score_args("score2percentile", scores, ref_scores)
    out = _counts_call(_as_f64(scores, dev), _as_f64(ref_scores, dev), N.PCT_OF_SCORE, pct=True)[2].reshape(tuple(scores.shape))
    dtype = _torch_dtype(out_dtype)
    if dtype is not None:
        out = out.to(dtype)
    return out if F.is_tensor(scores) else out.cpu().numpy()


# ------------------------------------------------------------------------------------------------------------------------------
# the device call
# ------------------------------------------------------------------------------------------------------------------------------
def _host_inputs(scores, coords, patch_size, scale, *, binarize, thresh, convert_to_percentiles):
    """Numpy inputs: ``(xy int32 [N, 2], v float64 [N], paint uint8 [N])`` with the value checks done, or None when an input
    is a device tensor (``_device_inputs`` then works on the device)."""
    if F.is_tensor(scores) or F.is_tensor(coords):
        return None
    xy, _, _ = scaled_geometry(coords, patch_size, scale)
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    if len(s):
        _check_values(int(xy.min()), int(xy.max()), bool(np.isfinite(s).all()))
    v, paint = patch_values(s, binarize=binarize, thresh=thresh, convert_to_percentiles=convert_to_percentiles)
    return xy.astype(np.int32), v, paint


def _device_inputs(host, scores, coords, patch_size, scale, dev, *, binarize, thresh, convert_to_percentiles):
    """``(xy int32 [N, 2], v float64 [N], paint uint8 [N], pw, ph)`` on ``dev``."""
    import torch
    _, pw, ph = scaled_geometry(np.zeros((0, 2), dtype=np.int64), patch_size, scale)
    if host is not None:
        return tuple(torch.from_numpy(a).to(dev) for a in host) + (pw, ph)
    s = (scores if F.is_tensor(scores) else torch.from_numpy(np.asarray(scores))).to(dev, torch.float64).reshape(-1).contiguous()
    c = (coords if F.is_tensor(coords) else torch.from_numpy(np.asarray(coords))).to(dev)
    sc = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
    c = c.to(torch.float64)
    xyf = torch.ceil(torch.stack([c[:, 0] * float(sc[0]), c[:, 1] * float(sc[1])], dim=1))   # (scalars: no host-to-device copy)
    n = s.numel()
    if n and not torch.cuda.is_current_stream_capturing():
        bad = torch.stack([(xyf < 0).any(), (xyf >= 2.0 ** 31).any(), ~torch.isfinite(s).all()]).cpu().numpy()   # one synchronisation
        _check_values(-1 if bad[0] else 0, 2 ** 31 if bad[1] else 0, not bad[2])
    if convert_to_percentiles:   # (the finiteness check above has refused a NaN already)
        s = _counts_call(s, s, N.PCT_RANKDATA, pct=True)[2]
    s = torch.div(s, torch.full_like(s, 100.0))   # tensor / tensor: a true division (by a Python scalar torch multiplies by 1 / 100)
    keep = s >= threshold_of(n, binarize, thresh)
    v = torch.where(keep, torch.ones_like(s) if binarize else s, torch.zeros_like(s))
    return xyf.to(torch.int32).contiguous(), v.contiguous(), keep.to(torch.uint8), pw, ph


def _workspace(n, pw, ph, w, h, dev):
    """The scratch of the per-tile patch lists (``_frontend.scratch``); the library sizes it 0 for a call beyond the kernel's envelope.
    It keeps its name and signature because tests/test_gpu_workspace_guard.py replaces it with a fenced buffer."""
    ws, need = F.scratch("hipt_heatmap_workspace_bytes", n, pw, ph, w, h, dev=dev)
    if n and not need:
        raise ValueError(f"heatmap: {n} patches of {pw} x {ph} on a {w} x {h} canvas are beyond the kernel's envelope "
                         f"(patches x tiles per patch < 2^31)")
    return ws


def heatmap_overlay(scores, coords, patch_size, scale, region_size, *, binarize=False, thresh=0.5, convert_to_percentiles=False,
                    device=None):
    """``(overlay float64 [h, w], count int32 [h, w])``: per pixel the mean over the covering patches of the patch value (the
    score / 100 where it reaches the threshold, else 0; 1 or 0 and the mean rounded half to even when ``binarize``), and the
    number of covering patches.  Numpy in, numpy out; device tensors in, tensors out."""
    import torch
    scores, coords = F.as_array(scores), F.as_array(coords)
    n, w, h = _check_geometry(scores, coords, patch_size, scale, region_size)
    how = dict(binarize=binarize, thresh=thresh, convert_to_percentiles=convert_to_percentiles)
    host = _host_inputs(scores, coords, patch_size, scale, **how)
    dev = F.resolve_device("heatmap", device, (scores, coords))
    with torch.cuda.device(dev):
        xy, v, paint, pw, ph = _device_inputs(host, scores, coords, patch_size, scale, dev, **how)
        ws = _workspace(n, pw, ph, w, h, dev)
        overlay = torch.empty((h, w), dtype=torch.float64, device=dev)
        count = torch.empty((h, w), dtype=torch.int32, device=dev)
        N.call("hipt_heatmap_overlay", N.ptr(xy), N.ptr(v), N.ptr(paint), n, pw, ph, w, h, int(bool(binarize)), N.ptr(overlay),
               N.ptr(count), None, N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    if F.is_tensor(scores):
        return overlay, count
    return overlay.cpu().numpy(), count.cpu().numpy()


def render_heatmap(scores, coords, patch_size, scale, region_size, *, canvas=None, mask=None, alpha=0.4, binarize=False, thresh=0.5,
                   convert_to_percentiles=False, cmap="coolwarm", blur=False, device=None, return_overlay=False):
    """The heat-map image, uint8 ``[h, w, 3]``, of ``scores [N]`` at ``coords [N, 2]`` (level-0 pixels relative to the region's
    top-left corner; ``patch_size`` level-0 pixels; ``scale`` = 1 / downsample; ``region_size = (w, h)`` canvas pixels).

    A pixel is painted with ``cmap(overlay)`` where a covering patch reaches the threshold and ``mask`` (bool ``[h, w]``) is true or
    absent; elsewhere it keeps ``canvas`` (uint8 ``[h, w, 3]``; absent: white).  With ``alpha < 1`` the whole image is then blended
    with the canvas, ``rint(float32(img) * float32(alpha) + float32(canvas) * float32(1 - alpha))`` saturated to uint8.
    Numpy in, numpy out; ``scores`` as a device tensor: everything stays on the device and a tensor comes back.
    ``return_overlay=True`` returns ``(img, overlay float64 [h, w])``."""
    import torch
    if blur:
        raise NotImplementedError("render_heatmap: blur=True is not supported (cv2's fixed-point uint8 Gaussian blur cannot be "
                                  "reproduced without cv2; DESIGN.md 14)")
    scores, coords, mask, canvas = F.as_array(scores), F.as_array(coords), F.as_array(mask), F.as_array(canvas)
    n, w, h = _check_geometry(scores, coords, patch_size, scale, region_size)
    F.check_image("heatmap", "mask", mask, (h, w), ("bool",))
    F.check_image("heatmap", "canvas", canvas, (h, w, 3), ("uint8",))
    alpha = float(alpha)
    if math.isnan(alpha):
        raise ValueError("heatmap: alpha is NaN")
    table = F.table_host(colour_table, cmap)
    how = dict(binarize=binarize, thresh=thresh, convert_to_percentiles=convert_to_percentiles)
    host = _host_inputs(scores, coords, patch_size, scale, **how)
    dev = F.resolve_device("heatmap", device, (scores, coords, mask, canvas))
    with torch.cuda.device(dev):
        xy, v, paint, pw, ph = _device_inputs(host, scores, coords, patch_size, scale, dev, **how)
        lut = F.table_on(colour_table, cmap, table, dev)
        mask_d = F.to_device(mask, dev)
        canvas_d = F.to_device(canvas, dev)
        ws = _workspace(n, pw, ph, w, h, dev)
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        overlay = torch.empty((h, w), dtype=torch.float64, device=dev) if return_overlay else None
        N.call("hipt_heatmap_render", N.ptr(xy), N.ptr(v), N.ptr(paint), n, pw, ph, w, h, int(bool(binarize)), N.ptr(mask_d),
               N.ptr(canvas_d), N.ptr(lut), alpha, N.ptr(img), N.ptr(overlay), N.ptr(ws), ws.numel(), N.stream_ptr(dev))
    if not F.is_tensor(scores):
        img = img.cpu().numpy()
        overlay = overlay.cpu().numpy() if return_overlay else None
    return (img, overlay) if return_overlay else img


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's method
# ------------------------------------------------------------------------------------------------------------------------------
def screen_coords(scores, coords, top_left, bot_right):
    """The patches whose corner lies inside the box, both ends included (wsi_core/wsi_utils.py:129-135)."""
    keep = np.logical_and(np.all(coords >= np.array(top_left), axis=1), np.all(coords <= np.array(bot_right), axis=1))
    return scores[keep], coords[keep]


def sample_rois(scores, coords, k=5, mode="range_sample", seed=1, score_start=0.45, score_end=0.55, top_left=None, bot_right=None):
    """``wsi_core.wsi_utils.sample_rois`` (:137-158): the patches ``create_heatmaps.py`` saves beside a heat-map.  The scores become
    percentiles (device tensors: on the device); the bounding-box screen, the window of ``range_sample`` with ``np.random.seed(seed)``
    and ``np.random.choice``, and the ``argsort`` behind ``topk`` / ``reverse_topk`` follow on the host in the reference's order, so
    a seed picks what it picks there.  Returns ``{'sampled_coords', 'sampled_scores'}`` as numpy arrays (k winners), whatever came
    in.  As in the reference, an empty window of ``range_sample`` yields index -1: the last patch."""
    if mode not in ("range_sample", "topk", "reverse_topk"):
        raise NotImplementedError(f"sample_rois: mode {mode!r}")
    scores, coords = F.as_array(scores), F.as_array(coords)
    if scores.ndim == 2:
        scores = scores.flatten()
    scores = to_percentiles(scores)
    if F.is_tensor(scores):
        scores = scores.cpu().numpy()
    if F.is_tensor(coords):
        coords = coords.cpu().numpy()
    if top_left is not None and bot_right is not None:
        scores, coords = screen_coords(scores, coords, top_left, bot_right)
    if mode == "range_sample":
        np.random.seed(seed)
        indices = np.where(np.logical_and(scores >= score_start, scores <= score_end))[0]
        sampled_ids = -1 if len(indices) < 1 else np.random.choice(indices, min(k, len(indices)), replace=False)
    elif mode == "topk":
        sampled_ids = scores.argsort()[::-1][:k]
    else:
        sampled_ids = scores.argsort()[:k]
    return {"sampled_coords": coords[sampled_ids], "sampled_scores": scores[sampled_ids]}


def compute_from_batches(model, feature_extractor, batches, clam_pred=None, ref_scores=None, out_dtype="float32", on_batch=None):
    """The loop body of ``vis_utils.heatmap_utils.compute_from_patches`` (:60-89) over any iterable of ``(roi, coords)``: features
    = ``feature_extractor(roi)``, A = ``model(features, attention_only=True)``, row ``clam_pred`` of it where the model has more
    than one branch, as a column ``[n, 1]``; with ``ref_scores`` every score becomes its percentile among them (``score2percentile``,
    on the device, stored as ``out_dtype``: a torch or numpy dtype or its name; float32 is the dtype of the reference's array).  ``roi`` goes to the
    extractor as the loader hands it over.  ``on_batch(scores, coords, features)`` is called once per batch, in order, for the
    caller's writer (the reference appends to an h5 file there).  Returns ``(scores [sum n, 1] tensor, coords [sum n, 2] numpy)``."""
    import torch
    out_dtype = _torch_dtype(out_dtype)
    if ref_scores is not None:
        ref_scores = F.as_array(ref_scores)
        _check_score_args("compute_from_batches", None, ref_scores)   # (the reference scores are looked at once, not per batch)
    ref = None
    all_scores, all_coords = [], []
    for roi, coords in batches:
        with torch.no_grad():
            features = feature_extractor(roi)
            a = model(features, attention_only=True)
            if a.size(0) > 1:   # CLAM multi-branch attention
                if clam_pred is None:
                    raise ValueError(f"compute_from_batches: the model has {a.size(0)} attention branches; clam_pred says which to take")
                a = a[clam_pred]
            a = a.reshape(-1, 1)
            if ref_scores is not None:
                if ref is None or ref.device != a.device:
                    _check_one_device("compute_from_batches", (a, ref_scores))
                    ref = _as_f64(ref_scores, F.resolve_device("heatmap", None, (a, ref_scores)))
                F.check_no_nan("compute_from_batches", scores=a)
                a = _counts_call(_as_f64(a, ref.device), ref, N.PCT_OF_SCORE, pct=True)[2].reshape(-1, 1).to(out_dtype)
        c = coords.cpu().numpy() if F.is_tensor(coords) else np.asarray(coords)
        if on_batch is not None:
            on_batch(a, c, features)
        all_scores.append(a)
        all_coords.append(c)
    if not all_scores:
        return torch.zeros((0, 1), dtype=out_dtype), np.zeros((0, 2), dtype=np.int64)
    return torch.cat(all_scores), np.concatenate(all_coords)


def vis_heatmap(wsi_object, scores, coords, vis_level=-1, top_left=None, bot_right=None, patch_size=(256, 256), blank_canvas=False,
                canvas_color=(220, 20, 50), alpha=0.4, blur=False, overlap=0.0, segment=True, use_holes=True,
                convert_to_percentiles=False, binarize=False, thresh=0.5, max_size=None, custom_downsample=1, cmap="coolwarm",
                device=None, device_mask=False):
    """``WholeSlideImage.visHeatmap`` with its keyword arguments and defaults; returns a ``PIL.Image``.

    ``wsi_object`` is used by duck typing: ``level_downsamples``, ``level_dim``, ``wsi.get_best_level_for_downsample``,
    ``wsi.read_region`` and (with ``segment``) ``get_seg_mask``.  The canvas is fetched with ONE ``read_region`` of the whole
    region (the reference reads it once for painting and again block by block for the blend, the same pixels).  ``canvas_color``
    and ``overlap`` are accepted and unused, as in the reference with ``blur=False``.  The caller's ``scores`` are not modified.
    ``device_mask=True`` (with ``segment``) builds the tissue mask on the device from ``contours_tissue`` / ``holes_tissue``
    (``segment.get_seg_mask_like``; no cv2, no ``get_seg_mask`` method needed) and hands the tensor to ``render_heatmap``."""
    from PIL import Image
    if blur:
        raise NotImplementedError("vis_heatmap: blur=True is not supported (DESIGN.md 14)")
    if vis_level < 0:
        vis_level = wsi_object.wsi.get_best_level_for_downsample(32)
    downsample = wsi_object.level_downsamples[vis_level]
    scale = [1 / downsample[0], 1 / downsample[1]]
    scores = np.asarray(scores)
    coords = np.asarray(coords)
    if scores.ndim == 2:
        scores = scores.flatten()
    threshold = threshold_of(len(scores), binarize, thresh)   # 1 / N counts the patches BEFORE the screening, as the reference
    if top_left is not None and bot_right is not None:
        scores, coords = screen_coords(scores, coords, top_left, bot_right)
        coords = coords - top_left
        top_left, bot_right = tuple(top_left), tuple(bot_right)
        w, h = tuple((np.array(bot_right) * scale).astype(int) - (np.array(top_left) * scale).astype(int))
        region_size = (int(w), int(h))
    else:
        region_size = tuple(int(v) for v in wsi_object.level_dim[vis_level])
        top_left = (0, 0)
    if segment and device_mask:
        from .segment import get_seg_mask_like
        mask = get_seg_mask_like(wsi_object, region_size, scale, use_holes=use_holes, offset=tuple(top_left), device=device)
    else:
        mask = wsi_object.get_seg_mask(region_size, scale, use_holes=use_holes, offset=tuple(top_left)) if segment else None
    canvas = None if blank_canvas else np.array(wsi_object.wsi.read_region(top_left, vis_level, region_size).convert("RGB"))
    img = render_heatmap(scores, coords, patch_size, scale, region_size, canvas=canvas, mask=mask, alpha=alpha, binarize=binarize,
                         thresh=threshold, convert_to_percentiles=convert_to_percentiles, cmap=cmap, device=device)
    img = Image.fromarray(img)
    w, h = img.size
    if custom_downsample > 1:
        img = img.resize((int(w / custom_downsample), int(h / custom_downsample)))
    if max_size is not None and (w > max_size or h > max_size):
        factor = max_size / w if w > h else max_size / h
        img = img.resize((int(w * factor), int(h * factor)))
    return img
