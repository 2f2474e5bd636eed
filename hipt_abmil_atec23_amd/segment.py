"""The tissue mask of ``WholeSlideImage.segmentTissue`` on the HIP library (csrc/segment.hip).

``segmentTissue`` (wsi_core/WholeSlideImage.py:111-203) makes a binary picture of the segmentation level in four whole-image cv2
calls -- ``cvtColor(RGB2HSV)``'s saturation, ``medianBlur``, ``threshold`` (fixed or Otsu), ``morphologyEx(MORPH_CLOSE)`` -- traces
its contours and filters them by area.  The four pixel stages are 8-bit integer work (Otsu: integer counts and a short float64
scan), restated from OpenCV's published implementation and run on the device: ``tissue_mask`` is one native call, the stage
functions expose each step.  Contour tracing (``cv2.findContours(mask, RETR_CCOMP, CHAIN_APPROX_NONE)``) runs on the device too
(csrc/contours.hip): ``trace_contours`` keeps the points there, ``find_contours`` returns cv2's format and is what to
hand ``segment_tissue`` as ``find_contours=``; with None it imports cv2, as before.  The area filter (``filter_contours``,
``contour_area``) is pure numpy.

cv2 is not a dependency and was not available to compare against: agreement with cv2's own bytes is argued from OpenCV's source
(DESIGN.md 26), not measured; the tests compare with a numpy restatement of the same definitions (tests/segment_ref.py).
For the contours: the set of borders and every border's point sequence follow the published algorithm (Suzuki and Abe 1985) and
equal a sequential restatement of it (tests/contour_ref.py); the ORDER of the list, and agreement with cv2's own return values,
are argued from OpenCV's source and not measured.
"""
from __future__ import annotations

import numpy as np

from . import _frontend as F
from . import _native as N

MAX_MEDIAN, MAX_CLOSE = N.SEGMENT_MAX_MEDIAN, N.SEGMENT_MAX_CLOSE


def _check_median(what: str, k) -> int:
    k = F.check_int(what, "the median window", k, 1, 1 << 30)
    if k % 2 == 0 or k > MAX_MEDIAN:
        raise ValueError(f"{what}: the median window is odd and at most {MAX_MEDIAN}, got {k}")
    return k


def tissue_mask(img, sthresh=20, sthresh_up=255, mthresh=7, close=0, use_otsu=False, out=None, return_parts=False, device=None):
    """The binary picture ``segmentTissue`` traces: ``img`` -- uint8 ``[H, W, 3]`` or ``[H, W, 4]`` (``np.array(read_region(...))`` is
    RGBA; the fourth channel is ignored), a numpy array or a device tensor -- through saturation, ``mthresh x mthresh`` median,
    threshold (``> sthresh``, or Otsu's level with ``use_otsu``; foreground value ``sthresh_up``) and a ``close x close`` closing
    (0: none).  Returns a uint8 device tensor ``[H, W]`` (``out`` where given); with ``return_parts`` also the median plane, the
    saturation plane and the int32 ``[1]`` tensor of the threshold used.  One native call on the current stream; a device tensor
    is not copied to the host, and Otsu's level never leaves the device.  ValueError -- before any native call -- for another
    dtype or shape, a CPU tensor, thresholds outside 0 .. 255, an even ``mthresh`` or one above 15, ``close`` outside 0 .. 128."""
    import torch
    what = "tissue_mask"
    sthresh = F.check_int(what, "sthresh", sthresh, 0, 255)
    sthresh_up = F.check_int(what, "sthresh_up", sthresh_up, 0, 255)
    mthresh = _check_median(what, mthresh)
    close = F.check_int(what, "close", close, 0, MAX_CLOSE)
    x = F.as_device_u8(what, img, device, dims=3, channels=(3, 4))
    h, w, ch = (int(v) for v in x.shape)
    dev = x.device
    out = F.check_out(what, out, (h, w), torch.uint8, dev, not_alias=(x,))
    with torch.cuda.device(dev):
        med = sat = thr = None
        if return_parts:
            med = torch.empty((h, w), dtype=torch.uint8, device=dev)
            sat = torch.empty((h, w), dtype=torch.uint8, device=dev)
            thr = torch.empty((1,), dtype=torch.int32, device=dev)
        ws, need = F.scratch("hipt_segment_workspace_bytes", h, w, close, dev=dev)
        N.call("hipt_segment_mask", N.ptr(x), h, w, ch, sthresh, sthresh_up, mthresh, close, int(bool(use_otsu)), N.ptr(out), N.ptr(sat),
               N.ptr(med), N.ptr(thr), N.ptr(ws), need, N.stream_ptr(dev))
    return (out, med, sat, thr) if return_parts else out


def saturation_u8(img, out=None, device=None):
    """The S channel of ``cv2.cvtColor(img, cv2.COLOR_RGB2HSV)`` for a uint8 ``[H, W, 3|4]`` image, as a uint8 device tensor ``[H, W]``."""
    import torch
    x = F.as_device_u8("saturation_u8", img, device, dims=3, channels=(3, 4))
    h, w, ch = (int(v) for v in x.shape)
    out = F.check_out("saturation_u8", out, (h, w), torch.uint8, x.device, not_alias=(x,))
    with torch.cuda.device(x.device):
        N.call("hipt_segment_saturation", N.ptr(x), h, w, ch, N.ptr(out), N.stream_ptr(x.device))
    return out


def median_blur_u8(x, ksize, out=None, device=None):
    """``cv2.medianBlur(x, ksize)`` of a uint8 plane ``[H, W]``: the exact median, borders replicated; ``ksize`` odd, 1 .. 15."""
    import torch
    ksize = _check_median("median_blur_u8", ksize)
    x = F.as_device_u8("median_blur_u8", x, device, dims=2)
    h, w = (int(v) for v in x.shape)
    out = F.check_out("median_blur_u8", out, (h, w), torch.uint8, x.device, not_alias=(x,))
    with torch.cuda.device(x.device):
        N.call("hipt_segment_median", N.ptr(x), h, w, ksize, N.ptr(out), N.stream_ptr(x.device))
    return out


def otsu_threshold(x, device=None):
    """``(hist int32 [256], thresh int32 [1])`` of a uint8 plane, both on the device: the counts, and the level
    ``cv2.threshold(x, 0, 255, cv2.THRESH_OTSU)`` returns."""
    import torch
    x = F.as_device_u8("otsu_threshold", x, device, dims=2)
    h, w = (int(v) for v in x.shape)
    with torch.cuda.device(x.device):
        hist = torch.empty((256,), dtype=torch.int32, device=x.device)
        thr = torch.empty((1,), dtype=torch.int32, device=x.device)
        N.call("hipt_segment_otsu", N.ptr(x), h, w, N.ptr(hist), N.ptr(thr), N.stream_ptr(x.device))
    return hist, thr


def morph_close_u8(x, size, out=None, device=None):
    """``cv2.morphologyEx(x, cv2.MORPH_CLOSE, np.ones((size, size), np.uint8))`` of a uint8 plane (any bytes, not only a binary
    picture); ``size`` 0 .. 128, 0 and 1 give a copy."""
    import torch
    size = F.check_int("morph_close_u8", "size", size, 0, MAX_CLOSE)
    x = F.as_device_u8("morph_close_u8", x, device, dims=2)
    h, w = (int(v) for v in x.shape)
    out = F.check_out("morph_close_u8", out, (h, w), torch.uint8, x.device, not_alias=(x,))
    with torch.cuda.device(x.device):
        ws, need = F.scratch("hipt_segment_workspace_bytes", h, w, size, dev=x.device)
        N.call("hipt_segment_close", N.ptr(x), h, w, size, N.ptr(out), N.ptr(ws), need, N.stream_ptr(x.device))
    return out


# ---- contours ------------------------------------------------------------------------------------------------------------------
def _order_borders(start, kind, parent):
    """The ONE place that decides the order of the list (argued from OpenCV's tree insertion, not measured against cv2): top-level
    borders in descending raster order of their start pixel, each followed at once by its hole borders in descending raster order
    of theirs.  ``start`` / ``parent`` are pixel numbers ``y * W + x`` (``parent``: the start of the outer border a hole lies on),
    ``kind`` is 0 outer / 1 hole.  Returns the permutation: ``order[j]`` is the table row of the j-th border of the list."""
    top = np.where(kind == 0, start, parent)
    return np.lexsort((-start, kind, -top))


def _hierarchy(kind) -> np.ndarray:
    """int32 ``[C, 4]`` = ``[next, previous, first_child, parent]`` of a list in ``_order_borders``' order (``kind`` in that order):
    two levels, siblings linked in list order, -1 for none."""
    c = len(kind)
    idx = np.arange(c)
    hier = np.full((c, 4), -1, dtype=np.int32)
    outer = np.flatnonzero(kind == 0)
    hier[outer[:-1], 0] = outer[1:]
    hier[outer[1:], 1] = outer[:-1]
    hole = kind == 1
    after_hole = np.append(hole[1:], False)    # the next border of the list is a hole
    before_hole = np.insert(hole[:-1], 0, False)
    hier[hole & after_hole, 0] = idx[hole & after_hole] + 1
    hier[hole & before_hole, 1] = idx[hole & before_hole] - 1
    hier[~hole & after_hole, 2] = idx[~hole & after_hole] + 1
    hier[hole, 3] = np.maximum.accumulate(np.where(hole, -1, idx))[hole]
    return hier


def _check_mask(what: str, mask) -> None:
    if not isinstance(mask, np.ndarray) and not F.is_tensor(mask):
        raise ValueError(f"{what}: the mask is a numpy array or a device tensor, got {type(mask).__name__}")
    shape = [int(v) for v in mask.shape]
    if str(mask.dtype).replace("torch.", "") != "uint8" or len(shape) != 2:
        raise ValueError(f"{what}: the mask is uint8 [H, W], got {mask.dtype} {shape}")
    if shape[0] < 1 or shape[1] < 1 or (shape[0] + 2) * (shape[1] + 2) > N.CONTOURS_MAX_PLANE:
        raise ValueError(f"{what}: a mask of {shape[0]} x {shape[1]}: at least one pixel, and (H + 2) * (W + 2) at most "
                         f"{N.CONTOURS_MAX_PLANE} (8192 x 8192 is inside)")


def trace_contours(mask, device=None):
    """``cv2.findContours(mask, cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)`` with the result left on the device: ``(points int32 [P, 2]
    of (x, y), offsets int64 [C + 1], hierarchy int32 [C, 4])``; contour ``j`` is ``points[offsets[j]:offsets[j + 1]]``, a row of
    ``hierarchy`` is ``[next, previous, first_child, parent]``.  ``mask``: uint8 ``[H, W]``, a numpy array or a device tensor; any
    non-zero byte is foreground, and foreground may touch the edge.  Suzuki-Abe border following, foreground 8-connected and
    background 4-connected (the header states the rules); the same mask gives the same bytes in every run.  The set of borders and
    every border's points follow the published algorithm; the order of the list (``_order_borders``) and agreement with cv2's own
    return values are argued, not measured.  Two native calls on the current stream with ONE small read-back between them (the
    table of borders), so the call synchronises and cannot be captured into a graph.  ValueError -- before any native call -- for
    another dtype or rank, a CPU tensor, an empty plane or one with ``(H + 2) * (W + 2)`` above 2^27; RuntimeError after the
    read-back for a plane of more than 2^22 pixels that holds more than 2^24 border pixels or 2^22 borders."""
    import torch
    what = "trace_contours"
    _check_mask(what, mask)
    x = F.as_device_u8(what, mask, device, dims=2)
    h, w = (int(v) for v in x.shape)
    dev = x.device
    with torch.cuda.device(dev):
        rows = min(h * w, N.CONTOURS_MAX_BORDERS) + 1
        table = torch.empty((rows, 4), dtype=torch.int32, device=dev)
        ws, need = F.scratch("hipt_contours_workspace_bytes", h, w, dev=dev)
        N.call("hipt_contours_trace", N.ptr(x), h, w, N.ptr(table), N.ptr(ws), need, N.stream_ptr(dev))
        head = table[0].cpu().numpy()   # the read-back: (border pixels, borders, passes, unsettled)
        nb, c = int(head[0]), int(head[1])
        if nb > min(h * w, N.CONTOURS_MAX_BORDER_PIXELS) or c > rows - 1:
            raise RuntimeError(f"{what}: {nb} border pixels / {c} borders in a mask of {h} x {w}: beyond the room of "
                               f"{N.CONTOURS_MAX_BORDER_PIXELS} / {N.CONTOURS_MAX_BORDERS}")
        if c == 0:
            return (torch.empty((0, 2), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev),
                    torch.empty((0, 4), dtype=torch.int32, device=dev))
        tab = table[1:1 + c].cpu().numpy().astype(np.int64)
        start, kind, length, parent = tab[:, 0], tab[:, 1], tab[:, 2], tab[:, 3]
        if (length < 1).any():
            raise RuntimeError(f"{what}: a border of the {h} x {w} mask was not ranked (internal error)")
        order = _order_borders(start, kind, parent)
        offsets = np.zeros(c + 1, dtype=np.int64)
        np.cumsum(length[order], out=offsets[1:])
        p = int(offsets[-1])
        where = np.empty(c, dtype=np.int32)
        where[order] = offsets[:-1]
        points = torch.empty((p, 2), dtype=torch.int32, device=dev)
        where_dev = torch.from_numpy(where).to(dev)
        N.call("hipt_contours_emit", h, w, N.ptr(table), N.ptr(where_dev), c, p, N.ptr(points), N.ptr(ws), need, N.stream_ptr(dev))
        return points, torch.from_numpy(offsets).to(dev), torch.from_numpy(_hierarchy(kind[order])).to(dev)


def find_contours(mask, device=None):
    """``cv2.findContours(mask, cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)`` in cv2's return format, traced on the device
    (``trace_contours``): ``(contours, hierarchy)``, a tuple of int32 ``[n, 1, 2]`` arrays and an int32 ``[1, C, 4]`` array; an empty
    mask gives ``((), None)``.  Hand it to ``segment_tissue`` as ``find_contours=segment.find_contours``: the mask then stays on the
    device.  What is argued and what is measured: see ``trace_contours``."""
    points, offsets, hierarchy = trace_contours(mask, device)
    if hierarchy.shape[0] == 0:
        return (), None
    pts, off = points.cpu().numpy(), offsets.cpu().numpy()
    return tuple(pts[off[j]:off[j + 1]].reshape(-1, 1, 2) for j in range(len(off) - 1)), hierarchy.cpu().numpy()[None]


find_contours.takes_device_mask = True   # segment_tissue hands such a tracer the device tensor, not the read-back copy


# ---- host glue: pure numpy ------------------------------------------------------------------------------------------------------
def contour_area(cont) -> float:
    """``cv2.contourArea(cont)``: the shoelace formula in float64 over the closed polygon ``cont`` (``[n, 1, 2]`` or ``[n, 2]``)."""
    p = np.asarray(cont, dtype=np.float64).reshape(-1, 2)
    if len(p) == 0:
        return 0.0
    q = np.roll(p, 1, axis=0)   # the previous vertex; the first one's is the last
    return float(abs(0.5 * np.sum(q[:, 0] * p[:, 1] - p[:, 0] * q[:, 1])))


def scale_contours(contours, scale):
    """``WholeSlideImage.scaleContourDim``: ``[np.array(cont * scale, dtype='int32') for cont in contours]`` -- a float64 product,
    then truncation toward zero."""
    return [np.array(cont * scale, dtype="int32") for cont in contours]


def scale_holes(holes, scale):
    """``WholeSlideImage.scaleHolesDim``: the same for the list of every contour's list of holes."""
    return [[np.array(hole * scale, dtype="int32") for hole in hs] for hs in holes]


def _draw_order(areas) -> np.ndarray:
    """The ONE place that decides ``get_seg_mask``'s draw order: by area, descending, stable (equal areas keep their order; the
    reference's ``sorted`` over ``zip(contours, holes)`` compares arrays on a tie and raises, so a tie has no behaviour to match)."""
    return np.argsort(-np.asarray(areas, dtype=np.float64), kind="stable")


def _int_points(what: str, cont) -> np.ndarray:
    a = np.asarray(cont)
    if a.dtype.kind not in "iu" or a.size % 2 or (a.size and (a.ndim < 2 or a.shape[-1] != 2)):
        raise ValueError(f"{what}: a contour is an integer array [n, 1, 2] or [n, 2] of (x, y), got {a.dtype} {list(a.shape)}")
    a = a.reshape(-1, 2)
    if a.size and (a.min() < -(1 << 31) or a.max() >= 1 << 31):
        raise ValueError(f"{what}: a contour's coordinates must fit int32")
    return a.astype(np.int32)


def _flatten_lists(what: str, contours, holes):
    """cv2-style lists as one polygon list: every contour followed at once by its holes.  ``(points int32 [P, 2], offsets int64,
    first [n]: the polygon index of contour i, n_holes [n])``."""
    contours = list(contours)
    holes = [[] for _ in contours] if holes is None else [list(hs) for hs in holes]
    if len(holes) != len(contours):
        raise ValueError(f"{what}: {len(contours)} contours but {len(holes)} lists of holes (one list per contour, possibly empty)")
    polys, first, n_holes = [], [], []
    for cont, hs in zip(contours, holes):
        first.append(len(polys))
        n_holes.append(len(hs))
        polys.append(_int_points(what, cont))
        polys += [_int_points(what, hole) for hole in hs]
    offsets = np.zeros(len(polys) + 1, dtype=np.int64)
    np.cumsum([len(p) for p in polys], out=offsets[1:])
    points = np.concatenate(polys) if polys else np.zeros((0, 2), np.int32)
    return np.ascontiguousarray(points, dtype=np.int32), offsets, np.array(first, np.int64), np.array(n_holes, np.int64)


def _split_traced(what: str, n_polys: int, hierarchy):
    """``(first, n_holes)`` of a traced polygon list: without a hierarchy every polygon is a contour without holes; with one
    (``[C, 4]``, column 3 the parent; read back if it is a device tensor) the polygons without a parent are the contours and each
    one's holes are the polygons that follow it at once and name it as their parent -- the order ``trace_contours`` returns."""
    if hierarchy is None:
        return np.arange(n_polys, dtype=np.int64), np.zeros(n_polys, dtype=np.int64)
    hier = hierarchy.cpu().numpy() if F.is_tensor(hierarchy) else np.asarray(hierarchy)
    if hier.shape != (n_polys, 4):
        raise ValueError(f"{what}: the hierarchy of {n_polys} polygons is [{n_polys}, 4], got {list(hier.shape)}")
    parent = hier[:, 3].astype(np.int64)
    first = np.flatnonzero(parent == -1)
    owner = np.maximum.accumulate(np.where(parent == -1, np.arange(n_polys), -1))   # the last contour at or before each polygon
    if n_polys and (parent[0] != -1 or not np.array_equal(np.where(parent == -1, -1, owner), parent)):
        raise ValueError(f"{what}: every hole must follow its contour at once (the order trace_contours returns)")
    return first, np.diff(np.append(first, n_polys)) - 1


def seg_mask(contours, holes, region_size, scale, use_holes=False, offset=(0, 0), out=None, device=None, order=None, _max_cols=0):
    """``WholeSlideImage.get_seg_mask`` (wsi_core/WholeSlideImage.py:741-757) on the device: the bool mask ``[h, w]`` (``region_size =
    (w, h)``) of the contours scaled by ``scale`` (``(cont * scale).astype(int32)``) and moved by ``(offset * scale * -1)
    .astype(int32)``, drawn in descending order of their scaled area as ``cv2.drawContours(..., thickness=-1)`` fills them -- each
    contour with 1 and, with ``use_holes``, all its holes together with 0; later contours overwrite earlier ones.  One native call
    (csrc/fill.hip); the same input gives the same bytes in every run.

    ``contours`` / ``holes``: cv2-style lists -- integer arrays ``[n, 1, 2]`` or ``[n, 2]``, and one list of such arrays per contour
    (``None``: no holes), what ``filter_contours`` and ``segment_tissue`` produce -- or, with ``holes=None``, a traced polygon list
    ``(points int32 [P, 2], offsets int64 [C + 1])`` or ``(points, offsets, hierarchy)`` as ``trace_contours`` returns it, numpy
    arrays or device tensors: with a hierarchy the polygons without a parent are the contours and their children the holes (the
    small hierarchy is read back; hand it over as a numpy array to avoid that).  Device tensors are not copied to the host, and a
    device tensor comes back either way (``out`` where given: a contiguous bool or uint8 ``[h, w]`` tensor, fully written).

    The draw order needs every contour's scaled area: with ``order=None`` it is computed on the host from the same scaled integers
    (a stable descending sort: equal areas keep their order, where the reference's ``sorted`` raises), which for device tensors
    costs ONE read-back of the points and so synchronises -- the call cannot then be captured into a graph.  ``order``: a
    precomputed draw order, a permutation of the contour indices; with it and device tensors the points stay where they are
    (one scalar, the largest coordinate, is still read to check the envelope, and the small collection table is uploaded: the
    native call itself is one launch that can be captured, this front-end is not) and every workgroup walks every collection,
    as the rows a contour lies on are then unknown.

    Agreement with cv2's own bytes is argued, not measured (DESIGN.md 32 lists what carries the risk); for contours whose points
    are at most a pixel apart after scaling the mask does not depend on any of it.  No contours at all give an all-zero mask (the
    reference raises).  ValueError -- before any native call -- for a malformed contour, a canvas side outside 1 ..
    65 535, more than 2^27 points, scaled and moved coordinates beyond +-2^20, a CPU tensor, an ``order`` that is no permutation."""
    import torch
    what = "seg_mask"
    w, h = (F.check_int(what, f"region_size[{k}]", v, 1, N.FILL_MAX_DIM) for k, v in enumerate(region_size))
    _max_cols = F.check_int(what, "_max_cols", _max_cols, 0, N.FILL_MAX_COLS)
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
    if not np.isfinite(scale).all():
        raise ValueError(f"{what}: scale must be finite, got {scale.tolist()}")
    if np.shape(offset) != (2,):
        raise ValueError(f"{what}: offset is (x, y), got {offset!r}")
    off = (np.array(offset) * np.array(scale) * -1).astype(np.int32)     # the reference's expression, in its order
    if isinstance(contours, tuple) and len(contours) in (2, 3) and (F.is_tensor(contours[0]) or np.asarray(contours[0]).ndim == 2
                                                                    and np.asarray(contours[1]).ndim == 1):
        if holes is not None:
            raise ValueError(f"{what}: with a traced polygon list the holes come from its hierarchy; holes must be None")
        points, offsets = F.as_array(contours[0]), F.as_array(contours[1])
        kinds = (str(points.dtype).replace("torch.", ""), str(offsets.dtype).replace("torch.", ""))
        if kinds != ("int32", "int64") or len(points.shape) != 2 or points.shape[1] != 2 or len(offsets.shape) != 1 or offsets.shape[0] < 1:
            raise ValueError(f"{what}: a traced polygon list is (points int32 [P, 2], offsets int64 [C + 1]), got {kinds[0]} "
                             f"{list(points.shape)}, {kinds[1]} {list(offsets.shape)}")
        first, n_holes = _split_traced(what, int(offsets.shape[0]) - 1, contours[2] if len(contours) == 3 else None)
    else:
        points, offsets, first, n_holes = _flatten_lists(what, contours, holes)
    n, n_polys, n_points = len(first), int(offsets.shape[0]) - 1, int(points.shape[0])
    if n_points > N.FILL_MAX_POINTS:
        raise ValueError(f"{what}: {n_points} points; at most {N.FILL_MAX_POINTS}")
    if order is not None:
        order = np.asarray(order, dtype=np.int64).reshape(-1)
        if not np.array_equal(np.sort(order), np.arange(n)):
            raise ValueError(f"{what}: order must be a permutation of the {n} contour indices")
    on_device = F.is_tensor(points)
    host = None   # (points, offsets) on the host, where they are there or have to be fetched
    if not on_device:
        host = (points, offsets)
    elif order is None:
        host = (points.cpu().numpy(), offsets.cpu().numpy())             # the read-back
    y_lo = np.full(n_polys, -(1 << 31), dtype=np.int64)
    y_hi = np.full(n_polys, (1 << 31) - 1, dtype=np.int64)
    if host is not None:
        hp, ho = host
        if len(ho) != n_polys + 1 or ho[0] != 0 or ho[-1] != n_points or (np.diff(ho) < 0).any():
            raise ValueError(f"{what}: offsets must rise from 0 to the number of points, {n_points}")
        bound = int(np.abs(hp.astype(np.int64)).max()) if n_points else 0
        scaled = np.array(hp * scale, dtype="int32") + off               # what the kernel computes where it loads a vertex
        lens = np.diff(ho)
        full = lens > 0
        y_lo[:], y_hi[:] = 0, -1                                         # an empty polygon lies on no row
        if full.any():
            y_lo[full] = np.minimum.reduceat(scaled[:, 1], ho[:-1][full])
            y_hi[full] = np.maximum.reduceat(scaled[:, 1], ho[:-1][full])
        if order is None:
            areas = np.array([contour_area(scaled[ho[p]:ho[p + 1]]) for p in first], dtype=np.float64)
            order = _draw_order(areas)
    else:
        bound = int(points.abs().max()) if n_points else 0               # one scalar: the envelope is checked, never assumed
    reach = bound * float(np.abs(scale).max()) + int(np.abs(off.astype(np.int64)).max())
    if not reach <= N.FILL_COORD_BOUND:
        raise ValueError(f"{what}: coordinates up to {bound} scaled by {scale.tolist()} and moved by {off.tolist()} leave the envelope of "
                         f"+-{N.FILL_COORD_BOUND} canvas pixels")
    dev = F.resolve_device(what, device, (points, offsets, out), exc=ValueError)
    rows = []
    for i in order:
        p = int(first[i])
        rows.append((p, p + 1, 1, y_lo[p], y_hi[p]))
        if use_holes and n_holes[i] > 0:
            q = p + 1 + int(n_holes[i])
            rows.append((p + 1, q, 0, y_lo[p + 1:q].min(), y_hi[p + 1:q].max()))
    table = np.clip(np.array(rows, dtype=np.int64).reshape(-1, N.FILL_COLLECTION_INTS), -(1 << 31), (1 << 31) - 1).astype(np.int32)
    if out is not None and F.is_tensor(out) and out.dtype == torch.uint8:
        out = F.check_out(what, out, (h, w), torch.uint8, dev)
    else:
        out = F.check_out(what, out, (h, w), torch.bool, dev)
    with torch.cuda.device(dev):
        pts_d, off_d = F.to_device(points, dev), F.to_device(offsets, dev)
        table_d = torch.from_numpy(table).to(dev) if len(table) else None
        _fill(pts_d, n_points, off_d, n_polys, table_d, len(table), scale, off, bound, h, w, _max_cols, out, dev)
    return out


def _fill(points, n_points, offsets, n_polys, table, n_collections, scale, off, bound, h, w, max_cols, out, dev):
    """the native call of ``seg_mask``: everything resident, one launch on the current stream of ``dev``"""
    N.call("hipt_fill_contours", N.ptr(points) if n_points else None, n_points, N.ptr(offsets), n_polys, N.ptr(table), n_collections,
           float(scale[0]), float(scale[1]), int(off[0]), int(off[1]), bound, h, w, max_cols, N.ptr(out), N.stream_ptr(dev))


def get_seg_mask_like(wsi_object, region_size, scale, use_holes=False, offset=(0, 0), out=None, device=None, order=None):
    """``WholeSlideImage.get_seg_mask`` for an object with ``contours_tissue`` / ``holes_tissue`` (what ``segment_tissue`` sets): the
    bool mask as a device tensor (``seg_mask``).  Bind it as the method with ``WholeSlideImage.get_seg_mask = lambda self, *a, **k:
    segment.get_seg_mask_like(self, *a, **k).cpu().numpy()``, or hand the tensor to ``render_heatmap(mask=...)`` as it is."""
    return seg_mask(wsi_object.contours_tissue, wsi_object.holes_tissue, region_size, scale, use_holes=use_holes, offset=offset, out=out,
                    device=device, order=order)


def filter_contours(contours, hierarchy, filter_params):
    """``segmentTissue``'s nested ``_filter_contours``: ``hierarchy`` is cv2's after the reference's ``[:, 2:]`` slice, so column 1
    is the parent.  A foreground contour (parent -1) stays if its area less its holes' areas is not 0 and strictly above
    ``a_t``; of its holes the ``max_n_holes`` largest (a stable descending sort: equal areas keep their order) that are strictly
    above ``a_h``.  Returns ``(foreground_contours, hole_contours)``.  Where the reference would raise KeyError for a missing
    ``max_n_holes`` / ``a_h``, all holes are kept / ``a_h`` is 0."""
    hierarchy = np.asarray(hierarchy).reshape(-1, 2) if len(contours) else np.zeros((0, 2), dtype=np.int64)
    filtered, all_holes = [], []
    for cont_idx in np.flatnonzero(hierarchy[:, 1] == -1):
        holes = np.flatnonzero(hierarchy[:, 1] == cont_idx)
        a = contour_area(contours[cont_idx]) - np.array([contour_area(contours[i]) for i in holes]).sum()
        if a == 0:
            continue
        if filter_params["a_t"] < a:
            filtered.append(cont_idx)
            all_holes.append(holes)
    foreground = [contours[i] for i in filtered]
    hole_contours = []
    for hole_ids in all_holes:
        holes = sorted([contours[i] for i in hole_ids], key=contour_area, reverse=True)[:filter_params.get("max_n_holes")]
        hole_contours.append([h for h in holes if contour_area(h) > filter_params.get("a_h", 0)])
    return foreground, hole_contours


def _cv2_find_contours(mask):
    try:
        import cv2
    except ImportError:
        raise ImportError("segment_tissue: cv2 is not installed and no tracer was given: pass find_contours=segment.find_contours, the "
                          "device tracer of this package, or another function that takes the uint8 mask [H, W] and returns (contours, "
                          "hierarchy) as cv2.findContours(mask, cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE) does") from None
    return cv2.findContours(mask, cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)


def segment_tissue(wsi_object, seg_level=0, sthresh=20, sthresh_up=255, mthresh=7, close=0, use_otsu=False, filter_params={'a_t': 100},
                   ref_patch_size=512, exclude_ids=[], keep_ids=[], find_contours=None):
    """``WholeSlideImage.segmentTissue`` with the pixel stages on the device.  ``wsi_object`` has ``wsi.read_region``, ``level_dim``
    and ``level_downsamples`` as the reference's class does; its ``contours_tissue`` / ``holes_tissue`` are set, ready for
    ``tiling.process_contours_like``.  ``find_contours(mask)`` returns ``(contours, hierarchy)`` like ``cv2.findContours(mask,
    cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)``; None imports cv2 and calls just that, or raises ImportError; ``segment.find_contours``
    traces on the device and is handed the device mask (any tracer whose ``takes_device_mask`` attribute is true is), every other
    tracer the mask read back once.  A tracer may return ``hierarchy`` None for no contours, as cv2 does.  Bind it as the method
    with ``WholeSlideImage.segmentTissue = segment.segment_tissue``."""
    if find_contours is None:
        find_contours = _cv2_find_contours
    img = np.array(wsi_object.wsi.read_region((0, 0), seg_level, wsi_object.level_dim[seg_level]))
    mask = tissue_mask(img, sthresh, sthresh_up, mthresh, close, use_otsu)
    if not getattr(find_contours, "takes_device_mask", False):
        mask = mask.cpu().numpy()
    scale = wsi_object.level_downsamples[seg_level]
    scaled_ref_patch_area = int(ref_patch_size ** 2 / (scale[0] * scale[1]))
    filter_params = dict(filter_params)
    for key in ("a_t", "a_h"):
        if key in filter_params:
            filter_params[key] = filter_params[key] * scaled_ref_patch_area
    contours, hierarchy = find_contours(mask)
    hierarchy = np.zeros((0, 2), dtype=np.int32) if hierarchy is None else np.asarray(hierarchy).reshape(-1, 4)[:, 2:]
    foreground, holes = filter_contours(contours, hierarchy, filter_params)
    contours_tissue = [np.array(cont * scale, dtype="int32") for cont in foreground]
    holes_tissue = [[np.array(hole * scale, dtype="int32") for hole in hs] for hs in holes]
    if len(keep_ids) > 0:
        contour_ids = set(keep_ids) - set(exclude_ids)
    else:
        contour_ids = set(np.arange(len(contours_tissue))) - set(exclude_ids)
    wsi_object.contours_tissue = [contours_tissue[i] for i in contour_ids]
    wsi_object.holes_tissue = [holes_tissue[i] for i in contour_ids]
