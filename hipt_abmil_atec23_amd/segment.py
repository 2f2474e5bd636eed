"""The tissue mask of ``WholeSlideImage.segmentTissue`` on the HIP library (csrc/segment.hip).

``segmentTissue`` (wsi_core/WholeSlideImage.py:111-203) makes a binary picture of the segmentation level in four whole-image cv2
calls -- ``cvtColor(RGB2HSV)``'s saturation, ``medianBlur``, ``threshold`` (fixed or Otsu), ``morphologyEx(MORPH_CLOSE)`` -- traces
its contours and filters them by area.  The four pixel stages are 8-bit integer work (Otsu: integer counts and a short float64
scan), restated from OpenCV's published implementation and run on the device: ``tissue_mask`` is one native call, the stage
functions expose each step.  Contour tracing (``cv2.findContours``, a sequential border follower) stays on the host:
``segment_tissue`` takes the tracer as ``find_contours=`` and imports cv2 only when none is given.  The area filter
(``filter_contours``, ``contour_area``) is pure numpy.

cv2 is not a dependency and was not available to compare against: agreement with cv2's own bytes is argued from OpenCV's source
(DESIGN.md 26), not measured; the tests compare with a numpy restatement of the same definitions (tests/segment_ref.py).
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


# ---- host glue: pure numpy ------------------------------------------------------------------------------------------------------
def contour_area(cont) -> float:
    """``cv2.contourArea(cont)``: the shoelace formula in float64 over the closed polygon ``cont`` (``[n, 1, 2]`` or ``[n, 2]``)."""
    p = np.asarray(cont, dtype=np.float64).reshape(-1, 2)
    if len(p) == 0:
        return 0.0
    q = np.roll(p, 1, axis=0)   # the previous vertex; the first one's is the last
    return float(abs(0.5 * np.sum(q[:, 0] * p[:, 1] - p[:, 0] * q[:, 1])))


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
        raise ImportError("segment_tissue: cv2 is not installed and no tracer was given: pass find_contours=, a function that takes the "
                          "uint8 mask [H, W] and returns (contours, hierarchy) as cv2.findContours(mask, cv2.RETR_CCOMP, "
                          "cv2.CHAIN_APPROX_NONE) does") from None
    return cv2.findContours(mask, cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)


def segment_tissue(wsi_object, seg_level=0, sthresh=20, sthresh_up=255, mthresh=7, close=0, use_otsu=False, filter_params={'a_t': 100},
                   ref_patch_size=512, exclude_ids=[], keep_ids=[], find_contours=None):
    """``WholeSlideImage.segmentTissue`` with the pixel stages on the device.  ``wsi_object`` has ``wsi.read_region``, ``level_dim``
    and ``level_downsamples`` as the reference's class does; its ``contours_tissue`` / ``holes_tissue`` are set, ready for
    ``tiling.process_contours_like``.  ``find_contours(mask)`` returns ``(contours, hierarchy)`` like ``cv2.findContours(mask,
    cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)``; None imports cv2 and calls just that, or raises ImportError.  The mask is read back
    once.  Bind it as the method with ``WholeSlideImage.segmentTissue = segment.segment_tissue``."""
    if find_contours is None:
        find_contours = _cv2_find_contours
    img = np.array(wsi_object.wsi.read_region((0, 0), seg_level, wsi_object.level_dim[seg_level]))
    mask = tissue_mask(img, sthresh, sthresh_up, mthresh, close, use_otsu).cpu().numpy()
    scale = wsi_object.level_downsamples[seg_level]
    scaled_ref_patch_area = int(ref_patch_size ** 2 / (scale[0] * scale[1]))
    filter_params = dict(filter_params)
    for key in ("a_t", "a_h"):
        if key in filter_params:
            filter_params[key] = filter_params[key] * scaled_ref_patch_area
    contours, hierarchy = find_contours(mask)
    hierarchy = np.asarray(hierarchy).reshape(-1, 4)[:, 2:]
    foreground, holes = filter_contours(contours, hierarchy, filter_params)
    contours_tissue = [np.array(cont * scale, dtype="int32") for cont in foreground]
    holes_tissue = [[np.array(hole * scale, dtype="int32") for hole in hs] for hs in holes]
    if len(keep_ids) > 0:
        contour_ids = set(keep_ids) - set(exclude_ids)
    else:
        contour_ids = set(np.arange(len(contours_tissue))) - set(exclude_ids)
    wsi_object.contours_tissue = [contours_tissue[i] for i in contour_ids]
    wsi_object.holes_tissue = [holes_tissue[i] for i in contour_ids]
