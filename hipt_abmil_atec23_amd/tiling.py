"""Patch coordinates from tissue contours on the device: ``WholeSlideImage.process_contour`` and the contour
checking functions of ``wsi_core/util_classes.py`` (``isInContourV1 / V2 / V3_Easy / V3_Hard``, ``isInHoles``), the step of
``create_patches_fp.py`` and of the heat-map ROIs (``datasets/wsi_dataset.py``) that decides which grid positions become patches.

The geometry runs in ``csrc/tiling.hip`` (``hipt_point_polygon_test``, ``hipt_tile_contours``): exact integer arithmetic in doubled
coordinates, one launch for all contours of a slide.  This module restates the reference's glue around it -- bounding box, clamps,
ranges, shifts, order and dtype of the result -- and refuses, before any native call, what the kernels' int32 arithmetic cannot
hold.  There is no CPU execution path: numpy arrays and CPU tensors are accepted as inputs and copied to the HIP device.

    coords = process_contour(cont, holes, wsi.level_dim[0], wsi.level_downsamples[level], patch_size=256, step_size=256)
    per_contour, all_coords = process_contours(wsi.contours_tissue, wsi.holes_tissue, wsi.level_dim[0], wsi.level_downsamples[level])
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _frontend as F
from . import _native as N

MODES = {"basic": N.TILE_BASIC, "center": N.TILE_CENTER, "four_pt": N.TILE_FOUR_PT, "four_pt_easy": N.TILE_FOUR_PT,
         "four_pt_hard": N.TILE_FOUR_PT_HARD}
_MODE_NAMES = "'basic', 'center', 'four_pt' (= 'four_pt_easy'), 'four_pt_hard'"
BOUND = N.TILING_COORD_BOUND   # every doubled coordinate lies strictly inside +-BOUND


def _as_polygon(a, what):
    """An integer polygon as int64 [n, 2] on the host (cv2's [n, 1, 2] contours included)."""
    if F.is_tensor(a):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.size == 0:
        return np.zeros((0, 2), np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{what}: polygon vertices must be integers, got {a.dtype}")
    if a.ndim == 3 and a.shape[1] == 1:
        a = a[:, 0, :]
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f"{what}: a polygon is [n, 2] or [n, 1, 2], got {a.shape}")
    return a.astype(np.int64)


def _check_bound(value, what):
    if not -BOUND < value < BOUND:
        raise ValueError(f"{what}: doubled coordinate {value} is outside +-2^30 (the kernels' exact int32 differences); nothing was launched")


def _pack(polys, what):
    """verts int32 [V, 2], poly_off int32 [P + 1] of a list of int64 polygons, the vertex range checked."""
    off = np.zeros(len(polys) + 1, np.int64)
    np.cumsum([len(p) for p in polys], out=off[1:])
    if off[-1] >= 2 ** 30:
        raise ValueError(f"{what}: {off[-1]} vertices in one call (at most 2^30 - 1)")
    verts = np.concatenate(polys) if polys else np.zeros((0, 2), np.int64)
    if len(verts):
        _check_bound(2 * int(verts.max()), what)
        _check_bound(2 * int(verts.min()), what)
    return np.ascontiguousarray(verts, dtype=np.int32).reshape(-1, 2), off.astype(np.int32)


# ------------------------------------------------------------------------------------------------------------------------------
# the primitive
# ------------------------------------------------------------------------------------------------------------------------------
def _doubled_points(points):
    """int32-ranged doubled points [Q, 2] as an int64 tensor where ``points`` lives; integers or exact multiples of 0.5."""
    import torch
    t = points if F.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(np.asarray(points)))
    t = t.detach()
    if t.ndim == 1 and t.numel() == 2:
        t = t.reshape(1, 2)
    if t.ndim != 2 or t.shape[1] != 2:
        raise ValueError(f"point_polygon_test: points are [Q, 2], got {tuple(t.shape)}")
    if t.dtype == torch.bool or t.is_complex():
        raise ValueError(f"point_polygon_test: points must be integers or multiples of 0.5, got {t.dtype}")
    if t.is_floating_point():
        d = t.to(torch.float64) * 2
        if t.numel() and not bool((torch.isfinite(d) & (d == d.round())).all()):
            raise ValueError("point_polygon_test: points must be integers or exact multiples of 0.5")
        if t.numel() and float(d.abs().max()) >= BOUND:
            _check_bound(int(d.abs().max()), "point_polygon_test")
        d = d.to(torch.int64)
    else:
        d = t.to(torch.int64) * 2
    if d.numel():
        _check_bound(int(d.max()), "point_polygon_test")
        _check_bound(int(d.min()), "point_polygon_test")
    return d


def point_polygon_test(polygons, points, poly_id=None, device=None):
    """``cv2.pointPolygonTest(polygon, point, False)`` for many points: int8 [Q] in {-1, 0, +1} on the device (outside, on the
    boundary, inside; DESIGN.md 21 states the rule).  ``polygons``: one integer polygon ([n, 2] or cv2's [n, 1, 2]) or a list of
    them; ``points``: [Q, 2], integers or exact multiples of 0.5; ``poly_id`` [Q]: the polygon of each point (needed with more
    than one polygon; points grouped by polygon are the fast case).  numpy arrays or tensors; CPU inputs are copied to the device."""
    import torch
    single = not isinstance(polygons, (list, tuple))
    polys = [_as_polygon(p, "point_polygon_test") for p in ([polygons] if single else polygons)]
    verts, off = _pack(polys, "point_polygon_test")
    d = _doubled_points(points)
    Q = d.shape[0]
    if poly_id is None:
        if len(polys) != 1:
            raise ValueError(f"point_polygon_test: {len(polys)} polygons need a poly_id per point")
        ids = torch.zeros(Q, dtype=torch.int64)
    else:
        ids = (poly_id if F.is_tensor(poly_id) else torch.from_numpy(np.ascontiguousarray(np.asarray(poly_id)))).detach().reshape(-1)
        if ids.is_floating_point() or ids.dtype == torch.bool or ids.numel() != Q:
            raise ValueError(f"point_polygon_test: poly_id must be {Q} integers")
        if Q and (int(ids.min()) < 0 or int(ids.max()) >= len(polys)):
            raise ValueError(f"point_polygon_test: poly_id outside [0, {len(polys)})")
    dev = F.resolve_device("tiling", device, (points, poly_id), staged=True)
    v_d, off_d = F.to_device(verts, dev), F.to_device(off, dev)
    p_d = d.to(dev, torch.int32).contiguous()
    id_d = ids.to(dev, torch.int32).contiguous()
    out = torch.empty(Q, dtype=torch.int8, device=dev)
    N.call("hipt_point_polygon_test", N.ptr(v_d), len(verts), N.ptr(off_d), len(polys), N.ptr(p_d), N.ptr(id_d), Q, N.ptr(out),
           N.stream_ptr(dev))
    return out


# ------------------------------------------------------------------------------------------------------------------------------
# a slide's polygons on the device
# ------------------------------------------------------------------------------------------------------------------------------
class PackedSlide:
    """The contours and holes of a slide, packed and resident on a device (``pack_slide``): what ``process_contours`` uploads once
    when it is handed lists.  ``boxes[c]`` is cv2.boundingRect of contour c: (min_x, min_y, max_x - min_x + 1, max_y - min_y + 1)."""

    def __init__(self, verts, poly_off, ranges, boxes, device):
        self.verts, self.poly_off, self.ranges, self.boxes, self.device = verts, poly_off, ranges, boxes, device
        self.n_verts, self.n_polys = int(verts.shape[0]), int(poly_off.shape[0]) - 1

    def __len__(self):
        return len(self.ranges)


class _HostSlide:
    """``pack_slide`` in two steps: the host checks now, the copy to the device (and the question whether there is one) later."""

    def __init__(self, contours, holes):
        self.contours = list(contours)
        holes = [[] for _ in self.contours] if holes is None else list(holes)
        if len(holes) != len(self.contours):
            raise ValueError(f"tiling: {len(self.contours)} contours but {len(holes)} lists of holes (one list per contour)")
        polys, self.ranges, self.boxes = [], [], []
        for c, cont in enumerate(self.contours):
            if cont is None:
                raise ValueError(f"tiling: contour {c} is None (the reference's process_contour fails there too: cv2.contourArea(None))")
            p = _as_polygon(cont, "tiling")
            if len(p) == 0:
                raise ValueError(f"tiling: contour {c} has no vertices")
            begin = len(polys)
            polys.append(p)
            polys.extend(_as_polygon(h, "tiling") for h in (holes[c] if holes[c] is not None else []))
            self.ranges.append((begin, len(polys)))
            x0, y0, x1, y1 = int(p[:, 0].min()), int(p[:, 1].min()), int(p[:, 0].max()), int(p[:, 1].max())
            self.boxes.append((x0, y0, x1 - x0 + 1, y1 - y0 + 1))
        self.verts, self.off = _pack(polys, "tiling")

    def upload(self, device):
        dev = F.resolve_device("tiling", device, self.contours, staged=True)
        return PackedSlide(F.to_device(self.verts, dev), F.to_device(self.off, dev), self.ranges, self.boxes, dev)


def pack_slide(contours, holes, device=None):
    """Pack ``contours`` (a list of integer polygons) and ``holes`` (one list of polygons per contour) and copy them to the device."""
    if isinstance(contours, PackedSlide):
        return contours
    return _HostSlide(contours, holes).upload(device)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference's glue (wsi_core/WholeSlideImage.py:415-470), in Python integers
# ------------------------------------------------------------------------------------------------------------------------------
def _int(v, what):
    if isinstance(v, (float, np.floating)) and float(v).is_integer():   # (a whole float counts: level_dim and the ROI come from arithmetic)
        return int(v)
    return F.check_int("tiling", what, v)


def _pair(v, what):
    if isinstance(v, (tuple, list, np.ndarray)):
        if len(v) != 2:
            raise ValueError(f"tiling: {what} is a pair, got {v!r}")
        return v[0], v[1]
    return v, v


def contour_mode(contour_fn):
    """The kernel's mode of a ``contour_fn`` name of process_contour or of datasets/wsi_dataset.py."""
    if not isinstance(contour_fn, str):
        raise TypeError(f"tiling: contour_fn must be one of the names {_MODE_NAMES}; a Contour_Checking_fn instance "
                        f"({type(contour_fn).__name__}) is a Python callable per candidate and cannot run on the device")
    if contour_fn not in MODES:
        raise ValueError(f"tiling: contour_fn {contour_fn!r} is none of {_MODE_NAMES}")
    return MODES[contour_fn]


def _settings(level_dim0, patch_downsample, patch_size, step_size, contour_fn, center_shift):
    mode = contour_mode(contour_fn)
    img_w, img_h = (_int(v, "level_dim0") for v in _pair(level_dim0, "level_dim0"))
    ds = tuple(int(v) for v in _pair(patch_downsample, "patch_downsample"))   # int(self.level_downsamples[patch_level][k])
    patch_size, step_size = _int(patch_size, "patch_size"), _int(step_size, "step_size")
    if ds[0] < 1 or ds[1] < 1 or patch_size < 1 or step_size < 1:
        raise ValueError(f"tiling: patch_size {patch_size}, step_size {step_size} and int(patch_downsample) {ds} must all be >= 1")
    ref_ps = (patch_size * ds[0], patch_size * ds[1])
    step = (step_size * ds[0], step_size * ds[1])
    ps0 = ref_ps[0]   # the contour checks and the hole test take ref_patch_size[0] alone
    if contour_fn == "four_pt_easy":
        center_shift = 0.5   # datasets/wsi_dataset.py:22 hands 0.5 whatever the caller asked for
    shift = int(ps0 // 2 * center_shift) if mode >= N.TILE_FOUR_PT else 0
    if shift < 0:
        raise ValueError(f"tiling: center_shift {center_shift} gives a negative shift")
    if ps0 >= BOUND // 4 or shift >= BOUND // 4:
        raise ValueError(f"tiling: ref_patch_size {ps0} / shift {shift} outside the kernels' range (< 2^28)")
    return mode, (img_w, img_h), ref_ps, step, ps0, shift


def _grid(box, img, ref_ps, step, use_padding, top_left, bot_right):
    """(start_x, start_y, nx, ny) of one contour, or None where the ROI misses it; nx, ny = len(np.arange(start, stop, step))."""
    start_x, start_y, w, h = box
    if use_padding:
        stop_y, stop_x = start_y + h, start_x + w
    else:
        stop_y = min(start_y + h, img[1] - ref_ps[1] + 1)
        stop_x = min(start_x + w, img[0] - ref_ps[0] + 1)
    if bot_right is not None:
        stop_y, stop_x = min(bot_right[1], stop_y), min(bot_right[0], stop_x)
    if top_left is not None:
        start_y, start_x = max(top_left[1], start_y), max(top_left[0], start_x)
    if bot_right is not None or top_left is not None:
        if stop_x - start_x <= 0 or stop_y - start_y <= 0:
            return None   # "Contour is not in specified ROI, skip"
    nx = max(0, -(-(stop_x - start_x) // step[0]))
    ny = max(0, -(-(stop_y - start_y) // step[1]))
    return start_x, start_y, nx, ny


class TilePlan:
    """One ``hipt_tile_contours`` call, laid out: the device arrays, the scalars and the output flags.  ``run()`` is the launch and
    nothing else (no allocation, no copy, no synchronisation), so it can be captured into a graph; ``grids[c]`` is
    (start_x, start_y, step_x, step_y, nx, ny, keep_off) of contour c, with nx = ny = 0 where it has no candidate;
    ``flags[keep_off + i]`` belongs to candidate i = ix * ny + iy, the order of ``meshgrid(indexing='ij')`` flattened."""

    def __init__(self, slide, grids, desc, units, n_units, mode, ps0, shift, flags):
        self.slide, self.grids, self.desc, self.units, self.n_units = slide, grids, desc, units, n_units
        self.mode, self.ps0, self.shift, self.flags = mode, ps0, shift, flags

    def run(self):
        s = self.slide
        N.call("hipt_tile_contours", N.ptr(s.verts), s.n_verts, N.ptr(s.poly_off), s.n_polys, N.ptr(self.desc), len(self.grids),
               N.ptr(self.units), self.n_units, self.mode, self.ps0, self.shift, N.ptr(self.flags), C.c_int64(self.flags.numel()),
               N.stream_ptr(s.device))
        return self.flags

    def coordinates(self, flags=None):
        """The per-contour int64 [n, 2] coordinates from the flags (one read-back), in the reference's order."""
        f = (self.flags if flags is None else flags).cpu().numpy()
        out = []
        for sx, sy, stx, sty, nx, ny, off in self.grids:
            i = np.flatnonzero(f[off:off + nx * ny]).astype(np.int64)
            ix, iy = (i // ny, i % ny) if ny else (i, i)
            out.append(np.stack([sx + ix * stx, sy + iy * sty], axis=1).astype(np.int64).reshape(-1, 2))
        return out


def plan_contours(contours, holes, level_dim0, patch_downsample, patch_level_dim=None, patch_size=256, step_size=256,
                  contour_fn="four_pt", use_padding=True, top_left=None, bot_right=None, center_shift=0.5, device=None):
    """Everything of ``process_contours`` up to the launch: checks, the reference's grid arithmetic, the device arrays."""
    import torch
    mode, img, ref_ps, step, ps0, shift = _settings(level_dim0, patch_downsample, patch_size, step_size, contour_fn, center_shift)
    if top_left is not None:
        top_left = tuple(_int(v, "top_left") for v in _pair(top_left, "top_left"))
    if bot_right is not None:
        bot_right = tuple(_int(v, "bot_right") for v in _pair(bot_right, "bot_right"))
    # (the polygons are checked on the host first; the device is asked for last)
    slide = contours if isinstance(contours, PackedSlide) else _HostSlide(contours, holes)
    boxes = slide.boxes
    if max(step) >= BOUND:
        raise ValueError(f"tiling: step {step} outside the kernels' range")
    grids, desc, total = [], [], 0
    off_c = 0 if mode == N.TILE_BASIC else ps0 // 2
    for c, box in enumerate(boxes):
        g = _grid(box, img, ref_ps, step, use_padding, top_left, bot_right)
        sx, sy, nx, ny = g if g is not None else (box[0], box[1], 0, 0)
        n = nx * ny
        if n >= 2 ** 31 or total + n >= 2 ** 31:
            raise ValueError(f"tiling: {total + n} candidates in one call (at most 2^31 - 1)")
        if n:
            ex, ey = sx + (nx - 1) * step[0], sy + (ny - 1) * step[1]
            for v in (2 * (sx + off_c - shift), 2 * (sy + off_c - shift), 2 * (ex + off_c + shift), 2 * (ey + off_c + shift),
                      2 * sx + ps0, 2 * sy + ps0, 2 * ex + ps0, 2 * ey + ps0):
                _check_bound(v, "tiling")
        else:
            nx = ny = 0
        grids.append((sx, sy, step[0], step[1], nx, ny, total))
        desc.append((slide.ranges[c][0], slide.ranges[c][1], sx if n else 0, sy if n else 0, step[0] if n else 1, step[1] if n else 1,
                     nx, ny, total))
        total += n
    counts = np.array([-(-(g[4] * g[5]) // N.TILING_TILE) for g in grids], np.int64)
    which = np.repeat(np.arange(len(grids), dtype=np.int64), counts)
    first = (np.arange(int(counts.sum()), dtype=np.int64) - np.repeat(np.cumsum(counts) - counts, counts)) * N.TILING_TILE
    units = np.stack([which, first], axis=1).astype(np.int32).reshape(-1, 2)
    if isinstance(slide, _HostSlide):
        slide = slide.upload(device)
    dev = slide.device
    desc_d = F.to_device(np.array(desc, np.int32).reshape(-1, N.TILING_CONTOUR_INTS), dev)
    units_d = F.to_device(units, dev)
    flags = torch.zeros(total, dtype=torch.uint8, device=dev)
    return TilePlan(slide, grids, desc_d, units_d, len(units), mode, ps0, shift, flags)


def process_contours(contours, holes, level_dim0, patch_downsample, patch_level_dim=None, patch_size=256, step_size=256,
                     contour_fn="four_pt", use_padding=True, top_left=None, bot_right=None, center_shift=0.5, device=None,
                     return_flags=False):
    """``WholeSlideImage.process_contour`` for every contour of a slide in ONE kernel launch and one read-back.

    ``contours``: a list of integer polygons ([n, 2] or cv2's [n, 1, 2]; ``wsi.contours_tissue``) or a ``PackedSlide``;
    ``holes``: one list of polygons per contour (``wsi.holes_tissue``; None with a ``PackedSlide``); ``level_dim0``: (width, height)
    of level 0; ``patch_downsample``: ``wsi.level_downsamples[patch_level]`` (its ``int()`` is taken, as the reference does);
    ``patch_level_dim``: what the reference reads only for ``cont=None``, which it cannot finish either -- accepted and not read.
    The other arguments are process_contour's; ``contour_fn`` also takes the names of datasets/wsi_dataset.py (``four_pt_easy``,
    whose shift is always 0.5) and ``center_shift`` is that file's (``int(ref_patch_size // 2 * center_shift)``).

    Returns ``(per_contour, coords)``: the int64 [n, 2] top-left corners of each contour in the reference's order (empty where the
    reference returns ``{}``), and their concatenation -- what the reference appends to the ``.h5`` contour by contour.
    ``return_flags=True`` returns ``(flags, grids)`` instead: the uint8 keep-flags on the device and the grids they index
    (``TilePlan``), nothing read back or synchronised."""
    plan = plan_contours(contours, holes, level_dim0, patch_downsample, patch_level_dim, patch_size, step_size, contour_fn, use_padding,
                         top_left, bot_right, center_shift, device)
    plan.run()
    if return_flags:
        return plan.flags, plan.grids
    per = plan.coordinates()
    return per, (np.concatenate(per) if per else np.zeros((0, 2), np.int64))


def process_contour(cont, holes, level_dim0, patch_downsample, patch_level_dim=None, patch_size=256, step_size=256, contour_fn="four_pt",
                    use_padding=True, top_left=None, bot_right=None, center_shift=0.5, device=None):
    """One contour and its holes: the int64 [n, 2] coordinates ``process_contour`` returns as ``asset_dict['coords']``
    ([0, 2] where it returns ``{}``).  See ``process_contours``."""
    per, _ = process_contours([cont], [list(holes) if holes is not None else []], level_dim0, patch_downsample, patch_level_dim, patch_size,
                              step_size, contour_fn, use_padding, top_left, bot_right, center_shift, device)
    return per[0]


def _dicts(wsi_object, coords, patch_level, save_path, patch_size):
    """process_contour's return value for one contour (wsi_core/WholeSlideImage.py:484-499)."""
    if len(coords) == 0:
        return {}, {}
    attr = {"patch_size": patch_size,
            "patch_level": patch_level,
            "downsample": wsi_object.level_downsamples[patch_level],
            "downsampled_level_dim": tuple(np.array(wsi_object.level_dim[patch_level])),
            "level_dim": wsi_object.level_dim[patch_level],
            "name": wsi_object.name,
            "save_path": save_path}
    return {"coords": coords}, {"coords": attr}


def process_contours_like(wsi_object, patch_level=0, save_path="", patch_size=256, step_size=256, **kwargs):
    """Every contour of a reference ``WholeSlideImage`` (``contours_tissue``, ``holes_tissue``, ``level_dim``, ``level_downsamples``)
    in one launch: the list of ``(asset_dict, attr_dict)`` its ``process_contours`` loop gets from ``process_contour``, one per
    contour and with the reference's keys (``({}, {})`` where no candidate survives).  Writing them to the ``.h5`` stays the caller's."""
    per, _ = process_contours(wsi_object.contours_tissue, wsi_object.holes_tissue, wsi_object.level_dim[0],
                              wsi_object.level_downsamples[patch_level], wsi_object.level_dim[patch_level], patch_size, step_size, **kwargs)
    return [_dicts(wsi_object, c, patch_level, save_path, patch_size) for c in per]


def process_contour_like(self, cont, contour_holes, patch_level, save_path, patch_size=256, step_size=256, contour_fn="four_pt",
                         use_padding=True, top_left=None, bot_right=None):
    """``WholeSlideImage.process_contour`` with the reference's signature and return value (what ``dropin.install(tiling=True)`` binds)."""
    coords = process_contour(cont, contour_holes, self.level_dim[0], self.level_downsamples[patch_level], self.level_dim[patch_level],
                             patch_size, step_size, contour_fn, use_padding, top_left, bot_right)
    return _dicts(self, coords, patch_level, save_path, patch_size)
