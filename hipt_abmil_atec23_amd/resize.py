"""Pillow's ``Image.resize`` of 8-bit RGB images on the HIP library (csrc/resize.hip).

The reference resizes on the host in three places: the background of the hierarchical heat-maps
(HIPT_4K/hipt_heatmap_utils.py:385, HIPT_4K/hipt_4k.py:204), every patch of the ResNet extraction routes when
``--custom_downsample > 1`` or ``--target_patch_size`` is set (datasets/dataset_h5.py:92,202) and the end of ``visHeatmap``.
For 8-bit images Pillow's arithmetic is integer behind a small table of fixed-point weights, so the device result is Pillow's byte
for byte: ``resize_table`` builds the table of one axis on the host in Python doubles (cached, and copied to a device once),
``hipt_resize_u8`` runs the two separable passes -- horizontal first, the intermediate image rounded and clipped to uint8 as
Pillow stores it.

Covered: ``Image.resize(size, resample)`` of an RGB image with ``reducing_gap=None`` and no ``box``; bicubic (RGB's default),
bilinear, box and lanczos.  Not covered: ``box=``, ``reducing_gap=``, other modes, planar input, nearest and hamming.
"""
from __future__ import annotations

import math

import numpy as np

from . import _frontend as F
from . import _native as N

PRECISION_BITS = 22
MAX_KSIZE = N.RESIZE_MAX_KSIZE
ROUTE_AUTO, ROUTE_GENERAL, ROUTE_FUSED = N.RESIZE_ROUTE_AUTO, N.RESIZE_ROUTE_GENERAL, N.RESIZE_ROUTE_FUSED
_ROUTES = {None: ROUTE_AUTO, "auto": ROUTE_AUTO, "general": ROUTE_GENERAL, "fused": ROUTE_FUSED}
_PIL_FILTERS = {1: "lanczos", 2: "bilinear", 3: "bicubic", 4: "box"}   # Image.LANCZOS, BILINEAR, BICUBIC, BOX
_table_cache = {}   # (in_len, out_len, filter, device or None) -> (k, bounds)


def _bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _box(x: float) -> float:
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _sinc(x: float) -> float:
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x: float) -> float:
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


_FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0), "box": (_box, 0.5), "lanczos": (_lanczos, 3.0)}


def filter_name(resample) -> str:
    """``"bicubic"`` / ``"bilinear"`` / ``"box"`` / ``"lanczos"`` from a name or Pillow's integer constant; ValueError otherwise."""
    if isinstance(resample, str) and resample.lower() in _FILTERS:
        return resample.lower()
    if not isinstance(resample, (str, bool)) and isinstance(resample, (int, np.integer)) and int(resample) in _PIL_FILTERS:
        return _PIL_FILTERS[int(resample)]
    raise ValueError(f"resize: filter {resample!r}; the kernels know {sorted(_FILTERS)} (Pillow's constants {sorted(_PIL_FILTERS)})")


def resize_table(in_len: int, out_len: int, resample="bicubic"):
    """``(k int32 [out_len, ksize], bounds int32 [out_len, 2])`` of one axis, Pillow's ``precompute_coeffs`` and
    ``normalize_coeffs_8bpc`` in Python doubles: output ``xx`` is ``clip((2^21 + sum_x src[xmin + x] * k[xx, x]) >> 22)`` over
    ``x < xmax`` with ``bounds[xx] = (xmin, xmax)``.  ValueError for a table the kernels cannot take: a ``ksize`` above
    ``MAX_KSIZE`` (512), or weights with which the int32 accumulator could overflow.  The arrays are cached: do not write to them."""
    name = filter_name(resample)
    in_len, out_len = int(in_len), int(out_len)
    if in_len < 1 or out_len < 1:
        raise ValueError(f"resize: lengths {in_len} -> {out_len} are not positive")
    key = (in_len, out_len, name, None)
    if key in _table_cache:
        return _table_cache[key]
    f, s = _FILTERS[name]
    scale = filterscale = in_len / out_len
    if filterscale < 1.0:
        filterscale = 1.0
    support = s * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    if ksize > MAX_KSIZE:
        raise ValueError(f"resize: {name} from {in_len} to {out_len} samples takes {ksize} taps; the kernels take {MAX_KSIZE}")
    ss = 1.0 / filterscale
    k = np.zeros((out_len, ksize), dtype=np.int32)
    bounds = np.zeros((out_len, 2), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_len):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)         # int() truncates towards zero, as the C cast does; then the clamp
        xmax = min(int(center + support + 0.5), in_len) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:                                         # left to right, as the C loop adds
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k[xx, :xmax] = [int(v * one + 0.5) if v >= 0 else int(v * one - 0.5) for v in w]
        bounds[xx] = (xmin, xmax)
    reach = 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << (PRECISION_BITS - 1))
    if reach >= 1 << 31:
        raise ValueError(f"resize: {name} from {in_len} to {out_len} samples: the accumulator could reach {reach}, beyond int32")
    k.setflags(write=False)
    bounds.setflags(write=False)
    _table_cache[key] = (k, bounds)
    return k, bounds


def _device_table(in_len, out_len, name, dev):
    """The table of one axis on ``dev``, copied there once (a later call with the same geometry can be captured into a graph)."""
    import torch
    key = (in_len, out_len, name, str(dev))
    if key not in _table_cache:
        k, b = resize_table(in_len, out_len, name)
        _table_cache[key] = (torch.from_numpy(np.array(k)).to(dev), torch.from_numpy(np.array(b)).to(dev))
    return _table_cache[key]


def _check_size(size):
    try:
        ow, oh = size
    except (TypeError, ValueError):
        raise ValueError(f"resize: size is (width, height) in positive integers, got {size!r}") from None
    return F.check_int("resize", "size's width", ow, 1), F.check_int("resize", "size's height", oh, 1)


def resize_u8(x, size, resample="bicubic", out=None, *, _route=None):
    """``Image.fromarray(x).resize(size, resample)`` of every image of ``x``, on the device, byte for byte.

    ``x``: a uint8 device tensor ``[H, W, 3]`` or ``[n, H, W, 3]`` (RGB, interleaved); ``size = (width, height)`` in Pillow's
    order; ``resample``: ``"bicubic"`` (Pillow's default for RGB), ``"bilinear"``, ``"box"``, ``"lanczos"`` or Pillow's integer
    constant of one of them.  Returns a tensor of the same rank on the same device (``out``, where given: contiguous uint8 of the
    result's shape on that device, not ``x``).  Equal sizes give a copy.  One or two launches on the current stream, nothing is
    copied to the host.  ValueError -- before any native call -- for a CPU tensor, another dtype or channel count, a non-positive
    size or an unknown filter."""
    import torch
    if not F.is_tensor(x):
        raise ValueError(f"resize_u8: x is a uint8 device tensor, got {type(x).__name__}")
    if x.dtype != torch.uint8 or x.dim() not in (3, 4) or x.shape[-1] != 3:
        raise ValueError(f"resize_u8: x is uint8 [H, W, 3] or [n, H, W, 3], got {x.dtype} {list(x.shape)}")
    ow, oh = _check_size(size)
    name = filter_name(resample)
    if _route not in _ROUTES:
        raise ValueError(f"resize_u8: route {_route!r}; the routes are 'general' and 'fused'")
    route = _ROUTES[_route]
    dev = F.resolve_device("resize_u8", None, (x,), exc=ValueError)
    batched = x.dim() == 4
    n = int(x.shape[0]) if batched else 1
    h, w = int(x.shape[-3]), int(x.shape[-2])
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"resize_u8: nothing to resize in {list(x.shape)}")
    if max(h, w, oh, ow) >= 1 << 24 or n * max(h, oh) * max(w, ow) * 3 >= 1 << 40:
        raise ValueError(f"resize_u8: {n} images of {h} x {w} -> {oh} x {ow} are beyond the kernels' index range")
    kx = bx = ky = by = None
    if ow != w:
        resize_table(w, ow, name)   # (its refusals, before anything reaches the device)
    if oh != h:
        resize_table(h, oh, name)
    shape = (n, oh, ow, 3) if batched else (oh, ow, 3)
    out = F.check_out("resize_u8", out, shape, torch.uint8, dev, not_alias=(x,))
    x = x.detach().contiguous()
    if x.data_ptr() % 16:
        x = x.clone()   # (a view into a larger tensor: the kernels read 16-byte vectors)
    if out.data_ptr() % 4:
        raise ValueError("resize_u8: out needs 4-byte alignment")
    with torch.cuda.device(dev):
        ksx = ksy = 0
        if ow != w:
            kx, bx = _device_table(w, ow, name, dev)
            ksx = int(kx.shape[1])
        if oh != h:
            ky, by = _device_table(h, oh, name, dev)
            ksy = int(ky.shape[1])
        ws, need = F.scratch("hipt_resize_workspace_bytes", n, h, w, oh, ow, route, dev=dev, floor=0)   # (no scratch: ws is None)
        N.call("hipt_resize_u8", N.ptr(x), n, h, w, oh, ow, N.ptr(kx), N.ptr(bx), ksx, N.ptr(ky), N.ptr(by), ksy, N.ptr(out), N.ptr(ws),
               need, route, N.stream_ptr(dev))
    return out


def target_size(patch_size, target_patch_size=-1, custom_downsample=1):
    """The reference's rule (datasets/dataset_h5.py:157-162): ``(t, t)`` for ``target_patch_size = t > 0``, else
    ``(patch_size // custom_downsample,) * 2`` for ``custom_downsample > 1``, else None (no resize)."""
    if target_patch_size > 0:
        return (int(target_patch_size),) * 2
    if custom_downsample > 1:
        return (int(patch_size) // int(custom_downsample),) * 2
    return None


def resize_patches(x, target_patch_size=-1, custom_downsample=1):
    """What ``Whole_Slide_Bag_FP.__getitem__`` does to every patch (``img.resize(self.target_patch_size)``,
    datasets/dataset_h5.py:200-202) for a batch of patches ``x`` (uint8 ``[n, P, P, 3]`` on the device): ``x`` itself when neither
    ``target_patch_size > 0`` nor ``custom_downsample > 1``, else the bicubic resize to ``target_size(P, ...)``, ready for
    ``resnet50_baseline`` / ``resnet18_baseline``'s uint8 ``[B, H, W, 3]`` input."""
    F.check_int("resize_patches", "target_patch_size", target_patch_size)
    F.check_int("resize_patches", "custom_downsample", custom_downsample)
    if not hasattr(x, "dim") or x.dim() != 4 or x.shape[1] != x.shape[2]:
        raise ValueError(f"resize_patches: x is a batch of square patches, uint8 [n, P, P, 3], got {list(getattr(x, 'shape', []))}")
    size = target_size(int(x.shape[1]), int(target_patch_size), int(custom_downsample))
    if size is None:
        return x
    return resize_u8(x, size, "bicubic")
