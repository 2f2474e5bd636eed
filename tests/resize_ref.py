"""Pillow's ``Image.resize`` of an 8-bit RGB image, restated in numpy (it imports nothing from the package).

Two separable passes, horizontal first, the intermediate image stored as uint8.  Per axis, from ``I`` to ``O`` samples with a filter
of support ``S``: ``scale = I / O`` in double, ``fs = max(scale, 1)``, ``support = S * fs``, ``ksize = ceil(support) * 2 + 1``; output
``xx`` reads the ``xmax`` inputs from ``xmin`` on, ``xmin = max(int(center - support + 0.5), 0)``, ``xmax = min(int(center + support +
0.5), I) - xmin`` around ``center = (xx + 0.5) * scale``, with the weights ``f((x + xmin - center + 0.5) / fs)`` divided by their sum
(added left to right) and rounded to 22 fractional bits, half away from zero.  A pixel is ``clip((2^21 + sum(src * k)) >> 22)`` in
int32.  A pass whose output length equals its input length is skipped."""
import math

import numpy as np

PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"bicubic": (_bicubic, 2.0), "bilinear": (_bilinear, 1.0), "box": (_box, 0.5), "lanczos": (_lanczos, 3.0)}


def table(in_len, out_len, resample="bicubic"):
    """``(k int32 [out_len, ksize], bounds int32 [out_len, 2])``: the fixed-point weights and ``(xmin, xmax)`` of every output."""
    f, s = FILTERS[resample]
    scale = filterscale = in_len / out_len
    if filterscale < 1.0:
        filterscale = 1.0
    support = s * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    k = np.zeros((out_len, ksize), dtype=np.int32)
    bounds = np.zeros((out_len, 2), dtype=np.int32)
    for xx in range(out_len):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)   # int() truncates towards zero, as the C cast does
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_len:
            xmax = in_len
        xmax -= xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:   # left to right
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        for x, v in enumerate(w):
            k[xx, x] = int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5)
        bounds[xx] = (xmin, xmax)
    return k, bounds


def accumulator_bound(k):
    """The largest magnitude the int32 accumulator of a table can reach on 8-bit input."""
    return 255 * int(np.abs(k.astype(np.int64)).sum(axis=1).max()) + (1 << (PRECISION_BITS - 1))


def _pass_last_axis_but_one(img, k, bounds):
    """One pass along axis -2 of ``img`` uint8 [..., I, C] -> uint8 [..., O, C]."""
    out = np.empty(img.shape[:-2] + (k.shape[0], img.shape[-1]), dtype=np.uint8)
    src = img.astype(np.int32)
    for xx in range(k.shape[0]):
        xmin, xmax = int(bounds[xx, 0]), int(bounds[xx, 1])
        acc = np.full(img.shape[:-2] + (img.shape[-1],), 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for x in range(xmax):
            acc = acc + src[..., xmin + x, :] * k[xx, x]
        out[..., xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(img, size, resample="bicubic"):
    """``img`` uint8 [H, W, 3] (or [n, H, W, 3]), ``size = (width, height)``: Pillow's ``Image.fromarray(img).resize(size, resample)``."""
    img = np.ascontiguousarray(img)
    assert img.dtype == np.uint8 and img.ndim in (3, 4)
    ow, oh = int(size[0]), int(size[1])
    h, w = img.shape[-3], img.shape[-2]
    out = img
    if ow != w:
        out = _pass_last_axis_but_one(out, *table(w, ow, resample))
    if oh != h:
        out = np.swapaxes(_pass_last_axis_but_one(np.swapaxes(out, -3, -2), *table(h, oh, resample)), -3, -2)
    return np.ascontiguousarray(out) if out is not img else img.copy()
