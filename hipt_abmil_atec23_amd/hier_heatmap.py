"""Hierarchical region attention heat-maps (the reference's ``create_hierarchical_heatmaps_indiv``,
HIPT_4K/hipt_heatmap_utils.py:347-485, and its method form ``HIPT_4K.get_region_attention_heatmaps``, HIPT_4K/hipt_4k.py:167-303)
on the HIP library (csrc/hier_heatmap.hip).

The reference takes the [CLS] attention maps of ViT-256 and ViT-4K of a region and of three copies of it shifted towards the
top-left corner, upscales each to the picture's size, ranks the upscaled values (``rankdata * 100 / len``), adds the shifted
layers by slicing and colours the quotient: 48 pictures of a region (6 + 6 heads, 36 pairs), each with its own passes over
millions of pixels in numpy.  Here the maps stay on the device at their own size (``region_attention_maps``).  Nearest-neighbour
upscaling by ``f`` repeats every value ``f * f`` times, so the rank among the upscaled values is a closed form of two integer
counts over the original ones (``closed_form_percentiles``; ``hipt_hier_ranks``), and one kernel (``hipt_hier_render``) forms a
pixel's scores once and writes every picture from them.  All arithmetic is integer, float64 in the reference's order, or the
float32 blend of ``heatmap`` -- the pictures are the reference's byte for byte.

Host work, by design: the colour table (matplotlib) and the PNG files.  The background -- Pillow's ``region.resize`` -- is
``resize.resize_u8`` on the region tensor already on the device, Pillow's bytes; ``host_resize=True`` is Pillow itself.
As in ``heatmap`` the blend is cv2.addWeighted's documented formula, not cv2 itself.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _frontend as F
from . import _native as N

SCALES = (1, 2, 4, 8, 16)
PICTURES = ("4k", "256", "blend", "256th")


# ------------------------------------------------------------------------------------------------------------------------------
# host side
# ------------------------------------------------------------------------------------------------------------------------------
def closed_form_percentiles(x, f: int) -> np.ndarray:
    """float64, the shape of ``x``: ``rankdata(u) * 100 / len(u)`` of ``u`` = every value of the float32 vector ``x[..., :]``
    repeated ``f * f`` times, read at the copies of each value -- what ``hipt_hier_ranks`` computes, in numpy.  With ``less`` values
    below ``x[i]`` and ``eq`` equal to it (itself included), the copies of ``x[i]`` occupy the 1-based positions
    ``less f^2 + 1 .. (less + eq) f^2``, whose mean is ``less f^2 + (eq f^2 + 1) / 2``."""
    x = np.asarray(x, dtype=np.float32)
    flat = x.reshape(-1, x.shape[-1])
    less = (flat[:, None, :] < flat[:, :, None]).sum(axis=2)
    eq = (flat[:, None, :] == flat[:, :, None]).sum(axis=2)
    f2 = float(f) * float(f)
    rank = less.astype(np.float64) * f2 + 0.5 * (eq.astype(np.float64) * f2 + 1.0)
    return (rank * 100.0 / (flat.shape[1] * f2)).reshape(x.shape)


def cmap_map(function, cmap, n: int = 1024):
    """A segmented colormap with ``function`` applied to the colours of ``cmap`` at its breakpoints
    (hipt_heatmap_utils.py:69-105): a ``LinearSegmentedColormap`` of ``n`` entries named 'colormap'.  ``cmap`` must be segmented
    itself (jet is).  A breakpoint enters a channel's list where that channel had it, or where the function moved the colour."""
    import matplotlib.colors
    seg = cmap._segmentdata
    own = {key: [float(p[0]) for p in seg[key]] for key in ("red", "green", "blue")}
    steps = sorted(set(own["red"]) | set(own["green"]) | set(own["blue"]))
    old = np.array([np.array(cmap(s)[0:3]) for s in steps])
    new = np.array([function(c) for c in old])
    cdict = {}
    for ch, key in enumerate(("red", "green", "blue")):
        cdict[key] = [(s, new[k, ch], new[k, ch]) for k, s in enumerate(steps) if s in own[key] or new[k, ch] != old[k, ch]]
    return matplotlib.colors.LinearSegmentedColormap("colormap", cdict, n)


def half_jet():
    """The default colormap of the reference's method (hipt_4k.py:167): ``cmap_map(lambda x: x / 2 + 0.5, jet)``, 1024 entries."""
    import matplotlib
    return cmap_map(lambda x: x / 2 + 0.5, matplotlib.colormaps["jet"])


def colour_table_n(cmap="coolwarm") -> np.ndarray:
    """uint8 ``[cmap.N, 3]``: ``(cmap(i) * 255)[:3].astype(uint8)`` of every entry of a matplotlib colormap of any size.  ``cmap(v)``
    of a float ``v`` in [0, 1] is entry ``min(trunc(v * N), N - 1)``, which is the kernel's look-up.  (``heatmap.colour_table`` is
    the 256-entry table with the under and over colours that ``visHeatmap`` needs.)"""
    if isinstance(cmap, str):
        import matplotlib
        if cmap == "half_jet":
            cmap = half_jet()
        elif cmap not in matplotlib.colormaps:
            raise ValueError(f"hier_heatmap: {cmap!r} is not a matplotlib colormap")
        else:
            cmap = matplotlib.colormaps[cmap]
    n = int(cmap.N)
    if not 2 <= n <= N.HIER_MAX_LUT:
        raise ValueError(f"hier_heatmap: colormap of {n} entries; the kernel's table holds 2 .. {N.HIER_MAX_LUT}")
    rgba = cmap(np.arange(n))
    return np.ascontiguousarray((rgba * 255)[:, :3].astype(np.uint8))


def host_table(cmap, what="hier_heatmap"):
    """The colour table of ``cmap`` -- a name, a matplotlib colormap or a uint8 ``[N, 3]`` array or tensor -- checked and still where
    it is: a table the kernels cannot hold is refused before anything runs.  ``_frontend.table_on`` takes it to the device."""
    if F.is_tensor(cmap) or isinstance(cmap, np.ndarray):
        if str(cmap.dtype).replace("torch.", "") != "uint8" or len(cmap.shape) != 2 or cmap.shape[1] != 3 or \
                not 2 <= cmap.shape[0] <= N.HIER_MAX_LUT:
            raise ValueError(f"{what}: a colour table is uint8 [N, 3] with 2 <= N <= {N.HIER_MAX_LUT}, got {cmap.dtype} {list(cmap.shape)}")
        return cmap
    return F.table_host(colour_table_n, cmap)


def shifted_regions(region_u8, offset: int = 128):
    """The four regions of hipt_heatmap_utils.py:370-375 from one uint8 ``[H, W, 3]`` region, as a list: the region itself, and for
    k = 1, 2, 3 its crop from ``(k offset, k offset)`` to the bottom-right corner with a white (255) margin added below and to the
    right.  The margin is ``offset * k`` for k = 1 and 2 and ``offset * 4`` for k = 3, exactly as the reference writes it: region 4
    is ``offset`` pixels larger than the region each way, and ``prepare_img_tensor``'s centre crop then moves it by a further
    ``offset / 2`` pixels.  The aim is the reference's pictures, so that is reproduced, not repaired.  A numpy array gives numpy
    arrays; a tensor gives tensors on its device (nothing is copied to the host)."""
    import torch
    as_numpy = not F.is_tensor(region_u8)
    r = torch.from_numpy(np.ascontiguousarray(region_u8)) if as_numpy else region_u8
    if r.dtype != torch.uint8 or r.dim() != 3 or r.shape[2] != 3:
        raise ValueError(f"shifted_regions: the region is uint8 [H, W, 3], got {r.dtype} {list(r.shape)}")
    offset = int(offset)
    h, w = int(r.shape[0]), int(r.shape[1])
    if offset < 0 or 3 * offset >= min(h, w):
        raise ValueError(f"shifted_regions: offset {offset} leaves nothing of a {h} x {w} region after three shifts")
    out = [r]
    for k, margin in ((1, offset), (2, offset * 2), (3, offset * 4)):
        ch, cw = h - k * offset, w - k * offset
        t = torch.full((ch + margin, cw + margin, 3), 255, dtype=torch.uint8, device=r.device)
        t[:ch, :cw] = r[k * offset:, k * offset:]
        out.append(t)
    return [t.numpy() for t in out] if as_numpy else out


# ------------------------------------------------------------------------------------------------------------------------------
# the attention maps, at their own size, on the device
# ------------------------------------------------------------------------------------------------------------------------------
def _region_tensor(hipt, region):
    """A region (PIL image, uint8 ``[H, W, 3]`` array or tensor) as the normalised float32 ``[1, 3, H, W]`` tensor on ViT-256's
    device: ToTensor + Normalize(0.5, 0.5) by ``hipt_u8_normalize``, the bits ``eval_transforms`` computes on the host."""
    import torch
    d256 = hipt.model256.weight_device
    t = region if F.is_tensor(region) else torch.from_numpy(np.array(region))   # (a copy: a PIL image's array is read-only)
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"hier_heatmap: a region is uint8 [H, W, 3], got {t.dtype} {list(t.shape)}")
    t = t.to(d256).contiguous()
    N.require_cuda(t, "hier_heatmap")
    h, w = int(t.shape[0]), int(t.shape[1])
    x = torch.empty((1, 3, h, w), dtype=torch.float32, device=d256)
    N.call("hipt_u8_normalize", N.ptr(t), 1, 1, h * w, N.ptr(x), N.HIPT_F32, N.stream_ptr(d256))
    return x


def region_attention_maps(hipt, regions):
    """``(a256 [R, n, nh, 256] float32, a4k [R, nh, n] float32)``: the raw [CLS] attention maps of R regions (PIL images, or uint8
    ``[H, W, 3]`` arrays or tensors; all of one grid of n = ``(H // 256) * (W // 256)`` patches after ``prepare_img_tensor``'s
    centre crop) as device tensors.  Region by region the calls ``_get_region_attention_scores`` makes (hipt_4k.py:137-158), so the same kernels and the
    same bits; there is no upscaling and no copy to the host.  ``hipt`` needs ``model256`` and ``model4k``."""
    import torch

    from .hipt_4k import center_crop_box
    d4k = hipt.model4k.weight_device
    a256s, a4ks, grid_shape = [], [], None
    with torch.no_grad():
        for region in regions:
            x = _region_tensor(hipt, region)
            w, h = int(x.shape[2]), int(x.shape[3])
            w_256, h_256 = w // 256, h // 256
            if w_256 == 0 or h_256 == 0:
                raise ValueError(f"region {tuple(x.shape)} is smaller than one 256x256 patch")
            if grid_shape is None:
                grid_shape = (w_256, h_256)
            elif grid_shape != (w_256, h_256):
                raise ValueError(f"region_attention_maps: regions of {grid_shape} and {(w_256, h_256)} patches in one call")
            W, Hh = w_256 * 256, h_256 * 256
            if (W, Hh) != (w, h):   # prepare_img_tensor's CenterCrop (hipt_4k.py:308-330)
                t, l = center_crop_box(w, W), center_crop_box(h, Hh)
                x = x[:, :, t:t + W, l:l + Hh]
            n = w_256 * h_256
            b256 = x.unfold(2, 256, 256).unfold(3, 256, 256).permute(0, 2, 3, 1, 4, 5).reshape(n, 3, 256, 256).contiguous()
            features_cls256 = hipt.model256(b256)
            a256 = hipt.model256.get_last_selfattention_cls(b256)   # [n, heads, 257]
            a256s.append(a256[:, :, 1:])
            grid = features_cls256.reshape(w_256, h_256, -1).transpose(0, 1).transpose(0, 2).unsqueeze(dim=0).to(d4k)
            a4k = hipt.model4k.get_last_selfattention_cls(grid)   # [1, heads, 1 + n]
            a4ks.append(a4k[0, :, 1:])
    if not a256s:
        raise ValueError("region_attention_maps: no regions")
    return torch.stack(a256s).contiguous(), torch.stack(a4ks).contiguous()


# ------------------------------------------------------------------------------------------------------------------------------
# the device calls
# ------------------------------------------------------------------------------------------------------------------------------
def hier_ranks(x, f: int):
    """float64 device tensor, the shape of ``x``: the percentile ranks of every vector ``x[..., :]`` (float32, on the device) as if
    upscaled by ``f`` (``hipt_hier_ranks``; ``closed_form_percentiles`` is the same in numpy)."""
    import torch
    if not F.is_tensor(x) or x.dtype != torch.float32 or x.dim() < 1:
        raise ValueError("hier_ranks: x is a float32 device tensor [..., L]")
    N.require_cuda(x, "hier_ranks")
    L = int(x.shape[-1])
    if not 1 <= L <= N.HIER_MAX_L or not 1 <= int(f) <= N.HIER_MAX_UPSCALE:
        raise ValueError(f"hier_ranks: L={L}, f={f} outside 1 <= L <= {N.HIER_MAX_L}, 1 <= f <= {N.HIER_MAX_UPSCALE}")
    x = x.detach().contiguous()
    out = torch.empty(x.shape, dtype=torch.float64, device=x.device)
    v = x.numel() // L
    if v >= 2 ** 31:
        raise ValueError(f"hier_ranks: {v} vectors in one call")
    if v:
        N.call("hipt_hier_ranks", N.ptr(x), v, L, int(f), N.ptr(out), N.stream_ptr(x.device))
    return out


def _check_pairs(pairs, nh):
    if pairs is None:
        return None, nh * nh
    pairs = [(int(j), int(i)) for j, i in pairs]
    if not pairs:
        raise ValueError("hier_heatmap: pairs is empty (None asks for every pair)")
    if len(set(pairs)) != len(pairs) or any(not (0 <= j < nh and 0 <= i < nh) for j, i in pairs):
        raise ValueError(f"hier_heatmap: pairs are distinct (j, i) with heads 0 .. {nh - 1}, got {pairs}")
    flat = (C.c_int32 * (2 * len(pairs)))(*[v for p in pairs for v in p])
    return flat, len(pairs)


def compose_heatmaps(a256, a4k, w_256, h_256, base, *, offset=128, scale=4, alpha=0.5, cmap="coolwarm", threshold=None, w256=2,
                     pairs=None, which=("4k", "256", "blend"), out=None):
    """The pictures of one region from its raw attention maps, as a dict of uint8 device tensors.

    ``a256 [R >= 2, n, nh, 256]`` and ``a4k [4, nh, n]`` float32 device tensors (``region_attention_maps`` of ``shifted_regions``;
    n = ``w_256 * h_256`` patches, the reference's naming: tensor dimension 2 is "w", the picture's rows); ``base`` uint8
    ``[Hs, Ws, 3]`` = ``[w_256 * 256 / scale, h_256 * 256 / scale, 3]``, the region at the picture's size.  ``which`` names the
    pictures wanted: ``"4k"`` ``[nh, Hs, Ws, 3]`` (the reference's ``_1024[j]``), ``"256"`` ``[nh, Hs, Ws, 3]``, ``"blend"``
    ``[pairs, Hs, Ws, 3]`` (``_factorized_4k[j]_256[i]``; ``pairs`` = distinct ``(j, i)``, None: all, j major); with a
    ``threshold`` also ``"256th"`` ``[nh, Hs, Ws, 3]``.  ``w256`` weighs the 256 level in the blended score: 2 in
    ``create_hierarchical_heatmaps_indiv`` (:475-480), 1 in the method (hipt_4k.py:295-300).  ``cmap``: a matplotlib name or
    colormap (or ``"half_jet"``), or a uint8 ``[N, 3]`` table.  ``out`` may hand in the buffers to write (same keys).  Two rank
    launches and one render launch on the current stream; nothing is copied to the host."""
    import torch
    scale, offset, w_256, h_256 = int(scale), int(offset), int(w_256), int(h_256)
    if scale not in SCALES:
        raise ValueError(f"hier_heatmap: scale {scale}; the pictures exist at {SCALES}")
    if offset < 0:
        raise ValueError(f"hier_heatmap: offset {offset} is negative")
    which = tuple(which)
    if not which or any(k not in PICTURES for k in which):
        raise ValueError(f"hier_heatmap: which = {which}; the pictures are {PICTURES}")
    if threshold is not None and "256th" not in which:
        which = which + ("256th",)
    if threshold is None and "256th" in which:
        raise ValueError("hier_heatmap: the picture '256th' needs a threshold")
    alpha, w256 = float(alpha), float(w256)
    if alpha != alpha or not w256 > 0 or (threshold is not None and float(threshold) != float(threshold)):
        raise ValueError("hier_heatmap: alpha / threshold is NaN, or w256 is not positive")
    for name, a in (("a256", a256), ("a4k", a4k)):
        if not F.is_tensor(a) or a.dtype != torch.float32:
            raise ValueError(f"hier_heatmap: {name} is a float32 device tensor")
    n = w_256 * h_256
    if a4k.dim() != 3 or a4k.shape[0] != 4 or a4k.shape[2] != n:
        raise ValueError(f"hier_heatmap: a4k must be [4, nh, {n}] for a {w_256} x {h_256} grid, got {list(a4k.shape)}")
    nh = int(a4k.shape[1])
    if a256.dim() != 4 or a256.shape[0] < 2 or tuple(a256.shape[1:]) != (n, nh, 256):
        raise ValueError(f"hier_heatmap: a256 must be [R >= 2, {n}, {nh}, 256], got {list(a256.shape)}")
    if not (1 <= nh <= N.HIER_MAX_HEADS and 1 <= n <= N.HIER_MAX_L):
        raise ValueError(f"hier_heatmap: {nh} heads, {n} patches outside 1 .. {N.HIER_MAX_HEADS} heads, 1 .. {N.HIER_MAX_L} patches")
    hs, ws = w_256 * 256 // scale, h_256 * 256 // scale
    dev = F.resolve_device("heatmap", None, (a4k, a256))
    F.check_no_nan("hier_heatmap", a256=a256[:2], a4k=a4k)
    base = F.as_array(base)
    F.check_image("heatmap", "base", base, (hs, ws, 3), ("uint8",))
    table = host_table(cmap)
    base_d = F.to_device(base, dev)
    flat_pairs, npairs = _check_pairs(pairs, nh) if "blend" in which else (None, 0)
    shapes = {"4k": (nh, hs, ws, 3), "256": (nh, hs, ws, 3), "blend": (npairs, hs, ws, 3), "256th": (nh, hs, ws, 3)}
    res = {k: F.check_out("hier_heatmap", None if out is None else out.get(k), shapes[k], torch.uint8, dev, name=f"out[{k!r}]") for k in which}
    with torch.cuda.device(dev):
        table = F.table_on(colour_table_n, cmap, table, dev)
        pct4k = hier_ranks(a4k, 256 // scale)                                          # [4, nh, n]
        pct256 = hier_ranks(a256[:2].permute(0, 2, 1, 3).contiguous(), 16 // scale)    # [2, nh, n, 256]
        off = [(offset * k) // scale for k in (1, 2, 3)]
        N.call("hipt_hier_render", N.ptr(pct4k), N.ptr(pct256), nh, w_256, h_256, scale, off[0], off[1], off[2], N.ptr(base_d),
               N.ptr(table), int(table.shape[0]), alpha, w256, C.cast(flat_pairs, C.c_void_p) if flat_pairs is not None else None,
               npairs, int(threshold is not None), float(threshold) if threshold is not None else 0.0, N.ptr(res.get("4k")),
               N.ptr(res.get("256")), N.ptr(res.get("blend")), N.ptr(res.get("256th")), N.stream_ptr(dev))
    return res


def _as_region_array(region) -> np.ndarray:
    a = region.cpu().numpy() if F.is_tensor(region) else np.asarray(region)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"hier_heatmap: the region is an RGB image (uint8 [H, W, 3]), got {a.dtype} {list(a.shape)}")
    return a


def _region_and_background(hipt, region, scale, base, host_resize):
    """``(the region on ViT-256's device, the background)``: ``base`` where given, else the reference's ``region.resize((Ws, Hs))``
    (:385) by ``resize_u8`` on the device or, with ``host_resize``, by Pillow on the host."""
    import torch
    if scale not in SCALES:
        raise ValueError(f"hier_heatmap: scale {scale}; the pictures exist at {SCALES}")
    if F.is_tensor(region) and region.is_cuda:
        r_dev, r_np = region, None
    else:
        r_np = _as_region_array(region)
        r_dev = torch.from_numpy(np.array(r_np)).to(hipt.model256.weight_device)   # (a copy: a PIL image's array is read-only)
    h, w = int(r_dev.shape[0]), int(r_dev.shape[1])
    if h % 256 or w % 256 or not h or not w:
        raise ValueError(f"hier_heatmap: a {h} x {w} region; the shifted layers line up only on whole 256-pixel patches")
    if base is None and not host_resize:
        from .resize import resize_u8
        base = resize_u8(r_dev, (w // scale, h // scale))
    elif base is None:
        from PIL import Image
        pil = region if isinstance(region, Image.Image) else Image.fromarray(_as_region_array(region) if r_np is None else r_np)
        base = np.array(pil.resize((w // scale, h // scale)))
    return r_dev, base


def hierarchical_heatmaps(hipt, region, offset=128, scale=4, alpha=0.5, cmap="coolwarm", threshold=None, w256=2, pairs=None,
                          which=("4k", "256", "blend"), base=None, host_resize=False):
    """The hierarchical heat-maps of one region (a PIL image or a uint8 ``[H, W, 3]`` array or tensor; H and W multiples of 256) as
    a dict of uint8 device tensors (``compose_heatmaps`` names them): the four ``shifted_regions`` go through ViT-256 and ViT-4K
    (``region_attention_maps``), the ranks and the pictures follow on the device.  ``base`` (uint8 ``[Hs, Ws, 3]``) is the
    background; absent, it is the reference's ``region.resize((Ws, Hs))`` (:385) -- computed on the device by ``resize_u8``, the same
    bytes, or with ``host_resize=True`` by Pillow on the host."""
    r_dev, base = _region_and_background(hipt, region, scale, base, host_resize)
    w_256, h_256 = int(r_dev.shape[0]) // 256, int(r_dev.shape[1]) // 256   # (the reference's naming: tensor dimension 2, the image's rows, is "w")
    a256, a4k = region_attention_maps(hipt, shifted_regions(r_dev, offset))
    return compose_heatmaps(a256, a4k, w_256, h_256, base, offset=offset, scale=scale, alpha=alpha, cmap=cmap, threshold=threshold,
                            w256=w256, pairs=pairs, which=which)


def create_hierarchical_heatmaps_indiv(region, hipt, output_dir, fname, offset=128, scale=4, alpha=0.5, cmap="coolwarm",
                                       threshold=None):
    """hipt_heatmap_utils.py:347-485 with ``hipt`` (a ``HIPT_4K``, or anything with ``model256`` and ``model4k``) in place of the two
    models and their devices: saves ``{fname}_1024[j].png`` (the ViT-4K heads), ``{fname}_256[i].png``,
    ``{fname}_factorized_4k[j]_256[i].png`` and, with a ``threshold``, ``{fname}_256th[i].png`` under ``output_dir``.  Returns the
    list of files written."""
    from PIL import Image
    res = hierarchical_heatmaps(hipt, region, offset=offset, scale=scale, alpha=alpha, cmap=cmap, threshold=threshold, w256=2)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    nh = host["4k"].shape[0]
    files = []

    def save(img, name):
        path = os.path.join(output_dir, name)
        Image.fromarray(img).save(path)
        files.append(path)
    if threshold is not None:
        for i in range(nh):
            save(host["256th"][i], "%s_256th[%d].png" % (fname, i))
    for j in range(nh):
        save(host["4k"][j], "%s_1024[%s].png" % (fname, j))
    for i in range(nh):
        save(host["256"][i], "%s_256[%s].png" % (fname, i))
    for j in range(nh):
        for i in range(nh):
            save(host["blend"][j * nh + i], "%s_factorized_4k[%s]_256[%s].png" % (fname, j, i))
    return files


def create_hierarchical_heatmaps_indiv_like(region, model256, model4k, output_dir, fname, offset=128, scale=4, alpha=0.5, cmap="coolwarm",
                                            threshold=None, device256=None, device4k=None):
    """The reference's own signature (what ``dropin.install(hier_heatmaps=True)`` binds): the models are used where they are;
    ``device256`` / ``device4k`` are accepted and unused."""
    import types
    hipt = types.SimpleNamespace(model256=model256, model4k=model4k)
    create_hierarchical_heatmaps_indiv(region, hipt, output_dir, fname, offset=offset, scale=scale, alpha=alpha, cmap=cmap,
                                       threshold=threshold)


def hierarchical_heatmaps_concat_select(hipt, region, heads4k=(0, 5), heads256=(2,), offset=128, scale=4, alpha=0.5, cmap="coolwarm",
                                        w256=2, base=None, host_resize=False):
    """The side-by-side grid of hipt_heatmap_utils.py:584-667 (``create_hierarchical_heatmaps_concat_select``) as one uint8 device
    tensor ``[(1 + len(heads256)) * Hs, (1 + len(heads4k)) * Ws, 3]``: the background and the ViT-4K pictures of ``heads4k`` on top,
    and under them, for every head i of ``heads256``, its ViT-256 picture and the blended pictures of the pairs (j, i).  The tiles
    are the pictures of ONE ``hierarchical_heatmaps`` call with ``pairs=`` set, copied into the canvas on the device.  The top row
    shows the four-layer ViT-4K score, as every other picture of the family does; the reference's top row (:644) colours the first
    layer's ranks alone."""
    import torch
    heads4k, heads256 = [int(j) for j in heads4k], [int(i) for i in heads256]
    if not heads4k or not heads256:
        raise ValueError("hier_heatmap: concat_select needs at least one ViT-4K head and one ViT-256 head")
    pairs = [(j, i) for i in heads256 for j in heads4k]
    r_dev, base = _region_and_background(hipt, region, scale, base, host_resize)
    res = hierarchical_heatmaps(hipt, r_dev, offset=offset, scale=scale, alpha=alpha, cmap=cmap, w256=w256, pairs=pairs, base=base)
    hs, ws = int(res["4k"].shape[1]), int(res["4k"].shape[2])
    dev = res["4k"].device
    canvas = torch.empty(((1 + len(heads256)) * hs, (1 + len(heads4k)) * ws, 3), dtype=torch.uint8, device=dev)
    canvas[:hs, :ws] = F.to_device(F.as_array(base), dev)
    for c, j in enumerate(heads4k):
        canvas[:hs, (c + 1) * ws:(c + 2) * ws] = res["4k"][j]
    for r, i in enumerate(heads256):
        canvas[(r + 1) * hs:(r + 2) * hs, :ws] = res["256"][i]
        for c in range(len(heads4k)):
            canvas[(r + 1) * hs:(r + 2) * hs, (c + 1) * ws:(c + 2) * ws] = res["blend"][r * len(heads4k) + c]
    return canvas


def create_hierarchical_heatmaps_concat_select(region, hipt, output_dir, fname, offset=128, scale=4, alpha=0.5, cmap="coolwarm",
                                               heads4k=(0, 5), heads256=(2,)):
    """Saves ``hierarchical_heatmaps_concat_select``'s grid as ``{fname}_heatmap.png`` (the reference's name, :668) under
    ``output_dir`` and returns the path.  The file is RGB; the reference's is the same layout with an opaque alpha channel."""
    from PIL import Image
    canvas = hierarchical_heatmaps_concat_select(hipt, region, heads4k=heads4k, heads256=heads256, offset=offset, scale=scale,
                                                 alpha=alpha, cmap=cmap)
    path = os.path.join(output_dir, "%s_heatmap.png" % fname)
    Image.fromarray(canvas.cpu().numpy()).save(path)
    return path
