"""Patch-level ViT-256 attention heat-maps (the reference's ``create_patch_heatmaps_indiv`` and ``create_patch_heatmaps_concat``,
HIPT_4K/attention_visualization_utils.py:293-421; the copies in HIPT_4K/hipt_heatmap_utils.py:158-290 call a
``get_patch_attention_scores`` that file never defines) on the HIP library (csrc/patch_heatmap.hip), in batches.

The reference runs ViT-256 twice on one 256 x 256 patch -- on the patch and on its crop from (16, 16) with a white margin -- takes the
last block's [CLS] attention as a 16 x 16 map per head, upscales it by 16, ranks the 65 536 values (``rankdata * 100 / len``), adds
the second map shifted by ``offset`` and colours the quotient: twelve full-size numpy passes a patch, one patch at a time.  Here a
batch of patches goes through ViT-256 in one call (``patch_attention_maps``), the ranks are the closed form of ``hier_heatmap``
(``hipt_hier_ranks`` with f = 16; the upscaled maps never exist) and one kernel (``hipt_patch_render``) forms a pixel's score per
head once and writes both pictures -- or the reference's mosaics -- from it.  All arithmetic is integer, float64 in the reference's
order, or the float32 blend of ``heatmap``: the pictures are the reference's byte for byte.

The crop shift is the literal 16 whatever ``offset`` is (:311, :370); ``offset`` only moves the second layer's scores.  That is
reproduced, not repaired.  Host work, by design: the colour table (matplotlib) and the PNG files.  As in ``heatmap`` the blend is
cv2.addWeighted's documented formula, not cv2 itself.
"""
from __future__ import annotations

import os

import numpy as np

from . import _frontend as F
from . import _native as N
from . import hier_heatmap as HH

SIDE = 256     # pixels along a patch
SHIFT = 16     # the reference's crop of the second layer: a literal, not ``offset``


def _patch_batch(patches, what):
    """``(tensor uint8 [P, 256, 256, 3], single)`` of one patch or a batch: PIL images, uint8 arrays or tensors (or a list of them)."""
    import torch
    if isinstance(patches, (list, tuple)):
        if not patches:
            raise ValueError(f"{what}: no patches")
        items = [p if F.is_tensor(p) else torch.from_numpy(np.array(p)) for p in patches]   # (a copy: a PIL image's array is read-only)
        if any(t.dim() != 3 for t in items) or len({(t.dtype, tuple(t.shape), t.device) for t in items}) != 1:
            raise ValueError(f"{what}: a list holds uint8 [256, 256, 3] patches of one kind")
        t, single = torch.stack(items), False
    else:
        t = patches if F.is_tensor(patches) else torch.from_numpy(np.array(patches))
        single = t.dim() == 3
        if single:
            t = t[None]
    if t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[1:]) != (SIDE, SIDE, 3):
        raise ValueError(f"{what}: patches are uint8 [P, {SIDE}, {SIDE}, 3] (or one [{SIDE}, {SIDE}, 3]), got {t.dtype} {list(t.shape)}")
    if not 1 <= t.shape[0] <= N.PATCH_MAX_P:
        raise ValueError(f"{what}: {t.shape[0]} patches in one call (1 .. {N.PATCH_MAX_P})")
    return t, single


def shifted_patches(patches_u8):
    """uint8 ``[P, 2, 256, 256, 3]`` from ``[P, 256, 256, 3]``: layer 1 is the patch, layer 2 its crop ``(16, 16, 256, 256)`` with a
    white (255) margin of 16 pixels added to the right and below (attention_visualization_utils.py:310-311).  A numpy array gives a
    numpy array; a tensor gives a tensor on its device (nothing is copied to the host)."""
    import torch
    as_numpy = not F.is_tensor(patches_u8)
    t = torch.from_numpy(np.ascontiguousarray(patches_u8)) if as_numpy else patches_u8
    if t.dtype != torch.uint8 or t.dim() != 4 or tuple(t.shape[1:]) != (SIDE, SIDE, 3):
        raise ValueError(f"shifted_patches: patches are uint8 [P, {SIDE}, {SIDE}, 3], got {t.dtype} {list(t.shape)}")
    out = torch.full((t.shape[0], 2, SIDE, SIDE, 3), 255, dtype=torch.uint8, device=t.device)
    out[:, 0] = t
    out[:, 1, :SIDE - SHIFT, :SIDE - SHIFT] = t[:, SHIFT:, SHIFT:]
    return out.numpy() if as_numpy else out


def patch_attention_maps(model256, patches):
    """``a256 [P, 2, nh, 256]`` float32 on ViT-256's device: the raw [CLS] attention of the last block over the 256 tokens of every
    patch and of its shifted copy (``shifted_patches``) -- one ``get_last_selfattention_cls`` call over the 2 P layers, normalised
    on the device by ``hipt_u8_normalize`` as ``region_attention_maps`` does (the bits of ``eval_transforms``)."""
    import torch
    t, _ = _patch_batch(patches, "patch_attention_maps")
    dev = model256.weight_device
    t = t.to(dev).contiguous()
    N.require_cuda(t, "patch_attention_maps")
    p = int(t.shape[0])
    layers = shifted_patches(t)   # [P, 2, 256, 256, 3]
    x = torch.empty((2 * p, 3, SIDE, SIDE), dtype=torch.float32, device=dev)
    with torch.no_grad():
        N.call("hipt_u8_normalize", N.ptr(layers), 1, 2 * p, SIDE * SIDE, N.ptr(x), N.HIPT_F32, N.stream_ptr(dev))
        a = model256.get_last_selfattention_cls(x)   # [2 P, nh, 257]
    return a[:, :, 1:].reshape(p, 2, a.shape[1], SIDE).contiguous()


def mosaic_shape(nh: int, cols: int):
    """``(rows, cols)`` in pixels of the mosaic of ``nh`` pictures, ``cols`` tiles across (``getConcatImage`` of rows of ``cols``)."""
    return ((nh + cols - 1) // cols) * SIDE, cols * SIDE


def compose_patch_heatmaps(a256, patches, *, offset=16, alpha=0.5, cmap="coolwarm", threshold=None, concat=False, cols=3, out=None,
                           which=None):
    """The pictures of P patches from their raw attention maps, as a dict of uint8 device tensors.

    ``a256 [P, 2, nh, 256]`` float32 device tensor (``patch_attention_maps``); ``patches`` uint8 ``[P, 256, 256, 3]`` (tensor or
    array).  ``"256"`` is the heat-map of every head and, with a ``threshold``, ``"256th"`` the thresholded one: ``[P, nh, 256, 256,
    3]`` each, or with ``concat=True`` the mosaic ``[P, ceil(nh / cols) * 256, cols * 256, 3]`` with head i at tile ``(i // cols,
    i % cols)`` and unused tiles 0 -- ``cols=3`` is the reference's ``_concat`` layout.  ``offset`` (0 .. 256) shifts the second
    layer's scores; ``cmap`` is a matplotlib name or colormap (or ``"half_jet"``), or a uint8 ``[N, 3]`` table.  ``which`` names the
    pictures wanted (default: both where there is a threshold); ``out`` may hand in the buffers to write (same keys).  One rank
    launch and one render launch on the current stream; nothing is copied to the host."""
    import torch
    offset, cols = int(offset), int(cols)
    if not 0 <= offset <= SIDE:
        raise ValueError(f"patch_heatmap: offset {offset} outside 0 .. {SIDE}")
    if concat and not 1 <= cols <= N.HIER_MAX_HEADS:
        raise ValueError(f"patch_heatmap: cols {cols} outside 1 .. {N.HIER_MAX_HEADS}")
    if which is None:
        which = ("256",) if threshold is None else ("256", "256th")
    which = tuple(which)
    if not which or any(k not in ("256", "256th") for k in which) or len(set(which)) != len(which):
        raise ValueError(f"patch_heatmap: which = {which}; the pictures are ('256', '256th')")
    if threshold is None and "256th" in which:
        raise ValueError("patch_heatmap: the picture '256th' needs a threshold")
    alpha = float(alpha)
    if alpha != alpha or (threshold is not None and float(threshold) != float(threshold)):
        raise ValueError("patch_heatmap: alpha / threshold is NaN")
    if not F.is_tensor(a256) or a256.dtype != torch.float32:
        raise ValueError("patch_heatmap: a256 is a float32 device tensor")
    if a256.dim() != 4 or a256.shape[1] != 2 or a256.shape[3] != SIDE:
        raise ValueError(f"patch_heatmap: a256 must be [P, 2, nh, 256], got {list(a256.shape)}")
    p, nh = int(a256.shape[0]), int(a256.shape[2])
    if not (1 <= nh <= N.HIER_MAX_HEADS and 1 <= p <= N.PATCH_MAX_P):
        raise ValueError(f"patch_heatmap: {nh} heads, {p} patches outside 1 .. {N.HIER_MAX_HEADS} heads, 1 .. {N.PATCH_MAX_P} patches")
    patches = F.as_array(patches)
    F.check_image("heatmap", "patches", patches, (p, SIDE, SIDE, 3), ("uint8",))
    table = HH.host_table(cmap, "patch_heatmap")
    F.check_no_nan("patch_heatmap", a256=a256)
    dev = F.resolve_device("heatmap", None, (a256,))
    patches_d = F.to_device(patches, dev)
    shape = (p,) + mosaic_shape(nh, cols) + (3,) if concat else (p, nh, SIDE, SIDE, 3)
    res = {k: F.check_out("patch_heatmap", None if out is None else out.get(k), shape, torch.uint8, dev, not_alias=(patches_d,),
                          name=f"out[{k!r}]") for k in which}   # (hipt_patch_render refuses the patches as an output: never in place)
    if len(res) == 2 and res["256"].data_ptr() == res["256th"].data_ptr():
        raise ValueError("patch_heatmap: out['256'] and out['256th'] are one buffer")
    with torch.cuda.device(dev):
        table = F.table_on(HH.colour_table_n, cmap, table, dev)
        pct = HH.hier_ranks(a256, 16)   # [P, 2, nh, 256]
        N.call("hipt_patch_render", N.ptr(pct), N.ptr(patches_d), p, nh, N.ptr(table), int(table.shape[0]), offset, alpha,
               int(threshold is not None), float(threshold) if threshold is not None else 0.0, cols if concat else 0,
               N.ptr(res.get("256")), N.ptr(res.get("256th")), N.stream_ptr(dev))
    return res


def patch_heatmaps(model256, patches, offset=16, alpha=0.5, cmap="coolwarm", threshold=None, concat=False, cols=3, which=None):
    """The whole route for one patch or a batch (PIL images, uint8 arrays or device tensors; a list of them is a batch): the two
    layers through ViT-256 (``patch_attention_maps``), the ranks and the pictures on the device (``compose_patch_heatmaps``, which
    names the result).  One patch gives the pictures without the leading batch dimension."""
    t, single = _patch_batch(patches, "patch_heatmaps")
    t = t.to(model256.weight_device).contiguous()
    a256 = patch_attention_maps(model256, t)
    res = compose_patch_heatmaps(a256, t, offset=offset, alpha=alpha, cmap=cmap, threshold=threshold, concat=concat, cols=cols,
                                 which=which)
    return {k: v[0] for k, v in res.items()} if single else res


def _save(img, output_dir, name, files):
    from PIL import Image
    path = os.path.join(output_dir, name)
    Image.fromarray(img).save(path)
    files.append(path)


def create_patch_heatmaps_indiv(patch, model256, output_dir, fname, threshold=0.5, offset=16, alpha=0.5, cmap="coolwarm",
                                device256=None):
    """attention_visualization_utils.py:293-349: saves ``{fname}_256th[i].png`` (with a ``threshold``) and ``{fname}_256[i].png`` of
    every head under ``output_dir``.  The model is used where it is; ``device256`` is accepted and unused.  Returns the files."""
    res = patch_heatmaps(model256, patch, offset=offset, alpha=alpha, cmap=cmap, threshold=threshold)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    if host["256"].ndim != 4:
        raise ValueError("create_patch_heatmaps_indiv: one patch at a time (patch_heatmaps takes batches)")
    files = []
    if threshold is not None:
        for i in range(host["256th"].shape[0]):
            _save(host["256th"][i], output_dir, "%s_256th[%d].png" % (fname, i), files)
    for i in range(host["256"].shape[0]):
        _save(host["256"][i], output_dir, "%s_256[%s].png" % (fname, i), files)
    return files


def create_patch_heatmaps_concat(patch, model256, output_dir, fname, threshold=0.5, offset=16, alpha=0.5, cmap="coolwarm",
                                 device256=None):
    """attention_visualization_utils.py:352-421: saves the mosaics ``{fname}_256th.png`` (with a ``threshold``) and
    ``{fname}_256hm.png``, three heads across.  The files are RGB; the reference's are the same pixels with an opaque alpha channel.
    ``device256`` is accepted and unused.  Returns the files."""
    res = patch_heatmaps(model256, patch, offset=offset, alpha=alpha, cmap=cmap, threshold=threshold, concat=True, cols=3)
    host = {k: v.cpu().numpy() for k, v in res.items()}
    if host["256"].ndim != 3:
        raise ValueError("create_patch_heatmaps_concat: one patch at a time (patch_heatmaps takes batches)")
    files = []
    if threshold is not None:
        _save(host["256th"], output_dir, "%s_256th.png" % fname, files)
    _save(host["256"], output_dir, "%s_256hm.png" % fname, files)
    return files
