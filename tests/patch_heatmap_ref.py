"""The patch-level heat-maps of HIPT_4K/attention_visualization_utils.py:293-421 restated in numpy, the long way, from their
description: Pillow crops the patch and adds the margin, the 16 x 16 attention maps are really upscaled (np.repeat) and really
ranked by scipy (rankdata * 100 / len over 65 536 values), the second layer is really shifted by slicing, matplotlib colours the
scores, tests/heatmap_ref.py blends them and Pillow pastes the mosaic.  Test infrastructure only.

One place is written more carefully than the reference: the mosaic is returned as RGB.  The reference's canvas is RGBA, created
fully transparent, and every pasted picture is opaque; a canvas pixel no picture covers stays fully transparent and carries no
colour, so the RGB mosaic takes it premultiplied: 0.  With the reference's six heads, three across, no such pixel exists."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as R  # noqa: E402
import hier_heatmap_ref as HR  # noqa: E402

S = 256


def add_margin(img, top, right, bottom, left, color):
    from PIL import Image
    out = Image.new(img.mode, (img.width + right + left, img.height + top + bottom), color)
    out.paste(img, (left, top))
    return out


def layers(patch_u8):
    """(layer 1, layer 2) uint8 [256, 256, 3]: the patch, and its crop from (16, 16) with a white margin right and below."""
    from PIL import Image
    patch = Image.fromarray(patch_u8)
    second = add_margin(patch.crop((16, 16, 256, 256)), top=0, left=0, bottom=16, right=16, color=(255, 255, 255))
    return np.array(patch.copy()), np.array(second)


def ranked(a):
    """A raw map [256] -> the ranks of its upscaled [256, 256] form."""
    up = HR.upscale(np.asarray(a, dtype=np.float32).reshape(16, 16), 16)
    return HR.rank(up.flatten()).reshape(S, S)


def score(a1, a2, offset):
    """float64 [256, 256] from the raw maps [256] of the two layers."""
    s1, s2 = ranked(a1), ranked(a2)
    new2 = np.zeros_like(s2)
    new2[offset:S, offset:S] = s2[:(S - offset), :(S - offset)]
    ov = np.ones_like(s2) * 100
    ov[offset:S, offset:S] += 100
    return (s1 + new2) / ov


def thresholded(sc, patch, cmap, alpha, threshold):
    mask = sc.copy()
    mask[mask < threshold] = 0
    mask[mask > threshold] = 0.95
    hm = R.blend(HR.colours(cmap, mask), patch, alpha)
    hm[mask == 0] = 0
    inverse = patch.copy()
    inverse[mask == 0.95] = 0
    return hm + inverse   # uint8: wraps


def pictures(a256, patch, offset=16, alpha=0.5, cmap=None, threshold=None):
    """One patch: a256 [2, nh, 256] float32, patch uint8 [256, 256, 3] -> dict of '256' [nh, 256, 256, 3], with a threshold
    '256th' [nh, 256, 256, 3]; 'score' (the float64 scores, [nh, 256, 256]) rides along for the tests that pick a threshold."""
    nh = a256.shape[1]
    sc = [score(a256[0, i], a256[1, i], offset) for i in range(nh)]
    out = {"score": np.stack(sc), "256": np.stack([R.blend(HR.colours(cmap, s), patch, alpha) for s in sc])}
    if threshold is not None:
        out["256th"] = np.stack([thresholded(s, patch, cmap, alpha, threshold) for s in sc])
    return out


def concat_image(imgs, how="horizontal", gap=0):
    """getConcatImage: PIL images side by side (or stacked) on a transparent RGBA canvas."""
    from PIL import Image
    gap_dist = (len(imgs) - 1) * gap
    if how == "vertical":
        w, h = max(img.width for img in imgs), sum(img.height for img in imgs) + gap_dist
        dst, at = Image.new("RGBA", (w, h), color=(255, 255, 255, 0)), 0
        for img in imgs:
            dst.paste(img, (0, at))
            at += img.height + gap
    else:
        w, h = sum(img.width for img in imgs) + gap_dist, min(img.height for img in imgs)
        dst, at = Image.new("RGBA", (w, h), color=(255, 255, 255, 0)), 0
        for img in imgs:
            dst.paste(img, (at, 0))
            at += img.width + gap
    return dst


def mosaic(pics, cols=3):
    """uint8 [rows * 256, cols * 256, 3]: getConcatImage([getConcatImage(p[0:cols]), getConcatImage(p[cols:2 cols]), ...], 'vertical')
    of the pictures [nh, 256, 256, 3], premultiplied to RGB (the module's note)."""
    from PIL import Image
    imgs = [Image.fromarray(p) for p in pics]
    rows = [concat_image(imgs[i:i + cols]) for i in range(0, len(imgs), cols)]
    rgba = np.array(concat_image(rows, how="vertical"))
    assert set(np.unique(rgba[:, :, 3])) <= {0, 255}
    return rgba[:, :, :3] * (rgba[:, :, 3:] == 255)


def synthetic_maps(p, nh, seed, levels=97):
    """Seeded attention-like maps with ties: a256 [P, 2, nh, 256] float32, positive, quantised to `levels` values."""
    rng = np.random.default_rng(seed)
    return (rng.integers(1, levels, (p, 2, nh, 256)) / np.float32(levels * 64)).astype(np.float32)


def synthetic_patches(p, seed):
    return np.random.default_rng(seed).integers(0, 256, (p, S, S, 3), dtype=np.uint8)
