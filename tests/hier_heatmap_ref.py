"""The hierarchical heat-maps of HIPT_4K/hipt_heatmap_utils.py:381-483 restated in numpy, the long way: the attention maps are
really upscaled (np.repeat), every patch and every map is really ranked by scipy (rankdata * 100 / len), the shifted layers are
really built by slicing, matplotlib colours the scores and tests/heatmap_ref.py blends them.  The patch concatenation is the
w_256 x h_256 form the reference keeps commented out (hipt_heatmap_utils.py:39-49).  Test infrastructure only.

One place is written more carefully than the reference: a layer whose offset is not smaller than the picture is left out
(``max(s - o, 0)`` rows), where the reference's negative slice end would raise on such a small picture."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as R  # noqa: E402


def rank(v):
    from scipy.stats import rankdata
    return rankdata(v) * 100 / len(v)


def upscale(a, f):
    """Nearest-neighbour upscaling of the last two axes by an integer factor (what nn.functional.interpolate does there)."""
    return np.repeat(np.repeat(a, f, axis=-2), f, axis=-1)


def upscaled_maps(a256, a4k, w_256, h_256, scale):
    """Raw maps (a256 [R, n, nh, 256], a4k [R, nh, n]) -> what _get_region_attention_scores returns per region:
    [R, n, nh, 256 / scale, 256 / scale] and [R, nh, w_256 * 256 / scale, h_256 * 256 / scale]."""
    a256, a4k = np.asarray(a256), np.asarray(a4k)
    r, n, nh, _ = a256.shape
    up256 = upscale(a256.reshape(r, n, nh, 16, 16), 16 // scale)
    up4k = upscale(a4k.reshape(a4k.shape[0], nh, w_256, h_256), 256 // scale)
    return up256, up4k


def concat_scores256(attns, w_256, h_256, size):
    blocks = [rank(attn.flatten()).reshape(size) for attn in attns]
    return np.concatenate([np.concatenate(blocks[i:i + h_256], axis=1) for i in range(0, h_256 * w_256, h_256)])


def concat_scores4k(attn, size):
    return rank(attn.flatten()).reshape(size)


def shifted(score, o):
    hs, ws = score.shape
    new = np.zeros_like(score)
    new[o:hs, o:ws] = score[:max(hs - o, 0), :max(ws - o, 0)]
    return new


def overlay(shape, offsets, unit=100):
    ov = np.ones(shape) * unit
    hs, ws = shape
    for o in offsets:
        ov[o:hs, o:ws] += unit
    return ov


def scores(a256, a4k, w_256, h_256, offset, scale):
    """(score4k [nh] of [Hs, Ws], overlay4k, score256 [nh] of [Hs, Ws], sum256 [nh], (o2, o3, o4))."""
    up256, up4k = upscaled_maps(a256, a4k, w_256, h_256, scale)
    nh = up4k.shape[1]
    o2, o3, o4 = (offset * 1) // scale, (offset * 2) // scale, (offset * 3) // scale
    b = 256 // scale
    size = (w_256 * b, h_256 * b)
    overlay4k = overlay(size, (o2, o3, o4))
    score4k = []
    for j in range(nh):
        s1, s2, s3, s4 = (concat_scores4k(up4k[r][j], size) for r in range(4))
        score4k.append((s1 + shifted(s2, o2) + shifted(s3, o3) + shifted(s4, o4)) / overlay4k)
    score256, sum256 = [], []
    for i in range(nh):
        s1 = concat_scores256(up256[0][:, i, :, :], w_256, h_256, (b, b))
        s2 = concat_scores256(up256[1][:, i, :, :], w_256, h_256, (b, b))
        sum256.append(s1 + shifted(s2, o2))
        score256.append(sum256[-1] / overlay(size, (o2,)))
    return score4k, overlay4k, score256, sum256, (o2, o3, o4)


def colours(cmap, score):
    return (cmap(score) * 255)[:, :, :3].astype(np.uint8)


def pictures(a256, a4k, w_256, h_256, base, offset=128, scale=4, alpha=0.5, cmap=None, threshold=None, w256=2, pairs=None):
    """dict of uint8 arrays: '4k' [nh, Hs, Ws, 3], '256' [nh, ...], 'blend' [pairs, ...] and, with a threshold, '256th' [nh, ...];
    'score256' (the float64 scores) rides along for the tests that pick a threshold."""
    score4k, overlay4k, score256, sum256, (o2, _, _) = scores(a256, a4k, w_256, h_256, offset, scale)
    nh = len(score4k)
    size = overlay4k.shape
    out = {"score256": score256}
    out["4k"] = np.stack([R.blend(colours(cmap, s), base, alpha) for s in score4k])
    out["256"] = np.stack([R.blend(colours(cmap, s), base, alpha) for s in score256])
    if threshold is not None:
        th = []
        for i in range(nh):
            mask = score256[i].copy()
            mask[mask < threshold] = 0
            mask[mask > threshold] = 0.95
            hm = R.blend(colours(cmap, mask), base, alpha)
            hm[mask == 0] = 0
            inverse = base.copy()
            inverse[mask == 0.95] = 0
            th.append(hm + inverse)   # uint8: wraps
        out["256th"] = np.stack(th)
    blend = []
    for j, i in (pairs if pairs is not None else [(j, i) for j in range(nh) for i in range(nh)]):
        if w256 == 2:     # hipt_heatmap_utils.py:475-480
            overlay256 = overlay(size, (o2,), unit=100 * 2)
            s256 = sum256[i] * 2 / overlay256
        elif w256 == 1:   # hipt_4k.py:295-300
            overlay256 = overlay(size, (o2,))
            s256 = sum256[i] / overlay256
        else:
            raise ValueError("the reference weighs the 256 level by 1 or 2")
        score = (score4k[j] * overlay4k + s256 * overlay256) / (overlay4k + overlay256)
        blend.append(R.blend(colours(cmap, score), base, alpha))
    out["blend"] = np.stack(blend)
    return out


def synthetic_maps(w_256, h_256, nh, seed, levels=97):
    """Seeded attention-like maps with ties: a256 [4, n, nh, 256], a4k [4, nh, n] float32, positive, quantised to `levels` values."""
    rng = np.random.default_rng(seed)
    n = w_256 * h_256
    a256 = (rng.integers(1, levels, (4, n, nh, 256)) / np.float32(levels * 64)).astype(np.float32)
    a4k = (rng.integers(1, levels, (4, nh, n)) / np.float32(levels * 4)).astype(np.float32)
    return a256, a4k


def rank_case(v, l, seed, ties):
    """float32 [v, l]: random values; with ties a few repeated values and both zeros."""
    rng = np.random.default_rng(seed)
    if not ties:
        return rng.standard_normal((v, l)).astype(np.float32)
    x = (rng.integers(-3, 4, (v, l)) / np.float32(4)).astype(np.float32)
    x[x == 0] = np.where(rng.integers(0, 2, int((x == 0).sum())) == 1, np.float32(-0.0), np.float32(0.0))
    return x


def long_way_percentiles(x, f):
    """rankdata * 100 / len of every vector of x with each value repeated f * f times (what upscaling a map by f does to its
    values), read back at one copy of each value: the oracle of the closed form."""
    x = np.asarray(x, dtype=np.float32)
    out = np.empty(x.shape, dtype=np.float64)
    for v in range(x.shape[0]):
        up = np.repeat(x[v], f * f)   # (ranks depend on the multiset alone; copy k * f * f is a copy of value k)
        out[v] = rank(up)[::f * f]
    return out
