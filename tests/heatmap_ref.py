"""Numpy restatement of the reference's heat-map rasteriser (wsi_core/WholeSlideImage.py:576-684 with blur=False), written from
its description: two loops over the patches with slice arithmetic, then the blend.  It is the yardstick of the device kernels
(tests/test_gpu_heatmap.py compares bit for bit) and the CPU side of tools/heatmap_bench.py.

Differences from the reference, all deliberate: the caller's scores are not modified; the counter is int32 (the reference's
uint16 wraps at 65 536 covering patches); the blend is DEFINED as cv2.addWeighted's documented formula in float32,
``sat_u8(rint(float32(img) * float32(alpha) + float32(canvas) * float32(1 - alpha)))`` with every operation rounded on its own --
cv2 itself is not a dependency of the tests.
"""
import numpy as np


def percentiles(scores):
    from scipy.stats import rankdata
    return rankdata(scores, "average") / len(scores) * 100


def scaled(coords, patch_size, scale):
    """(xy int [N, 2], (pw, ph)): the two ceil() lines."""
    scale = np.broadcast_to(np.asarray(scale, dtype=np.float64), (2,))
    ps = np.ceil(np.broadcast_to(np.asarray(patch_size), (2,)) * scale).astype(int)
    xy = np.ceil(np.asarray(coords) * scale).astype(int)
    return xy, ps


def normalised(scores, binarize, thresh, convert_to_percentiles):
    """(scores / 100 after the optional percentile conversion, threshold)"""
    s = np.array(scores, dtype=np.float64).reshape(-1)
    n = len(s)
    if binarize:
        threshold = 1.0 / n if thresh < 0 else thresh
    else:
        threshold = 0.0
    if convert_to_percentiles and n:
        s = percentiles(s)
    return s / 100, threshold


def overlay(scores, coords, patch_size, scale, region_size, binarize=False, thresh=0.5, convert_to_percentiles=False):
    """(overlay float64 [h, w], counter int32 [h, w]): the first loop and the division."""
    w, h = region_size
    xy, (pw, ph) = scaled(coords, patch_size, scale)
    assert xy.size == 0 or xy.min() >= 0, "negative coordinates would wrap around in the slices"
    s, threshold = normalised(scores, binarize, thresh, convert_to_percentiles)
    acc = np.zeros((h, w), dtype=np.float64)
    counter = np.zeros((h, w), dtype=np.int32)
    for idx in range(len(xy)):
        score = s[idx]
        x, y = xy[idx]
        if score >= threshold:
            if binarize:
                score = 1.0
        else:
            score = 0.0
        acc[y:y + ph, x:x + pw] += score
        counter[y:y + ph, x:x + pw] += 1
    covered = counter != 0
    if binarize:
        acc[covered] = np.around(acc[covered] / counter[covered])
    else:
        acc[covered] = acc[covered] / counter[covered]
    return acc, counter


def blend(img, canvas, alpha):
    a, b = np.float32(alpha), np.float32(1 - alpha)
    p = img.astype(np.float32) * a
    q = canvas.astype(np.float32) * b
    return np.clip(np.rint(p + q), 0, 255).astype(np.uint8)


def render(scores, coords, patch_size, scale, region_size, canvas=None, mask=None, alpha=0.4, binarize=False, thresh=0.5,
           convert_to_percentiles=False, cmap="coolwarm"):
    """uint8 [h, w, 3]: the second loop (colour and paint, patch by patch) and the blend."""
    import matplotlib
    w, h = region_size
    ov, _ = overlay(scores, coords, patch_size, scale, region_size, binarize, thresh, convert_to_percentiles)
    xy, (pw, ph) = scaled(coords, patch_size, scale)
    s, threshold = normalised(scores, binarize, thresh, convert_to_percentiles)
    base = np.full((h, w, 3), 255, dtype=np.uint8) if canvas is None else np.array(canvas, dtype=np.uint8)
    img = base.copy()
    if isinstance(cmap, str):
        cmap = matplotlib.colormaps[cmap]
    for idx in range(len(xy)):
        if s[idx] >= threshold:
            x, y = xy[idx]
            raw = ov[y:y + ph, x:x + pw]
            block = img[y:y + ph, x:x + pw].copy()
            colour = (cmap(raw) * 255)[:, :, :3].astype(np.uint8)
            if mask is not None:
                m = mask[y:y + ph, x:x + pw]
                block[m] = colour[m]
            else:
                block = colour
            img[y:y + ph, x:x + pw] = block
    if alpha < 1.0:
        img = blend(img, base, alpha)
    return img
