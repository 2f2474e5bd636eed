"""A numpy restatement of the pixel stages of ``segmentTissue`` as DESIGN.md 26 defines them (from OpenCV's published
implementation): plain and slow, one function per stage, and a seeded fixture maker.  The tests of the device kernels compare
with this byte for byte; test_segment_host.py checks it against scipy's filters."""
import numpy as np

FLT_EPSILON = float(np.finfo(np.float32).eps)


def sdiv_table():
    """sdiv[0] = 0, sdiv[v] = rint(255 * 4096 / v): a float64 quotient rounded half to even"""
    t = np.zeros(256, dtype=np.int64)
    v = np.arange(1, 256, dtype=np.float64)
    t[1:] = np.rint((255.0 * 4096.0) / v).astype(np.int64)
    return t


def saturation(img):
    """uint8 [H, W, 3|4] -> uint8 [H, W]; a fourth channel is ignored"""
    rgb = img[:, :, :3].astype(np.int64)
    v = rgb.max(axis=2)
    d = v - rgb.min(axis=2)
    return ((d * sdiv_table()[v] + 2048) >> 12).astype(np.uint8)


def median(x, k):
    """the exact median (element k k // 2 of the sorted window) of the k x k window, indices clamped"""
    h, w = x.shape
    r = k // 2
    p = np.pad(x, r, mode="edge")
    win = np.stack([p[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k)], axis=-1)
    return np.sort(win, axis=-1)[:, :, (k * k) // 2].astype(np.uint8)


def histogram(x):
    return np.bincount(x.reshape(-1), minlength=256).astype(np.int64)


def otsu_sigmas(hist):
    """(sigma per level -- NaN where the level is skipped -- in the scan's own order of float64 operations)"""
    n = int(hist.sum())
    scale = 1.0 / n
    mu = float(sum(i * int(hist[i]) for i in range(256))) * scale
    mu1 = q1 = 0.0
    out = np.full(256, np.nan)
    for i in range(256):
        p = int(hist[i]) * scale
        mu1 *= q1
        q1 += p
        q2 = 1.0 - q1
        if min(q1, q2) < FLT_EPSILON or max(q1, q2) > 1.0 - FLT_EPSILON:
            continue
        mu1 = (mu1 + i * p) / q1
        mu2 = (mu - q1 * mu1) / q2
        out[i] = q1 * q2 * (mu1 - mu2) * (mu1 - mu2)
    return out


def otsu(hist):
    """the first level with a strictly larger sigma; 0 if none"""
    best, max_sigma = 0, 0.0
    for i, s in enumerate(otsu_sigmas(hist)):
        if s > max_sigma:   # (NaN compares false)
            best, max_sigma = i, s
    return best


def threshold(x, t, maxval):
    return np.where(x > t, maxval, 0).astype(np.uint8)


def _window_pass(x, c, axis, erode):
    """one separable pass: offsets -(c // 2) .. c - 1 - c // 2 along ``axis``; outside counts 0 (dilate) / 255 (erode)"""
    a = c // 2
    border = 255 if erode else 0
    n = x.shape[axis]
    pad = [(0, 0), (0, 0)]
    pad[axis] = (a, c - 1 - a)
    p = np.pad(x, pad, mode="constant", constant_values=border)
    views = [np.take(p, range(i, i + n), axis=axis) for i in range(c)]
    return (np.minimum if erode else np.maximum).reduce(views).astype(np.uint8)


def dilate(x, c):
    return _window_pass(_window_pass(x, c, 1, False), c, 0, False)


def erode(x, c):
    return _window_pass(_window_pass(x, c, 1, True), c, 0, True)


def close(x, c):
    return x.copy() if c == 0 else erode(dilate(x, c), c)


def tissue_mask(img, sthresh=20, sthresh_up=255, mthresh=7, close_size=0, use_otsu=False):
    """(mask, median plane, saturation plane, threshold used)"""
    sat = saturation(img)
    med = median(sat, mthresh)
    t = otsu(histogram(med)) if use_otsu else sthresh
    return close(threshold(med, t, sthresh_up), close_size), med, sat, t


def make_image(h, w, channels=3, seed=0):
    """Smooth blobs of pink-purple "tissue" on a near-white ground, with noise; channels = 4 adds a random alpha plane."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    field = np.zeros((h, w))
    for _ in range(4):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        s = rng.uniform(0.06, 0.18) * max(h, w, 8)
        field += np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    field = np.clip(field, 0, 1)[:, :, None]
    ground = np.array([238.0, 236.0, 240.0])
    tissue = np.array([176.0, 92.0, 158.0])
    img = ground * (1 - field) + tissue * field + rng.normal(0, 3, (h, w, 3))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if channels == 4:
        img = np.concatenate([img, rng.integers(0, 256, (h, w, 1), dtype=np.uint8)], axis=2)
    return img


# the whole-call cases of the GPU tests: shapes x settings (mthresh, close, use_otsu)
SHAPES = [(37, 53, 3), (130, 257, 4), (1, 1, 3), (1, 200, 4), (200, 1, 3), (64, 64, 3)]
SETTINGS = [(7, 4, False), (5, 100, True), (11, 2, False), (1, 0, False), (15, 0, True)]


def case_image(shape):
    h, w, c = shape
    return make_image(h, w, c, seed=1000 + h * 7 + w)
