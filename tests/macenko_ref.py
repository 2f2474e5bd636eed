"""Numpy restatement of the Macenko normalisation the device implements (include/hipt_abmil.h), steps 1-7 of the
contract, with a ``dtype`` switch: float64 is the reference, float32 the yardstick for what single precision costs.  Order
statistics are ``np.partition``; eigenvectors come from ``np.linalg.eigh`` with the sign convention (largest-magnitude component
positive).  Also the synthetic H&E fixtures of the tests: images made from the stain model itself."""
import numpy as np

HE_REF = np.array([[0.5626, 0.2159], [0.7201, 0.8012], [0.4062, 0.5581]])
MAXC_REF = np.array([1.9705, 1.0308])


def rank(n, q):
    """k of ``percentile``: the k-th smallest of n values, 1-based; ``round`` is Python's (half to even)"""
    return 1 + round(0.01 * q * (n - 1))


def percentile(t, q):
    k = rank(len(t), q)
    return np.partition(t, k - 1)[k - 1]


def to_hwc(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[-1] == 3, img.shape
    return img


def optical_density(img, Io=240, dtype=np.float64):
    """OD [h * w, 3] through the 256-entry table, as the device takes it"""
    table = -np.log((np.arange(256, dtype=dtype) + dtype(1)) / dtype(Io))
    return table.astype(dtype)[to_hwc(img).reshape(-1, 3)]


def fit(img, Io=240, alpha=1, beta=0.15, dtype=np.float64):
    """dict(status, HE [3, 2], maxC [2], E [3, 2], phi (min, max), n) of one uint8 [h, w, 3] image; status 1 = fallback"""
    dtype = np.dtype(dtype).type
    OD = optical_density(img, Io, dtype)
    tissue = ~np.any(OD < dtype(beta), axis=1)
    n = int(tissue.sum())
    out = dict(status=1, n=n, HE=np.zeros((3, 2), dtype), maxC=np.zeros(2, dtype))
    if n < 2:
        return out
    T = OD[tissue]
    cov = np.cov(T.T).astype(dtype)   # unbiased: divides by n - 1
    if not np.isfinite(cov).all():
        return out
    _, vec = np.linalg.eigh(cov)   # ascending eigenvalues
    E = vec[:, 1:3].astype(dtype)
    for j in range(2):
        if E[np.argmax(np.abs(E[:, j])), j] < 0:
            E[:, j] = -E[:, j]
    That = T @ E
    phi = np.arctan2(That[:, 1], That[:, 0])
    lo, hi = percentile(phi, alpha), percentile(phi, 100 - alpha)
    vmin = E @ np.array([np.cos(lo), np.sin(lo)], dtype)
    vmax = E @ np.array([np.cos(hi), np.sin(hi)], dtype)
    HE = np.stack([vmin, vmax], 1) if vmin[0] > vmax[0] else np.stack([vmax, vmin], 1)
    HE = HE.astype(dtype)
    if not np.isfinite(HE).all():
        return out
    with np.errstate(all="ignore"):
        C = concentrations(OD, HE)
        maxC = np.array([percentile(C[0], 99), percentile(C[1], 99)], dtype)
    if not np.isfinite(maxC).all() or (maxC <= 0).any():
        return out
    out.update(status=0, HE=HE, maxC=maxC, E=E, phi=(lo, hi))
    return out


def concentrations(OD, HE):
    """C [2, n] = (HE^T HE)^-1 HE^T OD^T: the 2 x 2 normal equations"""
    dtype = OD.dtype.type
    G = HE.T @ HE
    det = G[0, 0] * G[1, 1] - G[0, 1] * G[1, 0]
    inv = np.array([[G[1, 1], -G[0, 1]], [-G[1, 0], G[0, 0]]], dtype) / det
    return ((inv @ HE.T) @ OD.T).astype(dtype)


def apply(img, HE, maxC, Io=240, he_ref=HE_REF, maxc_ref=MAXC_REF, dtype=np.float64, exact=False):
    """the normalised uint8 [h, w, 3] image (``exact``: the real values before the clip and the truncation)"""
    dtype = np.dtype(dtype).type
    img = to_hwc(img)
    OD = optical_density(img, Io, dtype)
    HE, maxC = np.asarray(HE, dtype), np.asarray(maxC, dtype)
    C = concentrations(OD, HE)
    C2 = C * (np.asarray(maxc_ref, dtype) / maxC)[:, None]
    with np.errstate(over="ignore"):
        v = dtype(Io) * np.exp(-(np.asarray(he_ref, dtype) @ C2))
    if exact:
        return v.T.reshape(img.shape)
    return np.minimum(v, dtype(255)).astype(np.uint8).T.reshape(img.shape)   # positive: the cast truncates toward zero


def normalize(img, Io=240, alpha=1, beta=0.15, he_ref=HE_REF, maxc_ref=MAXC_REF, dtype=np.float64):
    """(normalised uint8 [h, w, 3], status); a fallback image comes back unchanged"""
    f = fit(img, Io, alpha, beta, dtype)
    if f["status"]:
        return to_hwc(img).copy(), 1
    return apply(img, f["HE"], f["maxC"], Io, he_ref, maxc_ref, dtype), 0


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
def smooth_field(rng, h, w, waves=3):
    """a smooth field in [0, 1]: a few seeded low-frequency cosines"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.zeros((h, w))
    for _ in range(waves):
        fy, fx = rng.uniform(0.3, 2.0, 2)
        f += np.cos(2 * np.pi * (fy * y / max(h, 1) + fx * x / max(w, 1)) + rng.uniform(0, 2 * np.pi))
    f -= f.min()
    return f / max(f.max(), 1e-12)


def stain_matrix(rng, jitter=0.04):
    """HE_REF perturbed, columns re-normalised"""
    M = HE_REF + rng.uniform(-jitter, jitter, HE_REF.shape)
    return M / np.linalg.norm(M, axis=0, keepdims=True)


def synth_image(h, w, seed, he=None, conc_max=(1.6, 0.9), background=0.2, flat=False, pure=0.15, Io=240):
    """uint8 [h, w, 3] from the stain model: I = Io exp(-(HE C)) - 1, two smooth concentration fields, a share of near-white
    background pixels, uint8 rounding.  A share ``pure`` of the pixels holds only H and as many only E: more than the 1 % either
    percentile cuts off, so the extreme angles are the stains themselves and the fit must recover ``he``.  ``flat``: the
    concentrations are quantised to a few levels, so that large areas hold the same bytes (many equal phi and C keys).
    Returns (image, the stain matrix it was made with)."""
    rng = np.random.default_rng(seed)
    he = stain_matrix(rng) if he is None else np.asarray(he, np.float64)
    c0 = 0.15 + conc_max[0] * smooth_field(rng, h, w)
    c1 = 0.10 + conc_max[1] * smooth_field(rng, h, w)
    if flat:
        c0, c1 = np.round(c0 * 3) / 3 + 0.05, np.round(c1 * 4) / 4 + 0.05
    if pure > 0:
        kind = rng.uniform(size=(h, w))
        c0, c1 = np.where(kind < pure, 0, c0 + 0.3 * (kind > 1 - pure)), np.where(kind > 1 - pure, 0, c1 + 0.3 * (kind < pure))
    od = np.einsum("cj,jhw->hwc", he, np.stack([c0, c1]))
    img = Io * np.exp(-od) - 1.0
    if background > 0:
        white = smooth_field(rng, h, w, 2) > 1.0 - background
        img[white] = rng.uniform(232, 250, (int(white.sum()), 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8), he


# name -> (h, w, seed, keywords of synth_image): the smallest sizes at which the kernels can still go wrong -- one 16-pixel-aligned
# image smaller than a workgroup's 4096 pixels, two odd ones (one workgroup, several), several workgroups, a multi-slab one
FIXTURES = {
    "8x8": (8, 8, 1, dict(background=0)),
    "37x53": (37, 53, 2, {}),
    "37x53_flat": (37, 53, 6, dict(flat=True)),
    "131x97": (131, 97, 3, {}),
    "300x200": (300, 200, 4, {}),
    "300x200_b": (300, 200, 8, {}),
    "300x200_flat": (300, 200, 5, dict(flat=True)),
    "300x200_clean": (300, 200, 4, dict(background=0)),
    "512x512": (512, 512, 7, {}),
}
_made = {}


def fixture(name):
    """(uint8 [h, w, 3] image, the stain matrix it was made with); made once, do not write to it"""
    if name not in _made:
        h, w, seed, kw = FIXTURES[name]
        img, he = synth_image(h, w, seed, **kw)
        img.setflags(write=False)
        _made[name] = (img, he)
    return _made[name]


def large_image(seed=21, scale=4, h=525, w=1024):
    """(uint8 [2100, 4096, 3], its stain matrix): 8.6 M pixels, more than the 1024 workgroups x 4096 pixels of one trip through an
    image, so some workgroups take two trips and some three.  A 525 x 1024 synthetic image with every pixel repeated 4 x 4: cheap
    to make, full of ties, and NOT periodic -- a part of it does not have the statistics of the whole."""
    img, he = synth_image(h, w, seed)
    return np.ascontiguousarray(np.repeat(np.repeat(img, scale, axis=0), scale, axis=1)), he


def white_image(h, w):
    return np.full((h, w, 3), 255, np.uint8)


def one_tissue_pixel_image(h, w):
    img = white_image(h, w)
    img[h // 2, w // 3] = (120, 60, 140)
    return img


def angle_deg(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = abs(float(a @ b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return float(np.degrees(np.arccos(min(1.0, c))))
