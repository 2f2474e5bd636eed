"""The oracle of the tiling tests: cv2.pointPolygonTest's sign as stated there, in numpy int64 over doubled
coordinates, and the glue of ``WholeSlideImage.process_contour`` (wsi_core/WholeSlideImage.py:415-506) with the contour checking
functions of wsi_core/util_classes.py:53-111 restated literally.  Also the shapes the tests and tools/tiling_bench.py cut their
contours from.  Nothing here touches a device."""
import numpy as np

BOUND = 1 << 30


# ---- the point test -------------------------------------------------------------------------------------------------------------
def ppt_doubled(poly, p2):
    """poly: integer [n, 2]; p2: DOUBLED points, integer [Q, 2].  int8 [Q]: 0 on a closed edge segment, else +1 / -1 by the parity
    of the edges with exactly one endpoint at y <= p.y whose point at height p.y lies right of p."""
    poly = np.asarray(poly, dtype=np.int64).reshape(-1, 2)
    p2 = np.asarray(p2, dtype=np.int64).reshape(-1, 2)
    out = np.full(len(p2), -1, np.int8)
    n = len(poly)
    if n == 0 or len(p2) == 0:
        return out
    a = 2 * poly
    b = np.roll(a, -1, axis=0)
    ax, ay, bx, by = a[:, 0][None], a[:, 1][None], b[:, 0][None], b[:, 1][None]
    step = max(1, (1 << 22) // n)
    for s in range(0, len(p2), step):
        px, py = p2[s:s + step, 0][:, None], p2[s:s + step, 1][:, None]
        d = (py - ay) * (bx - ax) - (px - ax) * (by - ay)
        cross = (ay <= py) != (by <= py)
        box = (px >= np.minimum(ax, bx)) & (px <= np.maximum(ax, bx)) & (py >= np.minimum(ay, by)) & (py <= np.maximum(ay, by))
        on = ((d == 0) & box).any(axis=1)
        right = cross & (d != 0) & ((d > 0) == (by > ay))
        odd = (right.sum(axis=1) & 1).astype(bool)
        out[s:s + step] = np.where(on, 0, np.where(odd, 1, -1))
    return out


def double_points(pts):
    """Points that are integers or multiples of 0.5, doubled exactly to int64 [Q, 2]."""
    d = np.asarray(pts, dtype=np.float64).reshape(-1, 2) * 2
    assert np.array_equal(d, np.round(d))
    return d.astype(np.int64)


# ---- stand-ins with cv2's call surface (tests/golden/make_golden_tiling.py puts them in sys.modules['cv2']) -------------------------
def pointPolygonTest(contour, pt, measureDist):
    assert measureDist is False
    return float(ppt_doubled(np.asarray(contour).reshape(-1, 2), double_points([pt]))[0])


def boundingRect(contour):
    c = np.asarray(contour).reshape(-1, 2)
    x0, y0, x1, y1 = int(c[:, 0].min()), int(c[:, 1].min()), int(c[:, 0].max()), int(c[:, 1].max())
    return x0, y0, x1 - x0 + 1, y1 - y0 + 1


def contourArea(contour):
    c = np.asarray(contour, dtype=np.int64).reshape(-1, 2)
    x, y = c[:, 0], c[:, 1]
    return abs(float((x * np.roll(y, -1) - np.roll(x, -1) * y).sum())) / 2.0


# ---- the glue ------------------------------------------------------------------------------------------------------------------------
def contour_points(pt, contour_fn, ps, shift):
    """The points one candidate is tested at against the contour, as the four checking classes form them."""
    if contour_fn == "basic":
        return [(pt[0], pt[1])]
    center = (pt[0] + ps // 2, pt[1] + ps // 2)
    if contour_fn == "center" or shift <= 0:
        return [center]
    return [(center[0] - shift, center[1] - shift), (center[0] + shift, center[1] + shift),
            (center[0] + shift, center[1] - shift), (center[0] - shift, center[1] + shift)]


def process_contour(cont, holes, level_dim0, patch_downsample, patch_size=256, step_size=256, contour_fn="four_pt", use_padding=True,
                    top_left=None, bot_right=None, center_shift=0.5):
    """int64 [n, 2]: what process_contour returns as asset_dict['coords'] ([0, 2] where it returns {})."""
    if contour_fn == "four_pt_easy":   # datasets/wsi_dataset.py:21-22
        contour_fn, center_shift = "four_pt", 0.5
    start_x, start_y, w, h = boundingRect(cont)
    patch_downsample = (int(patch_downsample[0]), int(patch_downsample[1]))
    ref_patch_size = (patch_size * patch_downsample[0], patch_size * patch_downsample[1])
    img_w, img_h = level_dim0
    if use_padding:
        stop_y = start_y + h
        stop_x = start_x + w
    else:
        stop_y = min(start_y + h, img_h - ref_patch_size[1] + 1)
        stop_x = min(start_x + w, img_w - ref_patch_size[0] + 1)
    if bot_right is not None:
        stop_y = min(bot_right[1], stop_y)
        stop_x = min(bot_right[0], stop_x)
    if top_left is not None:
        start_y = max(top_left[1], start_y)
        start_x = max(top_left[0], start_x)
    if bot_right is not None or top_left is not None:
        w, h = stop_x - start_x, stop_y - start_y
        if w <= 0 or h <= 0:
            return np.zeros((0, 2), np.int64)
    ps = ref_patch_size[0]
    shift = int(ps // 2 * center_shift) if contour_fn in ("four_pt", "four_pt_hard") else 0
    step_size_x = step_size * patch_downsample[0]
    step_size_y = step_size * patch_downsample[1]
    x_range = np.arange(start_x, stop_x, step=step_size_x)
    y_range = np.arange(start_y, stop_y, step=step_size_y)
    x_coords, y_coords = np.meshgrid(x_range, y_range, indexing="ij")
    cand = np.array([x_coords.flatten(), y_coords.flatten()]).transpose().astype(np.int64).reshape(-1, 2)
    if len(cand) == 0:
        return np.zeros((0, 2), np.int64)
    k = len(contour_points((0, 0), contour_fn, ps, shift))
    pts = np.array([contour_points((int(x), int(y)), contour_fn, ps, shift) for x, y in cand], dtype=np.int64).reshape(-1, 2)
    res = ppt_doubled(cont, 2 * pts).reshape(len(cand), k) >= 0
    keep = res.all(axis=1) if contour_fn == "four_pt_hard" else res.any(axis=1)
    hole_pt = 2 * cand + ps   # pt + ps / 2, true division
    for hole in holes:
        keep &= ~(ppt_doubled(hole, hole_pt) > 0)
    return cand[keep]


# ---- shapes ------------------------------------------------------------------------------------------------------------------------------
def blob(seed, cx, cy, r, n):
    """A star-shaped integer polygon of n vertices around (cx, cy): radius r modulated by a few seeded harmonics."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) * (2 * np.pi / n)
    rad = np.ones(n)
    for k in range(2, 7):
        rad += rng.uniform(-0.12, 0.12) * np.cos(k * t + rng.uniform(0, 2 * np.pi))
    return np.stack([np.rint(cx + r * rad * np.cos(t)), np.rint(cy + r * rad * np.sin(t))], axis=1).astype(np.int32)


def pixel_chain(poly):
    """The 8-connected pixel boundary through the polygon's vertices (what CHAIN_APPROX_NONE keeps): every step moves by at most one
    pixel in x and in y.  Consecutive duplicates are dropped; the chain may touch itself."""
    poly = np.asarray(poly, dtype=np.int64).reshape(-1, 2)
    out = []
    for a, b in zip(poly, np.roll(poly, -1, axis=0)):
        m = int(max(abs(b[0] - a[0]), abs(b[1] - a[1])))
        if m == 0:
            continue
        k = np.arange(m)[:, None]
        out.append(a[None] + (2 * k * (b - a)[None] + m) // (2 * m))
    chain = np.concatenate(out) if out else poly[:1]
    return chain.astype(np.int32)


_L = np.array([[0, 0], [2, 0], [6, 0], [6, 2], [3, 2], [3, 4], [3, 6], [0, 6], [0, 3]])
# the smallest shapes that can break the point test: collinear vertices, horizontal / vertical / diagonal edges, both orientations, a
# chain that visits a vertex twice
SHAPES = {
    "square": np.array([[0, 0], [4, 0], [4, 4], [0, 4]]),
    "L_collinear": _L,
    "L_clockwise": _L[::-1].copy(),
    "diamond": np.array([[3, 0], [6, 3], [3, 6], [0, 3]]),
    "touching_chain": np.array([[0, 0], [1, 1], [2, 0], [3, 1], [2, 2], [1, 1], [0, 2], [-1, 1]]),
    "blob": blob(1, 20, 18, 14, 37),
    "chain": pixel_chain(blob(2, 15, 15, 11, 12)),
}


def lattice2(poly, margin=2):
    """Every integer and half-integer point of the polygon's box plus a margin, DOUBLED, int64 [Q, 2]: all vertices, points on every
    edge, rays through vertices and along horizontal edges are among them."""
    poly = np.asarray(poly).reshape(-1, 2)
    lo, hi = poly.min(axis=0) - margin, poly.max(axis=0) + margin
    xs, ys = np.arange(2 * lo[0], 2 * hi[0] + 1), np.arange(2 * lo[1], 2 * hi[1] + 1)
    return np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.int64)
