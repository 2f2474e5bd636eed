"""A sequential restatement of ``WholeSlideImage.get_seg_mask`` (wsi_core/WholeSlideImage.py:741-757) as this project states it
(DESIGN.md 32): the contours are scaled, sorted by area and drawn one by one with ``cv2.drawContours(..., thickness=-1)``, the holes
of a contour all together after it.  ``drawContours`` with a negative thickness is OpenCV's ``CollectPolyEdges`` followed by
``FillEdgeCollection``: every polygon edge is drawn as an 8-connected line and entered into an edge table in 16.16 fixed point, and
the table is scanned row by row with the active edges paired in sorted order.  Plain Python loops over points, edges and rows: the
oracle of the device tests, sharing nothing with the kernel's counters and closed forms.  cv2 is not a dependency and OpenCV's source
was not at hand: the four details that carry the risk of a difference from cv2's own bytes are marked (*) below; none of them matters
for a contour whose consecutive points are at most one pixel apart (every line is its two end points, every table edge spans one
row at an integer x), which is what ``get_seg_mask`` draws: traced borders scaled down to the visualisation level."""
import numpy as np

SHIFT = 16
HALF = 1 << (SHIFT - 1)


def scale_points(cont, scale):
    """``(cont * scale).astype(int32)`` of ``scaleContourDim``: a float64 product, then truncation toward zero.  ``[n, 2]`` int32."""
    return np.array(np.asarray(cont).reshape(-1, 1, 2) * np.asarray(scale, dtype=np.float64), dtype="int32").reshape(-1, 2)


def scale_offset(offset, scale):
    """``(offset * scale * -1).astype(int32)``, in that order of operations."""
    return (np.array(offset) * np.array(scale) * -1).astype(np.int32)


def shoelace(pts):
    """``cv2.contourArea`` of a closed integer polygon, float64."""
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 2)
    if len(p) == 0:
        return 0.0
    q = np.roll(p, 1, axis=0)
    return float(abs(0.5 * np.sum(q[:, 0] * p[:, 1] - p[:, 0] * q[:, 1])))


def draw_order(areas):
    """Indices by area, descending, STABLE: contours of equal area keep their order.  The reference's ``sorted(zip(contours, holes),
    key=area, reverse=True)`` compares the arrays themselves on a tie and raises, so a tie has no reference behaviour to match."""
    return sorted(range(len(areas)), key=lambda i: -areas[i])


def line_points(x0, y0, x1, y1):
    """The 8-connected line of OpenCV's integer line iterator as a loop: ``D + 1`` points.  (*) The walk goes left to right: the end
    points are swapped when ``x1 < x0``."""
    if x1 < x0:
        x0, y0, x1, y1 = x1, y1, x0, y0
    dx, dy = x1 - x0, y1 - y0
    sy = 1 if dy >= 0 else -1
    ady = abs(dy)
    x_major = dx >= ady          # x on a tie
    big, small = (dx, ady) if x_major else (ady, dx)
    err = big - 2 * small
    x, y = x0, y0
    pts = [(x, y)]
    for _ in range(big):
        if err < 0:              # step the minor axis
            if x_major:
                y += sy
            else:
                x += 1
            err += 2 * big
        err -= 2 * small
        if x_major:
            x += 1
        else:
            y += sy
        pts.append((x, y))
    return pts


def _trunc_div(a, b):
    """integer division that truncates toward zero, as C's does"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def fill_collection(img, polys, value):
    """One ``drawContours(..., thickness=-1)``: ``polys`` is a list of ``[n, 2]`` integer arrays already scaled and offset; the union
    of every edge's line and of the scan fill is set to ``value`` in ``img`` (clipped to it)."""
    h, w = img.shape
    rows = {}                                    # y -> the fixed-point x of every edge active on that row
    for poly in polys:
        p = [(int(x), int(y)) for x, y in np.asarray(poly).reshape(-1, 2)]
        if not p:
            continue
        prev = p[-1]                             # the closing edge comes first
        for cur in p:
            for x, y in line_points(prev[0], prev[1], cur[0], cur[1]):       # (a) the border line
                if 0 <= x < w and 0 <= y < h:
                    img[y, x] = value
            if prev[1] != cur[1]:                                             # (b) the edge table; horizontal edges stay out
                (x0, y0), (x1, y1) = (prev, cur) if prev[1] < cur[1] else (cur, prev)
                dx = _trunc_div((x1 - x0) << SHIFT, y1 - y0)                  # (*) truncates toward zero
                for y in range(max(y0, 0), min(y1, h)):                       # (*) y0 <= y < y1: the last row is not filled
                    rows.setdefault(y, []).append((x0 << SHIFT) + (y - y0) * dx)
            prev = cur
    for y, xs in rows.items():
        xs.sort()
        for k in range(0, len(xs) - 1, 2):       # an edge table of a closed polygon has an even number of entries per row
            xa, xb = (xs[k] + HALF) >> SHIFT, (xs[k + 1] + HALF) >> SHIFT     # (*) + 0.5 and floor at BOTH ends, both included
            xa, xb = max(xa, 0), min(xb, w - 1)
            if xa <= xb:
                img[y, xa:xb + 1] = value
    return img


def seg_mask_ref(contours, holes, region_size, scale, use_holes=False, offset=(0, 0), return_order=False):
    """``get_seg_mask``: ``contours`` a list of ``[n, 1, 2]`` / ``[n, 2]`` integer arrays, ``holes`` a list (one entry per contour) of
    lists of such arrays, ``region_size = (w, h)``.  bool ``[h, w]``."""
    w, h = (int(v) for v in region_size)
    img = np.zeros((h, w), dtype=np.uint8)
    off = scale_offset(offset, scale)
    conts = [scale_points(c, scale) for c in contours]
    hls = [[scale_points(hole, scale) for hole in hs] for hs in holes]
    order = draw_order([shoelace(c) for c in conts])
    for i in order:
        fill_collection(img, [conts[i] + off], 1)
        if use_holes and len(hls[i]):
            fill_collection(img, [hole + off for hole in hls[i]], 0)       # all holes of one contour together: even-odd among them
    return (img.astype(bool), order) if return_order else img.astype(bool)
