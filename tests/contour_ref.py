"""A sequential restatement of ``cv2.findContours(mask, cv2.RETR_CCOMP, cv2.CHAIN_APPROX_NONE)`` as this project states it (DESIGN.md
27): Suzuki and Abe's raster scan with border following (Topological structural analysis of digitized binary images by border
following, CVGIP 30, 1985, algorithm 1), 8-connected foreground, 4-connected background, on a plane surrounded by a frame of zeros.
Plain Python over a list of rows: the oracle of the device tests, written from the paper's steps -- a marked picture, one border
followed point by point -- and sharing nothing with the kernels' labels, states and ranks.  cv2 is not a dependency: the order of
the list is this project's reading of OpenCV's tree insertion, not a measurement."""
import numpy as np

# the eight neighbours, counter-clockwise on screen from east, as (dy, dx); rows grow downwards
NB = [(0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1)]


def _follow(f, i, j, first, nbd):
    """Steps 3.1 - 3.5 from the start (i, j); ``first`` is the direction of the pixel the first, clockwise, search begins at.  Marks
    ``f`` with ``nbd`` / ``-nbd`` and returns the border's points as (x, y)."""
    found = None
    for k in range(1, 9):   # (3.1) clockwise: decreasing direction; `first` itself is background, so it may come last
        d = (first - k) % 8
        if f[i + NB[d][0]][j + NB[d][1]] != 0:
            found = d
            break
    if found is None:
        f[i][j] = -nbd
        return [(j - 1, i - 1)]
    i1, j1 = i + NB[found][0], j + NB[found][1]
    i2, j2, i3, j3 = i1, j1, i, j    # (3.2)
    pts = []
    while True:
        pts.append((j3 - 1, i3 - 1))
        back = NB.index((i2 - i3, j2 - j3))
        east_was_zero = False
        for k in range(1, 9):   # (3.3) counter-clockwise from the element after (i2, j2)
            d = (back + k) % 8
            if f[i3 + NB[d][0]][j3 + NB[d][1]] != 0:
                break
            if d == 0:
                east_was_zero = True
        i4, j4 = i3 + NB[d][0], j3 + NB[d][1]
        if east_was_zero:       # (3.4)
            f[i3][j3] = -nbd
        elif f[i3][j3] == 1:
            f[i3][j3] = nbd
        if (i4, j4) == (i, j) and (i3, j3) == (i1, j1):   # (3.5)
            return pts
        i2, j2, i3, j3 = i3, j3, i4, j4


def borders(mask):
    """Every border in the raster scan's order of discovery: a list of ``(kind, points, parent)`` with kind 0 outer / 1 hole, points a
    list of (x, y), parent the list index of the outer border a hole runs on (None for an outer border: RETR_CCOMP has two levels)."""
    mask = np.asarray(mask)
    h, w = mask.shape
    f = [[0] * (w + 2)] + [[0] + [1 if v else 0 for v in row] + [0] for row in mask.tolist()] + [[0] * (w + 2)]
    out = []
    info = {1: (1, None)}   # nbd -> (kind, the list index of its outer border); 1 is the frame, a hole border
    nbd = 1
    for i in range(1, h + 1):
        lnbd = 1
        row = f[i]
        for j in range(1, w + 1):
            v = row[j]
            if v == 0:
                continue
            kind = None
            if v == 1 and row[j - 1] == 0:
                kind, first = 0, 4    # an outer border; the search begins at the west neighbour
            elif v >= 1 and row[j + 1] == 0:
                kind, first = 1, 0    # a hole border; it begins at the east neighbour, a pixel of the hole
                if v > 1:
                    lnbd = v
            if kind is not None:
                nbd += 1
                lkind, louter = info[lnbd]
                if kind == 0:
                    info[nbd] = (0, len(out))
                    parent = None
                else:
                    parent = louter   # the last border met is the outer border around this hole, or a hole border of the same one
                    info[nbd] = (1, parent)
                out.append((kind, _follow(f, i, j, first, nbd), parent))
            if row[j] != 1:
                lnbd = abs(row[j])
    return out


def order(found):
    """The order of the list: top-level borders in descending raster order of their start pixel, each followed at once by its
    holes in descending raster order of theirs.  Returns indices into ``found``."""
    def raster(b):
        x, y = found[b][1][0]
        return (y, x)
    seq = []
    for t in sorted((b for b in range(len(found)) if found[b][0] == 0), key=raster, reverse=True):
        seq.append(t)
        seq += sorted((b for b in range(len(found)) if found[b][2] == t and found[b][0] == 1), key=raster, reverse=True)
    return seq


def find_contours(mask):
    """``(contours, hierarchy)`` in cv2's format: a tuple of int32 ``[n, 1, 2]`` arrays of (x, y) and an int32 ``[1, C, 4]`` array of
    ``[next, previous, first_child, parent]``; ``((), None)`` for a mask without foreground."""
    found = borders(mask)
    if not found:
        return (), None
    seq = order(found)
    pos = {b: k for k, b in enumerate(seq)}
    hier = np.full((len(seq), 4), -1, dtype=np.int32)
    last_sibling = {}
    for k, b in enumerate(seq):
        parent = found[b][2]
        key = -1 if parent is None else pos[parent]
        hier[k, 3] = key
        if key in last_sibling:
            hier[k, 1] = last_sibling[key]
            hier[last_sibling[key], 0] = k
        elif key >= 0:
            hier[key, 2] = k
        last_sibling[key] = k
    return tuple(np.array(found[b][1], dtype=np.int32).reshape(-1, 1, 2) for b in seq), hier[None]


def trace(mask):
    """The same as ``(points int32 [P, 2], offsets int64 [C + 1], hierarchy int32 [C, 4])``."""
    contours, hier = find_contours(mask)
    if hier is None:
        return np.zeros((0, 2), np.int32), np.zeros((1,), np.int64), np.zeros((0, 4), np.int32)
    offsets = np.zeros(len(contours) + 1, dtype=np.int64)
    np.cumsum([len(c) for c in contours], out=offsets[1:])
    return np.concatenate([c.reshape(-1, 2) for c in contours]), offsets, hier[0]


# ---- masks ----------------------------------------------------------------------------------------------------------------------
def random_mask(h, w, density, seed):
    return (np.random.default_rng(seed).random((h, w)) < density).astype(np.uint8) * 255


def smooth_mask(h, w, seed, sigma=6.0, level=0.0):
    """Tissue-like: seeded noise smoothed by a box filter run three times (close to a Gaussian of ``sigma``), thresholded; blobs with
    holes and islands."""
    from scipy import ndimage
    a = np.random.default_rng(seed).standard_normal((h, w))
    size = max(3, int(round(sigma * 2)) | 1)
    for _ in range(3):
        a = ndimage.uniform_filter(a, size=size, mode="wrap")
    return (a > level * a.std()).astype(np.uint8) * 255
