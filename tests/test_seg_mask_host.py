"""CPU tests of the device tissue-mask fill.  They pin the sequential restatement the device is compared with
(tests/seg_mask_ref.py) by two checks that share nothing with it -- scipy's ``binary_fill_holes`` on traced unit-step contours, and
exact integer crossing numbers on polygons with long edges -- then the kernel's closed forms of a row (csrc/fill_line.h, compiled
into a small host program) against the restatement's loops, the draw order, the reference's scale / offset arithmetic, the entry
point declared, exported and bound, and the refusals, which come before anything touches a device."""
import os
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
from scipy import ndimage

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_ref as CR  # noqa: E402
import seg_mask_ref as SM  # noqa: E402
import test_gpu_contours as TC  # noqa: E402  (the seventeen masks of the contour tests)

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import segment as SG  # noqa: E402

BADARG, UNSUPPORTED = -1, -4
CSRC = os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc")


# ---- check 1: unit-step contours against scipy ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TC.NAMES)
def test_filled_outer_contours_equal_binary_fill_holes(name):
    assert len(TC.NAMES) == 17
    mask = TC.make(name)
    h, w = mask.shape
    contours, hier = CR.find_contours(mask)
    outer = [c for k, c in enumerate(contours) if hier[0][k][3] == -1]
    got = SM.seg_mask_ref(outer, [[] for _ in outer], (w, h), [1.0, 1.0], use_holes=False)
    assert got.dtype == bool and got.shape == (h, w)
    assert np.array_equal(got, ndimage.binary_fill_holes(mask != 0))       # scipy's default: a 4-connected background


def test_holes_cut_the_traced_holes_out_again():
    """with use_holes the traced hole borders are drawn with 0: they run on FOREGROUND pixels, so what remains is the mask less the
    pixels of its hole borders, and never more than the mask's filled outline"""
    mask = TC.make("nested")
    h, w = mask.shape
    contours, hier = CR.find_contours(mask)
    outer = [k for k in range(len(contours)) if hier[0][k][3] == -1]
    holes = [[contours[j] for j in range(len(contours)) if hier[0][j][3] == k] for k in outer]
    got = SM.seg_mask_ref([contours[k] for k in outer], holes, (w, h), [1.0, 1.0], use_holes=True)
    filled = ndimage.binary_fill_holes(mask != 0)
    assert (got <= filled).all() and got.sum() < filled.sum()
    # the island inside the big blob's hole is the smaller contour: it is drawn later and survives the hole of the first
    assert got[5, 5] and not got[4, 4] and got[1, 1]


# ---- check 2: long edges against exact crossing numbers -----------------------------------------------------------------------
def strictly_inside(poly, px, py):
    """even-odd rule by exact integer arithmetic: False on the boundary"""
    odd = False
    n = len(poly)
    for k in range(n):
        (ax, ay), (bx, by) = poly[k - 1], poly[k]
        cross = (bx - ax) * (py - ay) - (by - ay) * (px - ax)
        if cross == 0 and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by):
            return False
        if (ay <= py) != (by <= py) and ((cross > 0) == (by > ay)):
            odd = not odd
    return odd


def segment_meets_box(a, b, lo, hi):
    """does the closed segment a-b meet the closed box [lo, hi]?  Liang-Barsky over the rationals"""
    t0, t1 = Fraction(0), Fraction(1)
    for k in range(2):
        d = b[k] - a[k]
        if d == 0:
            if not lo[k] <= a[k] <= hi[k]:
                return False
            continue
        ta, tb = Fraction(lo[k] - a[k], d), Fraction(hi[k] - a[k], d)
        t0, t1 = max(t0, min(ta, tb)), min(t1, max(ta, tb))
        if t0 > t1:
            return False
    return True


def near_region(poly, px, py):
    """Chebyshev distance at most 1 between pixel (px, py) and the closed region of the polygon: the 3 x 3 square around the pixel
    meets an edge, or lies wholly inside"""
    if any(segment_meets_box(poly[k - 1], poly[k], (px - 1, py - 1), (px + 1, py + 1)) for k in range(len(poly))):
        return True
    return strictly_inside(poly, px, py)


def star(cx, cy, r_out, r_in, n, turn=0.3):
    out = []
    for k in range(2 * n):
        r = r_out if k % 2 == 0 else r_in
        a = turn + np.pi * k / n
        out.append((int(round(cx + r * np.cos(a))), int(round(cy + r * np.sin(a)))))
    return out


POLYGONS = {
    "star": star(30, 26, 25, 9, 7),                                        # edges in all eight octants
    "pentagram": [star(24, 24, 22, 22, 5, 0.1)[k] for k in (0, 4, 8, 2, 6)],   # self-intersecting: even-odd leaves the core empty
    "sliver": [(2, 3), (55, 9), (3, 5)],
    "clipped": [(-20, 10), (30, -15), (75, 30), (25, 70)],
    "steps": [(5, 5), (40, 5), (40, 20), (20, 20), (20, 35), (50, 35), (50, 50), (5, 50)],
    "random": [tuple(int(v) for v in p) for p in np.random.default_rng(5).integers(-5, 65, size=(9, 2))],
}


@pytest.mark.parametrize("name", list(POLYGONS))
def test_long_edges_against_exact_crossing_numbers(name):
    poly = POLYGONS[name]
    w, h = 60, 56
    got = SM.fill_collection(np.zeros((h, w), np.uint8), [np.array(poly)], 1).astype(bool)
    inside = np.array([[strictly_inside(poly, x, y) for x in range(w)] for y in range(h)])
    assert inside.sum() > 20
    assert (got >= inside).all(), np.argwhere(inside & ~got)[:5]
    stray = [(x, y) for y, x in np.argwhere(got) if not near_region(poly, int(x), int(y))]
    assert not stray, stray[:5]
    if name == "pentagram":
        assert not got[24, 24] and got.sum() > 0


def test_two_overlapping_holes_fill_even_odd():
    a = np.array([(10, 10), (30, 10), (30, 30), (10, 30)])
    b = a + 10
    img = np.ones((48, 48), np.uint8)
    SM.fill_collection(img, [a, b], 0)
    assert img[15, 15] == 0 and img[35, 35] == 0 and img[25, 25] == 1 and img[5, 5] == 1   # the overlap is crossed twice: kept
    assert img[20, 25] == 0 and img[25, 20] == 0                                            # ... but the borders inside it are lines


# ---- the kernel's closed forms of a row against the loops ---------------------------------------------------------------------
MAIN = r"""
#include <stdio.h>
#include "fill_line.h"
int main(void) {
    const int R = 6;
    for (int x0 = -R; x0 <= R; ++x0) for (int y0 = -R; y0 <= R; ++y0) for (int x1 = -R; x1 <= R; ++x1) for (int y1 = -R; y1 <= R; ++y1) {
        printf("%d %d %d %d", x0, y0, x1, y1);
        for (int y = -R - 1; y <= R + 1; ++y) {
            int ca, cb, col;
            if (hipt_fill_line_run(x0, y0, x1, y1, y, &ca, &cb)) printf(" L%d:%d:%d", y, ca, cb);
            if (y0 != y1 && hipt_fill_crossing(x0, y0, x1, y1, y, &col)) printf(" X%d:%d", y, col);
        }
        printf("\n");
    }
    return 0;
}
"""


def test_closed_forms_of_a_row_equal_the_loops_in_a_13_x_13_box(tmp_path):
    src = tmp_path / "main.cpp"
    src.write_text(MAIN)
    exe = tmp_path / "closed_forms"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, str(src), "-o", str(exe)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(lines) == 13 ** 4
    for line in lines:
        tok = line.split()
        x0, y0, x1, y1 = (int(v) for v in tok[:4])
        runs = {}
        for x, y in SM.line_points(x0, y0, x1, y1):
            runs.setdefault(y, []).append(x)
        want = []
        for y in range(-7, 8):
            if y in runs:
                xs = sorted(runs[y])
                assert xs == list(range(xs[0], xs[-1] + 1))                # the pixels of a line on one row are one run
                want.append(f"L{y}:{xs[0]}:{xs[-1]}")
            if y0 != y1 and min(y0, y1) <= y < max(y0, y1):
                (xa, ya), (xb, yb) = ((x0, y0), (x1, y1)) if y0 < y1 else ((x1, y1), (x0, y0))
                xf = (xa << 16) + (y - ya) * SM._trunc_div((xb - xa) << 16, yb - ya)
                want.append(f"X{y}:{(xf + 32768) >> 16}")
        assert tok[4:] == want, line


def test_line_loop_literal_examples():
    assert SM.line_points(0, 0, 3, 0) == [(0, 0), (1, 0), (2, 0), (3, 0)]
    assert SM.line_points(2, 2, 2, 2) == [(2, 2)]
    assert SM.line_points(0, 0, 2, 2) == [(0, 0), (1, 1), (2, 2)]                       # a tie: x is the major axis
    assert SM.line_points(0, 0, 4, 1) == [(0, 0), (1, 0), (2, 0), (3, 1), (4, 1)]       # err = 2: -, -, then the minor step
    assert SM.line_points(4, 1, 0, 0) == SM.line_points(0, 0, 4, 1)                     # walked left to right either way
    assert SM.line_points(0, 0, 1, -3) == [(0, 0), (0, -1), (1, -2), (1, -3)]
    assert SM.line_points(0, 3, 0, 0) == [(0, 3), (0, 2), (0, 1), (0, 0)]               # vertical: no swap (x1 == x0)


# ---- order, scale, offset -----------------------------------------------------------------------------------------------------
def test_draw_order_is_by_area_descending_and_stable():
    sq = lambda x, y, s: np.array([(x, y), (x + s, y), (x + s, y + s), (x, y + s)], np.int32).reshape(-1, 1, 2)   # noqa: E731
    contours = [sq(0, 0, 4), sq(10, 0, 8), sq(0, 10, 4), sq(20, 20, 8), sq(2, 2, 6)]
    areas = [SM.shoelace(c) for c in contours]
    assert areas == [16.0, 64.0, 16.0, 64.0, 36.0] and areas == [SG.contour_area(c) for c in contours]
    assert SM.draw_order(areas) == [1, 3, 4, 0, 2]
    assert SG._draw_order(areas).tolist() == [1, 3, 4, 0, 2]
    # the order matters: a small contour drawn after the hole of a big one it lies in survives
    big, small, hole = sq(0, 0, 20), sq(8, 8, 4), sq(4, 4, 12)
    got, order = SM.seg_mask_ref([small, big], [[], [hole]], (24, 24), [1.0, 1.0], use_holes=True, return_order=True)
    assert order == [1, 0] and got[10, 10] and not got[6, 6] and got[2, 2]


def test_scale_and_offset_arithmetic_of_the_reference():
    cont = np.array([(-7, 9), (7, -9), (10, 10), (-1, 1)], np.int32).reshape(-1, 1, 2)
    want = [(-2, 2), (2, -2), (3, 3), (0, 0)]                               # float64 products truncated toward zero, not floored
    assert SM.scale_points(cont, [0.3, 0.3]).tolist() == [list(p) for p in want]
    got = SG.scale_contours([cont], [0.3, 0.3])
    assert got[0].dtype == np.int32 and got[0].shape == (4, 1, 2) and got[0].reshape(-1, 2).tolist() == [list(p) for p in want]
    holes = SG.scale_holes([[cont, cont[:2]], []], np.array([0.5, 0.25]))
    assert [len(hs) for hs in holes] == [2, 0] and holes[0][1].reshape(-1, 2).tolist() == [[-3, 2], [3, -2]]
    assert SM.scale_offset((10, 7), [0.3, 0.3]).tolist() == [-3, -2] and SM.scale_offset((10, 7), [0.3, 0.3]).dtype == np.int32
    assert SM.scale_offset((-10, 5), [0.25, 0.5]).tolist() == [2, -2]       # 2.5 -> 2, -2.5 -> -2
    # 1 / 3 is not exact: 9 * (1 / 3) is 3.0 in float64, 3 * 0.1 * 10 is not -- the product is taken once, as the reference does
    assert SM.scale_points(np.array([[9, 29]]), [1 / 3, 0.1]).tolist() == [[3, 2]]


# ---- the entry point and its refusals -----------------------------------------------------------------------------------------
def test_entry_point_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    decl = re.search(r"^int hipt_fill_contours\((.*?)\);", hdr, re.S | re.M).group(1)
    args = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert args == ["points", "n_points", "poly_off", "n_polys", "collections", "n_collections", "scale_x", "scale_y", "off_x", "off_y",
                    "coord_bound", "h", "w", "max_cols", "mask", "stream"]
    assert len(N.SIGNATURES["hipt_fill_contours"][1]) == len(args) and hasattr(N.lib(), "hipt_fill_contours")
    assert N.lib().hipt_abi_version() == N.ABI_VERSION    # additive: the version stays
    for macro, value in (("HIPT_FILL_MAX_DIM", N.FILL_MAX_DIM), ("HIPT_FILL_MAX_POINTS", N.FILL_MAX_POINTS),
                         ("HIPT_FILL_COORD_BOUND", N.FILL_COORD_BOUND), ("HIPT_FILL_MAX_COLS", N.FILL_MAX_COLS),
                         ("HIPT_FILL_COLLECTION_INTS", N.FILL_COLLECTION_INTS)):
        assert f"#define {macro} {value}\n" in hdr
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bfill\.hip\b", mk, re.M) and "fill_line.h" in mk
    src = open(os.path.join(CSRC, "fill.hip")).read()
    assert "asm" not in src.replace("assembly", "") and "hipMalloc" not in src and "Synchronize" not in src
    import hipt_abmil_atec23_amd as amd
    for name in ("seg_mask", "get_seg_mask_like", "scale_contours", "scale_holes"):
        assert getattr(amd, name) is getattr(SG, name)


def test_library_refuses_without_launching():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    base = dict(points=0x10000, n_points=100, poly_off=0x20000, n_polys=3, colls=0x30000, n_colls=2, sx=0.25, sy=0.25, offx=0, offy=0,
                bound=4096, h=64, w=200, max_cols=0, mask=0x40000)

    def fill(**kw):
        a = dict(base, **kw)
        return lib.hipt_fill_contours(a["points"], a["n_points"], a["poly_off"], a["n_polys"], a["colls"], a["n_colls"], a["sx"], a["sy"],
                                      a["offx"], a["offy"], a["bound"], a["h"], a["w"], a["max_cols"], a["mask"], None)
    assert fill(points=None) == BADARG and fill(poly_off=None) == BADARG and fill(colls=None) == BADARG and fill(mask=None) == BADARG
    assert fill(points=0x10004) == BADARG and fill(poly_off=0x20004) == BADARG and fill(colls=0x30002) == BADARG
    assert fill(h=0) == BADARG and fill(w=-1) == BADARG and fill(n_points=-1) == BADARG and fill(n_polys=-1) == BADARG
    assert fill(n_colls=-1) == BADARG and fill(bound=-1) == BADARG and fill(sx=float("nan")) == BADARG
    for bad in (1, 63, 65, 100, N.FILL_MAX_COLS + 64, -64):
        assert fill(max_cols=bad) == BADARG, bad
    # the envelope: the library's own error, nothing clipped
    assert fill(h=N.FILL_MAX_DIM + 1) == UNSUPPORTED and b"envelope" in lib.hipt_last_error()
    assert fill(w=N.FILL_MAX_DIM + 1) == UNSUPPORTED
    assert fill(n_points=N.FILL_MAX_POINTS + 1) == UNSUPPORTED
    assert fill(bound=4 * N.FILL_COORD_BOUND + 4) == UNSUPPORTED            # 0.25 * bound just beyond 2^20
    assert fill(bound=N.FILL_COORD_BOUND, sx=1.0, offx=1) == UNSUPPORTED and fill(bound=N.FILL_COORD_BOUND, sy=-1.0, offy=-1) == UNSUPPORTED
    assert fill(sx=float("inf")) == UNSUPPORTED and fill(bound=0, offx=-(1 << 31)) == UNSUPPORTED


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    before = N.calls
    sq = np.array([(1, 1), (5, 1), (5, 5), (1, 5)], np.int32).reshape(-1, 1, 2)

    def bad(*a, match=None, **kw):
        with pytest.raises(ValueError, match=match):
            SG.seg_mask(*a, **kw)
    bad([sq], [[]], (0, 8), [1, 1], match="region_size")
    bad([sq], [[]], (8, N.FILL_MAX_DIM + 1), [1, 1], match="region_size")
    bad([sq], [[]], (8.0, 8), [1, 1], match="region_size")
    bad([sq], [[]], (8, 8), [float("nan"), 1], match="finite")
    bad([sq], [[], []], (8, 8), [1, 1], match="lists of holes")
    bad([sq.astype(np.float32)], [[]], (8, 8), [1, 1], match="integer array")
    bad([np.zeros((3, 3), np.int32)], [[]], (8, 8), [1, 1], match="integer array")
    bad([sq], [[]], (8, 8), [1, 1], offset=(1, 2, 3), match="offset")
    bad([sq], [[]], (8, 8), [1, 1], order=[1], match="permutation")
    bad([sq, sq], None, (8, 8), [1, 1], order=[0, 0], match="permutation")
    bad([sq], [[]], (8, 8), [1, 1], _max_cols=-1, match="_max_cols")
    bad([sq * (1 << 19)], [[]], (8, 8), [4.0, 4.0], match="envelope")       # 5 * 2^19 * 4 is beyond 2^20
    bad([sq], [[]], (8, 8), [1, 1], offset=(-(1 << 21), 0), match="envelope")
    pts, off = np.zeros((4, 2), np.int32), np.array([0, 4], np.int64)
    bad((pts, off), [[]], (8, 8), [1, 1], match="holes must be None")
    bad((pts.astype(np.int64), off), None, (8, 8), [1, 1], match="traced polygon list")
    bad((pts, off.astype(np.int32)), None, (8, 8), [1, 1], match="traced polygon list")
    bad((pts, np.array([0, 3], np.int64)), None, (8, 8), [1, 1], match="offsets must rise")
    bad((pts, off, np.zeros((2, 4), np.int32)), None, (8, 8), [1, 1], match="hierarchy")
    hole_first = np.array([[-1, -1, -1, 1], [-1, -1, 0, -1]], np.int32)
    bad((pts, np.array([0, 2, 4], np.int64), hole_first), None, (8, 8), [1, 1], match="follow its contour")
    bad((torch.zeros((4, 2), dtype=torch.int32), torch.tensor([0, 4])), None, (8, 8), [1, 1], match="HIP device")   # a CPU tensor
    bad([sq], [[]], (8, 8), [1, 1], device="cpu", match="HIP device")
    assert N.calls == before
