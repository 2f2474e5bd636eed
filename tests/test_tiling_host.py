"""CPU tests of the tiling route: the oracle (tests/tiling_ref.py) against the goldens recorded from the reference's
own code and against an independent point-in-polygon (matplotlib's, plus an explicit on-segment test); the two C entry points
declared, exported and bound; the argument checks, which raise before any native call; the drop-in hook."""
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tiling_ref as TR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import tiling as T  # noqa: E402

GOLDENS = sorted(f[len("tiling_"):-len(".npz")] for f in os.listdir(GOLDEN) if f.startswith("tiling_") and f.endswith(".npz"))


def load_golden(name):
    g = np.load(os.path.join(GOLDEN, f"tiling_{name}.npz"))
    off = g["hole_off"]
    holes = [g["hole_verts"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    kw = dict(patch_size=int(g["patch_size"]), step_size=int(g["step_size"]), contour_fn=str(g["contour_fn"]),
              use_padding=bool(g["use_padding"]), center_shift=float(g["center_shift"]))
    if bool(g["has_roi"]):
        kw.update(top_left=tuple(int(v) for v in g["top_left"]), bot_right=tuple(int(v) for v in g["bot_right"]))
    return g["cont"], holes, tuple(int(v) for v in g["level_dim0"]), tuple(float(v) for v in g["downsample"]), kw, g["coords"]


def test_the_goldens_cover_the_glue():
    assert len(GOLDENS) >= 10
    fns = {str(np.load(os.path.join(GOLDEN, f"tiling_{n}.npz"))["contour_fn"]) for n in GOLDENS}
    assert fns == {"basic", "center", "four_pt", "four_pt_hard", "four_pt_easy"}
    assert any(len(load_golden(n)[5]) == 0 for n in GOLDENS) and max(len(load_golden(n)[5]) for n in GOLDENS) > 500


@pytest.mark.parametrize("name", GOLDENS)
def test_oracle_reproduces_the_reference_code(name):
    cont, holes, dim0, ds, kw, want = load_golden(name)
    got = TR.process_contour(cont, holes, dim0, ds, **kw)
    assert got.dtype == np.int64 == want.dtype and got.shape == want.shape and np.array_equal(got, want)


def on_segment(p2, a2, b2):
    """p on the closed segment a-b (all doubled, Python integers): collinear and within the box."""
    (px, py), (ax, ay), (bx, by) = p2, a2, b2
    return (py - ay) * (bx - ax) == (px - ax) * (by - ay) and min(ax, bx) <= px <= max(ax, bx) and min(ay, by) <= py <= max(ay, by)


@pytest.mark.parametrize("shape", sorted(TR.SHAPES))
def test_oracle_against_an_independent_point_in_polygon(shape):
    from matplotlib.path import Path
    poly = TR.SHAPES[shape]
    p2 = TR.lattice2(poly)   # every integer and half-integer point of the box and a margin
    got = TR.ppt_doubled(poly, p2)
    a2 = [(int(2 * x), int(2 * y)) for x, y in poly]
    edges = list(zip(a2, a2[1:] + a2[:1]))
    boundary = np.array([any(on_segment((int(x), int(y)), a, b) for a, b in edges) for x, y in p2])
    assert np.array_equal(got == 0, boundary)
    assert boundary.sum() >= len(poly) and (~boundary).sum() > len(poly)
    inside = Path(np.concatenate([poly, poly[:1]]).astype(np.float64), closed=True).contains_points(p2[~boundary] / 2.0)
    assert np.array_equal(got[~boundary] > 0, inside)   # every off-boundary point, none skipped
    assert inside.any() and not inside.all()


def test_degenerate_polygons_have_no_interior():
    p2 = TR.double_points([[1, 1], [2, 2], [3, 3], [1.5, 1.5], [2, 1], [0, 0]])
    assert list(TR.ppt_doubled(np.array([[1, 1]]), p2)) == [0, -1, -1, -1, -1, -1]
    assert list(TR.ppt_doubled(np.array([[1, 1], [3, 3]]), p2)) == [0, 0, 0, 0, -1, -1]
    assert list(TR.ppt_doubled(np.zeros((0, 2), int), p2)) == [-1] * 6


def test_entry_points_are_declared_exported_and_bound_under_abi_6():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"\bint hipt_point_polygon_test\(const int32_t\* verts, int V, const int32_t\* poly_off, int P,", hdr)
    assert re.search(r"\bint hipt_tile_contours\(const int32_t\* verts, int V, const int32_t\* poly_off, int P,", hdr)
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6
    for name, value in (("COORD_BOUND", N.TILING_COORD_BOUND), ("EDGE_CHUNK", N.TILING_EDGE_CHUNK), ("TILE", N.TILING_TILE),
                        ("CONTOUR_INTS", N.TILING_CONTOUR_INTS)):
        assert f"#define HIPT_TILING_{name} {value}\n" in hdr
    assert "enum { HIPT_TILE_BASIC = 0, HIPT_TILE_CENTER = 1, HIPT_TILE_FOUR_PT = 2, HIPT_TILE_FOUR_PT_HARD = 3 };" in hdr
    assert (N.TILE_BASIC, N.TILE_CENTER, N.TILE_FOUR_PT, N.TILE_FOUR_PT_HARD) == (0, 1, 2, 3)
    for name in ("hipt_point_polygon_test", "hipt_tile_contours"):
        decl = re.search(r"int %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(N.SIGNATURES[name][1]) == len(decl.split(","))
        assert hasattr(N.lib(), name)
    assert N.lib().hipt_abi_version() == 6
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert " tiling.hip " in mk and re.search(r"^SRCS\s*=.*\btiling\.hip capi\.hip$", mk, re.M)
    src = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "tiling.hip")).read()
    assert not re.search(r"\b(float|double)\b", re.sub(r"//[^\n]*", "", src))   # integer geometry: no floating point in the file
    import hipt_abmil_atec23_amd as amd
    for name in ("point_polygon_test", "process_contour", "process_contours", "process_contours_like", "pack_slide", "plan_contours"):
        assert getattr(amd, name) is getattr(T, name)


BADARG, UNSUPPORTED = -1, -4


def test_c_argument_checks_return_their_codes_without_a_device():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    v, o, p, i, out = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000
    assert lib.hipt_point_polygon_test(v, 4, o, 1, p, i, 0, out, None) == 0        # no points: nothing to do
    assert lib.hipt_point_polygon_test(v, -1, o, 1, p, i, 5, out, None) == BADARG
    assert lib.hipt_point_polygon_test(v, 4, None, 1, p, i, 5, out, None) == BADARG
    assert lib.hipt_point_polygon_test(v, 4, o, 1, p, i, 5, None, None) == BADARG
    assert lib.hipt_point_polygon_test(v + 2, 4, o, 1, p, i, 5, out, None) == BADARG and b"alignment" in lib.hipt_last_error()

    def tile(mode=2, ps=256, shift=64, U=3, keep=out, keep_len=100, units=i, desc=p, C=1):
        return lib.hipt_tile_contours(v, 4, o, 1, desc, C, units, U, mode, ps, shift, keep, keep_len, None)
    assert tile(U=0) == 0
    assert tile(mode=4) == BADARG and b"mode 4" in lib.hipt_last_error() and tile(mode=-1) == BADARG
    assert tile(ps=0) == UNSUPPORTED and tile(ps=1 << 28) == UNSUPPORTED and tile(shift=-1) == UNSUPPORTED and tile(shift=1 << 28) == UNSUPPORTED
    assert b"nothing was launched" in lib.hipt_last_error()
    assert tile(keep=None) == BADARG and tile(units=None) == BADARG and tile(desc=None) == BADARG
    assert tile(U=-1) == BADARG and tile(keep_len=-1) == BADARG and tile(C=-1) == BADARG
    assert tile(units=i + 1) == BADARG


def test_python_layer_refuses_bad_requests_before_any_native_call(monkeypatch):
    def no_call(*a, **k):
        raise AssertionError("a native call was made")
    monkeypatch.setattr(N, "call", no_call)
    sq = np.array([[0, 0], [400, 0], [400, 400], [0, 400]], dtype=np.int32)
    args = (sq, [], (1000, 1000), (1.0, 1.0))
    big = 1 << 29
    with pytest.raises(ValueError, match=r"outside \+-2\^30"):          # a vertex whose double leaves the range
        T.process_contour(np.array([[0, 0], [big, 0], [big, 8]]), [], (big, big), (1.0, 1.0))
    with pytest.raises(ValueError, match=r"outside \+-2\^30"):          # the vertices fit, the shifted test point does not
        T.process_contour(np.array([[big - 300, 0], [big - 1, 0], [big - 1, 8]]), [], (big, big), (1.0, 1.0))
    with pytest.raises(ValueError, match=r"outside \+-2\^30"):
        T.point_polygon_test(sq, np.array([[big, 0]]))
    with pytest.raises(ValueError, match="none of"):
        T.process_contour(*args, contour_fn="four_point")

    class isInContourV3_Easy:   # what datasets/wsi_dataset.py hands over
        def __call__(self, pt):
            return 1
    with pytest.raises(TypeError, match="'basic', 'center', 'four_pt'.*'four_pt_hard'"):
        T.process_contour(*args, contour_fn=isInContourV3_Easy())
    with pytest.raises(ValueError, match="multiples of 0.5"):
        T.point_polygon_test(sq, np.array([[1.25, 2.0]]))
    with pytest.raises(ValueError, match="multiples of 0.5"):
        T.point_polygon_test(sq, np.array([[float("nan"), 2.0]]))
    with pytest.raises(ValueError, match="poly_id"):
        T.point_polygon_test([sq, sq], np.array([[1, 2]]))
    with pytest.raises(ValueError, match="poly_id outside"):
        T.point_polygon_test([sq, sq], np.array([[1, 2]]), poly_id=np.array([2]))
    with pytest.raises(ValueError, match="2 contours but 1 lists of holes"):
        T.process_contours([sq, sq], [[]], (1000, 1000), (1.0, 1.0))
    with pytest.raises(ValueError, match="integers"):
        T.process_contour(sq.astype(np.float32), [], (1000, 1000), (1.0, 1.0))
    with pytest.raises(ValueError, match="is None"):
        T.process_contour(None, [], (1000, 1000), (1.0, 1.0), patch_level_dim=(1000, 1000))
    with pytest.raises(ValueError, match=">= 1"):
        T.process_contour(*args, step_size=0)
    with pytest.raises(ValueError, match=">= 1"):
        T.process_contour(sq, [], (1000, 1000), (0.5, 0.5))
    with pytest.raises(ValueError, match="must be an integer"):
        T.process_contour(*args, top_left=(0.5, 0), bot_right=(10, 10))
    # and a good request gets as far as the question for a device: there is no CPU execution path
    with pytest.raises(RuntimeError, match="HIP device"):
        T.process_contour(*args, device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        T.point_polygon_test(sq, np.array([[1.5, 2.0]]), device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        T.pack_slide([sq], [[]], device="cpu")


def test_plan_restates_the_reference_grid():
    """The grid arithmetic of plan_contours is host code: its candidate lattice is np.arange / meshgrid of the oracle's glue."""
    for name in GOLDENS:
        cont, holes, dim0, ds, kw, _ = load_golden(name)
        mode, img, ref_ps, step, ps0, shift = T._settings(dim0, ds, kw["patch_size"], kw["step_size"], kw["contour_fn"], kw["center_shift"])
        g = T._grid(TR.boundingRect(cont), img, ref_ps, step, kw["use_padding"], kw.get("top_left"), kw.get("bot_right"))
        if g is None:
            assert name == "blob_roi_miss"
            continue
        sx, sy, nx, ny = g
        box = TR.boundingRect(cont)
        stop = [box[0] + box[2], box[1] + box[3]]
        if not kw["use_padding"]:
            stop = [min(stop[0], dim0[0] - ref_ps[0] + 1), min(stop[1], dim0[1] - ref_ps[1] + 1)]
        if "bot_right" in kw:
            stop = [min(stop[0], kw["bot_right"][0]), min(stop[1], kw["bot_right"][1])]
        assert nx == len(np.arange(sx, stop[0], step[0])) and ny == len(np.arange(sy, stop[1], step[1]))
        assert shift == (int(ps0 // 2 * (0.5 if kw["contour_fn"] == "four_pt_easy" else kw["center_shift"]))
                         if kw["contour_fn"].startswith("four_pt") else 0)


def test_dropin_hook_binds_where_the_reference_module_imports(monkeypatch):
    from hipt_abmil_atec23_amd import dropin
    key = "wsi_core.WholeSlideImage.WholeSlideImage.process_contour"
    monkeypatch.delitem(sys.modules, "wsi_core.WholeSlideImage", raising=False)
    monkeypatch.delitem(sys.modules, "wsi_core", raising=False)
    assert key not in dropin.install(tiling=True)   # no such module here
    dropin.uninstall()
    pkg, mod = types.ModuleType("wsi_core"), types.ModuleType("wsi_core.WholeSlideImage")
    pkg.__path__ = []

    class WholeSlideImage:
        def process_contour(self, cont, contour_holes, patch_level, save_path, patch_size=256, step_size=256, contour_fn="four_pt",
                            use_padding=True, top_left=None, bot_right=None):
            return "theirs"
    theirs = WholeSlideImage.__dict__["process_contour"]
    mod.WholeSlideImage = WholeSlideImage
    monkeypatch.setitem(sys.modules, "wsi_core", pkg)
    monkeypatch.setitem(sys.modules, "wsi_core.WholeSlideImage", mod)
    assert key not in dropin.install()              # opt-in
    assert WholeSlideImage.__dict__["process_contour"] is theirs
    done = dropin.install(tiling=True)
    assert done[key].endswith("tiling.process_contour_like")
    assert WholeSlideImage.__dict__["process_contour"] is T.process_contour_like
    import inspect
    assert list(inspect.signature(T.process_contour_like).parameters) == list(inspect.signature(theirs).parameters)
    assert list(inspect.signature(dropin.install).parameters)[-2:] == ["hier_heatmaps", "tiling"]
    dropin.uninstall()
    assert WholeSlideImage.__dict__["process_contour"] is theirs
