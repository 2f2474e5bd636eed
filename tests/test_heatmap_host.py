"""CPU tests of the heat-map feature (no GPU): the numpy restatement against a canvas worked out by hand, the host pieces of
hipt_abmil_atec23_amd.heatmap (colour table, percentiles, ceil scaling, per-patch values), the argument checks, the ABI and the
drop-in hook."""
import os
import re
import sys
import types

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as R  # noqa: E402


# ---- the restatement, by hand --------------------------------------------------------------------------------------------------
def _hand_case():
    """Canvas 6 x 5 (w x h), patches 3 x 2 at scale 1: A at (0, 0) with score 40, B at (1, 1) with score 80 (overlaps A on
    pixels x 1..2 of row 1), C at (5, 4) with score 20 (clipped to the single corner pixel)."""
    scores = np.array([40.0, 80.0, 20.0])
    coords = np.array([[0, 0], [1, 1], [5, 4]])
    both = (0.4 + 0.8) / 2
    ov = np.array([[0.4, 0.4, 0.4, 0.0, 0.0, 0.0],
                   [0.4, both, both, 0.8, 0.0, 0.0],
                   [0.0, 0.8, 0.8, 0.8, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
                   [0.0, 0.0, 0.0, 0.0, 0.0, 0.2]])
    cnt = np.array([[1, 1, 1, 0, 0, 0],
                    [1, 2, 2, 1, 0, 0],
                    [0, 1, 1, 1, 0, 0],
                    [0, 0, 0, 0, 0, 0],
                    [0, 0, 0, 0, 0, 1]], dtype=np.int32)
    return scores, coords, ov, cnt


def test_restatement_against_a_hand_worked_canvas():
    import matplotlib
    scores, coords, ov, cnt = _hand_case()
    keep = scores.copy()
    got_ov, got_cnt = R.overlay(scores, coords, (3, 2), 1.0, (6, 5))
    assert np.array_equal(scores, keep)   # the caller's array is not modified
    assert got_ov.shape == (5, 6) and np.array_equal(got_ov.view(np.uint64), ov.view(np.uint64)) and np.array_equal(got_cnt, cnt)
    cmap = matplotlib.colormaps["coolwarm"]
    img = R.render(scores, coords, (3, 2), 1.0, (6, 5), alpha=1.0)
    for (y, x), c in np.ndenumerate(cnt):
        want = (np.array(cmap(ov[y, x])) * 255)[:3].astype(np.uint8) if c else np.array([255, 255, 255], dtype=np.uint8)
        assert np.array_equal(img[y, x], want), (y, x)
    # binarized at 0.5: A and C are below (they add 0 and do not paint), B is 1; the shared pixels are 1 / 2 = 0.5 -> 0 (half to even)
    bov, _ = R.overlay(scores, coords, (3, 2), 1.0, (6, 5), binarize=True, thresh=0.5)
    want = np.zeros((5, 6))
    want[1, 3] = want[2, 1:4] = 1.0
    assert np.array_equal(bov, want)
    bimg = R.render(scores, coords, (3, 2), 1.0, (6, 5), alpha=1.0, binarize=True, thresh=0.5)
    painted = np.any(bimg != 255, axis=2)
    assert painted[1, 1] and painted[1, 2] and not painted[0, 0] and not painted[1, 0]   # B paints the shared pixels, A paints nothing
    assert np.array_equal(bimg[1, 1], (np.array(cmap(0.0)) * 255)[:3].astype(np.uint8))
    # the blend: rint(255 * 0.4 + 255 * 0.6) in float32 on a bare white pixel
    blended = R.render(scores, coords, (3, 2), 1.0, (6, 5), alpha=0.4)
    a, b = np.float32(0.4), np.float32(1 - 0.4)
    assert blended[3, 0, 0] == np.uint8(np.rint(np.float32(255) * a + np.float32(255) * b))
    hole = np.ones((5, 6), dtype=bool)
    hole[1, 1] = False
    masked = R.render(scores, coords, (3, 2), 1.0, (6, 5), alpha=1.0, mask=hole)
    assert np.array_equal(masked[1, 1], [255, 255, 255]) and np.array_equal(masked[1, 2], img[1, 2])


# ---- host pieces of the package ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["coolwarm", "jet"])
def test_colour_table_against_the_colormap_itself(name):
    import matplotlib
    from hipt_abmil_atec23_amd import heatmap as H
    table = H.colour_table(name)
    assert table.shape == (258, 3) and table.dtype == np.uint8
    cmap = matplotlib.colormaps[name]
    rng = np.random.default_rng(3)
    v = np.concatenate([[0.0, 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 255 / 256, np.nextafter(255 / 256, 0.0), -0.0, -1e-300,
                         -0.25, -7.0, 1.5, 100.0, 1 / 256, np.nextafter(1 / 256, 0.0), 0.5], rng.uniform(-0.1, 1.1, 20000)])
    want = (cmap(v) * 255)[:, :3].astype(np.uint8)
    assert np.array_equal(table[H.table_index(v)], want)
    assert H.table_index(-0.25) == 256 and H.table_index(1.0) == 255 and H.table_index(1.5) == 257 and H.table_index(255 / 256) == 255


def test_unknown_colormap_and_odd_sized_colormap_are_refused():
    from matplotlib.colors import ListedColormap
    from hipt_abmil_atec23_amd import heatmap as H
    with pytest.raises(ValueError, match="not a matplotlib colormap"):
        H.colour_table("no_such_map")
    with pytest.raises(ValueError, match="256"):
        H.colour_table(ListedColormap(["r", "g", "b"]))


def test_percentiles_against_scipy_with_ties():
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(5)
    s = rng.integers(0, 40, size=333).astype(np.float64) / 7   # many ties
    s[::17] = 0.0
    assert np.array_equal(H.to_percentiles(s), R.percentiles(s))
    one = np.array([2.5])
    assert np.array_equal(H.to_percentiles(one), R.percentiles(one)) and H.to_percentiles(np.zeros(0)).shape == (0,)


def test_ceil_scaling_for_a_non_integer_scale():
    from hipt_abmil_atec23_amd import heatmap as H
    # float64 products, as numpy forms them: 7 * 0.3 = 2.0999999999999996 -> 3, 10 * 0.3 = 3.0 -> 3, 5 * 0.3 = 1.5 -> 2
    xy, pw, ph = H.scaled_geometry(np.array([[10, 7], [20, 0]]), (5, 10), 0.3)
    assert xy.tolist() == [[3, 3], [6, 0]] and (pw, ph) == (2, 3)
    # ... and where the product lands just above a whole number, ceil goes one up: 100 * 0.07 = 7.000000000000001 -> 8
    assert 100 * 0.07 > 7
    xy, pw, ph = H.scaled_geometry(np.array([[100, 30]]), (50, 256), 0.07)
    assert xy.tolist() == [[8, 3]] and (pw, ph) == (4, 18)
    # a pyramid level whose downsample is not a whole number, per axis
    xy, pw, ph = H.scaled_geometry(np.array([[4096, 8192]]), (256, 256), [1 / 32.0, 1 / 32.003])
    assert xy.tolist() == [[128, 256]] and (pw, ph) == (8, 8)
    rxy, rps = R.scaled(np.array([[100, 30]]), (50, 256), 0.07)
    assert rxy.tolist() == [[8, 3]] and rps.tolist() == [4, 18]


@pytest.mark.parametrize("binarize,thresh,pct", [(False, 0.5, False), (True, 0.5, False), (True, -1, False), (False, 0.5, True), (True, 0.3, True)])
def test_patch_values_follow_the_reference_loop(binarize, thresh, pct):
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(11)
    s = np.round(rng.uniform(-20, 120, 200), 0)
    s[::9] = 0.0
    keep = s.copy()
    v, paint = H.patch_values(s, binarize=binarize, thresh=thresh, convert_to_percentiles=pct)
    assert np.array_equal(s, keep) and v.dtype == np.float64 and paint.dtype == np.uint8
    sn, threshold = R.normalised(s, binarize, thresh, pct)
    assert threshold == H.threshold_of(len(s), binarize, thresh)
    want_v = np.array([(1.0 if binarize else x) if x >= threshold else 0.0 for x in sn])
    assert np.array_equal(v.view(np.uint64), want_v.view(np.uint64)) and np.array_equal(paint, (sn >= threshold).astype(np.uint8))


# ---- argument checks: all raise before any native call -------------------------------------------------------------------------
def test_error_paths_raise_without_a_native_call():
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords, _, _ = _hand_case()
    before = N.calls
    args = (scores, coords, (3, 2), 1.0, (6, 5))
    with pytest.raises(NotImplementedError, match="blur"):
        H.render_heatmap(*args, blur=True)
    with pytest.raises(ValueError, match="negative"):
        H.render_heatmap(scores, coords - 1, (3, 2), 1.0, (6, 5))
    with pytest.raises(ValueError, match="negative"):
        H.heatmap_overlay(scores, coords - 1, (3, 2), 1.0, (6, 5))
    with pytest.raises(ValueError, match="coords"):
        H.render_heatmap(scores, coords[:2], (3, 2), 1.0, (6, 5))
    with pytest.raises(ValueError, match="coords"):
        H.render_heatmap(scores, coords.astype(np.float64), (3, 2), 1.0, (6, 5))
    with pytest.raises(ValueError, match="scores"):
        H.render_heatmap(scores.reshape(1, 1, 3), coords, (3, 2), 1.0, (6, 5))
    with pytest.raises(ValueError, match="mask"):
        H.render_heatmap(*args, mask=np.ones((6, 5), dtype=bool))          # transposed
    with pytest.raises(ValueError, match="mask"):
        H.render_heatmap(*args, mask=np.ones((5, 6), dtype=np.uint8))      # not bool
    with pytest.raises(ValueError, match="canvas"):
        H.render_heatmap(*args, canvas=np.zeros((5, 6), dtype=np.uint8))   # no channel axis
    with pytest.raises(ValueError, match="canvas"):
        H.render_heatmap(*args, canvas=np.zeros((5, 6, 3), dtype=np.float32))
    with pytest.raises(ValueError, match="region_size"):
        H.render_heatmap(scores, coords, (3, 2), 1.0, (0, 5))
    with pytest.raises(ValueError, match="scale"):
        H.render_heatmap(scores, coords, (3, 2), 0.0, (6, 5))
    with pytest.raises(ValueError, match="NaN"):
        H.render_heatmap(np.array([1.0, np.nan, 2.0]), coords, (3, 2), 1.0, (6, 5))
    with pytest.raises(ValueError, match="alpha"):
        H.render_heatmap(*args, alpha=float("nan"))
    with pytest.raises(ValueError, match="colormap"):
        H.render_heatmap(*args, cmap="no_such_map")
    with pytest.raises(NotImplementedError, match="blur"):
        H.vis_heatmap(object(), scores, coords, blur=True)
    assert N.calls == before


def test_cpu_only_call_raises():
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords, _, _ = _hand_case()
    with pytest.raises(RuntimeError, match="HIP device"):
        H.render_heatmap(scores, coords, (3, 2), 1.0, (6, 5), device="cpu")
    with pytest.raises(RuntimeError, match="HIP device"):
        H.heatmap_overlay(torch.from_numpy(scores), torch.from_numpy(coords), (3, 2), 1.0, (6, 5))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            H.render_heatmap(scores, coords, (3, 2), 1.0, (6, 5))


# ---- ABI -----------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_symbols():
    import ctypes as C
    from hipt_abmil_atec23_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"#define\s+HIPT_ABI_VERSION\s+6\b", hdr) and N.ABI_VERSION == 6
    for name, restype in (("hipt_heatmap_workspace_bytes", "size_t"), ("hipt_heatmap_overlay", "int"), ("hipt_heatmap_render", "int")):
        decl = re.search(rf"\b{restype}\s+{name}\s*\(([^)]*)\)", hdr)
        assert decl, name
        res, args = N.SIGNATURES[name]
        assert res is (C.c_size_t if restype == "size_t" else C.c_int)
        assert len(args) == len(decl.group(1).split(",")), name
    for macro, val in (("HIPT_HEATMAP_TILE_W", N.HEATMAP_TILE_W), ("HIPT_HEATMAP_TILE_H", N.HEATMAP_TILE_H),
                       ("HIPT_HEATMAP_LUT_ENTRIES", N.HEATMAP_LUT_ENTRIES)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", hdr).group(1)) == val
    assert f"#define HIPT_HEATMAP_MAX_DIM (1 << {N.HEATMAP_MAX_DIM.bit_length() - 1})" in hdr
    lib = N.lib()
    assert all(hasattr(lib, n) for n in ("hipt_heatmap_workspace_bytes", "hipt_heatmap_overlay", "hipt_heatmap_render"))


def test_workspace_size_follows_the_tile_bound():
    """A patch touches at most (ceil(pw / TW) + 1) * (ceil(ph / TH) + 1) tiles, and never more tiles than the canvas has: the
    workspace is three int32 per tile, one per 1024 tiles and one per list entry, each array rounded up to 256 bytes."""
    from hipt_abmil_atec23_amd import _native as N
    lib = N.lib()
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731

    def want(n, pw, ph, w, h):
        ntx, nty = -(-w // N.HEATMAP_TILE_W), -(-h // N.HEATMAP_TILE_H)
        per = min(-(-pw // N.HEATMAP_TILE_W) + 1, ntx) * min(-(-ph // N.HEATMAP_TILE_H) + 1, nty)
        nt = ntx * nty
        return 3 * al(nt * 4) + al(-(-nt // 1024) * 4) + al(n * per * 4)

    for shape in ((600, 5, 3, 67, 45), (100000, 64, 64, 10176, 10176), (1, 1, 1, 1, 1), (750, 7, 5, 40, 40), (20000, 8, 8, 1500, 1100)):
        assert lib.hipt_heatmap_workspace_bytes(*shape) == want(*shape), shape
    assert lib.hipt_heatmap_workspace_bytes(0, 8, 8, 100, 100) == 0
    assert lib.hipt_heatmap_workspace_bytes(5, 0, 8, 100, 100) == 0 and lib.hipt_heatmap_workspace_bytes(5, 8, 8, (1 << 20) + 1, 4) == 0
    assert lib.hipt_heatmap_workspace_bytes(1 << 30, 64, 64, 4096, 4096) == 0   # 2^30 patches x 15 tiles: beyond 2^31 entries


def test_native_calls_refuse_bad_arguments_on_the_host():
    """The C entry points check their arguments before anything is enqueued, so they can be exercised without a device."""
    import ctypes as C
    from hipt_abmil_atec23_amd import _native as N
    lib = N.lib()
    null = C.c_void_p(0)
    assert lib.hipt_heatmap_overlay(null, null, null, 0, 8, 8, 16, 16, 0, null, null, null, null, 0, null) == -1        # no output
    assert lib.hipt_heatmap_render(null, null, null, 0, 8, 8, 16, 16, 0, null, null, null, 0.4, null, null, null, 0, null) == -1   # no image
    one = C.c_void_p(256)
    assert lib.hipt_heatmap_render(one, one, null, 4, 8, 8, 16, 16, 0, null, null, one, 0.4, one, null, null, 0, null) == -2   # no workspace
    assert b"workspace" in lib.hipt_last_error()
    assert lib.hipt_heatmap_render(one, one, null, 4, 8, 8, 1 << 21, 16, 0, null, null, one, 0.4, one, null, one, 1 << 20, null) == -4
    assert b"nothing was launched" in lib.hipt_last_error()


def test_makefile_builds_heatmap_without_contraction():
    src = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bheatmap\.hip\b", src, re.M) and "FLAGS_heatmap.hip = -ffp-contract=off" in src


def test_package_exports_lazily():
    import hipt_abmil_atec23_amd as amd
    from hipt_abmil_atec23_amd import heatmap as H
    assert amd.render_heatmap is H.render_heatmap and amd.heatmap_overlay is H.heatmap_overlay and amd.vis_heatmap is H.vis_heatmap


# ---- drop-in hook --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fake_wsi_core(monkeypatch):
    """A stand-in for the reference's wsi_core.WholeSlideImage module (the real one needs openslide and cv2)."""
    pkg = types.ModuleType("wsi_core")
    pkg.__path__ = []
    mod = types.ModuleType("wsi_core.WholeSlideImage")

    class WholeSlideImage:
        def visHeatmap(self, scores, coords, **kw):
            return "reference"

    mod.WholeSlideImage = WholeSlideImage
    pkg.WholeSlideImage = mod
    monkeypatch.setitem(sys.modules, "wsi_core", pkg)
    monkeypatch.setitem(sys.modules, "wsi_core.WholeSlideImage", mod)
    return WholeSlideImage


def test_install_binds_vis_heatmap_only_when_asked(fake_wsi_core):
    from hipt_abmil_atec23_amd import dropin
    from hipt_abmil_atec23_amd import heatmap as H
    original = fake_wsi_core.__dict__["visHeatmap"]
    try:
        done = dropin.install()
        assert fake_wsi_core.__dict__["visHeatmap"] is original and not any("visHeatmap" in k for k in done)
        done = dropin.install(heatmaps=True)
        assert fake_wsi_core.__dict__["visHeatmap"] is H.vis_heatmap
        assert done["wsi_core.WholeSlideImage.WholeSlideImage.visHeatmap"].endswith("heatmap.vis_heatmap")
        dropin.install(heatmaps=True)   # twice: the saved original is not overwritten
    finally:
        dropin.uninstall()
    assert fake_wsi_core.__dict__["visHeatmap"] is original


def test_install_heatmaps_is_a_no_op_without_the_reference(monkeypatch):
    from hipt_abmil_atec23_amd import dropin
    monkeypatch.delitem(sys.modules, "wsi_core.WholeSlideImage", raising=False)
    monkeypatch.delitem(sys.modules, "wsi_core", raising=False)
    try:
        done = dropin.install(heatmaps=True)
        assert not any("visHeatmap" in k for k in done) and "wsi_core.WholeSlideImage" not in sys.modules
    finally:
        dropin.uninstall()
