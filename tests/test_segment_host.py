"""CPU tests of the device tissue segmentation: the numpy restatement (tests/segment_ref.py) against scipy's filters
and hand-computed values; the Otsu fixtures' margin; the host glue (contour_area, filter_contours, segment_tissue with a stub
tracer); the six C entry points declared, exported and bound; the refusals, which return before anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_ref as SR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import segment as SG  # noqa: E402

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def planes():
    rng = np.random.default_rng(5)
    yield rng.integers(0, 256, (23, 31), dtype=np.uint8)
    yield (rng.integers(0, 2, (9, 40), dtype=np.uint8) * 255)
    yield rng.integers(0, 256, (1, 17), dtype=np.uint8)
    yield rng.integers(0, 256, (17, 1), dtype=np.uint8)


@pytest.mark.parametrize("k", [1, 3, 5, 7, 11, 15])
def test_median_is_scipys_median_filter(k):
    from scipy import ndimage
    for x in planes():
        assert np.array_equal(SR.median(x, k), ndimage.median_filter(x, size=k, mode="nearest")), (k, x.shape)


@pytest.mark.parametrize("c", [1, 2, 3, 4, 5, 8, 50, 100])
def test_dilation_and_erosion_are_scipys_filters_with_the_stated_window(c):
    """scipy's window of size c with origin o reads offsets -(c // 2) - o .. c - 1 - c // 2 - o: o = 0 is the window stated"""
    from scipy import ndimage
    for x in planes():
        d = ndimage.maximum_filter(x, size=(c, c), mode="constant", cval=0, origin=0)
        e = ndimage.minimum_filter(x, size=(c, c), mode="constant", cval=255, origin=0)
        assert np.array_equal(SR.dilate(x, c), d), (c, x.shape)
        assert np.array_equal(SR.erode(x, c), e), (c, x.shape)
        assert np.array_equal(SR.close(x, c), ndimage.minimum_filter(d, size=(c, c), mode="constant", cval=255, origin=0))
    # the window by hand: one bright pixel spreads to offsets -(c // 2) .. c - 1 - c // 2 of the OUTPUT that read it, mirrored
    x = np.zeros((1, 9), dtype=np.uint8)
    x[0, 4] = 200
    assert list(np.flatnonzero(SR.dilate(x, 2)[0])) == [4, 5]       # output x reads x - 1 .. x
    assert list(np.flatnonzero(SR.dilate(x, 4)[0])) == [3, 4, 5, 6]   # output x reads x - 2 .. x + 1
    assert np.array_equal(SR.close(x, 0), x)


def test_saturation_spot_values():
    def s(r, g, b):
        return int(SR.saturation(np.array([[[r, g, b]]], dtype=np.uint8))[0, 0])
    assert s(90, 90, 90) == 0 and s(255, 255, 255) == 0 and s(0, 0, 0) == 0
    assert s(255, 0, 0) == 255 and s(0, 7, 0) == 255 and s(1, 0, 1) == 255
    assert s(200, 100, 50) == 191    # 150 * rint(1044480 / 200 = 5222.4) = 783300; + 2048 >> 12 = 191
    assert s(176, 92, 158) == 122    # 84 * rint(5934.545...) = 84 * 5935 = 498540; + 2048 >> 12 = 122
    assert s(10, 20, 30) == 170      # 20 * 34816 = 696320; + 2048 >> 12 = 170
    assert s(238, 236, 240) == 4     # 4 * 4352 = 17408; + 2048 >> 12 = 4
    t = SR.sdiv_table()
    assert t[0] == 0 and t[1] == 1044480 and t[255] == 4096 and t[200] == 5222
    # half to even in integers is the same table (what the kernel computes)
    n = 255 << 12
    for v in range(1, 256):
        q, r = divmod(n, v)
        assert t[v] == (q + 1 if 2 * r > v else q + (q & 1) if 2 * r == v else q), v
    rgba = np.random.default_rng(3).integers(0, 256, (5, 6, 4), dtype=np.uint8)
    assert np.array_equal(SR.saturation(rgba), SR.saturation(rgba[:, :, :3]))


def test_otsu_two_spikes_constant_and_the_fixtures_margin():
    h = np.zeros(256, dtype=np.int64)
    h[40], h[180] = 700, 300
    assert SR.otsu(h) == 40
    h = np.zeros(256, dtype=np.int64)
    h[77] = 1000
    assert SR.otsu(h) == 0   # every level is skipped: the mask is src > 0
    assert np.array_equal(SR.tissue_mask(np.full((4, 4, 3), 9, dtype=np.uint8), mthresh=1, use_otsu=True)[0], np.zeros((4, 4), np.uint8))
    # every Otsu fixture of the GPU tests: the two largest DISTINCT sigmas are more than 1e-9 (relative) apart
    fixtures = [SR.tissue_mask(SR.case_image(s), mthresh=m, use_otsu=True)[1] for s in SR.SHAPES for (m, c, o) in SR.SETTINGS if o]
    fixtures += [SR.median(SR.saturation(SR.make_image(600, 700, 3, seed=77)), 7), SR.saturation(SR.make_image(130, 257, 3, seed=9)),
                 SR.median(SR.saturation(SR.make_image(96, 160, 4, seed=21)), 5), SR.median(SR.saturation(SR.make_image(96, 160, 4, seed=22)), 5)]
    for x in fixtures:
        s = SR.otsu_sigmas(SR.histogram(x))
        s = np.unique(s[~np.isnan(s)])
        if len(s) >= 2:
            assert (s[-1] - s[-2]) > 1e-9 * s[-1], x.shape


def square(x0, y0, side):
    """a closed square contour in cv2's shape [n, 1, 2], corners only"""
    return np.array([[[x0, y0]], [[x0 + side, y0]], [[x0 + side, y0 + side]], [[x0, y0 + side]]], dtype=np.int32)


def test_contour_area_is_the_shoelace_formula():
    assert SG.contour_area(square(3, 4, 10)) == 100.0
    assert SG.contour_area(square(3, 4, 10)[::-1]) == 100.0   # orientation does not matter
    assert SG.contour_area(np.array([[0, 0], [4, 0], [0, 3]])) == 6.0
    assert SG.contour_area(np.zeros((0, 1, 2), dtype=np.int32)) == 0.0 and SG.contour_area(square(1, 1, 0)) == 0.0
    assert SG.contour_area(np.array([[[0, 0]], [[5, 0]]])) == 0.0


def test_filter_contours_on_nested_squares():
    contours = [square(0, 0, 100),      # 0: area 10000, holes 1, 2, 3, 4
                square(10, 10, 10),     # 1: hole 100
                square(30, 10, 20),     # 2: hole 400
                square(60, 10, 10),     # 3: hole 100 (ties with 1: input order stays)
                square(10, 60, 3),      # 4: hole 9
                square(200, 0, 5),      # 5: area 25: dropped by a_t
                square(300, 0, 20),     # 6: area 400, its hole 7 eats all of it
                square(300, 0, 20),     # 7
                square(400, 0, 30)]     # 8: area 900 == a_t is NOT strictly above it
    parent = [-1, 0, 0, 0, 0, -1, -1, 6, -1]
    hierarchy = np.array([[-1, p] for p in parent])
    fg, holes = SG.filter_contours(contours, hierarchy, {"a_t": 900, "a_h": 50, "max_n_holes": 3})
    assert len(fg) == 1 and fg[0] is contours[0]
    assert len(holes) == 1 and [id(h) for h in holes[0]] == [id(contours[2]), id(contours[1]), id(contours[3])]
    fg, holes = SG.filter_contours(contours, hierarchy, {"a_t": 899, "a_h": 100, "max_n_holes": 8})
    assert [id(c) for c in fg] == [id(contours[0]), id(contours[8])]
    assert [id(h) for h in holes[0]] == [id(contours[2])] and holes[1] == []   # a_h is strict; 9 and the 100s go
    fg, holes = SG.filter_contours(contours, hierarchy, {"a_t": 0, "a_h": 0, "max_n_holes": 2})
    assert [id(c) for c in fg] == [id(contours[0]), id(contours[5]), id(contours[8])]   # 6: a == 0 is skipped
    assert [id(h) for h in holes[0]] == [id(contours[2]), id(contours[1])]             # truncated to the two largest
    assert SG.filter_contours([], np.zeros((0, 2)), {"a_t": 1}) == ([], [])


class FakeSlide:
    class _Wsi:
        def __init__(self, img):
            self.img, self.asked = img, None

        def read_region(self, origin, level, size):
            self.asked = (origin, level, size)
            return self.img

    def __init__(self, img):
        self.wsi = self._Wsi(img)
        self.level_dim = [(4 * img.shape[1], 4 * img.shape[0]), (img.shape[1], img.shape[0])]
        self.level_downsamples = [(1.0, 1.0), (4.0, 4.0)]


def test_segment_tissue_with_a_stub_tracer(monkeypatch):
    import torch
    img = SR.make_image(40, 50, 4, seed=3)
    seen = {}

    def fake_mask(im, sthresh, sthresh_up, mthresh, close, use_otsu):
        seen["args"] = (sthresh, sthresh_up, mthresh, close, use_otsu)
        return torch.from_numpy(SR.tissue_mask(im, sthresh, sthresh_up, mthresh, close, use_otsu)[0])
    monkeypatch.setattr(SG, "tissue_mask", fake_mask)
    contours = [square(0, 0, 70), square(5, 5, 20), square(100, 3, 65), square(200, 0, 80), square(210, 10, 7)]
    hierarchy = np.array([[[1, -1, 1, -1], [-1, -1, -1, 0], [3, 0, -1, -1], [-1, 2, 4, -1], [-1, -1, -1, 3]]])

    def tracer(mask):
        seen["mask"] = mask
        return contours, hierarchy
    slide = FakeSlide(img)
    # the scaled thresholds: int(32 ** 2 / (4 * 4)) = 64, so a_t = 64 * 64 = 4096 and a_h = 1 * 64 = 64
    SG.segment_tissue(slide, seg_level=1, sthresh=8, sthresh_up=200, mthresh=5, close=4, use_otsu=False,
                      filter_params={"a_t": 64, "a_h": 1, "max_n_holes": 8}, ref_patch_size=32, find_contours=tracer)
    assert slide.wsi.asked == ((0, 0), 1, (50, 40)) and seen["args"] == (8, 200, 5, 4, False)
    assert seen["mask"].dtype == np.uint8 and np.array_equal(seen["mask"], SR.tissue_mask(img, 8, 200, 5, 4, False)[0])
    # areas: 4900 - 400 = 4500 > 4096 stays; 4225 > 4096 stays; 6400 - 49 stays; hole 400 > 64 stays, hole 49 goes
    assert len(slide.contours_tissue) == 3 and [len(h) for h in slide.holes_tissue] == [1, 0, 0]
    assert all(c.dtype == np.int32 for c in slide.contours_tissue) and slide.holes_tissue[0][0].dtype == np.int32
    assert np.array_equal(slide.contours_tissue[1], contours[2] * 4) and np.array_equal(slide.holes_tissue[0][0], contours[1] * 4)
    # a fractional scale truncates like astype('int32')
    slide.level_downsamples[1] = (4.5, 4.0)
    SG.segment_tissue(slide, seg_level=1, filter_params={"a_t": 1, "a_h": 0, "max_n_holes": 8}, ref_patch_size=32, find_contours=tracer,
                      keep_ids=[0, 2], exclude_ids=[2])
    assert len(slide.contours_tissue) == 1 and np.array_equal(slide.contours_tissue[0], (contours[0] * (4.5, 4.0)).astype("int32"))
    assert slide.contours_tissue[0][1, 0, 0] == 315 and int(32 ** 2 / (4.5 * 4.0)) == 56
    SG.segment_tissue(slide, seg_level=1, filter_params={"a_t": 1, "a_h": 0, "max_n_holes": 8}, ref_patch_size=32, find_contours=tracer,
                      exclude_ids=[1])
    assert len(slide.contours_tissue) == 2 and np.array_equal(slide.contours_tissue[1], (contours[3] * (4.5, 4.0)).astype("int32"))
    # no tracer and no cv2: an ImportError that names the parameter
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError, match="find_contours="):
        SG.segment_tissue(slide, seg_level=1)


def test_entry_points_are_declared_exported_and_bound_under_abi_6():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    want = {"hipt_segment_workspace_bytes": ["h", "w", "close"],
            "hipt_segment_mask": ["src", "h", "w", "channels", "sthresh", "sthresh_up", "mthresh", "close", "use_otsu", "mask", "sat", "med",
                                  "thresh", "ws", "ws_bytes", "stream"],
            "hipt_segment_saturation": ["src", "h", "w", "channels", "sat", "stream"],
            "hipt_segment_median": ["src", "h", "w", "ksize", "dst", "stream"],
            "hipt_segment_otsu": ["src", "h", "w", "hist", "thresh", "stream"],
            "hipt_segment_close": ["src", "h", "w", "close", "dst", "ws", "ws_bytes", "stream"]}
    lib = N.lib()
    for name, args in want.items():
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, hdr, re.S | re.M).group(1)
        assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == args, name
        assert len(N.SIGNATURES[name][1]) == len(args) and hasattr(lib, name), name
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6 and lib.hipt_abi_version() == 6
    assert f"#define HIPT_SEGMENT_MAX_MEDIAN {N.SEGMENT_MAX_MEDIAN}\n" in hdr and f"#define HIPT_SEGMENT_MAX_CLOSE {N.SEGMENT_MAX_CLOSE}\n" in hdr
    assert "global: hipt_*;" in open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "hipt_abmil.map")).read()
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bsegment\.hip\b", mk, re.M) and "FLAGS_segment.hip = -ffp-contract=off" in mk
    import hipt_abmil_atec23_amd as amd
    for name in ("tissue_mask", "segment_tissue", "saturation_u8", "median_blur_u8", "otsu_threshold", "morph_close_u8", "contour_area",
                 "filter_contours"):
        assert getattr(amd, name) is getattr(SG, name)


def al256(v):
    return (v + 255) & ~255


def test_workspace_bytes_is_the_carve():
    lib = N.lib()
    for h, w in [(4096, 4096), (37, 53), (1, 1), (130, 257)]:
        base = al256(1024) + al256(4) + al256(h * w)   # histogram, threshold, median plane
        assert lib.hipt_segment_workspace_bytes(h, w, 0) == base
        for c in (1, 4, 100, 128):
            assert lib.hipt_segment_workspace_bytes(h, w, c) == base + 2 * al256(h * w)
    for h, w, c in [(0, 8, 0), (8, 0, 0), (-1, 8, 0), (1 << 16, 1 << 15, 0), (8, 8, -1), (8, 8, 129)]:
        assert lib.hipt_segment_workspace_bytes(h, w, c) == 0
    assert lib.hipt_segment_workspace_bytes(46340, 46340, 0) > 0   # h w just below 2^31


def test_library_refuses_without_launching():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    src, mask, sat, med, thr, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x70000

    def call(hw=(64, 64), ch=3, st=20, up=255, m=7, c=4, otsu=0, src=src, mask=mask, sat=sat, med=med, thr=thr, ws=ws, ws_bytes=1 << 30):
        return lib.hipt_segment_mask(src, hw[0], hw[1], ch, st, up, m, c, otsu, mask, sat, med, thr, ws, ws_bytes, None)
    assert call(src=None) == BADARG and call(mask=None) == BADARG and call(mask=src) == BADARG and call(mask=sat) == BADARG
    assert call(sat=med) == BADARG and call(thr=thr + 2) == BADARG
    assert call(hw=(0, 64)) == BADARG and call(hw=(64, -3)) == BADARG and call(hw=(1 << 16, 1 << 15)) == BADARG
    assert call(ch=1) == BADARG and call(ch=5) == BADARG and b"channels" in lib.hipt_last_error()
    assert call(st=-1) == BADARG and call(st=256) == BADARG and call(up=256) == BADARG and call(up=-1) == BADARG
    assert call(m=0) == BADARG and call(c=-1) == BADARG
    assert call(m=4) == UNSUPPORTED and call(m=17) == UNSUPPORTED and b"17" in lib.hipt_last_error()
    assert call(c=129) == UNSUPPORTED and b"129" in lib.hipt_last_error()
    need = lib.hipt_segment_workspace_bytes(64, 64, 4)
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws=ws + 16, ws_bytes=need) == WORKSPACE and call(ws=None, ws_bytes=0) == WORKSPACE
    assert call(ws=None, ws_bytes=need) == BADARG
    # the stage entries
    assert lib.hipt_segment_saturation(None, 8, 8, 3, sat, None) == BADARG and lib.hipt_segment_saturation(src, 8, 8, 2, sat, None) == BADARG
    assert lib.hipt_segment_saturation(src, 8, 8, 3, None, None) == BADARG and lib.hipt_segment_saturation(src, 0, 8, 3, sat, None) == BADARG
    assert lib.hipt_segment_median(src, 8, 8, 6, med, None) == UNSUPPORTED and lib.hipt_segment_median(src, 8, 8, 17, med, None) == UNSUPPORTED
    assert lib.hipt_segment_median(src, 8, 8, 0, med, None) == BADARG and lib.hipt_segment_median(src, 8, 8, 3, src, None) == BADARG
    assert lib.hipt_segment_median(None, 8, 8, 3, med, None) == BADARG and lib.hipt_segment_median(src, 1 << 16, 1 << 15, 3, med, None) == BADARG
    assert lib.hipt_segment_otsu(src, 8, 8, None, thr, None) == BADARG and lib.hipt_segment_otsu(src, 8, 8, sat, None, None) == BADARG
    assert lib.hipt_segment_otsu(None, 8, 8, sat, thr, None) == BADARG and lib.hipt_segment_otsu(src, 8, 8, sat + 1, thr, None) == BADARG
    assert lib.hipt_segment_close(src, 8, 8, 129, med, ws, 1 << 30, None) == UNSUPPORTED
    assert lib.hipt_segment_close(src, 8, 8, -1, med, ws, 1 << 30, None) == BADARG
    assert lib.hipt_segment_close(src, 8, 8, 4, src, ws, 1 << 30, None) == BADARG and lib.hipt_segment_close(None, 8, 8, 4, med, ws, 1 << 30, None) == BADARG
    assert lib.hipt_segment_close(src, 8, 8, 4, med, ws, lib.hipt_segment_workspace_bytes(8, 8, 4) - 1, None) == WORKSPACE


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    before = N.calls
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    p = torch.zeros((8, 8), dtype=torch.uint8)
    with pytest.raises(ValueError, match="HIP device"):   # a CPU tensor: there is no CPU path
        SG.tissue_mask(x)
    with pytest.raises(ValueError, match="HIP device"):
        SG.tissue_mask(np.zeros((8, 8, 3), dtype=np.uint8), device="cpu")
    for bad in (x.float(), p, torch.zeros((8, 8, 2), dtype=torch.uint8), np.zeros((8, 8, 3), dtype=np.float32), [[1]], torch.zeros((0, 8, 3), dtype=torch.uint8)):
        with pytest.raises(ValueError):
            SG.tissue_mask(bad)
    for kw in ({"sthresh": -1}, {"sthresh": 256}, {"sthresh_up": 300}, {"sthresh": 2.0}, {"sthresh": True}, {"mthresh": 4}, {"mthresh": 17},
               {"mthresh": 0}, {"close": -1}, {"close": 129}, {"close": 2.5}):
        with pytest.raises(ValueError):
            SG.tissue_mask(x, **kw)
    with pytest.raises(ValueError, match="odd"):
        SG.median_blur_u8(p, 6)
    with pytest.raises(ValueError, match="HIP device"):
        SG.median_blur_u8(p, 3)
    with pytest.raises(ValueError, match="HIP device"):
        SG.saturation_u8(x)
    with pytest.raises(ValueError):
        SG.saturation_u8(p)
    with pytest.raises(ValueError, match="HIP device"):
        SG.otsu_threshold(p)
    with pytest.raises(ValueError):
        SG.otsu_threshold(x)
    with pytest.raises(ValueError, match="size"):
        SG.morph_close_u8(p, 200)
    with pytest.raises(ValueError, match="HIP device"):
        SG.morph_close_u8(p, 4)
    assert N.calls == before
