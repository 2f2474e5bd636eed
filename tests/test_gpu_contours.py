"""GPU tests of the device contour tracer (csrc/contours.hip through ``segment.trace_contours`` / ``find_contours``).
Every comparison is exact: points, offsets, hierarchy and the order of the list equal the sequential restatement
(tests/contour_ref.py, pinned on the CPU by test_contours_host.py).

Without the kernels every test here fails at ``segment.trace_contours`` / ``segment.find_contours``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_ref as CR  # noqa: E402
import segment_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_memo = {}


def blank(h, w):
    return np.zeros((h, w), np.uint8)


def make(name):
    if name == "empty":
        return blank(6, 9)
    if name == "full_5x7":            # the border runs along the image's edge
        return np.full((5, 7), 255, np.uint8)
    if name == "corner_pixel":
        m = blank(4, 6)
        m[3, 5] = 1
        return m
    if name == "thin_L":
        m = blank(9, 8)
        m[1:8, 2] = 255
        m[7, 2:7] = 255
        return m
    if name == "diagonal_chain":
        m = blank(8, 8)
        m[np.arange(1, 7), np.arange(1, 7)] = 255
        return m
    if name == "ring_3x3":
        m = blank(5, 5)
        m[1:4, 1:4] = 255
        m[2, 2] = 0
        return m
    if name == "nested":              # a blob with a hole that holds an island with its own hole
        m = blank(16, 18)
        m[1:15, 1:17] = 255
        m[3:13, 3:15] = 0
        m[5:11, 5:13] = 255
        m[7:9, 7:11] = 0
        return m
    if name == "diagonal_holes":      # two holes that touch only by a corner: two holes
        m = blank(6, 6)
        m[1:5, 1:5] = 255
        m[2, 2] = m[3, 3] = 0
        return m
    if name == "checkerboard":        # one component, many one-pixel holes
        return ((np.indices((8, 8)).sum(0) % 2) == 0).astype(np.uint8) * 255
    if name == "mixed_bytes":
        m = CR.random_mask(19, 23, 0.55, seed=4)
        return (m != 0) * np.random.default_rng(9).integers(1, 256, m.shape).astype(np.uint8)
    if name.startswith("random_"):
        d = float(name.split("_")[1])
        return CR.random_mask(37, 53, d, seed=int(d * 10))
    if name == "1x1":
        return np.full((1, 1), 7, np.uint8)
    if name == "1x40":
        m = np.full((1, 40), 255, np.uint8)
        m[0, [5, 6, 20]] = 0
        return m
    if name == "40x1":
        m = np.full((40, 1), 255, np.uint8)
        m[[0, 17, 39], 0] = 0
        return m
    if name == "smooth":
        return CR.smooth_mask(256, 320, seed=2, sigma=5.0)
    raise KeyError(name)


NAMES = ["empty", "full_5x7", "corner_pixel", "thin_L", "diagonal_chain", "ring_3x3", "nested", "diagonal_holes", "checkerboard",
         "mixed_bytes", "random_0.3", "random_0.5", "random_0.7", "1x1", "1x40", "40x1", "smooth"]


def case(name):
    """(mask, the restatement's (points, offsets, hierarchy)); made once"""
    if name not in _memo:
        mask = np.ascontiguousarray(make(name))
        _memo[name] = (mask, CR.trace(mask))
    return _memo[name]


def same(got, want):
    import torch
    pts, off, hier = got
    assert pts.dtype == torch.int32 and off.dtype == torch.int64 and hier.dtype == torch.int32
    assert pts.is_cuda and off.is_cuda and hier.is_cuda
    assert tuple(pts.shape) == want[0].shape and tuple(off.shape) == want[1].shape and tuple(hier.shape) == want[2].shape
    assert np.array_equal(off.cpu().numpy(), want[1])
    assert np.array_equal(hier.cpu().numpy(), want[2])
    assert np.array_equal(pts.cpu().numpy(), want[0])


@pytest.mark.parametrize("name", NAMES)
def test_trace_and_find_contours_equal_the_restatement(name):
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import segment as SG
    mask, want = case(name)
    if name == "smooth":   # the ranking needs more passes than a wave has lanes and spans several workgroups
        assert int(np.diff(want[1]).max()) > 2048
    if name == "nested":
        assert want[2][:, 3].tolist().count(-1) == 2 and len(want[2]) == 4
    if name == "diagonal_holes":
        assert (want[2][:, 3] >= 0).sum() == 2
    before = N.calls
    same(SG.trace_contours(mask, device=DEV), want)
    assert N.calls > before
    contours, hier = SG.find_contours(mask, device=DEV)
    if name == "empty":
        assert contours == () and hier is None
        return
    assert isinstance(contours, tuple) and len(contours) == len(want[2]) and hier.dtype == np.int32 and hier.shape == (1, len(want[2]), 4)
    assert np.array_equal(hier[0], want[2])
    for k, c in enumerate(contours):
        assert c.dtype == np.int32 and c.shape == (want[1][k + 1] - want[1][k], 1, 2)
        assert np.array_equal(c.reshape(-1, 2), want[0][want[1][k]:want[1][k + 1]])


@pytest.mark.parametrize("name", ["random_0.5", "smooth"])
def test_same_bytes_for_array_and_tensor_on_another_stream_and_twice(name):
    import torch
    from hipt_abmil_atec23_amd import segment as SG
    mask, want = case(name)
    on_dev = torch.from_numpy(mask).to(DEV)
    first = SG.trace_contours(on_dev)
    same(first, want)
    again = SG.trace_contours(on_dev)
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        other = SG.trace_contours(on_dev)
    stream.synchronize()
    from_array = SG.trace_contours(mask, device=DEV)
    for got in (again, other, from_array):
        assert all(torch.equal(a, b) for a, b in zip(got, first))
    assert torch.equal(on_dev.cpu(), torch.from_numpy(mask))   # the input is left as it was


class FakeSlide:
    """the small synthetic slide of the segmentation tests: one picture, read as level 1 of a two-level slide"""
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


def test_segment_tissue_with_the_device_tracer_equals_the_restatement_as_tracer():
    import torch
    from hipt_abmil_atec23_amd import segment as SG
    img = SR.make_image(40, 50, 4, seed=3)
    kw = dict(seg_level=1, sthresh=8, sthresh_up=200, mthresh=5, close=4, use_otsu=False,
              filter_params={"a_t": 1, "a_h": 0, "max_n_holes": 8}, ref_patch_size=8)
    seen = {}

    def device_tracer(mask):
        seen["mask"] = mask
        return SG.find_contours(mask)
    device_tracer.takes_device_mask = True
    got, want, probe = FakeSlide(img), FakeSlide(img), FakeSlide(img)
    SG.segment_tissue(got, find_contours=SG.find_contours, **kw)
    SG.segment_tissue(want, find_contours=CR.find_contours, **kw)
    SG.segment_tissue(probe, find_contours=device_tracer, **kw)
    assert torch.is_tensor(seen["mask"]) and seen["mask"].is_cuda      # the mask was not read back for the device tracer
    assert len(want.contours_tissue) >= 1
    for s in (got, probe):
        assert len(s.contours_tissue) == len(want.contours_tissue) and len(s.holes_tissue) == len(want.holes_tissue)
        for a, b in zip(s.contours_tissue, want.contours_tissue):
            assert a.dtype == np.int32 and np.array_equal(a, b)
        for ha, hb in zip(s.holes_tissue, want.holes_tissue):
            assert len(ha) == len(hb) and all(np.array_equal(a, b) for a, b in zip(ha, hb))
