"""GPU tests of the device tissue-mask fill (csrc/fill.hip through ``segment.seg_mask`` / ``get_seg_mask_like`` and
``heatmap.vis_heatmap(device_mask=True)``).  Every comparison is exact: the mask equals the sequential restatement
(tests/seg_mask_ref.py, pinned on the CPU by test_seg_mask_host.py) bit for bit.

Without the kernel every test here fails at ``segment.seg_mask``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_ref as CR  # noqa: E402
import seg_mask_ref as SM  # noqa: E402
import test_gpu_contours as TC  # noqa: E402  (the masks of the contour tests)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_memo = {}


def poly(*pts):
    return np.array(pts, dtype=np.int32).reshape(-1, 1, 2)


def star(cx, cy, r_out, r_in, n, turn=0.3):
    return poly(*[(int(round(cx + (r_out if k % 2 == 0 else r_in) * np.cos(turn + np.pi * k / n))),
                   int(round(cy + (r_out if k % 2 == 0 else r_in) * np.sin(turn + np.pi * k / n)))) for k in range(2 * n)])


def traced(name):
    """(contours, holes) of one of the contour tests' masks, as ``segment_tissue`` would hand them on: cv2-style lists"""
    if name not in _memo:
        contours, hier = CR.find_contours(TC.make(name))
        outer = [k for k in range(len(contours)) if hier[0][k][3] == -1]
        _memo[name] = ([contours[k] for k in outer], [[contours[j] for j in range(len(contours)) if hier[0][j][3] == k] for k in outer])
    return _memo[name]


def check(contours, holes, region_size, scale, use_holes=False, offset=(0, 0), **kw):
    """the device mask equals the restatement's; returns it"""
    import torch
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import segment as SG
    want = SM.seg_mask_ref(contours, holes, region_size, scale, use_holes=use_holes, offset=offset)
    before = N.calls
    got = SG.seg_mask(contours, holes, region_size, scale, use_holes=use_holes, offset=offset, device=DEV, **kw)
    assert N.calls == before + 1
    assert got.is_cuda and got.dtype == torch.bool and tuple(got.shape) == (region_size[1], region_size[0])
    assert torch.equal(got.cpu(), torch.from_numpy(want)), np.argwhere(got.cpu().numpy() != want)[:8]
    return got


SQUARE = poly((5, 4), (30, 4), (30, 25), (5, 25))


@pytest.mark.parametrize("size", [(1, 1), (53, 37), (200, 64), (70, 9), (3, 130)])
def test_canvas_sizes(size):
    """1 x 1; odd sizes; a width that is no multiple of the wave; heights (37, 9, 130) that the four rows of a band do not divide"""
    w, h = size
    big = poly((-3, -2), (w + 4, -1), (w + 2, h + 3), (w // 2, h // 2), (-4, h + 1))
    got = check([SQUARE, big], [[], []], size, [1.0, 1.0])
    assert got.any()
    check([star(w // 2, h // 2, max(w, h) // 2 + 2, 3, 5)], [[]], size, [1.0, 1.0])


def test_degenerate_contours_and_one_that_touches_all_four_edges():
    one, two = poly((7, 9)), poly((3, 3), (17, 8))
    line = poly((2, 30), (10, 26), (18, 22), (26, 18), (14, 24))            # all points collinear
    frame = poly((0, 0), (52, 0), (52, 36), (0, 36))
    got = check([one, two, line], [[], [], []], (53, 37), [1.0, 1.0]).cpu().numpy()
    assert got[9, 7] and got[3, 3] and got[8, 17] and got.sum() == 1 + 15 + 25
    assert check([frame], [[]], (53, 37), [1.0, 1.0]).all()
    rim = check([frame], [[poly((1, 1), (51, 1), (51, 35), (1, 35))]], (53, 37), [1.0, 1.0], use_holes=True).cpu().numpy()
    assert rim[0].all() and rim[-1].all() and rim[:, 0].all() and rim[:, -1].all() and not rim[1:-1, 1:-1].any()
    check([], [], (53, 37), [1.0, 1.0])                                     # no contour at all: zeros (the reference raises)
    check([np.zeros((0, 1, 2), np.int32), one], [[], []], (53, 37), [1.0, 1.0])


def test_clipping_and_a_fully_written_mask():
    import torch
    from hipt_abmil_atec23_amd import segment as SG
    blob = star(40, 30, 36, 14, 6)
    got = check([blob], [[]], (53, 37), [1.0, 1.0], offset=(40, 30))        # moved by (-40, -30): half of it at negative coordinates
    assert got[0, 0] and not got.all()
    check([blob], [[]], (53, 37), [0.5, 0.5], offset=(52, 8))
    for dtype in (torch.bool, torch.uint8):
        out = torch.ones((37, 53), dtype=dtype, device=DEV)
        back = SG.seg_mask([blob], [[]], (53, 37), [1.0, 1.0], offset=(-500, 700), out=out)   # wholly outside
        assert back is out and not out.any()
        out.fill_(1)
        SG.seg_mask([blob], [[]], (53, 37), [1.0, 1.0], offset=(40, 30), out=out)
        assert torch.equal(out.cpu().bool(), got.cpu())
    with pytest.raises(ValueError, match="out must be"):
        SG.seg_mask([blob], [[]], (53, 37), [1.0, 1.0], out=torch.ones((37, 54), dtype=torch.bool, device=DEV))


@pytest.mark.parametrize("use_holes", [False, True])
@pytest.mark.parametrize("name", ["nested", "random_0.5", "smooth"])
def test_unit_step_contours_traced_from_masks(name, use_holes):
    """``nested`` holds a contour inside a larger contour's hole: only the draw order keeps it"""
    mask = TC.make(name)
    h, w = mask.shape
    contours, holes = traced(name)
    got = check(contours, holes, (w, h), [1.0, 1.0], use_holes=use_holes).cpu().numpy()
    if name == "nested":
        assert len(contours) == 2 and got[5, 5] and got[4, 4] != use_holes
    # scaled down, as get_seg_mask draws them: consecutive points at most a pixel apart, many of them equal
    check(contours, holes, (w // 2 + 1, h // 2 + 1), [0.5, 0.5], use_holes=use_holes, offset=(3, 5))
    check(contours, holes, ((w + 2) // 3, (h + 2) // 3), [1 / 3, 0.3], use_holes=use_holes)


def test_two_overlapping_holes_of_one_contour_fill_even_odd():
    a = poly((10, 8), (30, 8), (30, 24), (10, 24))
    got = check([poly((2, 2), (50, 2), (50, 34), (2, 34))], [[a, a + 10]], (53, 37), [1.0, 1.0], use_holes=True).cpu().numpy()
    assert not got[12, 15] and not got[30, 35] and got[20, 25] and got[3, 3]


@pytest.mark.parametrize("scale", [3.7, 1 / 3])
def test_long_edges_in_all_eight_octants(scale):
    st = star(0, 0, 60, 22, 8, turn=0.2)                                    # sixteen edges around the origin
    d = np.diff(np.concatenate([st, st[:1]]).reshape(-1, 2), axis=0)
    octants = {(int(dx > 0), int(dy > 0), int(abs(dx) > abs(dy))) for dx, dy in d}
    assert len(octants) == 8
    side = int(125 * scale) + 3
    check([st + 62], [[star(62, 62, 25, 8, 5)]], (side, side - 2), [scale, scale], use_holes=True)
    check([st + 62], [[]], (side, side), [scale, scale * 0.8], offset=(17, -9))


def test_column_chunks_give_the_same_bytes():
    import torch
    contours, holes = traced("smooth")
    mask = TC.make("smooth")
    sx, sy = 200 / mask.shape[1], 64 / mask.shape[0]
    extra = star(100, 30, 120, 20, 7)                                       # long edges that cross every chunk and leave the canvas
    args = (contours + [extra], holes + [[]], (200, 64), [sx, sy])
    whole = check(*args, use_holes=True)
    for cols in (64, 128):                                                  # 4 chunks, the last one 8 columns wide; 2 chunks
        assert torch.equal(check(*args, use_holes=True, _max_cols=cols), whole)


def test_lists_and_device_polygon_lists_give_the_same_bytes_twice():
    import torch
    from hipt_abmil_atec23_amd import segment as SG
    mask = TC.make("random_0.5")
    h, w = mask.shape
    contours, holes = traced("random_0.5")
    from_lists = check(contours, holes, (w, h), [1.0, 1.0], use_holes=True)
    points, offsets, hierarchy = SG.trace_contours(mask, device=DEV)
    for form in ((points, offsets, hierarchy), (points.cpu().numpy(), offsets.cpu().numpy(), hierarchy.cpu().numpy())):
        got = SG.seg_mask(form, None, (w, h), [1.0, 1.0], use_holes=True, device=DEV)
        assert torch.equal(got, from_lists)
        assert torch.equal(SG.seg_mask(form, None, (w, h), [1.0, 1.0], use_holes=True, device=DEV), got)      # twice: the same bytes
    # without a hierarchy every polygon is a contour, the hole borders too
    borders = list(CR.find_contours(mask)[0])
    everything = check(borders, [[] for _ in borders], (w, h), [0.5, 0.5])
    assert torch.equal(SG.seg_mask((points, offsets), None, (w, h), [0.5, 0.5]), everything)
    # a precomputed order: the points are not read back
    want, order = SM.seg_mask_ref(contours, holes, (w, h), [1.0, 1.0], use_holes=True, return_order=True)
    hier = hierarchy.cpu().numpy()
    out = torch.ones((h, w), dtype=torch.bool, device=DEV)
    SG.seg_mask((points, offsets, hier), None, (w, h), [1.0, 1.0], use_holes=True, order=order, out=out)
    assert torch.equal(out.cpu(), torch.from_numpy(want))
    with pytest.raises(ValueError, match="permutation"):
        SG.seg_mask((points, offsets, hier), None, (w, h), [1.0, 1.0], order=order[:-1])


class StubSlide:
    """what ``vis_heatmap`` reads of a slide, with the contours ``segment_tissue`` would have left; it has no ``get_seg_mask``"""
    level_downsamples = [(1.0, 1.0), (4.0, 4.0)]
    level_dim = [(400, 320), (100, 80)]

    class wsi:
        level = np.random.default_rng(31).integers(0, 256, size=(80, 100, 4), dtype=np.uint8)

        @staticmethod
        def get_best_level_for_downsample(d):
            return 1

        @classmethod
        def read_region(cls, location, level, size):
            from PIL import Image
            x, y = location[0] // 4, location[1] // 4
            return Image.fromarray(cls.level[y:y + size[1], x:x + size[0]])

    contours_tissue = [star(200, 160, 150, 70, 6), poly((10, 10), (90, 14), (60, 70))]
    holes_tissue = [[poly((170, 130), (230, 130), (230, 190), (170, 190))], []]


def test_vis_heatmap_with_the_device_mask_equals_render_with_the_restatements_mask():
    from PIL import Image
    from hipt_abmil_atec23_amd import heatmap as H
    from hipt_abmil_atec23_amd import segment as SG
    rng = np.random.default_rng(33)
    coords = np.stack([rng.integers(0, 24, 150) * 16, rng.integers(0, 19, 150) * 16], axis=1)
    scores = rng.uniform(0, 100, 150)
    slide = StubSlide()
    for kw, box, region in ((dict(), (0, 0), (100, 80)), (dict(top_left=(64, 32), bot_right=(336, 272)), (64, 32), (68, 60))):
        out = H.vis_heatmap(slide, scores, coords, vis_level=1, patch_size=(32, 32), device_mask=True, **kw)
        mask = SM.seg_mask_ref(slide.contours_tissue, slide.holes_tissue, region, [0.25, 0.25], use_holes=True, offset=box)
        assert 0 < mask.sum() < mask.size
        like = SG.get_seg_mask_like(slide, region, [0.25, 0.25], use_holes=True, offset=box)
        assert like.is_cuda and np.array_equal(like.cpu().numpy(), mask)
        canvas = slide.wsi.level[box[1] // 4:box[1] // 4 + region[1], box[0] // 4:box[0] // 4 + region[0], :3]
        keep = np.all(coords >= box, axis=1) & np.all(coords <= kw.get("bot_right", (10 ** 6, 10 ** 6)), axis=1)
        want = H.render_heatmap(scores[keep], coords[keep] - np.array(box), (32, 32), [0.25, 0.25], region, canvas=canvas, mask=mask, alpha=0.4,
                                thresh=H.threshold_of(len(scores), False, 0.5))
        assert isinstance(out, Image.Image) and np.array_equal(np.array(out), want)
    with pytest.raises(AttributeError):                                     # device_mask=False keeps today's call
        H.vis_heatmap(slide, scores, coords, vis_level=1, patch_size=(32, 32))
