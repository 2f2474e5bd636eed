"""GPU tests of the heat-map rasteriser (csrc/heatmap.hip through hipt_abmil_atec23_amd.heatmap): every output is compared with
the numpy restatement tests/heatmap_ref.py BIT FOR BIT -- the float64 overlay as uint64 views, counts and image bytes with
array_equal.  Inputs are seeded."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check(scores, coords, patch, scale, region, **kw):
    """Device against restatement for one input: image, overlay (from both entry points) and count.  Returns the device's."""
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import heatmap as H
    how = {k: kw[k] for k in ("binarize", "thresh", "convert_to_percentiles") if k in kw}
    keep = np.array(scores, copy=True)
    ref_ov, ref_cnt = R.overlay(scores, coords, patch, scale, region, **how)
    ref_img = R.render(scores, coords, patch, scale, region, **kw)
    before = N.calls
    img, ov = H.render_heatmap(scores, coords, patch, scale, region, return_overlay=True, **kw)
    ov2, cnt = H.heatmap_overlay(scores, coords, patch, scale, region, **how)
    assert N.calls == before + 2
    assert np.array_equal(scores, keep)
    w, h = region
    assert img.shape == (h, w, 3) and img.dtype == np.uint8 and ov.shape == (h, w) and cnt.dtype == np.int32
    assert np.array_equal(cnt, ref_cnt)
    assert np.array_equal(bits(ov), bits(ref_ov)), f"{(bits(ov) != bits(ref_ov)).sum()} overlay pixels differ"
    assert np.array_equal(bits(ov2), bits(ref_ov))
    assert np.array_equal(img, ref_img), f"{(img != ref_img).any(axis=2).sum()} image pixels differ"
    return img, ov, cnt


def odd_canvas_case(seed=0, n=600):
    """Canvas 67 x 45 (no multiple of the 32 x 8 tile), patches 5 x 3 on a 2 x 1 stride starting at (6, 4) -- bare canvas to the
    left and on top, patches cut by the right and bottom edges -- in shuffled index order, one patch wholly outside; scores
    with ties, exact zeros and a few negatives."""
    rng = np.random.default_rng(seed)
    grid = np.array([(x, y) for y in range(4, 45) for x in range(6, 67, 2)])
    coords = grid[rng.permutation(len(grid))[:n - 1]]
    assert (coords[:, 0] + 5 > 67).any() and (coords[:, 1] + 3 > 45).any()
    coords = np.concatenate([coords, [[70, 10]]])[rng.permutation(n)]
    scores = rng.integers(0, 30, size=n).astype(np.float64) * 3.5
    scores[rng.permutation(n)[:40]] = 0.0
    scores[rng.permutation(n)[:10]] = -3.0
    return scores, coords, (5, 3), 1.0, (67, 45)


def test_small_odd_canvas():
    case = odd_canvas_case()
    img, ov, cnt = check(*case, alpha=1.0)
    assert cnt[:4].max() == 0 and cnt[:, :6].max() == 0 and cnt.max() > 4   # bare canvas stays bare; real overlap elsewhere
    assert (img[:4] == 255).all()
    check(*case, alpha=0.4)


@pytest.mark.parametrize("dup", [700, 1500])
def test_long_list_sums_in_index_order(dup):
    """`dup` patches at ONE coordinate plus 50 scattered on a 40 x 40 canvas: a tile list of several LDS chunks (256 candidates
    each; 1500 is also past what the list sort holds in LDS), with scores from 1e-12 to 1e2 whose float64 sum depends on the
    order.  A permuted input changes the restatement's bits, and the device's in the same way."""
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(dup)
    n = dup + 50
    coords = np.concatenate([np.tile([[10, 10]], (dup, 1)), rng.integers(0, 38, size=(50, 2))])
    scores = 10.0 ** rng.uniform(-12, 2, size=n)
    order = rng.permutation(n)
    coords, scores = coords[order], scores[order]
    _, ov, cnt = check(scores, coords, (7, 5), 1.0, (40, 40), alpha=1.0)
    assert cnt.max() >= dup
    perm = rng.permutation(n)
    _, ov_p, cnt_p = check(scores[perm], coords[perm], (7, 5), 1.0, (40, 40), alpha=1.0)
    assert np.array_equal(cnt, cnt_p)
    assert not np.array_equal(bits(ov), bits(ov_p)), "the chosen scores do not make the sum depend on its order"
    ref_p, _ = R.overlay(scores[perm], coords[perm], (7, 5), 1.0, (40, 40))
    assert np.array_equal(bits(ov) != bits(ov_p), bits(R.overlay(scores, coords, (7, 5), 1.0, (40, 40))[0]) != bits(ref_p))
    again, _ = H.heatmap_overlay(scores, coords, (7, 5), 1.0, (40, 40))
    assert np.array_equal(bits(again), bits(ov))


def binarize_case():
    """Stacks of patches at one coordinate each, 4 x 4 on a 24 x 12 canvas; scores 80 / 20 / 3 are above 0.5, between, and below
    1 / N.  With thresh 0.5: A 1 of 2 and B 2 of 4 give exactly 0.5 (-> 0, half to even), C 1 of 3, D 2 of 3 (-> 1), E none above
    (not painted), F a single 80, G overlaps F's corner with a 20."""
    stacks = {(0, 0): [80, 20], (5, 0): [80, 20, 80, 20], (10, 0): [20, 80, 20], (15, 0): [80, 20, 80], (0, 6): [20, 3],
              (5, 6): [80], (7, 8): [20], (20, 7): [3]}
    coords = np.array([c for c, s in stacks.items() for _ in s])
    scores = np.array([v for s in stacks.values() for v in s], dtype=np.float64)
    order = np.random.default_rng(4).permutation(len(scores))
    return scores[order], coords[order], (4, 4), 1.0, (24, 12)


@pytest.mark.parametrize("thresh", [0.5, -1])
def test_binarize(thresh):
    import matplotlib
    case = binarize_case()
    img, ov, cnt = check(*case, alpha=1.0, binarize=True, thresh=thresh)
    check(*case, alpha=0.4, binarize=True, thresh=thresh, cmap="jet")
    cmap = matplotlib.colormaps["coolwarm"]
    zero, one = ((np.array(cmap(v)) * 255)[:3].astype(np.uint8) for v in (0.0, 1.0))
    white = np.array([255, 255, 255], dtype=np.uint8)
    if thresh == 0.5:
        assert ov[0, 0] == 0.0 and ov[0, 5] == 0.0 and ov[0, 10] == 0.0 and ov[0, 15] == 1.0 and ov[6, 5] == 1.0   # 1/2, 2/4, 1/3, 2/3, 1/1
        assert np.array_equal(img[0, 0], zero) and np.array_equal(img[0, 15], one)      # painted although a covering patch is below
        assert np.array_equal(img[6, 0], white) and cnt[6, 0] == 2                      # covered, nothing above: not painted
        assert ov[9, 8] == 0.0 and np.array_equal(img[9, 8], zero) and np.array_equal(img[10, 10], white)   # F + G: 1 / 2; G alone
    else:   # threshold 1 / N = 1 / 17: only the 3s are below
        assert ov[0, 0] == 1.0 and ov[6, 0] == 0.0 and np.array_equal(img[6, 0], zero) and np.array_equal(img[7, 20], white)


def test_half_to_even_above_one_and_the_under_colour_through_the_c_abi():
    """What the Python surface cannot reach: a binarized quotient of 1.5 or 2.5 (patch values are 0 or 1 there) and a negative
    overlay (values below the threshold become 0).  hipt_heatmap_render takes any v: two patches on one spot with v = (3, 0) give
    1.5 -> 2, (5, 0) give 2.5 -> 2, and without rounding v = (-0.5, -0.25) gives -0.375 -> the colormap's under colour."""
    import matplotlib
    import torch
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import heatmap as H
    dev = torch.device("cuda", torch.cuda.current_device())
    xy = torch.tensor([[0, 0], [0, 0], [4, 0], [4, 0], [8, 0], [8, 0]], dtype=torch.int32, device=dev)
    lut = torch.from_numpy(H.colour_table("jet")).to(dev)
    w, h, cmap = 12, 3, matplotlib.colormaps["jet"]
    ws = torch.empty(N.lib().hipt_heatmap_workspace_bytes(6, 3, 3, w, h), dtype=torch.uint8, device=dev)
    for binarize, v, want in ((1, [3.0, 0.0, 5.0, 0.0, 7.0, 0.0], [2.0, 2.0, 4.0]), (0, [-0.5, -0.25, 0.25, 0.5, 3.0, 1.0], [-0.375, 0.375, 2.0])):
        assert not binarize or want == list(np.around(np.array(v[0::2]) / 2))
        vt = torch.tensor(v, dtype=torch.float64, device=dev)
        img = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
        ov = torch.empty((h, w), dtype=torch.float64, device=dev)
        N.call("hipt_heatmap_render", N.ptr(xy), N.ptr(vt), None, 6, 3, 3, w, h, binarize, None, None, N.ptr(lut), 1.0, N.ptr(img), N.ptr(ov),
               N.ptr(ws), ws.numel(), N.stream_ptr(dev))
        ov, img = ov.cpu().numpy(), img.cpu().numpy()
        for k, x in enumerate((0, 4, 8)):
            assert ov[1, x] == want[k] and ov[1, x + 3] == 0.0
            assert np.array_equal(img[1, x], (np.array(cmap(want[k])) * 255)[:3].astype(np.uint8)), (binarize, k)
            assert np.array_equal(img[1, x + 3], [255, 255, 255])


def paint_case(seed=7):
    """Canvas 75 x 50, patches 9 x 6 (level-0 size 18 x 12 at scale 0.5) at random spots; raw scores from -50 to 180, so values
    above 1 reach the over colour and negative ones neither add nor paint; a mask with holes; a random canvas."""
    rng = np.random.default_rng(seed)
    n = 300
    coords = np.stack([rng.integers(0, 140, n), rng.integers(0, 96, n)], axis=1)
    scores = rng.uniform(-50, 180, n)
    mask = rng.uniform(size=(50, 75)) > 0.3
    mask[10:20, 30:50] = False
    canvas = rng.integers(0, 256, size=(50, 75, 3), dtype=np.uint8)
    return (scores, coords, (18, 12), 0.5, (75, 50)), mask, canvas


@pytest.mark.parametrize("alpha", [0.4, 1.0, 0.0])
@pytest.mark.parametrize("cmap", ["coolwarm", "jet"])
def test_painting_and_blend(alpha, cmap):
    case, mask, canvas = paint_case()
    img, ov, _ = check(*case, alpha=alpha, cmap=cmap, mask=mask, canvas=canvas)
    assert ov.max() > 1.0   # the over colour was reached
    blank, _, _ = check(*case, alpha=alpha, cmap=cmap, mask=mask)
    if alpha == 0.0:
        assert np.array_equal(img, canvas) and (blank == 255).all()
    else:
        assert not np.array_equal(img, blank)
        hole = ~mask & (ov > 0)
        assert hole.any() and (np.array_equal(img[hole], canvas[hole]) if alpha == 1.0 else True)
    check(*case, alpha=alpha, cmap=cmap, canvas=canvas)   # no mask


def test_percentile_path():
    scores, coords, patch, scale, region = odd_canvas_case(seed=2, n=400)
    check(scores, coords, patch, scale, region, alpha=0.4, convert_to_percentiles=True)
    check(scores, coords, patch, scale, region, alpha=1.0, convert_to_percentiles=True, binarize=True, thresh=0.7)


def test_empty_bag_returns_the_blended_canvas():
    rng = np.random.default_rng(1)
    canvas = rng.integers(0, 256, size=(21, 37, 3), dtype=np.uint8)
    none = (np.zeros(0), np.zeros((0, 2), dtype=np.int64), (8, 8), 1.0, (37, 21))
    img, ov, cnt = check(*none, alpha=0.4, canvas=canvas)
    assert np.array_equal(img, R.blend(canvas, canvas, 0.4)) and not ov.any() and not cnt.any()
    img, _, _ = check(*none, alpha=1.0, canvas=canvas)
    assert np.array_equal(img, canvas)
    img, _, _ = check(*none, alpha=0.4)
    assert (img == 255).all()


def test_one_size_up_twice_and_from_device_tensors():
    """Canvas 1500 x 1100, 20 000 patches of 8 x 8 on a stride-4 grid (about 52 000 tiles of 32 x 8; lists of some 5 to 10
    patches).  Two runs from numpy inputs and one from tensors already on the device must give the same bytes."""
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(12)
    grid = np.array([(x, y) for y in range(0, 1100, 4) for x in range(0, 1500, 4)])
    coords = grid[rng.permutation(len(grid))[:20000]] * 8   # level-0 pixels at scale 1 / 8
    scores = rng.uniform(0, 100, 20000)
    mask = np.ones((1100, 1500), dtype=bool)
    mask[300:500, 700:900] = False
    canvas = rng.integers(0, 256, size=(1100, 1500, 3), dtype=np.uint8)
    args = (scores, coords, 64, 1 / 8, (1500, 1100))
    img, ov, _ = check(*args, alpha=0.4, mask=mask, canvas=canvas)
    img2, ov2 = H.render_heatmap(*args, alpha=0.4, mask=mask, canvas=canvas, return_overlay=True)
    assert np.array_equal(img, img2) and np.array_equal(bits(ov), bits(ov2))
    dev = torch.device("cuda")
    t = [torch.from_numpy(a).to(dev) for a in (scores, coords, mask, canvas)]
    img3, ov3 = H.render_heatmap(t[0], t[1], 64, 1 / 8, (1500, 1100), alpha=0.4, mask=t[2], canvas=t[3], return_overlay=True)
    assert isinstance(img3, torch.Tensor) and img3.is_cuda and img3.dtype == torch.uint8 and ov3.dtype == torch.float64
    assert np.array_equal(img3.cpu().numpy(), img) and np.array_equal(bits(ov3.cpu().numpy()), bits(ov))
    ov4, cnt4 = H.heatmap_overlay(t[0], t[1], 64, 1 / 8, (1500, 1100))
    assert ov4.is_cuda and cnt4.dtype == torch.int32 and np.array_equal(bits(ov4.cpu().numpy()), bits(ov))


# ---- vis_heatmap ---------------------------------------------------------------------------------------------------------------
class FakeOpenSlide:
    """read_region / get_best_level_for_downsample of a two-level slide (400 x 320, and 100 x 80 at a downsample of 4)."""

    def __init__(self):
        self.level = np.random.default_rng(21).integers(0, 256, size=(80, 100, 4), dtype=np.uint8)
        self.read_calls, self.asked = [], []

    def get_best_level_for_downsample(self, d):
        self.asked.append(d)
        return 1

    def read_region(self, location, level, size):
        from PIL import Image
        self.read_calls.append((location, level, size))
        assert level == 1
        x, y = location[0] // 4, location[1] // 4
        return Image.fromarray(self.level[y:y + size[1], x:x + size[0]])


class FakeSlide:
    level_downsamples = [(1.0, 1.0), (4.0, 4.0)]
    level_dim = [(400, 320), (100, 80)]

    def __init__(self):
        self.wsi = FakeOpenSlide()
        self.mask_calls = []

    def get_seg_mask(self, region_size, scale, use_holes=False, offset=(0, 0)):
        self.mask_calls.append((region_size, tuple(scale), use_holes, offset))
        m = np.random.default_rng(22).uniform(size=(region_size[1], region_size[0])) > 0.2
        return m


def slide_patches():
    rng = np.random.default_rng(23)
    coords = np.stack([rng.integers(0, 24, 150) * 16, rng.integers(0, 19, 150) * 16], axis=1)
    return rng.uniform(0, 100, 150), coords


def test_vis_heatmap_whole_slide_level_choice_and_custom_downsample():
    from PIL import Image
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords = slide_patches()
    slide = FakeSlide()
    before = N.calls
    out = H.vis_heatmap(slide, scores, coords, patch_size=(32, 32), custom_downsample=2, cmap="jet")
    assert N.calls > before
    assert slide.wsi.asked == [32] and slide.wsi.read_calls == [((0, 0), 1, (100, 80))]
    assert slide.mask_calls == [((100, 80), (0.25, 0.25), True, (0, 0))]
    canvas = slide.wsi.level[:, :, :3]
    mask = FakeSlide().get_seg_mask((100, 80), (0.25, 0.25))
    want = R.render(scores, coords, (32, 32), [0.25, 0.25], (100, 80), canvas=canvas, mask=mask, alpha=0.4, cmap="jet")
    want = Image.fromarray(want).resize((50, 40))
    assert isinstance(out, Image.Image) and out.size == (50, 40) and np.array_equal(np.array(out), np.array(want))


def test_vis_heatmap_bounding_box_screening_shift_and_max_size():
    from PIL import Image
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords = slide_patches()
    slide = FakeSlide()
    top_left, bot_right = (64, 32), (336, 272)
    out = H.vis_heatmap(slide, scores.reshape(-1, 1), coords, vis_level=1, top_left=top_left, bot_right=bot_right, patch_size=(32, 32),
                        segment=False, binarize=True, thresh=-1, max_size=34, alpha=0.6)
    assert slide.wsi.asked == [] and slide.wsi.read_calls == [((64, 32), 1, (68, 60))] and slide.mask_calls == []
    inside = np.all(coords >= top_left, axis=1) & np.all(coords <= bot_right, axis=1)
    assert 0 < inside.sum() < len(coords)
    canvas = slide.wsi.level[8:68, 16:84, :3]
    # thresh = -1 is 1 / N of ALL the scores handed in, as the reference computes it before it screens
    want = R.render(scores[inside], coords[inside] - top_left, (32, 32), [0.25, 0.25], (68, 60), canvas=canvas, alpha=0.6, binarize=True,
                    thresh=1.0 / len(scores))
    want = Image.fromarray(want).resize((int(68 * (34 / 68)), int(60 * (34 / 68))))
    assert out.size == (34, 30) and np.array_equal(np.array(out), np.array(want))
    blank = H.vis_heatmap(FakeSlide(), scores, coords, vis_level=1, blank_canvas=True, segment=False, patch_size=(32, 32), alpha=1.0)
    assert np.array_equal(np.array(blank), R.render(scores, coords, (32, 32), [0.25, 0.25], (100, 80), alpha=1.0))


# ---- graph capture, error paths ------------------------------------------------------------------------------------------------
def test_render_is_capturable_into_a_graph_and_replays_on_new_scores():
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    (scores, coords, patch, scale, region), mask, canvas = paint_case(seed=9)
    dev = torch.device("cuda")
    new_scores = np.random.default_rng(10).uniform(-50, 180, len(scores))
    s_t, c_t, m_t, cv_t = (torch.from_numpy(a).to(dev) for a in (scores, coords, mask, canvas))
    kw = dict(alpha=0.4, mask=m_t, canvas=cv_t, cmap="jet")
    eager = H.render_heatmap(s_t, c_t, patch, scale, region, **kw)   # (also puts the colour table on the device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = H.render_heatmap(s_t, c_t, patch, scale, region, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager)
    s_t.copy_(torch.from_numpy(new_scores))
    graph.replay()
    torch.cuda.synchronize()
    want = R.render(new_scores, coords, patch, scale, region, alpha=0.4, mask=mask, canvas=canvas, cmap="jet")
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(out, H.render_heatmap(s_t, c_t, patch, scale, region, **kw))
    assert not np.array_equal(want, eager.cpu().numpy())


def test_error_paths_on_the_device_raise_without_a_native_call():
    import torch
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import heatmap as H
    (scores, coords, patch, scale, region), mask, canvas = paint_case()
    dev = torch.device("cuda")
    s_t, c_t = torch.from_numpy(scores).to(dev), torch.from_numpy(coords).to(dev)
    before = N.calls
    with pytest.raises(RuntimeError, match="expected all tensors on"):
        H.render_heatmap(s_t, c_t, patch, scale, region, canvas=torch.from_numpy(canvas))   # a canvas tensor left on the CPU
    with pytest.raises(RuntimeError, match="expected all tensors on"):
        H.heatmap_overlay(s_t, torch.from_numpy(coords), patch, scale, region)
    with pytest.raises(ValueError, match="negative"):
        H.render_heatmap(s_t, c_t - 5, patch, scale, region)
    bad = s_t.clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        H.render_heatmap(bad, c_t, patch, scale, region)
    with pytest.raises(ValueError, match="negative"):
        H.render_heatmap(scores, coords - 5, patch, scale, region)
    with pytest.raises(ValueError, match="mask"):
        H.render_heatmap(s_t, c_t, patch, scale, region, mask=torch.ones((75, 50), dtype=torch.bool, device=dev))
    with pytest.raises(ValueError, match="canvas"):
        H.render_heatmap(s_t, c_t, patch, scale, region, canvas=torch.zeros((50, 75, 3), dtype=torch.float32, device=dev))
    with pytest.raises(NotImplementedError):
        H.render_heatmap(s_t, c_t, patch, scale, region, blur=True)
    with pytest.raises(RuntimeError, match="HIP device"):
        H.render_heatmap(scores, coords, patch, scale, region, device="cpu")
    assert N.calls == before
