"""GPU tests of the device tissue segmentation (csrc/segment.hip through hipt_abmil_atec23_amd.segment).  Every
comparison is exact -- ``torch.equal`` against the numpy restatement (tests/segment_ref.py), no tolerance: the stages are 8-bit
integer work, and the Otsu fixtures leave a margin between their two best levels (test_segment_host.py checks it).

Without the kernels every test here fails at the import of ``hipt_abmil_atec23_amd.segment``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import segment_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_memo = {}


def memo(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


def ref(shape, setting, up=255):
    m, c, o = setting
    return memo(("ref", shape, setting, up), lambda: SR.tissue_mask(SR.case_image(shape), 20, up, m, c, o))


def plane(h, w, seed):
    """a saturation plane of the fixture maker: smooth regions, noise, 8-bit"""
    return memo(("plane", h, w, seed), lambda: SR.saturation(SR.make_image(h, w, 3, seed=seed)))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("setting", SR.SETTINGS, ids=["m%d-c%d-%s" % (m, c, "otsu" if o else "fixed") for m, c, o in SR.SETTINGS])
@pytest.mark.parametrize("shape", SR.SHAPES, ids=["%dx%dx%d" % s for s in SR.SHAPES])
def test_whole_call_and_its_parts_are_the_restatements(shape, setting):
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    m, c, o = setting
    img = SR.case_image(shape)
    want_mask, want_med, want_sat, want_t = ref(shape, setting)
    mask, med, sat, thr = SG.tissue_mask(dev(img), 20, 255, m, c, o, return_parts=True)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == shape[:2] and thr.dtype == torch.int32 and tuple(thr.shape) == (1,)
    assert torch.equal(sat.cpu(), torch.from_numpy(want_sat))
    assert torch.equal(med.cpu(), torch.from_numpy(want_med))
    assert int(thr.cpu()[0]) == want_t
    assert torch.equal(mask.cpu(), torch.from_numpy(want_mask))
    assert torch.equal(SG.tissue_mask(dev(img), 20, 255, m, c, o).cpu(), torch.from_numpy(want_mask))   # without the parts


@pytest.mark.parametrize("shape", [(37, 53, 3), (130, 257, 4)], ids=["37x53x3", "130x257x4"])
def test_foreground_value_sthresh_up_200(shape):
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    for setting in ((7, 4, False), (5, 100, True)):
        want = ref(shape, setting, 200)[0]
        assert set(np.unique(want)) <= {0, 200}
        got = SG.tissue_mask(dev(SR.case_image(shape)), 20, 200, *setting)
        assert torch.equal(got.cpu(), torch.from_numpy(want))


SIZES = [(130, 257, 9), (600, 700, 77)]   # the second: several workgroups meet at tile seams and in the histogram


@pytest.mark.parametrize("h,w,seed", SIZES, ids=["130x257", "600x700"])
def test_saturation_stage(h, w, seed):
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    for ch in (3, 4):
        img = SR.make_image(h, w, ch, seed=seed)
        assert torch.equal(SG.saturation_u8(dev(img)).cpu(), torch.from_numpy(SR.saturation(img)))


@pytest.mark.parametrize("h,w,seed,ks", [(130, 257, 9, (1, 3, 5, 7, 9, 11, 13, 15)), (600, 700, 77, (7,))], ids=["130x257", "600x700"])
def test_median_stage(h, w, seed, ks):
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    x = plane(h, w, seed)
    xd = dev(x)
    for k in ks:
        want = memo(("med", h, w, seed, k), lambda: SR.median(x, k))
        assert torch.equal(SG.median_blur_u8(xd, k).cpu(), torch.from_numpy(want)), k


@pytest.mark.parametrize("k", [7, 11])
def test_median_of_a_checkerboard_and_a_ramp(k):
    """Ties and exact rank: a checkerboard's window holds (k k + 1) / 2 of one value and (k k - 1) / 2 of the other; a ramp has every
    value of the window distinct along x and equal along y."""
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    yy, xx = np.mgrid[0:70, 0:131]
    board = np.where((yy + xx) % 2 == 0, 255, 0).astype(np.uint8)
    board2 = np.where((yy + xx) % 2 == 0, 128, 127).astype(np.uint8)
    ramp = ((xx * 2 + yy // 8) % 256).astype(np.uint8)
    for x in (board, board2, ramp):
        assert torch.equal(SG.median_blur_u8(dev(x), k).cpu(), torch.from_numpy(SR.median(x, k)))


@pytest.mark.parametrize("h,w,seed", SIZES, ids=["130x257", "600x700"])
def test_otsu_stage(h, w, seed):
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    x = plane(h, w, seed) if (h, w) == (130, 257) else memo(("med", h, w, seed, 7), lambda: SR.median(plane(h, w, seed), 7))
    hist, thr = SG.otsu_threshold(dev(x))
    assert hist.dtype == torch.int32 and thr.dtype == torch.int32
    assert torch.equal(hist.cpu().long(), torch.from_numpy(SR.histogram(x)))
    assert int(thr.cpu()[0]) == SR.otsu(SR.histogram(x))
    hist2, thr2 = SG.otsu_threshold(dev(np.full((9, 9), 77, dtype=np.uint8)))   # a constant plane: level 0
    assert int(thr2.cpu()[0]) == 0 and int(hist2.cpu()[77]) == 81 and int(hist2.cpu().sum()) == 81


@pytest.mark.parametrize("h,w,seed,cs", [(130, 257, 9, (0, 1, 2, 3, 4, 5, 7, 64, 100, 128)), (600, 700, 77, (4, 100))], ids=["130x257", "600x700"])
def test_closing_stage_on_grey_and_binary_planes(h, w, seed, cs):
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    grey = plane(h, w, seed)
    binary = SR.threshold(grey, 20, 255)
    for x in (grey, binary):
        xd = dev(x)
        for c in cs:
            assert torch.equal(SG.morph_close_u8(xd, c).cpu(), torch.from_numpy(SR.close(x, c))), c


def test_the_fourth_channel_is_ignored():
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    img = SR.make_image(96, 160, 4, seed=21)
    other = img.copy()
    other[:, :, 3] = 255 - other[:, :, 3]
    a = SG.tissue_mask(dev(img), mthresh=7, close=4)
    b = SG.tissue_mask(dev(other), mthresh=7, close=4)
    c = SG.tissue_mask(dev(np.ascontiguousarray(img[:, :, :3])), mthresh=7, close=4)
    assert torch.equal(a, b) and torch.equal(a, c) and 0 < float(a.float().mean()) < 255


def test_out_is_honoured_the_input_is_unmodified_and_numpy_equals_device_input():
    import torch

    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import segment as SG
    shape, setting = (130, 257, 4), (5, 100, True)
    img = SR.case_image(shape)
    want = torch.from_numpy(ref(shape, setting)[0])
    x = dev(img)
    size, gap, canary = shape[0] * shape[1], 256, 0xA5
    arena = torch.full((size + 2 * gap,), canary, dtype=torch.uint8, device=DEV)
    out = arena[gap:gap + size].view(shape[0], shape[1])
    before = N.calls
    got = SG.tissue_mask(x, 20, 255, *setting, out=out)
    assert N.calls == before + 1 and got.data_ptr() == out.data_ptr()   # one native call
    flat = arena.cpu()
    assert torch.equal(flat[gap:gap + size].view(shape[0], shape[1]), want)
    assert bool((flat[:gap] == canary).all()) and bool((flat[gap + size:] == canary).all())
    assert torch.equal(x.cpu(), torch.from_numpy(img))
    assert torch.equal(SG.tissue_mask(img, 20, 255, *setting, device=DEV).cpu(), want)   # a numpy image
    with pytest.raises(ValueError, match="out must be"):
        SG.tissue_mask(x, out=torch.empty((130, 256), dtype=torch.uint8, device=DEV))


def test_a_captured_graph_rederives_the_otsu_level_on_the_device():
    import torch

    from hipt_abmil_atec23_amd import segment as SG
    a, b = SR.make_image(96, 160, 4, seed=21), SR.make_image(96, 160, 4, seed=22)
    ra, rb = SR.tissue_mask(a, 20, 255, 5, 4, True), SR.tissue_mask(b, 20, 255, 5, 4, True)
    assert ra[3] != rb[3] and not np.array_equal(ra[0], rb[0])   # the two images have different levels and masks
    x = dev(a)
    out = torch.zeros((96, 160), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        warm = SG.tissue_mask(x, 20, 255, 5, 4, True)
    stream.synchronize()
    assert torch.equal(warm.cpu(), torch.from_numpy(ra[0]))
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        SG.tissue_mask(x, 20, 255, 5, 4, True, out=out)
    for img, want in ((b, rb), (a, ra), (b, rb)):
        x.copy_(torch.from_numpy(img))
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), torch.from_numpy(want[0]))


def test_nothing_is_written_past_the_workspace():
    import torch

    from hipt_abmil_atec23_amd import _native as N
    shape, canary = (130, 257, 4), 0x5A
    for setting in ((5, 100, True), (7, 0, False)):
        m, c, o = setting
        need = int(N.lib().hipt_segment_workspace_bytes(shape[0], shape[1], c))
        arena = torch.full((need + 4096,), canary, dtype=torch.uint8, device=DEV)
        assert arena.data_ptr() % 256 == 0
        x = dev(SR.case_image(shape))
        mask = torch.empty(shape[:2], dtype=torch.uint8, device=DEV)
        N.call("hipt_segment_mask", N.ptr(x), shape[0], shape[1], 4, 20, 255, m, c, int(o), N.ptr(mask), None, None, None, N.ptr(arena), need,
               N.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert bool((arena[need:].cpu() == canary).all())
        assert torch.equal(mask.cpu(), torch.from_numpy(ref(shape, setting)[0]))
