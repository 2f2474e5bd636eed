"""GPU tests of the device resize (csrc/resize.hip through hipt_abmil_atec23_amd.resize).  Every comparison is
``torch.equal`` against the installed Pillow's own bytes, with no tolerance; the images are seeded random bytes plus one image of
only 0 and 255 per geometry (both clamps fire on it).

Without the kernels every test here fails at the import of ``hipt_abmil_atec23_amd.resize``."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (H, W) -> (h, w)
PAIRS = [((512, 768), (128, 192)), ((60, 68), (30, 34)), ((37, 53), (40, 50)), ((64, 64), (200, 131)), ((100, 90), (100, 33)),
         ((33, 77), (7, 77)), ((300, 200), (17, 23)), ((1, 1), (5, 3)), ((9, 9), (1, 1)), ((48, 52), (48, 52))]
IDS = ["%dx%d-%dx%d" % (s + d) for s, d in PAIRS]
_memo = {}


def pil_filter(name):
    from PIL import Image
    return {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX, "lanczos": Image.LANCZOS}[name]


def batch(shape, n=3):
    """n distinct images: random bytes, and (the last one) only 0 and 255."""
    key = (shape, n)
    if key not in _memo:
        rng = np.random.default_rng(100 * shape[0] + shape[1])
        imgs = [rng.integers(0, 256, shape + (3,), dtype=np.uint8) for _ in range(n - 1)]
        imgs.append(rng.integers(0, 2, shape + (3,), dtype=np.uint8) * 255)
        _memo[key] = np.stack(imgs)
    return _memo[key]


def pillow(imgs, dst, name="bicubic"):
    """Pillow's resize of every image of a batch (made once per geometry and filter)."""
    from PIL import Image
    key = (imgs.shape, dst, name)
    if key not in _memo:
        _memo[key] = np.stack([np.array(Image.fromarray(a).resize((dst[1], dst[0]), pil_filter(name))) for a in imgs])
    return _memo[key]


def routes_of(src, dst):
    """The routes a geometry can be forced onto: the fused one needs both axes to change."""
    return ("general", "fused") if src[0] != dst[0] and src[1] != dst[1] else ("general",)


def check(src, dst, name, n, route):
    import torch

    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import resize as RZ
    imgs = batch(src)[3 - n:]   # n = 1: the two-valued image
    want = torch.from_numpy(pillow(batch(src), dst, name)[3 - n:])
    x = torch.from_numpy(imgs).to(DEV)
    before = N.calls
    got = RZ.resize_u8(x if n > 1 else x[0], (dst[1], dst[0]), name, _route=route)
    assert N.calls == before + 1
    assert got.dtype == torch.uint8 and got.device == x.device and tuple(got.shape) == ((n,) if n > 1 else ()) + dst + (3,)
    got = got.cpu().reshape(want.shape)
    assert torch.equal(got, want), (src, dst, name, n, route, int((got != want).sum()))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("src,dst", PAIRS, ids=IDS)
def test_bicubic_is_pillows_bytes_on_every_route(src, dst, n):
    for route in routes_of(src, dst) + (None,):
        check(src, dst, "bicubic", n, route)


@pytest.mark.parametrize("name", ["bilinear", "box", "lanczos"])
@pytest.mark.parametrize("src,dst", [PAIRS[2], PAIRS[6]], ids=[IDS[2], IDS[6]])
def test_the_other_filters_are_pillows_bytes_on_every_route(src, dst, name):
    for route in routes_of(src, dst) + (None,):
        check(src, dst, name, 3, route)


def test_pillows_integer_constants_and_default_filter():
    import torch
    from PIL import Image

    from hipt_abmil_atec23_amd import resize as RZ
    src, dst = PAIRS[1]
    x = torch.from_numpy(batch(src)).to(DEV)
    assert torch.equal(RZ.resize_u8(x, (dst[1], dst[0])).cpu(), torch.from_numpy(pillow(batch(src), dst, "bicubic")))   # RGB's default
    for name, const in (("lanczos", Image.LANCZOS), ("bilinear", Image.BILINEAR), ("bicubic", Image.BICUBIC), ("box", Image.BOX)):
        assert torch.equal(RZ.resize_u8(x, (dst[1], dst[0]), const).cpu(), torch.from_numpy(pillow(batch(src), dst, name)))


def test_one_axis_calls_and_the_equal_size_copy():
    import torch

    from hipt_abmil_atec23_amd import resize as RZ
    for src, dst in (((100, 90), (100, 33)), ((33, 77), (7, 77)), ((37, 53), (37, 60)), ((37, 53), (41, 53))):
        x = torch.from_numpy(batch(src)).to(DEV)
        got = RZ.resize_u8(x, (dst[1], dst[0]))
        assert torch.equal(got.cpu(), torch.from_numpy(pillow(batch(src), dst))), (src, dst)
        with pytest.raises(RuntimeError, match="fused"):   # a route that cannot take the geometry: the library's code, nothing launched
            RZ.resize_u8(x, (dst[1], dst[0]), _route="fused")
    x = torch.from_numpy(batch((48, 52))).to(DEV)
    same = RZ.resize_u8(x, (52, 48))
    assert same.data_ptr() != x.data_ptr() and torch.equal(same, x)
    one = RZ.resize_u8(x[1], (52, 48), "lanczos")
    assert tuple(one.shape) == (48, 52, 3) and torch.equal(one, x[1])


def test_out_is_written_in_place_and_nothing_around_it():
    import torch

    from hipt_abmil_atec23_amd import resize as RZ
    for (src, dst), route in ((PAIRS[2], "fused"), (PAIRS[2], "general"), (PAIRS[6], None), (PAIRS[4], None)):
        x = torch.from_numpy(batch(src)).to(DEV)
        size, gap, canary = 3 * dst[0] * dst[1] * 3, 256, 0xA5
        arena = torch.full((size + 2 * gap,), canary, dtype=torch.uint8, device=DEV)
        out = arena[gap:gap + size].view(3, dst[0], dst[1], 3)
        got = RZ.resize_u8(x, (dst[1], dst[0]), out=out, _route=route)
        assert got.data_ptr() == out.data_ptr()
        flat = arena.cpu()
        assert torch.equal(flat[gap:gap + size].view(3, dst[0], dst[1], 3), torch.from_numpy(pillow(batch(src), dst)))
        assert bool((flat[:gap] == canary).all()) and bool((flat[gap + size:] == canary).all())
    with pytest.raises(ValueError, match="out must be"):
        RZ.resize_u8(x, (33, 100), out=torch.empty((3, 100, 34, 3), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="out must be"):
        RZ.resize_u8(x, (90, 100), out=x)


def test_an_input_that_is_a_view_at_an_odd_address():
    """Image 1 of a batch of 37 x 53 images starts 5883 bytes into the allocation: the kernels read 16-byte vectors all the same."""
    import torch

    from hipt_abmil_atec23_amd import resize as RZ
    src, dst = PAIRS[2]
    x = torch.from_numpy(batch(src)).to(DEV)
    assert x[1].data_ptr() % 16
    assert torch.equal(RZ.resize_u8(x[1], (dst[1], dst[0])).cpu(), torch.from_numpy(pillow(batch(src), dst)[1]))


def test_a_non_default_stream_and_a_captured_graph():
    import torch

    from hipt_abmil_atec23_amd import resize as RZ
    src, dst = PAIRS[0]
    x = torch.from_numpy(batch(src)).to(DEV)
    want = torch.from_numpy(pillow(batch(src), dst))
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        fused = RZ.resize_u8(x, (dst[1], dst[0]))
        general = RZ.resize_u8(x, (dst[1], dst[0]), _route="general")
    stream.synchronize()
    assert torch.equal(fused.cpu(), want) and torch.equal(general.cpu(), want)
    out = torch.zeros_like(fused)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):   # (the tables reached the device above: nothing is copied while capturing)
        RZ.resize_u8(x, (dst[1], dst[0]), out=out)
    for _ in range(2):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), want)


def test_two_geometries_back_to_back_use_their_own_tables():
    import torch

    from hipt_abmil_atec23_amd import resize as RZ
    a, b = torch.from_numpy(batch((60, 68))).to(DEV), torch.from_numpy(batch((37, 53))).to(DEV)
    for _ in range(2):
        ga = RZ.resize_u8(a, (34, 30))
        gb = RZ.resize_u8(b, (50, 40))
        gc = RZ.resize_u8(a, (34, 30), "bilinear")   # the same geometry, another filter
        gd = RZ.resize_u8(a, (30, 34))               # the same lengths, the axes swapped
        assert torch.equal(ga.cpu(), torch.from_numpy(pillow(batch((60, 68)), (30, 34))))
        assert torch.equal(gb.cpu(), torch.from_numpy(pillow(batch((37, 53)), (40, 50))))
        assert torch.equal(gc.cpu(), torch.from_numpy(pillow(batch((60, 68)), (30, 34), "bilinear")))
        assert torch.equal(gd.cpu(), torch.from_numpy(pillow(batch((60, 68)), (34, 30))))


def test_resize_patches_is_pillows_resize_of_every_patch():
    import torch
    from PIL import Image

    from hipt_abmil_atec23_amd import resize as RZ
    patches = batch((64, 64), 5)
    x = torch.from_numpy(patches).to(DEV)
    got = RZ.resize_patches(x, custom_downsample=2)
    assert tuple(got.shape) == (5, 32, 32, 3)
    assert torch.equal(got.cpu(), torch.from_numpy(np.stack([np.array(Image.fromarray(p).resize((32, 32))) for p in patches])))
    got = RZ.resize_patches(x, target_patch_size=24, custom_downsample=2)   # the target size wins
    assert torch.equal(got.cpu(), torch.from_numpy(np.stack([np.array(Image.fromarray(p).resize((24, 24))) for p in patches])))
    assert RZ.resize_patches(x) is x


def test_hierarchical_heatmaps_default_and_host_resize_are_equal():
    import torch

    from hipt_abmil_atec23_amd import HIPT_4K, synth
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    m = HIPT_4K(None, None, DEV, DEV)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(DEV)
    region = synth.hash_u8_np((512, 768, 3), 21)
    dev = HH.hierarchical_heatmaps(m, torch.from_numpy(region).to(DEV), scale=4)
    host = HH.hierarchical_heatmaps(m, region, scale=4, host_resize=True)
    assert set(dev) == set(host) == {"4k", "256", "blend"}
    for k in dev:
        assert dev[k].is_cuda and torch.equal(dev[k], host[k]), k
