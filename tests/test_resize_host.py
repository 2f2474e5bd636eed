"""CPU tests of the device resize: the numpy restatement of Pillow's 8-bit arithmetic (tests/resize_ref.py) against the
installed Pillow, byte for byte; ``resize_table`` against the restatement's tables; the int32 bound of every table; the two C entry
points declared, exported and bound; the Python layer's and the library's refusals, which return before anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_ref as RR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import resize as RZ  # noqa: E402

# (H, W) -> (h, w)
PAIRS = [((512, 768), (128, 192)), ((60, 68), (30, 34)), ((37, 53), (40, 50)), ((64, 64), (200, 131)), ((100, 90), (100, 33)),
         ((33, 77), (7, 77)), ((300, 200), (17, 23)), ((1, 1), (5, 3)), ((9, 9), (1, 1)), ((48, 52), (48, 52))]
FILTERS = ("bicubic", "bilinear", "box", "lanczos")
BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4


def pil_filter(name):
    from PIL import Image
    return {"bicubic": Image.BICUBIC, "bilinear": Image.BILINEAR, "box": Image.BOX, "lanczos": Image.LANCZOS}[name]


def images(shape, seed):
    """Uniform random bytes, and an image of only 0 and 255 (both clamps fire on it)."""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, shape + (3,), dtype=np.uint8), (rng.integers(0, 2, shape + (3,), dtype=np.uint8) * 255)


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("src,dst", PAIRS, ids=["%dx%d-%dx%d" % (s + d) for s, d in PAIRS])
def test_restatement_is_pillow_byte_for_byte(src, dst, name):
    from PIL import Image
    for k, img in enumerate(images(src, 7 + src[0] + dst[1])):
        want = np.array(Image.fromarray(img).resize((dst[1], dst[0]), pil_filter(name)))
        got = RR.resize(img, (dst[1], dst[0]), name)
        assert got.dtype == np.uint8 and got.shape == want.shape == dst + (3,)
        assert np.array_equal(got, want), (k, int((got != want).sum()))


def test_both_clamps_fire_on_the_two_valued_image():
    """Bicubic and lanczos weights are negative in places: on an image of 0 and 255 the unclipped value leaves [0, 255] both ways."""
    img = images((37, 53), 7 + 37 + 50)[1].astype(np.int64)
    for name in ("bicubic", "lanczos"):
        k, b = RR.table(53, 50, name)
        raw = np.stack([(2 ** 21 + (img[:, b[xx, 0]:b[xx, 0] + b[xx, 1], :] * k[xx, :b[xx, 1], None]).sum(axis=1)) >> 22 for xx in range(50)])
        assert raw.min() < 0 and raw.max() > 255, name


def test_default_filter_of_rgb_is_bicubic():
    from PIL import Image
    img = images((60, 68), 1)[0]
    assert np.array_equal(np.array(Image.fromarray(img).resize((34, 30))), RR.resize(img, (34, 30), "bicubic"))


def test_restatement_takes_a_batch_as_image_by_image():
    a = np.stack([images((37, 53), s)[0] for s in (1, 2, 3)])
    got = RR.resize(a, (50, 40), "bicubic")
    assert got.shape == (3, 40, 50, 3) and all(np.array_equal(got[i], RR.resize(a[i], (50, 40), "bicubic")) for i in range(3))


@pytest.mark.parametrize("name", FILTERS)
def test_resize_table_is_the_restatements_and_within_int32(name):
    lengths = sorted({(a, b) for s, d in PAIRS for a, b in zip(s, d) if a != b} | {(4096, 1024), (512, 256), (256, 512)})
    for i, o in lengths:
        k, b = RZ.resize_table(i, o, name)
        wk, wb = RR.table(i, o, name)
        assert k.dtype == np.int32 and b.dtype == np.int32 and k.shape == wk.shape and b.shape == (o, 2)
        assert np.array_equal(k, wk) and np.array_equal(b, wb), (i, o)
        assert RR.accumulator_bound(k) < 2 ** 31 and RR.accumulator_bound(wk) < 2 ** 31
        assert (b[:, 0] >= 0).all() and (b[:, 1] >= 1).all() and (b[:, 0] + b[:, 1] <= i).all() and (b[:, 1] <= k.shape[1]).all()
        assert k.shape[1] <= RZ.MAX_KSIZE
        for xx in range(o):   # nothing behind xmax
            assert not k[xx, b[xx, 1]:].any()
        # what the launcher sizes its tiles by: a run of t outputs reads at most ceil((t - 1) * scale) + 1 + ksize inputs
        for t in (4, 8, 16, 32, 64):
            first, last = np.arange(0, o, t), np.minimum(np.arange(0, o, t) + t, o) - 1
            span = b[last, 0] + b[last, 1] - b[first, 0]
            assert (span <= int(np.ceil((t - 1) * (i / o))) + 1 + k.shape[1]).all(), (i, o, t)
        assert (np.diff(b[:, 0]) >= 0).all() and (np.diff(b[:, 0] + b[:, 1]) >= 0).all()
    assert RZ.resize_table(4096, 1024, name)[0] is RZ.resize_table(4096, 1024, name)[0]   # cached
    assert RZ.filter_name(pil_filter(name)) == name


def test_tables_the_kernels_cannot_take_are_refused():
    with pytest.raises(ValueError, match="taps"):
        RZ.resize_table(4096, 8, "lanczos")   # 3073 taps
    with pytest.raises(ValueError, match="taps"):
        RZ.resize_table(2000, 15, "bicubic")   # 535 taps
    assert RZ.resize_table(2000, 16, "bicubic")[0].shape[1] == 501
    with pytest.raises(ValueError, match="positive"):
        RZ.resize_table(0, 8)
    for bad in ("nearest", "hamming", 0, 5, 3.0, None, True):
        with pytest.raises(ValueError, match="filter"):
            RZ.filter_name(bad)


def test_entry_points_are_declared_exported_and_bound_under_abi_6():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"\bsize_t hipt_resize_workspace_bytes\(int n, int in_h, int in_w, int out_h, int out_w, int route\);", hdr)
    decl = re.search(r"\bint hipt_resize_u8\((.*?)\);", hdr, re.S).group(1)
    names = [a.split()[-1].lstrip("*") for a in decl.split(",")]
    assert names == ["src", "n", "in_h", "in_w", "out_h", "out_w", "kx", "bx", "ksize_x", "ky", "by", "ksize_y", "dst", "ws", "ws_bytes",
                     "route", "stream"]
    assert len(N.SIGNATURES["hipt_resize_u8"][1]) == 17 and len(N.SIGNATURES["hipt_resize_workspace_bytes"][1]) == 6
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6
    assert f"#define HIPT_RESIZE_MAX_KSIZE {N.RESIZE_MAX_KSIZE}\n" in hdr
    assert "enum { HIPT_RESIZE_AUTO = 0, HIPT_RESIZE_GENERAL = 1, HIPT_RESIZE_FUSED = 2 };" in hdr
    assert (N.RESIZE_ROUTE_AUTO, N.RESIZE_ROUTE_GENERAL, N.RESIZE_ROUTE_FUSED) == (0, 1, 2)
    lib = N.lib()
    assert hasattr(lib, "hipt_resize_u8") and hasattr(lib, "hipt_resize_workspace_bytes") and lib.hipt_abi_version() == 6
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bresize\.hip\b", mk, re.M) and "FLAGS_resize.hip" not in mk   # integer only: no contraction flag
    import hipt_abmil_atec23_amd as amd
    for name in ("resize_u8", "resize_table", "resize_patches"):
        assert getattr(amd, name) is getattr(RZ, name)


def al256(v):
    return (v + 255) & ~255


def test_workspace_bytes_is_the_carve_of_each_route():
    lib = N.lib()
    A, G, F = N.RESIZE_ROUTE_AUTO, N.RESIZE_ROUTE_GENERAL, N.RESIZE_ROUTE_FUSED
    for n, (h, w), (oh, ow) in [(1, (4096, 4096), (1024, 1024)), (256, (512, 512), (256, 256)), (3, (37, 53), (40, 50)), (2, (300, 200), (17, 23))]:
        mid = al256(n * h * ow * 3)   # the intermediate image [n, in_h, out_w, 3]
        assert lib.hipt_resize_workspace_bytes(n, h, w, oh, ow, G) == mid
        assert lib.hipt_resize_workspace_bytes(n, h, w, oh, ow, A) == mid   # the choice depends on the taps too: the larger need
        assert lib.hipt_resize_workspace_bytes(n, h, w, oh, ow, F) == 0
    for route in (A, G, F):   # one axis, or none: a single launch
        assert lib.hipt_resize_workspace_bytes(2, 100, 90, 100, 33, route) == 0
        assert lib.hipt_resize_workspace_bytes(2, 33, 77, 7, 77, route) == 0
        assert lib.hipt_resize_workspace_bytes(2, 48, 52, 48, 52, route) == 0
    assert lib.hipt_resize_workspace_bytes(0, 8, 8, 4, 4, G) == 0 and lib.hipt_resize_workspace_bytes(1, 8, 8, 4, 4, 3) == 0


def test_library_refuses_without_launching():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    src, dst, kx, bx, ky, by, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000

    def call(n=1, hw=(64, 64), ohw=(32, 32), ks=(9, 9), route=N.RESIZE_ROUTE_AUTO, src=src, dst=dst, tabs=(kx, bx, ky, by), ws=ws, ws_bytes=1 << 30):
        return lib.hipt_resize_u8(src, n, hw[0], hw[1], ohw[0], ohw[1], tabs[0], tabs[1], ks[0], tabs[2], tabs[3], ks[1], dst, ws, ws_bytes,
                                  route, None)
    # a route that cannot take the geometry: the fused one needs both axes to change, and a tile that fits the LDS
    assert call(hw=(100, 90), ohw=(100, 33), route=N.RESIZE_ROUTE_FUSED) == UNSUPPORTED and b"fused" in lib.hipt_last_error()
    assert call(hw=(33, 77), ohw=(7, 77), route=N.RESIZE_ROUTE_FUSED) == UNSUPPORTED
    assert call(hw=(48, 52), ohw=(48, 52), route=N.RESIZE_ROUTE_FUSED) == UNSUPPORTED
    assert call(hw=(4000, 4000), ohw=(16, 16), ks=(501, 501), route=N.RESIZE_ROUTE_FUSED) == UNSUPPORTED and b"LDS" in lib.hipt_last_error()
    # beyond the envelope
    assert call(ks=(513, 9)) == UNSUPPORTED and b"513" in lib.hipt_last_error()
    assert call(ks=(9, 513), route=N.RESIZE_ROUTE_GENERAL) == UNSUPPORTED
    assert call(hw=(1 << 24, 64)) == UNSUPPORTED
    assert call(n=1 << 20, hw=(1 << 12, 1 << 12)) == UNSUPPORTED
    # bad arguments
    assert call(route=3) == BADARG and call(route=-1) == BADARG
    assert call(n=0) == BADARG and call(ohw=(0, 32)) == BADARG and call(hw=(64, -1)) == BADARG
    assert call(src=None) == BADARG and call(dst=None) == BADARG and call(dst=src) == BADARG
    assert call(src=src + 8) == BADARG and call(dst=dst + 2) == BADARG and b"alignment" in lib.hipt_last_error()
    assert call(tabs=(None, bx, ky, by)) == BADARG and call(tabs=(kx, bx, ky, None)) == BADARG and call(ks=(0, 9)) == BADARG
    assert call(tabs=(kx + 2, bx, ky, by)) == BADARG
    # the general route's workspace: short, missing, misaligned
    need = lib.hipt_resize_workspace_bytes(1, 64, 64, 32, 32, N.RESIZE_ROUTE_GENERAL)
    assert need == al256(64 * 32 * 3)
    assert call(route=N.RESIZE_ROUTE_GENERAL, ws_bytes=need - 1) == WORKSPACE
    assert call(route=N.RESIZE_ROUTE_GENERAL, ws=None, ws_bytes=0) == WORKSPACE
    assert call(route=N.RESIZE_ROUTE_GENERAL, ws=None, ws_bytes=need) == BADARG
    assert call(route=N.RESIZE_ROUTE_GENERAL, ws=ws + 16, ws_bytes=need) == WORKSPACE


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    before = N.calls
    x = torch.zeros((8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="HIP device"):   # a CPU tensor: there is no CPU path
        RZ.resize_u8(x, (4, 4))
    with pytest.raises(ValueError, match="uint8"):
        RZ.resize_u8(x.float(), (4, 4))
    with pytest.raises(ValueError, match="uint8"):
        RZ.resize_u8(torch.zeros((8, 8, 4), dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError, match="uint8"):
        RZ.resize_u8(torch.zeros((8, 8), dtype=torch.uint8), (4, 4))
    with pytest.raises(ValueError, match="device tensor"):
        RZ.resize_u8(np.zeros((8, 8, 3), dtype=np.uint8), (4, 4))
    for size in ((0, 4), (4, -1), (4,), 4, (4.0, 4), (4, 4, 4), (True, 4)):   # (size and filter are looked at before the device)
        with pytest.raises(ValueError, match="size"):
            RZ.resize_u8(x, size)
    for bad in ("nearest", 0, 5, None):
        with pytest.raises(ValueError, match="filter"):
            RZ.resize_u8(x, (4, 4), bad)
    with pytest.raises(ValueError, match="route"):
        RZ.resize_u8(x, (4, 4), _route="tiled")
    with pytest.raises(ValueError, match="integers"):
        RZ.resize_patches(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), 4.0)
    with pytest.raises(ValueError, match="square"):
        RZ.resize_patches(torch.zeros((2, 8, 6, 3), dtype=torch.uint8), 4)
    with pytest.raises(ValueError, match="HIP device"):
        RZ.resize_patches(torch.zeros((2, 8, 8, 3), dtype=torch.uint8), custom_downsample=2)
    same = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    assert RZ.resize_patches(same) is same and RZ.resize_patches(same, -1, 1) is same   # neither applies: x itself
    assert RZ.target_size(256, 224, 2) == (224, 224) and RZ.target_size(256, -1, 2) == (128, 128) and RZ.target_size(256) is None
    assert N.calls == before
