"""CPU tests of the hierarchical heat-maps: the closed-form rank against scipy on really upscaled vectors, bit for
bit; the colour tables against matplotlib's own look-up; ``shifted_regions`` against Pillow; the two C entry points declared,
exported and bound, and their argument checks, which return before anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hier_heatmap_ref as HR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import hier_heatmap as HH  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("f", [1, 4, 16, 64])
def test_closed_form_rank_is_scipy_on_the_upscaled_vector(f, ties):
    for L in (1, 6, 255, 256, 1024):
        if L * f * f > 1 << 21:   # (1024 values at f = 64 are 4 M copies a vector: one vector of them is enough)
            x = HR.rank_case(1, L, 100 * L + f, ties)
        else:
            x = HR.rank_case(3, L, 100 * L + f, ties)
        if ties and L >= 255:
            assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        want = HR.long_way_percentiles(x, f)
        got = HH.closed_form_percentiles(x, f)
        assert got.dtype == np.float64 and np.array_equal(bits(got), bits(want)), (L, f, int((bits(got) != bits(want)).sum()))


def test_upscaled_map_ranks_are_the_closed_form_at_every_pixel():
    """The same through the restatement's own route: a [16, 16] map really upscaled to [64, 64] and ranked as the reference does."""
    x = HR.rank_case(2, 256, 7, True)
    for v in range(2):
        up = HR.upscale(x[v].reshape(16, 16), 4)
        want = HR.rank(up.flatten()).reshape(64, 64)
        got = HR.upscale(HH.closed_form_percentiles(x[v], 4).reshape(16, 16), 4)
        assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("name,entries", [("coolwarm", 256), ("half_jet", 1024)])
def test_colour_table_is_matplotlibs_lookup(name, entries):
    import matplotlib
    cmap = HH.half_jet() if name == "half_jet" else matplotlib.colormaps[name]
    table = HH.colour_table_n(name)
    assert table.dtype == np.uint8 and table.shape == (entries, 3) and cmap.N == entries
    assert np.array_equal(table, HH.colour_table_n(cmap))
    rng = np.random.default_rng(3)
    x = np.concatenate([[0.0, 1.0, 0.5, 0.95, 1.0 - 2.0 ** -53, 2.0 ** -1074], np.arange(entries + 1) / entries, rng.random(5000)])
    x = x.reshape(1, -1)
    want = (cmap(x) * 255)[:, :, :3].astype(np.uint8)
    entry = np.minimum(np.trunc(x * entries).astype(np.int64), entries - 1)
    assert np.array_equal(table[entry], want)


def test_half_jet_is_jet_halved_towards_white():
    import matplotlib
    jet, half = matplotlib.colormaps["jet"], HH.half_jet()
    assert half.N == 1024 and half.name == "colormap"
    x = np.linspace(0, 1, 41)
    # jet's own table has 256 entries and its ramps a slope of at most 1 / 0.11: it is a step of up to 0.036 / 2 coarser than the 1024 entries
    assert np.allclose(np.asarray(half(x))[:, :3], np.asarray(jet(x))[:, :3] / 2 + 0.5, atol=0.018)
    ends = np.asarray(half([0.0, 1.0]))[:, :3]
    assert np.array_equal(ends, [[0.5, 0.5, 0.75], [0.75, 0.5, 0.5]])   # jet's dark blue and dark red, halved towards white


def test_colour_table_refuses_what_the_kernel_cannot_hold():
    import matplotlib
    from matplotlib.colors import ListedColormap
    with pytest.raises(ValueError):
        HH.colour_table_n("no such colormap")
    with pytest.raises(ValueError):
        HH.colour_table_n(ListedColormap(["r"]))
    with pytest.raises(ValueError):
        HH.colour_table_n(matplotlib.colormaps["jet"].resampled(N.HIER_MAX_LUT + 1))


def test_shifted_regions_are_pillows_crop_and_margin():
    from PIL import Image
    rng = np.random.default_rng(11)
    a = rng.integers(0, 255, (512, 768, 3), dtype=np.uint8)   # (no 255: the margin is told from the image)
    region = Image.fromarray(a)
    w, h = region.size

    def add_margin(img, bottom, right):   # the reference's add_margin with top = left = 0
        out = Image.new(img.mode, (img.width + right, img.height + bottom), (255, 255, 255))
        out.paste(img, (0, 0))
        return out
    want = [region,
            add_margin(region.crop((128, 128, w, h)), 128, 128),
            add_margin(region.crop((128 * 2, 128 * 2, w, h)), 128 * 2, 128 * 2),
            add_margin(region.crop((128 * 3, 128 * 3, w, h)), 128 * 4, 128 * 4)]
    got = HH.shifted_regions(a)
    assert len(got) == 4 and all(isinstance(g, np.ndarray) and g.dtype == np.uint8 for g in got)
    for g, wnt in zip(got, want):
        assert np.array_equal(g, np.array(wnt))
    assert got[3].shape == (512 + 128, 768 + 128, 3)   # the reference's margin of 128 * 4: larger than the region
    with pytest.raises(ValueError):
        HH.shifted_regions(a[:300], offset=128)
    with pytest.raises(ValueError):
        HH.shifted_regions(a.astype(np.float32))


def test_entry_points_are_declared_exported_and_bound_under_abi_6():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"\bint hipt_hier_ranks\(const float\* x, int V, int L, int f, double\* pct, void\* stream\);", hdr)
    assert re.search(r"\bint hipt_hier_render\(const double\* pct4k, const double\* pct256, int nh, int w_256, int h_256, int scale,", hdr)
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6
    for name, value in (("L", N.HIER_MAX_L), ("UPSCALE", N.HIER_MAX_UPSCALE), ("HEADS", N.HIER_MAX_HEADS), ("LUT", N.HIER_MAX_LUT)):
        assert f"#define HIPT_HIER_MAX_{name} {value}\n" in hdr
    render = re.search(r"int hipt_hier_render\((.*?)\);", hdr, re.S).group(1)
    assert len(N.SIGNATURES["hipt_hier_ranks"][1]) == 6 and len(N.SIGNATURES["hipt_hier_render"][1]) == len(render.split(",")) == 23
    lib = N.lib()
    assert hasattr(lib, "hipt_hier_ranks") and hasattr(lib, "hipt_hier_render") and lib.hipt_abi_version() == 6
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert " hier_heatmap.hip " in mk and "FLAGS_hier_heatmap.hip = -ffp-contract=off" in mk
    import hipt_abmil_atec23_amd as amd
    for name in ("hierarchical_heatmaps", "compose_heatmaps", "region_attention_maps", "shifted_regions", "colour_table_n", "cmap_map",
                 "create_hierarchical_heatmaps_indiv"):
        assert getattr(amd, name) is getattr(HH, name)
    assert callable(amd.HIPT_4K.get_region_attention_heatmaps)


BADARG, UNSUPPORTED = -1, -4


def test_argument_checks_return_their_codes_without_a_device():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    p, q = 0x1000, 0x2000
    assert lib.hipt_hier_ranks(p, 3, 0, 1, q, None) == UNSUPPORTED and b"L=0" in lib.hipt_last_error()
    assert lib.hipt_hier_ranks(p, 3, 4097, 1, q, None) == UNSUPPORTED and b"L=4097" in lib.hipt_last_error()
    assert lib.hipt_hier_ranks(p, 3, 256, 0, q, None) == UNSUPPORTED
    assert lib.hipt_hier_ranks(p, 3, 256, 257, q, None) == UNSUPPORTED
    assert lib.hipt_hier_ranks(None, 3, 256, 4, q, None) == BADARG
    assert lib.hipt_hier_ranks(p, 3, 256, 4, None, None) == BADARG
    assert lib.hipt_hier_ranks(p, -1, 256, 4, q, None) == BADARG
    assert lib.hipt_hier_ranks(p + 2, 3, 256, 4, q, None) == BADARG and lib.hipt_hier_ranks(p, 3, 256, 4, q + 4, None) == BADARG
    assert lib.hipt_hier_ranks(None, 0, 256, 4, None, None) == 0   # no vectors: nothing to do

    def render(nh=6, w=2, h=3, scale=4, lut_n=256, outs=(0x3000, 0x4000, 0x5000, 0x6000), base=0x7000, lut=0x8000, use_thr=1, thr=0.5,
               pairs=None, npairs=0, w256=2.0, alpha=0.5, offs=(32, 64, 96), pct=(p, q)):
        return lib.hipt_hier_render(pct[0], pct[1], nh, w, h, scale, offs[0], offs[1], offs[2], base, lut, lut_n, alpha, w256, pairs,
                                    npairs, use_thr, thr, outs[0], outs[1], outs[2], outs[3], None)
    assert render(scale=3) == UNSUPPORTED and b"scale=3" in lib.hipt_last_error()
    assert render(scale=32) == UNSUPPORTED and render(scale=0) == UNSUPPORTED
    assert render(lut_n=1) == UNSUPPORTED and render(lut_n=4097) == UNSUPPORTED
    assert render(nh=0) == UNSUPPORTED and render(nh=9) == UNSUPPORTED
    assert render(w=0) == UNSUPPORTED and render(w=65, h=64) == UNSUPPORTED
    assert render(outs=(None, None, None, None)) == BADARG and b"no output" in lib.hipt_last_error()
    assert render(pct=(None, q)) == BADARG and render(pct=(p, None)) == BADARG and render(base=None) == BADARG and render(lut=None) == BADARG
    assert render(offs=(-1, 0, 0)) == BADARG
    assert render(alpha=float("nan")) == BADARG and render(w256=0.0) == BADARG and render(thr=float("nan")) == BADARG
    assert render(use_thr=0) == BADARG   # the threshold picture without a threshold
    assert render(outs=(0x3001, None, None, None)) == BADARG and render(base=0x7002) == BADARG and render(pct=(p + 4, q)) == BADARG
    assert render(outs=(0x7000, None, None, None)) == BADARG   # the base image as an output
    import ctypes as C
    twice = (C.c_int32 * 4)(1, 0, 1, 0)
    assert render(pairs=C.cast(twice, C.c_void_p), npairs=2) == BADARG and b"twice" in lib.hipt_last_error()
    beyond = (C.c_int32 * 2)(6, 0)
    assert render(pairs=C.cast(beyond, C.c_void_p), npairs=1) == BADARG
    one = (C.c_int32 * 2)(1, 0)
    assert render(pairs=C.cast(one, C.c_void_p), npairs=0) == BADARG


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    before = N.calls
    a256, a4k = torch.zeros((2, 6, 6, 256)), torch.zeros((4, 6, 6))
    base = np.zeros((128, 192, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="scale 3"):
        HH.compose_heatmaps(a256, a4k, 2, 3, base, scale=3)
    with pytest.raises(ValueError, match="which"):
        HH.compose_heatmaps(a256, a4k, 2, 3, base, which=("4k", "512"))
    with pytest.raises(ValueError, match="needs a threshold"):
        HH.compose_heatmaps(a256, a4k, 2, 3, base, which=("256th",))
    with pytest.raises(ValueError, match="a4k must be"):
        HH.compose_heatmaps(a256, a4k, 3, 3, base)
    with pytest.raises(ValueError, match="a256 must be"):
        HH.compose_heatmaps(a256[:1], a4k, 2, 3, base)
    with pytest.raises(ValueError, match="float32"):
        HH.compose_heatmaps(a256.double(), a4k, 2, 3, base)
    with pytest.raises(RuntimeError, match="HIP device"):   # CPU tensors: there is no CPU path
        HH.compose_heatmaps(a256, a4k, 2, 3, base)
    with pytest.raises(ValueError, match="pairs"):
        HH._check_pairs([(0, 0), (0, 0)], 6)
    with pytest.raises(ValueError, match="pairs"):
        HH._check_pairs([(0, 6)], 6)
    assert N.calls == before


def test_dropin_hook_binds_where_the_reference_module_imports(monkeypatch):
    import types

    from hipt_abmil_atec23_amd import dropin
    assert "HIPT_4K.hipt_heatmap_utils.create_hierarchical_heatmaps_indiv" not in dropin.install(hier_heatmaps=True)   # no such module here
    dropin.uninstall()
    pkg, mod = types.ModuleType("HIPT_4K"), types.ModuleType("HIPT_4K.hipt_heatmap_utils")
    pkg.__path__ = []
    mod.create_hierarchical_heatmaps_indiv = theirs = lambda *a, **k: None
    monkeypatch.setitem(sys.modules, "HIPT_4K", pkg)
    monkeypatch.setitem(sys.modules, "HIPT_4K.hipt_heatmap_utils", mod)
    done = dropin.install(hier_heatmaps=True)
    assert done["HIPT_4K.hipt_heatmap_utils.create_hierarchical_heatmaps_indiv"].endswith("create_hierarchical_heatmaps_indiv_like")
    assert mod.create_hierarchical_heatmaps_indiv is HH.create_hierarchical_heatmaps_indiv_like
    dropin.uninstall()
    assert mod.create_hierarchical_heatmaps_indiv is theirs
