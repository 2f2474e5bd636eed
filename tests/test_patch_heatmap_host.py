"""CPU tests of the patch-level heat-maps: ``shifted_patches`` against Pillow; the restatement
(tests/patch_heatmap_ref.py: really upscaled, really ranked) against the closed-form ranks and the index arithmetic the kernel uses,
bit for bit; the entry point declared, exported and bound under ABI 6; its argument checks, which return before anything touches a
device; the Python layer's refusals; the file names."""
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_heatmap_ref as PR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import hier_heatmap as HH  # noqa: E402
from hipt_abmil_atec23_amd import patch_heatmap as PH  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def test_shifted_patches_are_pillows_crop_and_margin():
    import torch
    patches = np.random.default_rng(4).integers(0, 255, (3, 256, 256, 3), dtype=np.uint8)   # (no 255: the margin is told from the image)
    got = PH.shifted_patches(patches)
    assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got.shape == (3, 2, 256, 256, 3)
    for p in range(3):
        first, second = PR.layers(patches[p])
        assert np.array_equal(got[p, 0], first) and np.array_equal(got[p, 1], second)
    assert (got[:, 1, 240:] == 255).all() and (got[:, 1, :, 240:] == 255).all() and np.array_equal(got[:, 1, :240, :240], patches[:, 16:, 16:])
    t = PH.shifted_patches(torch.from_numpy(patches))
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), got)
    with pytest.raises(ValueError):
        PH.shifted_patches(patches[0])
    with pytest.raises(ValueError):
        PH.shifted_patches(patches.astype(np.float32))
    with pytest.raises(ValueError):
        PH.shifted_patches(patches[:, :128])


def closed_form_score(a1, a2, offset):
    """The score as the kernel forms it: closed-form ranks at the maps' own size, gathered per pixel."""
    r1, r2 = HH.closed_form_percentiles(a1, 16), HH.closed_form_percentiles(a2, 16)
    y, x = np.mgrid[0:256, 0:256]
    s = r1[(y >> 4) * 16 + (x >> 4)]
    present = (y >= offset) & (x >= offset)
    yy, xx = np.maximum(y - offset, 0), np.maximum(x - offset, 0)
    both = (s + r2[(yy >> 4) * 16 + (xx >> 4)]) / 200.0
    return np.where(present, both, s / 100.0)


@pytest.mark.parametrize("offset", [0, 5, 16, 255, 256])
def test_restatement_is_the_closed_form_at_every_pixel(offset):
    a = PR.synthetic_maps(1, 1, 30 + offset)[0, :, 0]   # ties
    want = PR.score(a[0], a[1], offset)
    assert want.dtype == np.float64 and np.array_equal(bits(closed_form_score(a[0], a[1], offset)), bits(want))
    assert 0.0 < want.min() and want.max() <= 1.0
    overlap = (256 - offset) ** 2
    ov = np.ones((256, 256)) * 100
    ov[offset:, offset:] += 100
    assert int((ov == 200).sum()) == overlap


def test_constant_map_scores_one_value_everywhere():
    a = np.full((2, 256), 0.25, dtype=np.float32)
    sc = PR.score(a[0], a[1], 16)
    assert np.unique(sc).size == 1 and sc[0, 0] == (65536 + 1) / 2 * 100 / 65536 / 100


def test_mosaic_is_three_across_and_unused_tiles_are_zero():
    pics = np.random.default_rng(2).integers(1, 256, (6, 256, 256, 3), dtype=np.uint8)
    m = PR.mosaic(pics, 3)
    assert m.shape == (512, 768, 3) == PH.mosaic_shape(6, 3) + (3,)
    for i in range(6):
        assert np.array_equal(m[(i // 3) * 256:(i // 3 + 1) * 256, (i % 3) * 256:(i % 3 + 1) * 256], pics[i])
    m = PR.mosaic(pics, 4)
    assert m.shape == (512, 1024, 3) == PH.mosaic_shape(6, 4) + (3,)
    assert np.array_equal(m[256:, 256:512], pics[5]) and not m[256:, 512:].any()


def test_entry_point_is_declared_exported_and_bound_under_abi_6():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"\bint hipt_patch_render\(const double\* pct, const uint8_t\* patches, int P, int nh, const uint8_t\* lut, int lut_n,", hdr)
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6
    assert f"#define HIPT_PATCH_MAX_P {N.PATCH_MAX_P}\n" in hdr
    decl = re.search(r"int hipt_patch_render\((.*?)\);", hdr, re.S).group(1)
    assert len(N.SIGNATURES["hipt_patch_render"][1]) == len(decl.split(",")) == 14
    lib = N.lib()
    assert hasattr(lib, "hipt_patch_render") and lib.hipt_abi_version() == 6
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert " patch_heatmap.hip " in mk and "FLAGS_patch_heatmap.hip = -ffp-contract=off" in mk and " heat_paint.h " in mk
    # one copy of the look-up, the blend's use and the thresholded rule: both renderers take them from the shared header
    csrc = os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc")
    for name in ("hier_heatmap.hip", "patch_heatmap.hip"):
        src = open(os.path.join(csrc, name)).read()
        assert '#include "heat_paint.h"' in src and "hh_paint_threshold(" in src and "hh_threshold_entries(" in src
        assert "blend_u8(" not in src
    import hipt_abmil_atec23_amd as amd
    for name in ("patch_heatmaps", "compose_patch_heatmaps", "patch_attention_maps", "shifted_patches", "create_patch_heatmaps_indiv",
                 "create_patch_heatmaps_concat"):
        assert getattr(amd, name) is getattr(PH, name)
    for name in ("hierarchical_heatmaps_concat_select", "create_hierarchical_heatmaps_concat_select"):
        assert getattr(amd, name) is getattr(HH, name)


BADARG, UNSUPPORTED = -1, -4


def test_argument_checks_return_their_codes_without_a_device():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()

    def render(pct=0x1000, patches=0x2000, P=3, nh=6, lut=0x3000, lut_n=256, offset=16, alpha=0.5, use_thr=1, thr=0.5, cols=0, hm=0x4000,
               hm_thr=0x5000):
        return lib.hipt_patch_render(pct, patches, P, nh, lut, lut_n, offset, alpha, use_thr, thr, cols, hm, hm_thr, None)
    assert render(nh=0) == UNSUPPORTED and b"nh=0" in lib.hipt_last_error()
    assert render(nh=9) == UNSUPPORTED and render(lut_n=1) == UNSUPPORTED and render(lut_n=4097) == UNSUPPORTED
    assert render(P=N.PATCH_MAX_P + 1) == UNSUPPORTED
    assert render(P=-1) == BADARG
    assert render(offset=-1) == BADARG and render(offset=257) == BADARG and b"offset 257" in lib.hipt_last_error()
    assert render(cols=-1) == BADARG and render(cols=9) == BADARG
    assert render(alpha=float("nan")) == BADARG and render(thr=float("nan")) == BADARG
    assert render(hm=None, hm_thr=None) == BADARG and b"no output" in lib.hipt_last_error()
    assert render(use_thr=0) == BADARG   # the threshold picture without a threshold
    assert render(pct=None) == BADARG and render(patches=None) == BADARG and render(lut=None) == BADARG
    assert render(pct=0x1004) == BADARG and render(patches=0x2002) == BADARG and render(hm=0x4001) == BADARG and render(hm_thr=0x5002) == BADARG
    assert render(hm=0x2000) == BADARG and render(hm_thr=0x2000) == BADARG and render(hm=0x5000) == BADARG   # aliased buffers
    assert render(P=0) == 0 and render(P=0, pct=None, patches=None) == 0   # no patches: nothing to do


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    from matplotlib.colors import ListedColormap
    before = N.calls
    a256 = torch.zeros((3, 2, 6, 256))
    patches = np.zeros((3, 256, 256, 3), dtype=np.uint8)
    for bad in (-1, 257):
        with pytest.raises(ValueError, match="offset"):
            PH.compose_patch_heatmaps(a256, patches, offset=bad)
    with pytest.raises(ValueError, match="cols"):
        PH.compose_patch_heatmaps(a256, patches, concat=True, cols=0)
    with pytest.raises(ValueError, match="cols"):
        PH.compose_patch_heatmaps(a256, patches, concat=True, cols=N.HIER_MAX_HEADS + 1)
    with pytest.raises(ValueError, match="which"):
        PH.compose_patch_heatmaps(a256, patches, which=("4k",))
    with pytest.raises(ValueError, match="which"):
        PH.compose_patch_heatmaps(a256, patches, which=())
    with pytest.raises(ValueError, match="needs a threshold"):
        PH.compose_patch_heatmaps(a256, patches, which=("256th",))
    with pytest.raises(ValueError, match="NaN"):
        PH.compose_patch_heatmaps(a256, patches, alpha=float("nan"))
    with pytest.raises(ValueError, match="NaN"):
        PH.compose_patch_heatmaps(a256, patches, threshold=float("nan"))
    with pytest.raises(ValueError, match="float32"):
        PH.compose_patch_heatmaps(a256.double(), patches)
    with pytest.raises(ValueError, match="float32"):
        PH.compose_patch_heatmaps(a256.numpy(), patches)
    with pytest.raises(ValueError, match="a256 must be"):
        PH.compose_patch_heatmaps(a256[:, :1], patches)
    with pytest.raises(ValueError, match="a256 must be"):
        PH.compose_patch_heatmaps(a256[..., :255], patches)
    with pytest.raises(ValueError, match="heads"):
        PH.compose_patch_heatmaps(torch.zeros((3, 2, 9, 256)), patches)
    with pytest.raises(ValueError, match="patches must be"):
        PH.compose_patch_heatmaps(a256, patches[:2])
    with pytest.raises(ValueError, match="patches must be"):
        PH.compose_patch_heatmaps(a256, patches.astype(np.float32))
    with pytest.raises(ValueError, match="not a matplotlib colormap"):
        PH.compose_patch_heatmaps(a256, patches, cmap="no such colormap")
    with pytest.raises(ValueError, match="entries"):
        PH.compose_patch_heatmaps(a256, patches, cmap=ListedColormap(["r"]))
    with pytest.raises(ValueError, match="colour table"):
        PH.compose_patch_heatmaps(a256, patches, cmap=np.zeros((1, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="colour table"):
        PH.compose_patch_heatmaps(a256, patches, cmap=np.zeros((256, 4), dtype=np.uint8))
    nan = a256.clone()
    nan[1, 1, 2, 3] = float("nan")
    with pytest.raises(ValueError, match="contain NaN"):
        PH.compose_patch_heatmaps(nan, patches)
    with pytest.raises(RuntimeError, match="HIP device"):   # CPU tensors: there is no CPU path
        PH.compose_patch_heatmaps(a256, patches)
    with pytest.raises(ValueError, match="patches are uint8"):
        PH.patch_heatmaps(None, np.zeros((256, 128, 3), dtype=np.uint8))
    with pytest.raises(ValueError, match="no patches"):
        PH.patch_heatmaps(None, [])
    assert N.calls == before


def test_signatures_follow_the_reference_and_the_file_names_are_its(tmp_path, monkeypatch):
    for fn in (PH.create_patch_heatmaps_indiv, PH.create_patch_heatmaps_concat):
        params = inspect.signature(fn).parameters
        assert list(params)[:8] == ["patch", "model256", "output_dir", "fname", "threshold", "offset", "alpha", "cmap"] and "device256" in params
        assert (params["threshold"].default, params["offset"].default, params["alpha"].default) == (0.5, 16, 0.5)
    params = inspect.signature(PH.compose_patch_heatmaps).parameters
    assert list(params)[:9] == ["a256", "patches", "offset", "alpha", "cmap", "threshold", "concat", "cols", "out"]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(params)[2:])
    assert (params["offset"].default, params["alpha"].default, params["cmap"].default, params["threshold"].default,
            params["concat"].default, params["cols"].default, params["out"].default) == (16, 0.5, "coolwarm", None, False, 3, None)
    params = inspect.signature(HH.hierarchical_heatmaps_concat_select).parameters
    assert list(params)[:4] == ["hipt", "region", "heads4k", "heads256"] and params["heads4k"].default == (0, 5) and params["heads256"].default == (2,)

    # the files: the pictures come from a stand-in for the device route, the names and the PNG round trip are the functions' own
    import torch
    from PIL import Image
    rng = np.random.default_rng(8)
    calls = []

    def fake(model256, patch, offset=16, alpha=0.5, cmap="coolwarm", threshold=None, concat=False, cols=3, which=None):
        calls.append((threshold, concat, cols))
        shape = (512, 768, 3) if concat else (6, 256, 256, 3)
        res = {"256": torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))}
        if threshold is not None:
            res["256th"] = torch.from_numpy(rng.integers(0, 256, shape, dtype=np.uint8))
        fake.last = res
        return res
    monkeypatch.setattr(PH, "patch_heatmaps", fake)
    files = PH.create_patch_heatmaps_indiv(None, None, str(tmp_path), "p7", device256="cpu")
    names = ["p7_256th[%d].png" % i for i in range(6)] + ["p7_256[%d].png" % i for i in range(6)]
    assert [os.path.basename(f) for f in files] == names and sorted(os.listdir(tmp_path)) == sorted(names) and calls[-1] == (0.5, False, 3)
    for i in range(6):
        assert np.array_equal(np.array(Image.open(tmp_path / ("p7_256[%d].png" % i))), fake.last["256"][i].numpy())
        assert np.array_equal(np.array(Image.open(tmp_path / ("p7_256th[%d].png" % i))), fake.last["256th"][i].numpy())
    files = PH.create_patch_heatmaps_concat(None, None, str(tmp_path), "q", threshold=None)
    assert [os.path.basename(f) for f in files] == ["q_256hm.png"] and calls[-1] == (None, True, 3)
    files = PH.create_patch_heatmaps_concat(None, None, str(tmp_path), "q")
    assert [os.path.basename(f) for f in files] == ["q_256th.png", "q_256hm.png"]
    assert np.array_equal(np.array(Image.open(tmp_path / "q_256hm.png")), fake.last["256"].numpy())
    assert np.array_equal(np.array(Image.open(tmp_path / "q_256th.png")), fake.last["256th"].numpy())
