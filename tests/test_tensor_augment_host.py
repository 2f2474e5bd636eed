"""Host tests (no GPU) of the tensor-space augmentation (hipt_abmil_atec23_amd/tensor_augment.py, csrc/tensor_augment.hip):
the draw order, the two restatements against each other on the GPU tests' fixtures (the bar of the GPU colour test and the cap on
excused pixels are measured here, on the references alone), the record's layout, the C ABI and every refusal."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import tensor_augment_ref as R
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd import augment as A
from hipt_abmil_atec23_amd import tensor_augment as TA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BADARG, WORKSPACE = -1, -2
ENTRY_POINTS = ("hipt_augment_tensor_workspace_bytes", "hipt_augment_tensor")


# ---- draws ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", ["all", "spatial"])
def test_draw_order_is_torchvisions(policy):
    """rand, rand, uniform x 5, then for `all` randperm and uniform x 4, from one generator; 32 x 48: tx is drawn against the width"""
    rows, cols = 32, 48
    g = torch.Generator().manual_seed(4321)
    p = TA.draw_tensor_params(policy, g, rows, cols)
    after = torch.rand(1, generator=g)
    g = torch.Generator().manual_seed(4321)
    hf, vf = bool(torch.rand(1, generator=g) < 0.5), bool(torch.rand(1, generator=g) < 0.5)
    u = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=g).item())   # noqa: E731
    angle = u(-90.0, 90.0)
    tx, ty = int(round(u(-0.1 * cols, 0.1 * cols))), int(round(u(-0.1 * rows, 0.1 * rows)))
    scale, shear = u(0.9, 1.1), u(-0.1, 0.1)
    assert (p.hflip, p.vflip) == (hf, vf)
    assert p.draws["angle"] == angle and p.draws["translate"] == (tx, ty) and p.draws["scale"] == scale and p.draws["shear"] == (shear, 0.0)
    assert p.theta == tuple(A.inverse_affine_matrix([0.0, 0.0], angle, [float(tx), float(ty)], scale, (shear, 0.0)))
    if policy == "all":
        perm = torch.randperm(4, generator=g).tolist()
        b, c, s, h = u(0.9, 1.1), u(0.9, 1.1), u(0.9, 1.1), u(-0.1, 0.1)
        assert p.order == tuple(perm) and (p.brightness, p.contrast, p.saturation, p.hue) == (b, c, s, h)
    else:
        assert p.order == () and "perm" not in p.draws
    assert torch.equal(after, torch.rand(1, generator=g))   # the generator was consumed exactly so far


def test_translation_is_drawn_against_width_then_height():
    """over many regions of 32 x 48, |tx| reaches beyond what the height would allow and |ty| stays within it"""
    ps = TA.draw_tensor_region_params("spatial", 0, "s", 1, 0, 200, 32, 48)
    tx, ty = [abs(p.draws["translate"][0]) for p in ps], [abs(p.draws["translate"][1]) for p in ps]
    assert max(tx) in (4, 5) and max(ty) == 3


def test_draws_do_not_depend_on_batching_and_share_augments_seeds():
    a = TA.draw_tensor_region_params("all", 7, "s1", 2, 0, 9, 32, 48)
    parts = TA.draw_tensor_region_params("all", 7, "s1", 2, 0, 4, 32, 48) + TA.draw_tensor_region_params("all", 7, "s1", 2, 4, 5, 32, 48)
    assert [bytes(p.record()) for p in a] == [bytes(p.record()) for p in parts]
    assert [bytes(p.record()) for p in a] != [bytes(p.record()) for p in TA.draw_tensor_region_params("all", 7, "s1", 3, 0, 9, 32, 48)]
    g = torch.Generator().manual_seed(A.region_seed(7, "s1", 2, 5))
    assert bytes(TA.draw_tensor_params("all", g, 32, 48).record()) == bytes(a[5].record())
    with pytest.raises(ValueError, match="known"):
        TA.draw_tensor_params("HIPT_augment", torch.Generator(), 8, 8)
    # augment.py's own surface is as it was
    assert sorted(A.POLICIES) == sorted(["HIPT", "none", "HIPT_augment", "HIPT_augment01", "HIPT_augment_colour", "HIPT_wang", "HIPT_blur"])
    assert sorted(TA.TENSOR_POLICIES) == ["all", "spatial"]
    with pytest.raises(ValueError):
        A.draw_params("all", torch.Generator(), 8, 8)


# ---- the two restatements on the GPU tests' fixtures ---------------------------------------------------------------------------
def _cases(name):
    """(label, image, record) of a fixture: the drawn records of both policies and the hand-made ones"""
    imgs = R.fixture(name)
    n, H, W = R.FIXTURES[name]
    out = [(f"{pol}{i}", imgs[i], p) for pol in ("all", "spatial") for i, p in enumerate(R.drawn_records(pol, name))]
    out += [(lab, imgs[i % n], p) for i, (lab, p) in enumerate(R.spatial_records(H, W))]
    if n > 1:
        out += [(f"colour{i}", imgs[i % n], p) for i, p in enumerate(R.colour_records())]
    return out


# max |ref32 - ref64| over the non-excused pixels of a fixture's `all` / colour cases, as printed by
#   python -m pytest tests/test_tensor_augment_host.py -k restatements -s
# sq16 3.39e-06, ns32x48 4.09e-06, one256 3.24e-06 (the hue round trip and the division by std amplify the float32 roundings to some
# fifteen ulps of an output of at most 2.7).  The GPU test measures it again on the same cases and holds the kernel to 4 times it.
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_restatements_agree_and_few_pixels_are_excused(name):
    worst = 0.0
    for lab, img, p in _cases(name):
        a = R.ref32(img, p)
        b, ix, iy = R.ref64(img, p)
        ex = R.excused(ix, iy, img.shape[:2])
        assert ex.mean() <= R.EXCUSED_CAP, (lab, float(ex.mean()))
        if not p.order:
            # geometry only: float32 and float64 read the same source pixel off the boundaries, and the values are those of float32
            nb = None if ix is None else R.neighbour_values(img, p, ix, iy)
            same = np.abs(a - b) <= 1e-6
            assert same[:, ~ex].all(), lab
            if nb is not None:
                assert (a[None] == nb).all(1).any(0)[ex].all(), lab
        else:
            d = np.abs(a - b)[:, ~ex]
            worst = max(worst, float(d.max()))
            assert d.max() < 1e-4, (lab, float(d.max()))   # (sanity: far below one 8-bit level / std = 1.7e-2)
    print(f"{name}: max |ref32 - ref64| off the excused pixels = {worst:.3g}")


def test_quarter_turns_are_off_the_boundaries_on_the_non_square_fixture():
    """an exact quarter turn of 32 x 48 (W - H even) reads pixel centres: nothing is excused, most of the output is padding"""
    img = R.fixture("ns32x48")[0]
    for lab, p in R.quarter_turn_records():
        out, ix, iy = R.ref64(img, p)
        assert not R.excused(ix, iy, img.shape[:2]).any(), lab
        pad = (ix < -0.5) | (ix > 47.5) | (iy < -0.5) | (iy > 31.5)
        assert 0.3 < pad.mean() < 0.4 and np.array_equal(R.ref32(img, p)[:, pad], np.broadcast_to(pad_value()[:, None], (3, int(pad.sum()))))


def pad_value():
    return ((torch.zeros(3) - torch.tensor(R.MEAN)) / torch.tensor(R.STD)).numpy()


def test_injected_defects_exceed_the_bar_by_a_wide_factor():
    """What the GPU colour test would see of a wrong kernel: ref32 with a defect against ref64, over the bar 4 x max |ref32 - ref64|.
    Three of the five defects are far over it.  The other two cannot be seen by ANY test of the output, for a stated reason: without
    ``% 1`` the hue is off by a whole turn at most, and ``i % 6`` with ``f = 6h - floor(6h)`` is periodic in it; q and t are
    v (1 - s f) and v (1 - s (1 - f)) with s, f in [0, 1], so their clamp never acts.  They stay in the list and are held to the bar."""
    img = R.fixture("ns32x48")
    base, worst = 0.0, {d: 0.0 for d in R.DEFECTS}
    for i, p in enumerate(R.colour_records()):
        b, ix, iy = R.ref64(img[i % 3], p)
        keep = ~R.excused(ix, iy, (32, 48))
        base = max(base, float(np.abs(R.ref32(img[i % 3], p) - b)[:, keep].max()))
        for d in R.DEFECTS:
            worst[d] = max(worst[d], float(np.abs(R.ref32(img[i % 3], p, defect=d) - b)[:, keep].max()))
    factors = {d: worst[d] / (4 * base) for d in R.DEFECTS}
    print("defect factors over the bar:", {d: round(f, 2) for d, f in factors.items()})
    assert all(factors[d] > 100 for d in ("mean_early", "gray_perm", "norm_swapped")), factors
    assert all(factors[d] <= 1 for d in ("hue_nomod", "no_clamp_qt")), factors


# ---- the record and the C ABI --------------------------------------------------------------------------------------------------
def test_record_layout_matches_the_header_as_gcc_sees_it(tmp_path):
    cls = TA.TensorAugmentParams
    lines = ['printf("size %zu\\n", sizeof(hipt_tensor_augment_params));']
    lines += [f'printf("{f} %zu\\n", offsetof(hipt_tensor_augment_params, {f}));' for f, _ in cls._fields_]
    lines += ['printf("old %zu\\n", sizeof(hipt_augment_params));']
    src = tmp_path / "ta_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hipt_abmil.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "ta_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls) == 96 and C.sizeof(cls) % 8 == 0
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert int(got["old"]) == C.sizeof(A.AugmentParams)   # the uint8 kernel's record is untouched
    p = TA.TensorRegionParams(hflip=True, theta=(1.0, 0.25, -3.0, 0.5, 1.0, 2.0), order=(3, 1), contrast=1.05, hue=-0.1).record()
    assert p.flags == A.HFLIP | A.AFFINE and list(p.theta) == [1.0, 0.25, -3.0, 0.5, 1.0, 2.0] and p.n_ops == 2 and list(p.ops)[:2] == [3, 1]
    assert [np.float32(v) for v in p.mean] == [np.float32(v) for v in TA.IMAGENET_MEAN] and p.hue == np.float32(-0.1)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    lib = N.lib()
    for name in ENTRY_POINTS:
        decl = re.search(r"\b(?:int|size_t) %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(N.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and lib.hipt_abi_version() == N.ABI_VERSION == 6
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\btensor_augment\.hip\b", mk, re.M) and "FLAGS_tensor_augment.hip = -ffp-contract=off" in mk
    import hipt_abmil_atec23_amd as amd
    for name in ("TENSOR_POLICIES", "draw_tensor_params", "augment_tensor", "TensorAugment"):
        assert getattr(amd, name) is getattr(TA, name)


def al256(v):
    return (v + 255) & ~255


def test_workspace_bytes_is_one_partial_per_workgroup():
    lib = N.lib()
    for n, h, w in [(1, 1, 1), (3, 16, 16), (3, 32, 48), (1, 256, 256), (256, 256, 256), (2, 1024, 1024), (1, 4096, 4096)]:
        parts = min(-(-(h * w) // 1024), 256)
        assert lib.hipt_augment_tensor_workspace_bytes(n, h, w) == al256(8 * n * parts)
    assert lib.hipt_augment_tensor_workspace_bytes(0, 8, 8) == 0 and lib.hipt_augment_tensor_workspace_bytes(1, 0, 8) == 0
    assert lib.hipt_augment_tensor_workspace_bytes(1, 8, -1) == 0 and lib.hipt_augment_tensor_workspace_bytes(1, 1 << 16, 1 << 15) == 0


def test_library_refuses_without_launching():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    src, dst, prm, ws = 0x100000, 0x200000, 0x300000, 0x400000
    need = lib.hipt_augment_tensor_workspace_bytes(3, 32, 48)
    assert need > 0

    def call(src=src, n=3, hw=(32, 48), prm=prm, dst=dst, ws=ws, ws_bytes=need, il=0):
        return lib.hipt_augment_tensor(src, il, n, hw[0], hw[1], prm, dst, ws, ws_bytes, None)

    assert call(src=None) == BADARG and call(dst=None) == BADARG and call(prm=None) == BADARG
    assert call(n=0) == BADARG and call(n=-1) == BADARG and call(hw=(0, 48)) == BADARG and call(hw=(32, -1)) == BADARG
    assert call(hw=(1 << 16, 1 << 15)) == BADARG and b"2^30" in lib.hipt_last_error()
    assert call(dst=dst + 2) == BADARG and call(prm=prm + 1) == BADARG and b"alignment" in lib.hipt_last_error()
    assert call(dst=src) == BADARG and b"overlap" in lib.hipt_last_error()
    assert call(dst=src + 3 * 3 * 32 * 48 - 4) == BADARG and call(src=dst + 4 * 3 * 3 * 32 * 48 - 1) == BADARG
    for il in (0, 1):
        assert call(ws_bytes=need - 1, il=il) == WORKSPACE
        msg = lib.hipt_last_error().decode()
        assert msg.startswith("augment_tensor: workspace") and str(need - 1) in msg and str(need) in msg and "too small / unaligned" in msg
        assert call(ws=ws + 16, il=il) == WORKSPACE and call(ws=ws + 16, ws_bytes=need + 4096, il=il) == WORKSPACE
    assert call(ws=None) == BADARG and b"workspace missing" in lib.hipt_last_error()   # (NULL with 0 bytes is the one-launch route)


def test_python_layer_refuses_bad_requests_before_any_native_call():
    before = N.calls
    x = torch.zeros((2, 3, 8, 8), dtype=torch.uint8)
    ps = [TA.TensorRegionParams()] * 2
    with pytest.raises(ValueError, match="uint8"):
        TA.augment_tensor(x.float(), ps)
    with pytest.raises(ValueError, match="uint8"):
        TA.augment_tensor(np.zeros((2, 3, 8, 8), np.uint8), ps)
    with pytest.raises(ValueError, match="batch"):
        TA.augment_tensor(torch.zeros((2, 4, 8, 8), dtype=torch.uint8), ps)
    with pytest.raises(ValueError, match="batch"):
        TA.augment_tensor(x[0], ps[:1])
    with pytest.raises(ValueError, match="parameter records"):
        TA.augment_tensor(x, ps[:1])
    with pytest.raises(ValueError, match="std"):
        TA.augment_tensor(x, ps, std=(1.0, 0.0, 1.0))
    with pytest.raises(ValueError, match="mean"):
        TA.augment_tensor(x, ps, mean=(1.0, 2.0))
    with pytest.raises(ValueError, match="HIP device"):   # a CPU tensor: there is no CPU path
        TA.augment_tensor(x, ps)
    with pytest.raises(ValueError, match="HIP device"):
        TA.TensorAugment("all", 0)(x.permute(0, 2, 3, 1).contiguous(), "s", 1, 0)
    with pytest.raises(ValueError, match="known"):
        TA.TensorAugment("HIPT_wang")
    with pytest.raises(ValueError, match="uint8"):   # augment.py's refusal of float input is as it was
        A.augment_regions(torch.zeros(1, 3, 16, 16), [A.RegionParams()])
    assert N.calls == before


class _Stub:
    """stands in for a model: extract_slide_augmented must not reach it on the CPU"""
    def __call__(self, x):
        raise AssertionError("the model was called")


def test_extract_slide_augmented_routes_the_tensor_policies(tmp_path):
    from hipt_abmil_atec23_amd.feature_store import extract_slide_augmented
    batch = [(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), torch.zeros((1, 2), dtype=torch.int64))]
    for policy in ("spatial", "all"):
        with pytest.raises(ValueError, match="HIP device"):   # past the policy check, at the device check of the augmentation
            extract_slide_augmented(_Stub(), batch, str(tmp_path / policy), "s", policy, 1, include_original=False, coalesce=1)
    with pytest.raises(ValueError, match=r"unknown augmentation policy 'spatia'.*HIPT_wang.*spatial"):
        extract_slide_augmented(_Stub(), batch, str(tmp_path / "x"), "s", "spatia", 1)
    with pytest.raises(ValueError, match="uint8"):   # float regions are refused for both families
        extract_slide_augmented(_Stub(), [(batch[0][0].float(), batch[0][1])], str(tmp_path / "f"), "s", "all", 1, include_original=False,
                                coalesce=1)
