"""HIPT_* region augmentation (hipt_abmil_atec23_amd/augment.py, csrc/augment.hip).

The numpy restatement below is the yardstick: on the CPU it is checked against Pillow (the library torchvision calls for
PIL images) bit for bit, primitive by primitive and policy by policy, and on the GPU the kernel is checked against it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance

from hipt_abmil_atec23_amd import augment as A
from hipt_abmil_atec23_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
f32, f64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------
# restatement (HWC uint8 images; width = cols)
# ---------------------------------------------------------------------------------------------------------------------
def ref_lum(img):
    i = img.astype(np.int64)
    return ((i[..., 0] * 19595 + i[..., 1] * 38470 + i[..., 2] * 7471 + 0x8000) >> 16).astype(np.int64)


def ref_blend(d, img, f):
    t = f32(d).astype(f32) + f32(f) * (img.astype(f32) - np.asarray(d, dtype=f32))
    return np.clip(np.trunc(t), 0, 255).astype(np.uint8)


def ref_rgb2hsv(rgb):
    r, g, b = (rgb[..., i].astype(np.int32) for i in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    cr = (mx - mn).astype(f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = cr / mx.astype(f32)
        rc, gc, bc = ((mx - c).astype(f32) / cr for c in (r, g, b))
    h = np.where(r == mx, (bc - gc).astype(f32),
                 np.where(g == mx, ((2.0 + rc.astype(f64)) - bc.astype(f64)).astype(f32), ((4.0 + gc.astype(f64)) - rc.astype(f64)).astype(f32)))
    h = np.fmod(h.astype(f64) / 6.0 + 1.0, 1.0).astype(f32)
    with np.errstate(invalid="ignore"):
        uh = np.clip(np.trunc(h.astype(f64) * 255.0), 0, 255)
        us = np.clip(np.trunc(s.astype(f64) * 255.0), 0, 255)
    eq = mx == mn
    return np.stack([np.where(eq, 0, uh).astype(np.uint8), np.where(eq, 0, us).astype(np.uint8), mx.astype(np.uint8)], -1)


def ref_hsv2rgb(hsv):
    h, s, v = (hsv[..., i].astype(np.int32) for i in range(3))
    hh = h.astype(f32).astype(f64) * 6.0 / 255.0
    i = np.floor(hh)
    f = (hh - i.astype(f32).astype(f64)).astype(f32)
    fs = (s.astype(f32).astype(f64) / 255.0).astype(f32)
    vv = v.astype(f32).astype(f64)
    rnd = lambda x: np.clip(np.sign(x) * np.floor(np.abs(x) + 0.5), 0, 255).astype(np.uint8)  # C round(): half away from 0
    p = rnd(vv * (1.0 - fs.astype(f64)))
    q = rnd(vv * (1.0 - (fs * f).astype(f64)))
    t = rnd(vv * (1.0 - fs.astype(f64) * (1.0 - f.astype(f64))))
    vu = v.astype(np.uint8)
    sel = [(vu, t, p), (q, vu, p), (p, vu, t), (p, q, vu), (t, p, vu), (vu, p, q)]
    ii = i.astype(np.int64) % 6
    out = np.zeros(h.shape + (3,), np.uint8)
    for k, trip in enumerate(sel):
        m = ii == k
        out[m] = np.stack([c[m] for c in trip], -1)
    z = s == 0
    out[z] = np.stack([vu[z]] * 3, -1)
    return out


def ref_hue(img, shift):
    hsv = ref_rgb2hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + shift) % 256).astype(np.uint8)
    return ref_hsv2rgb(hsv)


def ref_affine(img, m):
    """Pillow transform(AFFINE, NEAREST, fill 0): 16.16 fixed point, or the exact-scale path when a1 == a3 == 0"""
    rows, cols = img.shape[:2]
    out = np.zeros_like(img)
    if m[1] == 0 and m[3] == 0:  # ImagingScaleAffine: positions accumulated in double, one addition per pixel
        xs = np.add.accumulate(np.array([m[2] + m[0] * 0.5] + [m[0]] * (cols - 1), dtype=f64))
        ys = np.add.accumulate(np.array([m[5] + m[4] * 0.5] + [m[4]] * (rows - 1), dtype=f64))
        xi = np.where(xs < 0, -1, np.trunc(np.where(xs < 0, 0, xs))).astype(np.int64)
        yi = np.where(ys < 0, -1, np.trunc(np.where(ys < 0, 0, ys))).astype(np.int64)
        yi, xi = np.meshgrid(yi, xi, indexing="ij")
    else:
        fix = lambda v: int(np.floor(v * 65536.0 + 0.5))
        a0, a1, a3, a4 = fix(m[0]), fix(m[1]), fix(m[3]), fix(m[4])
        xo, yo = fix(m[2] + m[1] * 0.5 + m[0] * 0.5), fix(m[5] + m[4] * 0.5 + m[3] * 0.5)
        y, x = np.meshgrid(np.arange(rows, dtype=np.int64), np.arange(cols, dtype=np.int64), indexing="ij")
        xi = (xo + y * a1 + x * a0) >> 16
        yi = (yo + y * a4 + x * a3) >> 16
    ok = (xi >= 0) & (xi < cols) & (yi >= 0) & (yi < rows)
    out[ok] = img[yi[ok], xi[ok]]
    return out


def ref_blur(img, w):
    """GaussianBlur((1,3)): torchvision's tensor path on the uint8 planes, restated (vertical taps, reflect padding, float32,
    round half to even)"""
    x = img.astype(f32)
    up = np.concatenate([x[1:2], x[:-1]], 0)
    dn = np.concatenate([x[1:], x[-2:-1]], 0)
    acc = (f32(w[0]) * up + f32(w[1]) * x) + f32(w[2]) * dn
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def ref_apply(img, p: A.RegionParams):
    if p.blur_sigma is not None:
        return ref_blur(img, A.blur_weights(p.blur_sigma))
    x = img
    if p.hflip:
        x = x[:, ::-1]
    if p.vflip:
        x = x[::-1]
    if p.affine is not None:
        x = ref_affine(np.ascontiguousarray(x), p.affine)
    for op in p.order:
        if op == A.OP_BRIGHTNESS:
            x = ref_blend(0, x, p.brightness)
        elif op == A.OP_CONTRAST:
            x = ref_blend(int(float(ref_lum(x).sum()) / ref_lum(x).size + 0.5), x, p.contrast)
        elif op == A.OP_SATURATION:
            x = ref_blend(ref_lum(x)[..., None], x, p.saturation)
        elif op == A.OP_HUE:
            x = ref_hue(x, p.hue_shift)
    return np.ascontiguousarray(x)


def pil_apply(img, p: A.RegionParams):
    """what torchvision's transforms do to a PIL image with these parameters"""
    x = Image.fromarray(img)
    if p.hflip:
        x = x.transpose(Image.Transpose.FLIP_LEFT_RIGHT)
    if p.vflip:
        x = x.transpose(Image.Transpose.FLIP_TOP_BOTTOM)
    if p.affine is not None:
        x = x.transform(x.size, Image.Transform.AFFINE, list(p.affine), Image.Resampling.NEAREST, fillcolor=(0, 0, 0))
    for op in p.order:
        if op == A.OP_BRIGHTNESS:
            x = ImageEnhance.Brightness(x).enhance(p.brightness)
        elif op == A.OP_CONTRAST:
            x = ImageEnhance.Contrast(x).enhance(p.contrast)
        elif op == A.OP_SATURATION:
            x = ImageEnhance.Color(x).enhance(p.saturation)
        elif op == A.OP_HUE:
            h, s, v = x.convert("HSV").split()
            nh = np.array(h, dtype=np.uint8)
            nh += np.uint8(p.hue_shift)  # (wraps, as np.array(hue * 255).astype(np.uint8) does on x86)
            x = Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB")
    return np.asarray(x)


def torch_blur(img, sigma):
    """torchvision F_t.gaussian_blur's op sequence, on torch (kernel_size (1, 3))"""
    t = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1)[None].float()
    k = torch.tensor(A.blur_weights(sigma), dtype=torch.float32)[:, None]  # [3, 1]: ky x kx
    k = k.expand(3, 1, 3, 1)
    t = torch.nn.functional.pad(t, [0, 0, 1, 1], mode="reflect")
    t = torch.nn.functional.conv2d(t, k, groups=3)
    return torch.round(t)[0].permute(1, 2, 0).to(torch.uint8).numpy()


def rand_img(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, (rows, cols, 3), dtype=np.uint8)


def primitive_cases(rows, cols):
    """(name, RegionParams): each primitive alone, the edge cases of the affine"""
    c = [rows * 0.5, cols * 0.5][::-1]
    M = lambda ang, t=(0, 0), sc=1.0, sh=0.0: tuple(A.inverse_affine_matrix(c, ang, t, sc, (sh, 0.0)))
    return [
        ("identity", A.RegionParams()),
        ("hflip", A.RegionParams(hflip=True)),
        ("vflip", A.RegionParams(vflip=True)),
        ("hvflip", A.RegionParams(hflip=True, vflip=True)),
        ("affine", A.RegionParams(affine=M(3.7, (5, -4), 1.013, 0.021))),
        ("affine_neg", A.RegionParams(affine=M(-4.2, (-3, 2), 0.981, -0.017))),
        ("rot+90", A.RegionParams(affine=M(90.0))),
        ("rot-90", A.RegionParams(affine=M(-90.0))),
        ("rot63", A.RegionParams(affine=M(63.3))),
        ("scale_path", A.RegionParams(affine=M(0.0, (3, -2), 1.0173))),
        ("scale_path_shrink", A.RegionParams(affine=M(0.0, (-1, 1), 0.9771))),
        ("translate_out", A.RegionParams(affine=M(2.0, (cols + 10, -rows // 3), 1.0))),
        ("brightness", A.RegionParams(order=(A.OP_BRIGHTNESS,), brightness=1.1734)),
        ("brightness_lo", A.RegionParams(order=(A.OP_BRIGHTNESS,), brightness=0.8123)),
        ("contrast", A.RegionParams(order=(A.OP_CONTRAST,), contrast=1.1621)),
        ("contrast_lo", A.RegionParams(order=(A.OP_CONTRAST,), contrast=0.8351)),
        ("saturation", A.RegionParams(order=(A.OP_SATURATION,), saturation=1.19)),
        ("saturation_lo", A.RegionParams(order=(A.OP_SATURATION,), saturation=0.81)),
        ("hue+", A.RegionParams(order=(A.OP_HUE,), hue=0.137)),
        ("hue-", A.RegionParams(order=(A.OP_HUE,), hue=-0.1)),
        ("affine+contrast", A.RegionParams(hflip=True, affine=M(-61.0), order=(A.OP_SATURATION, A.OP_CONTRAST), saturation=1.1,
                                           contrast=1.15)),
    ]


def policy_draws(policy, rows, cols, n, seed=0):
    return A.draw_region_params(policy, seed, "slideX", 1, 0, n, rows, cols)


POLICY_NAMES = ["HIPT_augment", "HIPT_augment01", "HIPT_augment_colour", "HIPT_wang", "HIPT_blur", "HIPT", "none"]


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the restatement against Pillow; draws; ABI; load_bag
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(200, 312), (1024, 1536), (97, 61)])
def test_primitives_match_pillow(rows, cols):
    img = rand_img(rows, cols, rows + cols)
    img[: rows // 4] //= 3  # (a darker band: the contrast mean is not 127)
    for name, p in primitive_cases(rows, cols):
        got, want = ref_apply(img, p), pil_apply(img, p)
        assert got.shape == want.shape and np.array_equal(got, want), f"{name}: {int((got != want).any(-1).sum())} pixels differ"


def test_scale_path_is_taken_and_differs_from_fixed_point():
    """angle 0 takes Pillow's separate scale path: the restatement follows it (and the fixed-point formula would not)"""
    rows, cols = 300, 448
    img = rand_img(rows, cols, 5)
    m = A.inverse_affine_matrix([cols * 0.5, rows * 0.5], 0.0, (2, -3), 1.0213, (0.0, 0.0))
    assert m[1] == 0 and m[3] == 0
    assert np.array_equal(ref_affine(img, m), pil_apply(img, A.RegionParams(affine=tuple(m))))


@pytest.mark.parametrize("rows,cols", [(200, 312), (1024, 1536)])
@pytest.mark.parametrize("policy", [p for p in POLICY_NAMES if p != "HIPT_blur"])
def test_policies_match_pillow(policy, rows, cols):
    img = rand_img(rows, cols, 11)
    for i, p in enumerate(policy_draws(policy, rows, cols, 4 if rows < 1000 else 2)):
        assert np.array_equal(ref_apply(img, p), pil_apply(img, p)), f"{policy} draw {i}: {p}"


@pytest.mark.parametrize("rows,cols", [(200, 312), (64, 33)])
def test_blur_restatement_matches_torch_gaussian_blur(rows, cols):
    img = rand_img(rows, cols, 3)
    for p in policy_draws("HIPT_blur", rows, cols, 3):
        d = np.abs(ref_blur(img, A.blur_weights(p.blur_sigma)).astype(int) - torch_blur(img, p.blur_sigma).astype(int))
        assert d.max() <= 1, p.blur_sigma


def test_hsv_round_trip_with_hue_shifts_is_exhaustive():
    """every RGB colour once (4096 x 4096): Pillow's RGB -> HSV, and HSV -> RGB after shifts of both signs"""
    c = np.arange(1 << 24, dtype=np.uint32)
    img = np.stack([(c >> 16) & 255, (c >> 8) & 255, c & 255], -1).astype(np.uint8).reshape(4096, 4096, 3)
    hsv = np.asarray(Image.fromarray(img).convert("HSV"))
    assert np.array_equal(ref_rgb2hsv(img), hsv)
    for hue in (0.0, 0.1, -0.1, 0.2, -0.2, 0.5, -0.5):
        shift = A.RegionParams(hue=hue).hue_shift
        h2 = hsv.copy()
        h2[..., 0] = ((h2[..., 0].astype(np.int32) + shift) % 256).astype(np.uint8)
        want = np.asarray(Image.fromarray(h2, "HSV").convert("RGB"))
        assert np.array_equal(ref_hsv2rgb(h2), want), hue
    assert A.RegionParams(hue=-0.1).hue_shift == 231


def test_draws_are_deterministic_in_range_and_batch_independent():
    rows, cols = 4096, 3072
    for policy in POLICY_NAMES:
        a = A.draw_region_params(policy, 7, "s1", 2, 0, 12, rows, cols)
        b = A.draw_region_params(policy, 7, "s1", 2, 0, 12, rows, cols)
        parts = A.draw_region_params(policy, 7, "s1", 2, 0, 5, rows, cols) + A.draw_region_params(policy, 7, "s1", 2, 5, 7, rows, cols)
        assert [bytes(p.record()) for p in a] == [bytes(p.record()) for p in b] == [bytes(p.record()) for p in parts], policy
        other = A.draw_region_params(policy, 7, "s1", 3, 0, 12, rows, cols)
        if A.POLICIES[policy] is not None:
            assert [bytes(p.record()) for p in a] != [bytes(p.record()) for p in other], policy
        spec = A.POLICIES[policy] or {}
        for p in a:
            d = p.draws
            if "affine" in spec:
                af = spec["affine"]
                assert af["degrees"][0] <= d["angle"] <= af["degrees"][1]
                if af["translate"] is not None:
                    assert abs(d["translate"][0]) <= round(0.025 * cols) and abs(d["translate"][1]) <= round(0.025 * rows)
                    assert 0.975 <= d["scale"] <= 1.025 and abs(d["shear"][0]) <= 0.025
            if "jitter" in spec:
                b_, c_, s_, h_ = spec["jitter"]
                assert sorted(d["perm"]) == [0, 1, 2, 3]
                assert b_[0] <= p.brightness <= b_[1] and c_[0] <= p.contrast <= c_[1] and s_[0] <= p.saturation <= s_[1]
                assert (h_ is None and A.OP_HUE not in p.order) or (h_ is not None and h_[0] <= p.hue <= h_[1])
            if "blur" in spec:
                assert 7.0 <= p.blur_sigma <= 9.0
    # the stable hash: not Python's hash(), pinned value
    assert A.region_seed(0, "slide", 1, 0) == A.region_seed(0, "slide", 1, 0) != A.region_seed(0, "slide", 1, 1)
    with pytest.raises(ValueError):
        A.draw_params("HIPT_macenko", torch.Generator(), 64, 64)


def test_draw_order_is_torchvisions():
    """flips, then angle / tx / ty / scale / shear, then randperm(4) and the factors, from one generator"""
    g = torch.Generator().manual_seed(1234)
    p = A.draw_params("HIPT_augment", g, 400, 200)
    g = torch.Generator().manual_seed(1234)
    hf, vf = bool(torch.rand(1, generator=g) < 0.5), bool(torch.rand(1, generator=g) < 0.5)
    u = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=g).item())
    angle = u(-5.0, 5.0)
    tx, ty = int(round(u(-0.025 * 200, 0.025 * 200))), int(round(u(-0.025 * 400, 0.025 * 400)))
    scale, shear = u(0.975, 1.025), u(-0.025, 0.025)
    perm = torch.randperm(4, generator=g).tolist()
    b, c, s, h = u(0.8, 1.2), u(0.8, 1.2), u(0.8, 1.2), u(-0.2, 0.2)
    assert (p.hflip, p.vflip) == (hf, vf)
    assert p.draws["angle"] == angle and p.draws["translate"] == (tx, ty) and p.draws["scale"] == scale and p.draws["shear"][0] == shear
    assert p.order == tuple(perm) and (p.brightness, p.contrast, p.saturation, p.hue) == (b, c, s, h)
    assert p.affine == tuple(A.inverse_affine_matrix([100.0, 200.0], angle, (tx, ty), scale, (shear, 0.0)))


def test_float_regions_are_refused():
    with pytest.raises(ValueError, match="uint8"):
        A.augment_regions(torch.zeros(1, 3, 16, 16), [A.RegionParams()])


def test_augment_struct_layout_matches_the_header_as_gcc_sees_it(tmp_path):
    cls = A.AugmentParams
    lines = [f'printf("size %zu\\n", sizeof(hipt_augment_params));']
    lines += [f'printf("{f} %zu\\n", offsetof(hipt_augment_params, {f}));' for f, _ in cls._fields_]
    lines += ['printf("HFLIP %d\\nVFLIP %d\\nAFFINE %d\\nBLUR %d\\n", HIPT_AUG_HFLIP, HIPT_AUG_VFLIP, HIPT_AUG_AFFINE, HIPT_AUG_BLUR);',
              'printf("BR %d\\nCO %d\\nSA %d\\nHU %d\\n", HIPT_AUG_BRIGHTNESS, HIPT_AUG_CONTRAST, HIPT_AUG_SATURATION, HIPT_AUG_HUE);']
    src = tmp_path / "aug_layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hipt_abmil.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0; }\n")
    exe = tmp_path / "aug_layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    assert [int(got[k]) for k in ("HFLIP", "VFLIP", "AFFINE", "BLUR")] == [A.HFLIP, A.VFLIP, A.AFFINE, A.BLUR]
    assert [int(got[k]) for k in ("BR", "CO", "SA", "HU")] == [A.OP_BRIGHTNESS, A.OP_CONTRAST, A.OP_SATURATION, A.OP_HUE]
    from hipt_abmil_atec23_amd import _native as N
    assert "hipt_augment_regions" in N.SIGNATURES and "hipt_augment_workspace_bytes" in N.SIGNATURES


def test_load_bag_augmentation_and_perturbation(tmp_path):
    from hipt_abmil_atec23_amd.feature_store import FeatureWriter, load_bag
    feats = {}
    for k, name in enumerate(["s", "saug1", "saug2"]):
        w = FeatureWriter(str(tmp_path), name, write_h5=False)
        feats[k] = torch.full((6, 4), float(k))
        w.append(feats[k], np.zeros((6, 2), np.int64))
        w.close()
    # defaults: today's behaviour (the plain file, no noise)
    assert torch.equal(load_bag(str(tmp_path), "s"), feats[0])
    assert torch.equal(load_bag(str(tmp_path), "s", rng=np.random.default_rng(0)), feats[0])
    # number_of_augs: k uniform in [0, n] (k = 0: the plain file), with a numpy Generator, a RandomState and Python's random
    seen = set()
    for rng in (np.random.default_rng(3), np.random.RandomState(3)):
        for _ in range(60):
            seen.add(int(load_bag(str(tmp_path), "s", number_of_augs=2, rng=rng)[0, 0]))
    import random
    random.seed(0)
    for _ in range(30):
        seen.add(int(load_bag(str(tmp_path), "s", number_of_augs=2)[0, 0]))
    assert seen == {0, 1, 2}
    # perturb_variance: randn_like * variance added (after sub-sampling)
    torch.manual_seed(5)
    got = load_bag(str(tmp_path), "s", perturb_variance=0.25)
    torch.manual_seed(5)
    assert torch.equal(got, feats[0] + torch.randn_like(feats[0]) * 0.25)
    sub = load_bag(str(tmp_path), "s", max_patches_per_slide=3, rng=np.random.default_rng(1), perturb_variance=0.0)
    assert sub.shape == (3, 4) and torch.equal(sub, torch.zeros(3, 4))


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the kernel against the restatement; extract_slide_augmented
# ---------------------------------------------------------------------------------------------------------------------
def _to_dev(imgs, interleaved):
    t = torch.from_numpy(np.stack(imgs))
    return (t if interleaved else t.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _from_dev(t, interleaved):
    t = t.cpu()
    return (t if interleaved else t.permute(0, 2, 3, 1)).contiguous().numpy()


def _check(imgs, params, interleaved, tol=0):
    got = _from_dev(A.augment_regions(_to_dev(imgs, interleaved), params), interleaved)
    for i, (img, p) in enumerate(zip(imgs, params)):
        want = ref_apply(img, p)
        d = np.abs(got[i].astype(int) - want.astype(int))
        assert d.max() <= tol, f"region {i} ({p}): {int((d > tol).any(-1).sum())} pixels off, max {d.max()}"


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("rows,cols", [(256, 512), (200, 312), (67, 45), (1024, 1536)])
def test_kernel_primitives_bit_exact(interleaved, rows, cols):
    cases = primitive_cases(rows, cols)
    imgs = [rand_img(rows, cols, 100 + i) for i in range(len(cases))]
    _check(imgs, [p for _, p in cases], interleaved)


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("rows,cols", [(512, 768), (200, 312), (33, 70)])
def test_kernel_policies_bit_exact(interleaved, rows, cols):
    for policy in POLICY_NAMES:
        params = policy_draws(policy, rows, cols, 6, seed=9)
        imgs = [rand_img(rows, cols, 200 + i) for i in range(len(params))]
        _check(imgs, params, interleaved, tol=1 if policy == "HIPT_blur" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True])
def test_kernel_blur_within_one_lsb_of_torch(interleaved):
    rows, cols = 160, 208
    params = policy_draws("HIPT_blur", rows, cols, 3)
    imgs = [rand_img(rows, cols, 300 + i) for i in range(3)]
    got = _from_dev(A.augment_regions(_to_dev(imgs, interleaved), params), interleaved)
    for g, img, p in zip(got, imgs, params):
        assert np.abs(g.astype(int) - torch_blur(img, p.blur_sigma).astype(int)).max() <= 1


@pytest.mark.gpu
@pytest.mark.parametrize("interleaved", [False, True])
def test_identity_records_copy_the_bytes(interleaved):
    for rows, cols in ((256, 256), (131, 77)):
        x = _to_dev([rand_img(rows, cols, 7 + i) for i in range(3)], interleaved)
        for policy in ("HIPT", "none"):
            assert torch.equal(A.RegionAugment(policy, 0)(x, "s", 1, 0), x)
        assert torch.equal(A.augment_regions(x, [A.RegionParams()] * 3), x)


@pytest.mark.gpu
def test_same_bits_alone_in_a_batch_and_on_two_streams():
    rows, cols = 512, 512
    aug = A.RegionAugment("HIPT_augment", 3)
    x = _to_dev([rand_img(rows, cols, 40 + i) for i in range(8)], True)
    batch = aug(x, "slide", 1, 0)
    alone = torch.cat([aug(x[i:i + 1], "slide", 1, i) for i in range(8)])
    assert torch.equal(batch, alone)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        a = aug(x[:4], "slide", 1, 0)
    with torch.cuda.stream(s2):
        b = aug(x[4:], "slide", 1, 4)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([a, b]), batch)


@pytest.fixture(scope="module")
def hipt():
    from hipt_abmil_atec23_amd import HIPT_4K
    m = HIPT_4K(None, None, DEV, DEV)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(DEV)
    m.set_compute_dtype("bf16")
    return m


@pytest.mark.gpu
def test_extract_slide_augmented_files(hipt, tmp_path):
    from hipt_abmil_atec23_amd.feature_store import extract_slide, extract_slide_augmented, load_coords
    n, rows, cols, n_augs = 6, 1024, 1024, 2
    regs = [torch.from_numpy(rand_img(rows, cols, 500 + i))[None].to(DEV) for i in range(n)]  # interleaved [1, rows, cols, 3]
    coords = [torch.tensor([[cols * i, 3 * i]], dtype=torch.int64) for i in range(n)]
    plain = torch.load(extract_slide(hipt, list(zip(regs, coords)), str(tmp_path / "plain"), "s", coalesce=4))
    files = {}
    for mem in ("resident", "host"):
        for co in (1, 8):
            b = regs if mem == "resident" else [r.cpu() for r in regs]
            d = str(tmp_path / f"{mem}{co}")
            paths = extract_slide_augmented(hipt, list(zip(b, coords)), d, "s", "HIPT_augment", n_augs, seed=5, coalesce=co)
            assert [os.path.basename(p) for p in paths] == ["s.pt", "saug1.pt", "saug2.pt"]
            files[(mem, co)] = [torch.load(p) for p in paths]
            for sid in ("s", "saug1", "saug2"):
                assert np.array_equal(load_coords(d, sid), torch.cat(coords).numpy())
    ref = files[("resident", 8)]
    assert torch.equal(ref[0], plain)
    for key, got in files.items():
        for a, b in zip(got, ref):
            assert torch.equal(a, b), key
    with torch.no_grad():
        x = torch.cat(regs)
        for k in range(1, n_augs + 1):
            params = A.draw_region_params("HIPT_augment", 5, "s", k, 0, n, rows, cols)
            want = torch.cat([hipt(A.augment_regions(x[i:i + 1], params[i:i + 1])) for i in range(n)]).float().cpu()
            assert torch.equal(ref[k], want), k
            assert not torch.equal(ref[k], plain)
    with pytest.raises(ValueError):
        extract_slide_augmented(hipt, [(r.float(), c) for r, c in zip(regs[:1], coords[:1])], str(tmp_path / "f"), "s", "HIPT_augment", 1)
