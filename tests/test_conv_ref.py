"""Host tests of tests/conv_ref.py (no GPU): the fp64 reference against two independent convolutions, the right-kernel emulation
inside the derived bound on every form and operand family, every wrong-kernel variant outside it, and the BN fold rule."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as CR  # noqa: E402

DTYPES = ["fp32", "bf16"]


def _packed(form, family, dtype):
    op = CR.operands(form, family, dtype)
    img, bias = CR.pack(op["weight"], op["gamma"], op["beta"], op["mean"], op["var"], op["eps"], dtype)
    if family == "cancel":
        op["resid"] = CR.cancel_resid(form, op["x"], img, bias, dtype)
    return op, img, bias


def _combos(family):
    return [c for c in CR.COMBOS if c[0]] if family == "cancel" else CR.COMBOS


# ---- the reference against independent ones ---------------------------------------------------------------------------------------
def _naive(x, w, bias, stride, pad):
    """seven loops: x [n, h, w, cin], w [cout, cin, kh, kw] -> [n, oh, ow, cout]"""
    n, h, wd, cin = x.shape
    cout, _, kh, kw = w.shape
    oh, ow = CR.out_hw(h, wd, kh, kw, stride, pad)
    y = np.zeros((n, oh, ow, cout))
    for b in range(n):
        for oy in range(oh):
            for ox in range(ow):
                for co in range(cout):
                    s = bias[co]
                    for ky in range(kh):
                        for kx in range(kw):
                            iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
                            if 0 <= iy < h and 0 <= ix < wd:
                                for ci in range(cin):
                                    s += x[b, iy, ix, ci] * w[co, ci, ky, kx]
                    y[b, oy, ox, co] = s
    return y


@pytest.mark.parametrize("shape", [(3, 2, 3, 3, 2, 1, 2, 5, 4), (2, 3, 1, 3, 1, 1, 2, 3, 4), (3, 2, 7, 7, 2, 3, 1, 8, 6)],
                         ids=["3x3s2p1", "1x3", "stem7x7s2p3"])
def test_conv_exact_against_seven_loops(shape):
    cin, cout, kh, kw, s, p, n, h, w = shape
    rng = np.random.RandomState(5)
    x, wt, bias = rng.randn(n, h, w, cin), rng.randn(cout, cin, kh, kw), rng.randn(cout)
    K = cin * kh * kw
    img = np.zeros((cout, K + 5))
    img[:, :K] = wt.transpose(0, 2, 3, 1).reshape(cout, K)
    y, S = CR.conv_exact(x, img, bias, None, False, kh, kw, s, p)
    ref = _naive(x, wt, bias, s, p)
    assert y.shape == ref.shape and float(np.abs(y - ref).max()) <= 1e-12
    assert float(np.abs(S - _naive(np.abs(x), np.abs(wt), np.abs(bias), s, p)).max()) <= 1e-12
    r = rng.randn(*y.shape)
    y2, S2 = CR.conv_exact(x, img, bias, r, True, kh, kw, s, p)
    assert np.array_equal(y2, np.maximum(y + r, 0)) and np.array_equal(S2, S + np.abs(r))
    img[0, K] = 1.0
    with pytest.raises(AssertionError, match="beyond K"):
        CR.conv_exact(x, img, bias, None, False, kh, kw, s, p)


@pytest.mark.parametrize("form", CR.FORMS, ids=lambda f: f.id)
def test_conv_exact_against_torch_fp64(form):
    f = form
    op, img, bias = _packed(f, "plain", "bf16")
    y, S = CR.conv_exact(op["x"], img, bias, op["resid"], False, *f.geom)
    wt = torch.from_numpy(img[:, :f.K].reshape(f.cout, f.kh, f.kw, f.cin)).permute(0, 3, 1, 2)
    if f.kh == f.kw:
        ref = F.conv2d(torch.from_numpy(op["x"]).permute(0, 3, 1, 2), wt, torch.from_numpy(bias), f.stride, f.pad)
    else:  # the C entry pads both axes alike
        ref = F.conv2d(torch.from_numpy(op["x"]).permute(0, 3, 1, 2), wt, torch.from_numpy(bias), f.stride, (f.pad, f.pad))
    ref = ref.permute(0, 2, 3, 1).numpy() + op["resid"]
    assert y.shape == (f.n, f.oh, f.ow, f.cout) == ref.shape
    assert bool((np.abs(y - ref) <= 1e-13 * S).all()), float((np.abs(y - ref) / S).max())


# ---- the table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", CR.FORMS, ids=lambda f: f.id)
def test_forms_populate_their_classes(form):
    cls = form.pixel_classes()
    assert set(form.classes) <= set(cls) and all(m.shape == (form.M,) for m in cls.values())
    for name in form.classes:
        assert cls[name].any(), f"{form.id}: class {name} is empty"
    assert np.array_equal(cls["interior"], ~cls["edge"]) and not (cls["corner"] & ~cls["edge"]).any()
    for b in range(1, form.n):   # an image seam inside a 128-row tile, not on its edge
        assert (b * form.oh * form.ow) % 128 != 0, form.id
    assert form.M <= 3 * 17 * 23 and form.cout % 64 == 0


def test_ragged_and_whole_tiles_are_all_there():
    ms = sorted(f.M for f in CR.FORMS if f.shape[:6] == (64, 64, 3, 3, 1, 1))
    assert ms == [1, 63, 64, 65, 127, 128, 129]
    c = CR.pixel_classes(2, 8, 8, 8, 8, 3, 3, 1, 1)
    assert c["seam"].sum() == 16 and c["corner"].sum() == 8 and c["interior"].sum() == 72 and not c["tile_tail128"].any()
    assert list(np.flatnonzero(c["tile_seam"])) == [63, 64, 65]
    c = CR.pixel_classes(1, 5, 13, 5, 13, 3, 3, 1, 1)
    assert list(np.flatnonzero(c["tile_tail64"])) == [64] and c["tile_tail128"].all() and not c["seam"].any()
    c = CR.pixel_classes(3, 4, 4, 8, 8, 3, 3, 2, 1)   # even map, stride 2: the top / left taps only
    assert c["seam"].sum() == 8 and c["corner"].sum() == 3


def test_rounding_helpers():
    v = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -3.3, 1e-40, 0.0, 2.0 ** -133, 2.0 ** -134, 3.0e38])
    t = torch.from_numpy(v).float().bfloat16().double().numpy()   # exact here: every value is an fp32 number or rounds alike
    assert np.array_equal(CR.round_bf16(v), t)
    assert CR.round_bf16(1.0 + 2.0 ** -8) == 1.0 and CR.round_bf16(1.0 + 3 * 2.0 ** -8) == 1.0 + 2.0 ** -6
    assert CR.ulp(1.5, "bf16") == 2.0 ** -7 and CR.ulp(1.5, "fp32") == 2.0 ** -23


# ---- the right kernel stays inside the bound ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", CR.FORMS, ids=lambda f: f.id)
def test_right_kernel_within_bound(form, dtype):
    f = form
    for family in f.families:
        op, img, bias = _packed(f, family, dtype)
        for resid, relu in _combos(family):
            r = op["resid"] if resid else None
            y, S = CR.conv_exact(op["x"], img, bias, r, relu, *f.geom)
            got = CR.emulate(op["x"], img, bias, r, relu, *f.geom, dtype)
            ratio = np.abs(got - y) / CR.bound(y, S, f.K, dtype)
            print(f"{f.id} {dtype} {family} resid={int(resid)} relu={int(relu)}: right kernel worst error / bound {ratio.max():.3f}")
            assert float(ratio.max()) < 1.0, (family, resid, relu, float(ratio.max()))
            if family == "cancel":   # the family does what it says: the result is a small fraction of its terms
                assert float(np.median(np.abs(y) / S)) < 1e-2


# ---- every wrong kernel is outside it --------------------------------------------------------------------------------------------------
def test_every_variant_has_a_catching_form():
    assert set(CR.CATCHES) == set(CR.VARIANTS)
    for name, where in CR.CATCHES.items():
        assert where, name
        for fid, family, combo, cls, bm in where:
            assert fid in CR.FORM and family in CR.FORM[fid].families and combo in _combos(family), (name, fid, family)
            assert cls == "all" or cls in CR.FORM[fid].classes, (name, fid, cls)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", CR.VARIANTS)
def test_variant_is_caught(name, dtype):
    for fid, family, (resid, relu), cls, bm in CR.CATCHES[name]:
        f = CR.FORM[fid]
        op, img, bias = _packed(f, family, dtype)
        r = op["resid"] if resid else None
        y, S = CR.conv_exact(op["x"], img, bias, r, relu, *f.geom)
        bad = CR.variant(name, f, op["x"], img, bias, r, relu, dtype, **({"bm": bm} if bm else {}))
        ratio = (np.abs(bad - y) / CR.bound(y, S, f.K, dtype)).reshape(f.M, f.cout)
        mask = np.ones(f.M, bool) if cls == "all" else f.pixel_classes()[cls]
        worst = float(ratio[mask].max())
        print(f"{name} {dtype} on {fid} {family} resid={int(resid)} relu={int(relu)}: {worst:.1f} x the bound in class {cls}")
        if name == "round_before_resid" and dtype == "fp32":   # the accumulator is fp32: this IS the right kernel (conv_ref.CATCHES)
            assert worst < 1.0, worst
            continue
        assert worst >= 3.0, (name, fid, worst)
        if cls not in ("all", "interior") and (~mask).any():   # and it corrupts that class only
            assert float(ratio[~mask].max()) < 1.0, (name, fid, float(ratio[~mask].max()))


# ---- the fold rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_fold_rule(dtype):
    f = CR.FORM["c64-64k3x3s1p1_2x8x8"]
    op = CR.operands(f, "bn_edges", dtype)
    img, bias = CR.pack(op["weight"], op["gamma"], op["beta"], op["mean"], op["var"], op["eps"], dtype)
    kb = CR.SLAB[dtype]
    assert img.shape == (64, (f.K + kb - 1) // kb * kb)
    # an independent statement in torch, element by element in the packed order
    w, g, v = (torch.from_numpy(op[k]).double() for k in ("weight", "gamma", "var"))
    scale = g / torch.sqrt(v + float(np.float32(op["eps"])))
    ref = (w * scale[:, None, None, None]).float()
    ref = (ref.bfloat16() if dtype == "bf16" else ref).double().numpy()
    for co, ky, kx, ci in [(0, 0, 0, 0), (5, 2, 1, 63), (63, 1, 2, 7), (17, 0, 2, 31)]:
        assert img[co, (ky * 3 + kx) * 64 + ci] == ref[co, ci, ky, kx]
    assert np.array_equal(img[:, :f.K].reshape(64, 3, 3, 64), ref.transpose(0, 2, 3, 1))
    fb = op["beta"].astype(np.float64) - op["mean"].astype(np.float64) * scale.numpy()
    assert bool((np.abs(bias - fb) <= 2.0 ** -24 * np.abs(fb)).all())
    # the edges are there: dead channels pack to exact zeros, negative gains flip the sign, eps alone decides the scale at var = 0
    assert not img[::16].any() and bool((op["gamma"][4::8] < 0).all()) and float(op["var"][3]) == 0.0 and op["var"][5] == np.float32(1e-12)
    assert abs(scale[3].item() * np.sqrt(1e-5) / float(op["gamma"][3]) - 1) < 1e-6 and float(np.abs(op["mean"]).max()) > 40
    CR.check_packed(img, bias, op, dtype)
    bad = img.copy()
    bad[5, 7] += CR.ulp(bad[5, 7], dtype)
    with pytest.raises(AssertionError):
        CR.check_packed(bad, bias, op, dtype)
    with pytest.raises(AssertionError):
        CR.check_packed(img, bias + 2.0 ** -22 * np.abs(bias), op, dtype)


def test_stem_pads_k_to_the_slab():
    f = CR.FORMS[0]
    for dtype, kp in (("fp32", 160), ("bf16", 192)):
        op = CR.operands(f, "plain", dtype)
        img, _ = CR.pack(op["weight"], op["gamma"], op["beta"], op["mean"], op["var"], op["eps"], dtype)
        assert img.shape == (64, kp) and not img[:, 147:].any() and img[:, :147].all()


def test_avgpool_bound():
    x = np.full((1, 990, 2), 100.0)
    assert np.allclose(CR.avgpool_bound(x), 990 * 2.0 ** -24 * 100.0)
