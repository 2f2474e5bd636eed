"""GPU tests of the Macenko normalisation (csrc/macenko.hip) against the numpy restatement (tests/macenko_ref.py):
``apply`` alone, ``fit``, the exactness of the selects against the device's own keys, ``normalize`` end to end, invariance under
batching / order / layout / repetition, graph capture, a fitted target, and ``extract_slide_normalised``.

Bars.  Output bytes against float64: no pixel off by more than 1 level and at most 2 % of an image's pixels off by 1 -- a
truncation boundary is crossed only where the float64 value lies within the float32 chain's error of an integer.  HE / maxC
against float64: within 4 x the distance the float32 restatement has from it on the same fixture (computed here), with a floor
of 16 float32 ulp of the largest entry."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import macenko_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

SINGLES = ("8x8", "37x53", "37x53_flat", "131x97", "300x200", "300x200_flat", "512x512")
# batches of three sizes-equal images: a stained one, a fallback (all white: n = 0; one tissue pixel: n = 1), one with ties
BATCHES = {
    "37x53": ("37x53", "white", "37x53_flat"),
    "300x200": ("300x200", "one_pixel", "300x200_flat"),
    "300x200_ok": ("300x200", "300x200_b", "300x200_flat"),
}
_ref = {}


def image(name, hw=None):
    if name == "white":
        return MR.white_image(*hw)
    if name == "one_pixel":
        return MR.one_tissue_pixel_image(*hw)
    return MR.fixture(name)[0]


def batch(key):
    names = BATCHES[key]
    hw = MR.FIXTURES[names[0]][:2]
    return np.stack([image(n, hw) for n in names])


def ref(name, hw=None):
    """float64 and float32 restatement of one image, computed once: fit dicts, normalised bytes"""
    key = (name, hw)
    if key not in _ref:
        img = image(name, hw)
        f64, f32 = MR.fit(img), MR.fit(img, dtype=np.float32)
        out = MR.apply(img, f64["HE"], f64["maxC"]) if f64["status"] == 0 else img.copy()
        _ref[key] = dict(img=img, f64=f64, f32=f32, out=out)
    return _ref[key]


def dev_u8(a, layout="hwc"):
    """uint8 [.., h, w, 3] numpy -> device tensor, interleaved ("hwc") or planar ("chw")"""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if layout == "hwc" else t.movedim(-1, -3).contiguous()


def as_hwc(t, layout):
    return (t if layout == "hwc" else t.movedim(-3, -1)).cpu().numpy()


def assert_bytes_close(got, want, what):
    d = np.abs(got.astype(int) - want.astype(int))
    share = float((d.max(axis=-1) > 0).mean())
    print(f"{what}: max level difference {int(d.max())}, share of pixels off {share:.5f}")
    assert d.max() <= 1, what
    assert share <= 0.02, what


def equals_u8_over_255(f, planar_u8):
    """bit for bit the IEEE quotient uint8 / 255 in float32 (numpy's; a device `tensor / 255` multiplies by a rounded reciprocal)"""
    return np.array_equal(f.cpu().numpy(), planar_u8.cpu().numpy().astype(np.float32) / np.float32(255))


def ulp32(v):
    return float(np.spacing(np.float32(np.abs(v).max())))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("name", SINGLES)
def test_apply_alone_against_float64(name, layout):
    from hipt_abmil_atec23_amd.macenko import macenko_apply
    r = ref(name)
    x = dev_u8(r["img"], layout)
    he = torch.from_numpy(r["f64"]["HE"].astype(np.float32))[None].cuda()
    mc = torch.from_numpy(r["f64"]["maxC"].astype(np.float32))[None].cuda()
    out = macenko_apply(x, he, mc)
    assert out.dtype == torch.uint8 and out.shape == x.shape
    assert_bytes_close(as_hwc(out, layout), r["out"], f"apply {name} {layout}")
    f = macenko_apply(x, he, mc, out_dtype=torch.float32)
    assert f.dtype == torch.float32 and tuple(f.shape) == (3,) + r["img"].shape[:2]
    planar = out if layout == "chw" else out.movedim(-1, -3)
    assert equals_u8_over_255(f, planar)
    # a status that is not 0: copied through, in both forms
    st = torch.ones(1, dtype=torch.int32, device="cuda")
    assert torch.equal(macenko_apply(x, he, mc, status=st), x)
    xp = x if layout == "chw" else x.movedim(-1, -3)
    assert equals_u8_over_255(macenko_apply(x, he, mc, status=st, out_dtype=torch.float32), xp)


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("name", SINGLES)
def test_fit_against_float64_within_four_times_the_float32_distance(name, layout):
    from hipt_abmil_atec23_amd.macenko import macenko_fit
    r = ref(name)
    he, mc, st = macenko_fit(dev_u8(r["img"], layout))
    assert he.shape == (1, 3, 2) and mc.shape == (1, 2) and st.shape == (1,) and st.dtype == torch.int32
    assert int(st[0]) == r["f64"]["status"] == 0
    for what, got, key in (("HE", he[0].cpu().numpy(), "HE"), ("maxC", mc[0].cpu().numpy(), "maxC")):
        want = r["f64"][key]
        yard = float(np.abs(r["f32"][key].astype(np.float64) - want).max())
        dist = float(np.abs(got.astype(np.float64) - want).max())
        bar = 4 * max(yard, 16 * ulp32(want) / 4)   # 4 x the float32 distance, floor 16 ulp
        print(f"fit {name} {layout} {what}: float32 restatement {yard:.3e}, device {dist:.3e}, bar {bar:.3e}")
        assert dist <= bar, (what, dist, bar)


def kth(values, k):
    return np.partition(values, k - 1)[k - 1]


def assert_selects_exact(x, n_want):
    """the keys of every pixel as the passes compute them (hipt_macenko_keys, from the device's E and matrix); minPhi, maxPhi and
    maxC must BE the k-th smallest of them, bit for bit.  Returns the tissue keys of phi."""
    from hipt_abmil_atec23_amd.macenko import macenko_fit, macenko_keys
    he, mc, st, aux = macenko_fit(x, _aux=True)
    keys, tissue = macenko_keys(x, aux)
    keys, tissue, a = keys[0].cpu().numpy(), tissue[0].cpu().numpy().astype(bool), aux[0].cpu()
    n = int(a.view(torch.int32)[14])
    assert int(st[0]) == 0 and n == int(tissue.sum()) == n_want
    phi = keys[0][tissue] + np.float32(0)   # (-0.0 and +0.0 are equal keys; + 0 makes them one value)
    assert float(a[6]) == kth(phi, MR.rank(n, 1)) and float(a[7]) == kth(phi, MR.rank(n, 99))
    npix = keys.shape[1]
    for j in range(2):
        assert float(mc[0, j]) == kth(keys[1 + j] + np.float32(0), MR.rank(npix, 99))
    return phi


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("name", SINGLES)
def test_selects_are_exact_order_statistics_of_the_devices_own_keys(name, layout):
    phi = assert_selects_exact(dev_u8(ref(name)["img"], layout), ref(name)["f64"]["n"])
    assert len(np.unique(phi)) < len(phi) or "flat" not in name   # the flat fixtures do hold ties


def test_an_image_of_several_trips_per_workgroup():
    """2100 x 4096: 2100 chunks of 4096 pixels over the 1024 workgroups an image gets at most, so workgroups take two or three
    trips through the image (the production shape, 4096 x 4096, takes four).  fit, the selects, normalize, both layouts."""
    from hipt_abmil_atec23_amd.macenko import macenko_fit, macenko_normalize
    img = MR.large_image()[0]
    assert img.shape == (2100, 4096, 3) and img.shape[0] * img.shape[1] > 2 * 1024 * 4096
    f64, f32 = MR.fit(img), MR.fit(img, dtype=np.float32)
    x = dev_u8(img, "hwc")
    he, mc, st = macenko_fit(x)
    assert int(st[0]) == f64["status"] == 0
    for what, got, key in (("HE", he[0].cpu().numpy(), "HE"), ("maxC", mc[0].cpu().numpy(), "maxC")):
        want = f64[key]
        yard = float(np.abs(f32[key].astype(np.float64) - want).max())
        dist = float(np.abs(got.astype(np.float64) - want).max())
        bar = max(4 * yard, 16 * ulp32(want))
        print(f"fit 2100x4096 {what}: float32 restatement {yard:.3e}, device {dist:.3e}, bar {bar:.3e}")
        assert dist <= bar, (what, dist, bar)
    assert_selects_exact(x, f64["n"])
    out = macenko_normalize(x)
    assert_bytes_close(out.cpu().numpy(), MR.apply(img, f64["HE"], f64["maxC"]), "normalize 2100x4096")
    xp = x.movedim(-1, -3).contiguous()
    hq, mq, sq = macenko_fit(xp)
    assert torch.equal(hq, he) and torch.equal(mq, mc) and torch.equal(sq, st)
    assert torch.equal(macenko_normalize(xp), out.movedim(-1, -3))


@pytest.mark.parametrize("layout", ["hwc", "chw"])
@pytest.mark.parametrize("key", sorted(BATCHES))
def test_normalize_end_to_end_and_fallbacks(key, layout):
    from hipt_abmil_atec23_amd.macenko import macenko_apply, macenko_fit, macenko_normalize
    names = BATCHES[key]
    hw = MR.FIXTURES[names[0]][:2]
    x = dev_u8(batch(key), layout)
    out, st = macenko_normalize(x, return_status=True)
    got = as_hwc(out, layout)
    for i, n in enumerate(names):
        r = ref(n, hw if n in ("white", "one_pixel") else None)
        assert int(st[i]) == r["f64"]["status"], n
        if r["f64"]["status"]:
            assert np.array_equal(got[i], r["img"]), n   # a fallback image is its input, bit for bit
        else:
            assert_bytes_close(got[i], r["out"], f"normalize {key}[{i}] {n} {layout}")
    he, mc, st2 = macenko_fit(x)
    assert torch.equal(st, st2)
    assert torch.equal(out, macenko_apply(x, he, mc, st2))   # normalize is fit then apply
    f = macenko_normalize(x, out_dtype=torch.float32)
    assert equals_u8_over_255(f, out if layout == "chw" else out.movedim(-1, -3))


def test_invariance_under_batching_order_layout_and_repetition():
    from hipt_abmil_atec23_amd.macenko import macenko_fit, macenko_normalize
    for key in ("37x53", "300x200"):
        b = batch(key)
        x = dev_u8(b, "hwc")
        he, mc, st = macenko_fit(x)
        out = macenko_normalize(x)
        he2, mc2, st2 = macenko_fit(x)
        assert torch.equal(he, he2) and torch.equal(mc, mc2) and torch.equal(st, st2) and torch.equal(out, macenko_normalize(x))
        for i in range(3):   # alone
            h1, m1, s1 = macenko_fit(x[i])
            assert torch.equal(h1[0], he[i]) and torch.equal(m1[0], mc[i]) and torch.equal(s1[0], st[i])
            assert torch.equal(macenko_normalize(x[i]), out[i])
        perm = [2, 0, 1]   # another order
        hp, mp, sp = macenko_fit(x[perm].contiguous())
        assert torch.equal(hp, he[perm]) and torch.equal(mp, mc[perm]) and torch.equal(sp, st[perm])
        assert torch.equal(macenko_normalize(x[perm].contiguous()), out[perm])
        xp = dev_u8(b, "chw")   # planar
        hq, mq, sq = macenko_fit(xp)
        assert torch.equal(hq, he) and torch.equal(mq, mc) and torch.equal(sq, st)
        assert torch.equal(macenko_normalize(xp), out.movedim(-1, -3))


def test_normalize_in_a_captured_graph():
    from hipt_abmil_atec23_amd.macenko import macenko_normalize
    a, b = dev_u8(batch("300x200"), "hwc"), dev_u8(batch("300x200_ok"), "hwc")
    want_a, want_b = macenko_normalize(a), macenko_normalize(b)
    x, out = a.clone(), torch.empty_like(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        macenko_normalize(x, out=out)   # (warm-up on the side stream)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        macenko_normalize(x, out=out)
    for src, want in ((b, want_b), (a, want_a)):
        x.copy_(src)
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, want)


@pytest.mark.parametrize("name", ["37x53", "300x200_clean"])
def test_an_image_normalised_to_its_own_fit_is_itself(name):
    from hipt_abmil_atec23_amd.macenko import MacenkoNormalizer, macenko_fit, macenko_normalize
    h, w, seed, _ = MR.FIXTURES[name]
    img = MR.synth_image(h, w, seed, background=0)[0]   # (background pixels are not in the stain plane)
    x = dev_u8(img, "hwc")
    he, mc, st = macenko_fit(x)
    assert int(st[0]) == 0
    out = macenko_normalize(x, target=(he[0], mc[0]))
    assert np.abs(out.cpu().numpy().astype(int) - img.astype(int)).max() <= 2
    # torchstain's call surface: [3, h, w] float 0..255 in, ([h, w, 3] int32, None, None) out
    chw = torch.from_numpy(img).permute(2, 0, 1).float()
    norm, H, E = MacenkoNormalizer().fit(chw).normalize(chw)
    assert H is None and E is None and norm.dtype == torch.int32 and tuple(norm.shape) == img.shape
    assert torch.equal(norm.cpu(), out.cpu().to(torch.int32))


def test_extract_slide_normalised_writes_the_models_features_of_the_normalised_regions(tmp_path):
    from hipt_abmil_atec23_amd import HIPT_4K, synth
    from hipt_abmil_atec23_amd.feature_store import extract_slide_normalised
    from hipt_abmil_atec23_amd.macenko import macenko_normalize
    dev = torch.device("cuda:0")
    m = HIPT_4K(None, None, dev, dev)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(dev)
    regions = [dev_u8(MR.synth_image(1024, 1024, 40 + i)[0], "chw")[None] for i in range(2)] + [dev_u8(MR.white_image(1024, 1024), "chw")[None]]
    coords = [np.array([[i * 1024, 0]], dtype=np.int64) for i in range(3)]
    for reference_input in (True, False):
        with torch.no_grad():
            want = torch.cat([m(macenko_normalize(r, out_dtype=torch.float32 if reference_input else torch.uint8)) for r in regions]).float().cpu()
        paths = [extract_slide_normalised(m, list(zip(regions, coords)), str(tmp_path), f"s{co}_{reference_input}", coalesce=co,
                                          reference_input=reference_input) for co in (1, 8)]
        assert all(isinstance(p, str) and p.fallbacks == 1 for p in paths)
        files = [torch.load(p) for p in paths]
        assert torch.equal(files[0], want) and torch.equal(files[1], want)
