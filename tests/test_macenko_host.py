"""CPU tests of the device Macenko normalisation: the numpy restatement (tests/macenko_ref.py) on its own --
ranks, an identity, the recovered stain matrix, what float32 costs against float64 on every fixture of the GPU tests -- the five
C entry points declared, exported and bound, and every refusal of the Python layer and of the library, which return before
anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import macenko_ref as MR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import macenko as MK  # noqa: E402

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
ENTRY_POINTS = ("hipt_macenko_workspace_bytes", "hipt_macenko_fit", "hipt_macenko_apply", "hipt_macenko_normalize", "hipt_macenko_keys")


def test_rank_of_percentile():
    assert MR.rank(1, 1) == 1 and MR.rank(1, 99) == 1
    assert MR.rank(2, 1) == 1 and MR.rank(2, 99) == 2
    assert MR.rank(3, 1) == 1 and MR.rank(3, 99) == 3
    assert MR.rank(101, 1) == 2 and MR.rank(101, 99) == 100
    assert MR.rank(51, 1) == 1 and MR.rank(151, 1) == 3   # 0.5 -> 0 and 1.5 -> 2: half to even
    t = np.random.default_rng(0).permutation(101).astype(np.float64)
    assert MR.percentile(t, 1) == 1.0 and MR.percentile(t, 99) == 99.0   # an element, never an interpolation


def reference_image(h, w, seed):
    """made with HE_REF, concentrations whose 99th percentiles are MAXC_REF, and a share of pure-H and pure-E pixels (the extreme
    angles are then the stains themselves)"""
    rng = np.random.default_rng(seed)
    c0, c1 = 0.4 + 1.4 * MR.smooth_field(rng, h, w), 0.3 + 0.8 * MR.smooth_field(rng, h, w)
    kind = rng.uniform(size=(h, w))
    C = np.stack([np.where(kind < 0.3, 0, c0), np.where(kind > 0.7, 0, c1)]).reshape(2, -1)
    for j in range(2):
        C[j] *= MR.MAXC_REF[j] / MR.percentile(C[j], 99)
    od = (MR.HE_REF @ C).T.reshape(h, w, 3)
    return np.clip(np.rint(240 * np.exp(-od) - 1), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("h,w,seed", [(64, 64, 1), (120, 90, 2)])
def test_reference_stained_image_comes_back_as_itself(h, w, seed):
    img = reference_image(h, w, seed)
    out, status = MR.normalize(img)
    assert status == 0 and np.abs(out.astype(int) - img.astype(int)).max() <= 2


@pytest.mark.parametrize("name", sorted(MR.FIXTURES))
def test_recovered_stain_matrix_is_near_the_one_the_image_was_made_with(name):
    """Macenko's vectors are the 1st / 99th percentile directions; every fixture holds 15 % pure-H and 15 % pure-E pixels, so those
    directions are the stains up to the uint8 rounding of a pixel (half a level in 30 or more: under a degree).  Bar: 2 degrees."""
    img, he = MR.fixture(name)
    f = MR.fit(img)
    assert f["status"] == 0
    assert MR.angle_deg(f["HE"][:, 0], he[:, 0]) < 2 and MR.angle_deg(f["HE"][:, 1], he[:, 1]) < 2
    assert abs(np.linalg.norm(f["HE"][:, 0]) - 1) < 1e-9 and f["HE"][0, 0] > f["HE"][0, 1]


@pytest.mark.parametrize("name", sorted(MR.FIXTURES))
def test_float32_restatement_is_within_one_level_of_float64(name):
    """the cap the GPU tests hold the device to: at most 1 level per pixel, on at most 0.5 % of the pixels"""
    img, _ = MR.fixture(name)
    a, sa = MR.normalize(img)
    b, sb = MR.normalize(img, dtype=np.float32)
    assert sa == sb == 0
    d = np.abs(a.astype(int) - b.astype(int))
    assert d.max() <= 1 and (d.max(axis=2) > 0).mean() <= 0.005


def test_fallbacks_of_the_restatement():
    for img in (MR.white_image(8, 8), MR.one_tissue_pixel_image(37, 53)):
        out, status = MR.normalize(img)
        assert status == 1 and np.array_equal(out, img)
    assert MR.fit(MR.one_tissue_pixel_image(37, 53))["n"] == 1 and MR.fit(MR.white_image(8, 8))["n"] == 0


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    lib = N.lib()
    for name in ENTRY_POINTS:
        decl = re.search(r"\b(?:int|size_t) %s\((.*?)\);" % name, hdr, re.S).group(1)
        assert len(decl.split(",")) == len(N.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert re.search(r"#define HIPT_ABI_VERSION %d\b" % N.ABI_VERSION, hdr) and lib.hipt_abi_version() == N.ABI_VERSION
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmacenko\.hip\b", mk, re.M) and "FLAGS_macenko.hip = -ffp-contract=off" in mk
    import hipt_abmil_atec23_amd as amd
    from hipt_abmil_atec23_amd import feature_store
    for name in ("macenko_fit", "macenko_apply", "macenko_normalize", "MacenkoNormalizer"):
        assert getattr(amd, name) is getattr(MK, name)
    assert amd.extract_slide_normalised is feature_store.extract_slide_normalised
    from hipt_abmil_atec23_amd import augment
    assert "HIPT_macenko" not in augment.POLICIES and "macenko" not in augment.POLICIES


def al256(v):
    return (v + 255) & ~255


def test_workspace_bytes_is_the_carve_and_holds_nothing_per_pixel():
    lib = N.lib()
    for r, h, w in [(1, 8, 8), (3, 37, 53), (2, 300, 200), (1, 4096, 4096), (256, 256, 256)]:
        nwg = min(-(-(h * w) // 4096), 1024)
        want = al256(1024) + al256(128 * r) + al256(80 * r * nwg) + al256(16384 * r) + al256(24 * r) + al256(8 * r) + al256(4 * r)
        assert lib.hipt_macenko_workspace_bytes(r, h, w) == want
    assert lib.hipt_macenko_workspace_bytes(1, 4096, 4096) < 4096 * 4096 // 100
    assert lib.hipt_macenko_workspace_bytes(0, 8, 8) == 0 and lib.hipt_macenko_workspace_bytes(1, 0, 8) == 0
    assert lib.hipt_macenko_workspace_bytes(1, 1 << 16, 1 << 15) == 0


def test_library_refuses_without_launching():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    src, dst, he, mc, st, ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x70000
    need = lib.hipt_macenko_workspace_bytes(2, 37, 53)

    def fit(src=src, il=0, r=2, hw=(37, 53), Io=240.0, alpha=1.0, beta=0.15, he=he, mc=mc, st=st, ws=ws, ws_bytes=need):
        return lib.hipt_macenko_fit(src, il, r, hw[0], hw[1], Io, alpha, beta, he, mc, st, None, ws, ws_bytes, None)

    def apply(src=src, r=2, hw=(37, 53), Io=240.0, he=he, mc=mc, dst=dst, f32=0):
        return lib.hipt_macenko_apply(src, 1, r, hw[0], hw[1], Io, he, mc, None, None, None, dst, f32, None)

    def normalize(src=src, r=2, hw=(37, 53), Io=240.0, alpha=1.0, beta=0.15, dst=dst, ws=ws, ws_bytes=need):
        return lib.hipt_macenko_normalize(src, 0, r, hw[0], hw[1], Io, alpha, beta, None, None, dst, 0, None, None, None, ws, ws_bytes, None)

    for call in (fit, normalize):
        assert call(r=0) == BADARG and call(hw=(0, 53)) == BADARG and call(hw=(37, -1)) == BADARG
        assert call(hw=(1 << 16, 1 << 15)) == UNSUPPORTED and b"2^31" in lib.hipt_last_error()
        assert call(Io=0.0) == BADARG and call(Io=-1.0) == BADARG and call(Io=float("nan")) == BADARG
        assert call(alpha=0.0) == BADARG and call(alpha=50.0) == BADARG and call(alpha=float("nan")) == BADARG
        assert b"alpha" in lib.hipt_last_error()
        assert call(beta=-0.1) == BADARG and b"beta" in lib.hipt_last_error()
        assert call(src=None) == BADARG
        name = "macenko_fit" if call is fit else "macenko_normalize"
        assert call(ws_bytes=need - 1) == WORKSPACE
        msg = lib.hipt_last_error().decode()
        assert msg.startswith(name + ": workspace") and str(need - 1) in msg and str(need) in msg and "too small / unaligned" in msg
        assert call(ws=ws + 16) == WORKSPACE and call(ws=None, ws_bytes=0) == WORKSPACE and call(ws=None) == BADARG
    assert fit(he=None) == BADARG and fit(mc=None) == BADARG and fit(st=None) == BADARG and fit(he=he + 2) == BADARG
    assert normalize(dst=None) == BADARG and normalize(dst=src) == BADARG
    assert apply(r=0) == BADARG and apply(hw=(1 << 16, 1 << 15)) == UNSUPPORTED and apply(Io=0.0) == BADARG
    assert apply(src=None) == BADARG and apply(he=None) == BADARG and apply(mc=None) == BADARG and apply(dst=None) == BADARG
    assert apply(dst=src) == BADARG and apply(dst=dst + 2, f32=1) == BADARG and apply(mc=mc + 1) == BADARG
    keys = lambda **kw: lib.hipt_macenko_keys(kw.get("src", src), 0, kw.get("r", 1), 8, 8, 240.0, kw.get("beta", 0.15), kw.get("aux", he), dst, st, None)  # noqa: E731
    assert keys(r=0) == BADARG and keys(src=None) == BADARG and keys(aux=None) == BADARG and keys(beta=-1.0) == BADARG


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    before = N.calls
    x = torch.zeros((2, 3, 8, 8), dtype=torch.uint8)
    he, mc = torch.zeros((2, 3, 2)), torch.ones((2, 2))

    def apply(v, **kw):
        n = v.shape[0] if v.ndim == 4 else 1
        return MK.macenko_apply(v, he[:n], mc[:n], **kw)
    calls = (MK.macenko_fit, MK.macenko_normalize, apply)
    for f in calls:
        with pytest.raises(ValueError, match="uint8"):
            f(x.float())
        with pytest.raises(ValueError, match="uint8"):
            f(np.zeros((3, 8, 8), np.uint8))
        with pytest.raises(ValueError, match="batch"):
            f(torch.zeros((2, 4, 8, 8), dtype=torch.uint8))
        with pytest.raises(ValueError, match="batch"):
            f(torch.zeros((8, 8), dtype=torch.uint8))
        with pytest.raises(ValueError, match="at least one"):
            f(torch.zeros((0, 3, 8, 8), dtype=torch.uint8))
        with pytest.raises(ValueError, match="HIP device"):   # a CPU tensor: there is no CPU path
            f(x)
        with pytest.raises(ValueError, match="HIP device"):
            f(x[0].permute(1, 2, 0))
    for f in calls[:2]:
        for kw, word in ((dict(Io=0), "Io"), (dict(Io=-3), "Io"), (dict(Io="a"), "numbers"), (dict(alpha=0), "alpha"), (dict(alpha=50), "alpha"),
                         (dict(alpha=float("nan")), "alpha"), (dict(beta=-0.01), "beta")):
            with pytest.raises(ValueError, match=word):
                f(x, **kw)
    for f in (MK.macenko_normalize, lambda v, **kw: MK.macenko_apply(v, he, mc, **kw)):
        with pytest.raises(ValueError, match="out_dtype"):
            f(x, out_dtype=torch.float16)
        with pytest.raises(ValueError, match="out must be"):
            f(x, out=torch.zeros((2, 3, 8, 8)))
        with pytest.raises(ValueError, match="out must be"):
            f(x, out=torch.zeros((2, 3, 8, 4), dtype=torch.uint8))
        with pytest.raises(ValueError, match="out must be"):
            f(x, out=x)
    with pytest.raises(ValueError, match="one per image"):
        MK.macenko_apply(x, he[:1], mc)
    with pytest.raises(ValueError, match="status"):
        MK.macenko_apply(x, he, mc, status=torch.zeros(3, dtype=torch.int32))
    from hipt_abmil_atec23_amd.feature_store import extract_slide_normalised
    with pytest.raises(TypeError, match="unknown"):
        extract_slide_normalised(None, [], "/nonexistent", "s", gamma=2)
    assert N.calls == before


def test_normalizer_refuses_stains():
    import torch
    before = N.calls
    with pytest.raises(NotImplementedError, match="stains"):
        MK.MacenkoNormalizer().normalize(torch.zeros((3, 8, 8)), stains=True)
    with pytest.raises(ValueError, match=r"\[3, h, w\]"):
        MK.MacenkoNormalizer(device="cpu")._u8(torch.zeros((8, 8, 3)))
    assert N.calls == before
