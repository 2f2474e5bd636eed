"""Tensor-space augmentation on the MI355X (csrc/tensor_augment.hip) against the two restatements of
tests/tensor_augment_ref.py: ``spatial`` bit for bit against ``ref32`` (a pixel whose float64 source coordinate lies within 2^-10 px
of a rounding boundary may read a neighbouring source pixel instead; at most 1 % of an image), ``all`` within 4 x max |ref32 - ref64|
of the float64 truth per fixture; determinism, batch independence, isolation between the regions of a batch, ``out=``, and
``extract_slide_augmented`` with the two policies end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tensor_augment_ref as R  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import tensor_augment as TA  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 4   # |kernel - ref64| <= MARGIN x max |ref32 - ref64| per fixture: the kernel's reduction order and its lack of fma contraction
#              differ from torch's; neither costs more than a couple of ulps of the mean, and every later op is continuous in it
PAD = ((torch.zeros(3) - torch.tensor(R.MEAN)) / torch.tensor(R.STD)).numpy()   # what zero padding becomes: -mean / std, in float32


def run(imgs, params, interleaved, **kw):
    """imgs uint8 [n, H, W, 3] (numpy) -> the kernel's float32 [n, 3, H, W] (numpy)"""
    t = torch.from_numpy(np.ascontiguousarray(imgs))
    t = (t if interleaved else t.permute(0, 3, 1, 2)).contiguous().to(DEV)
    return TA.augment_tensor(t, params, **kw).cpu().numpy()


def geometry_cases(name):
    imgs = R.fixture(name)
    n, H, W = R.FIXTURES[name]
    recs = [p for _, p in R.spatial_records(H, W)] + R.drawn_records("spatial", name)
    return R.cycle(imgs, len(recs)), recs


def colour_cases(name):
    imgs = R.fixture(name)
    n, H, W = R.FIXTURES[name]
    recs = R.drawn_records("all", name) + (R.colour_records() if n > 1 else [])
    return R.cycle(imgs, len(recs)), recs


@pytest.fixture(scope="module")
def refs():
    """every reference of this module, computed once: name -> (geometry: [(ref32, excused, neighbour values)], colour: [(ref32, ref64, excused)])"""
    out = {}
    for name in R.FIXTURES:
        gi, gr = geometry_cases(name)
        geo = []
        for img, p in zip(gi, gr):
            _, ix, iy = R.ref64(img, p)
            geo.append((R.ref32(img, p), R.excused(ix, iy, img.shape[:2]), None if ix is None else R.neighbour_values(img, p, ix, iy)))
        ci, cr = colour_cases(name)
        col = []
        for img, p in zip(ci, cr):
            b, ix, iy = R.ref64(img, p)
            col.append((R.ref32(img, p), b, R.excused(ix, iy, img.shape[:2])))
        out[name] = (geo, col)
    return out


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_spatial_is_bit_exact(name, interleaved, refs):
    imgs, recs = geometry_cases(name)
    before = N.calls
    got = run(imgs, recs, interleaved)
    assert N.calls == before + 1 and got.dtype == np.float32 and got.shape == (len(recs), 3) + imgs.shape[1:3]
    for i, (want, ex, nb) in enumerate(refs[name][0]):
        assert ex.mean() <= R.EXCUSED_CAP
        same = (got[i].view(np.uint32) == want.view(np.uint32)).all(0)
        assert same[~ex].all(), f"record {i}: {int((~same & ~ex).sum())} pixels differ from ref32 off the boundaries"
        if nb is not None and (~same & ex).any():
            ok = (got[i][None].view(np.uint32) == nb.view(np.uint32)).all(1).any(0)
            assert ok[ex].all(), f"record {i}: an excused pixel holds no neighbouring source pixel's value"


@pytest.mark.parametrize("interleaved", [False, True])
def test_exact_quarter_turns_stay_inside_the_region(interleaved):
    """32 x 48 turned by exactly +-90 degrees: most of the output is padding, -mean / std exactly; the rest are the image's own values"""
    img = R.fixture("ns32x48")[0]
    recs = [p for _, p in R.quarter_turn_records()]
    got = run(np.stack([img, img]), recs, interleaved)
    own = (torch.from_numpy(img).permute(2, 0, 1).float().div(255) - torch.tensor(R.MEAN).view(3, 1, 1)) / torch.tensor(R.STD).view(3, 1, 1)
    values = [set(np.unique(own[c].numpy().view(np.uint32)).tolist()) | {int(PAD[c:c + 1].view(np.uint32)[0])} for c in range(3)]
    for i, p in enumerate(recs):
        _, ix, iy = R.ref64(img, p)
        pad = (ix < -0.5) | (ix > 47.5) | (iy < -0.5) | (iy > 31.5)
        assert pad.mean() > 0.3
        for c in range(3):
            assert (got[i, c][pad] == PAD[c]).all()
            assert set(np.unique(got[i, c].view(np.uint32)).tolist()) <= values[c]
        assert np.array_equal(got[i], R.ref32(img, p))   # (W - H is even: the turn reads pixel centres, nothing is near a boundary)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("name", sorted(R.FIXTURES))
def test_all_is_within_the_margin_of_the_float64_truth(name, interleaved, refs):
    imgs, recs = colour_cases(name)
    got = run(imgs, recs, interleaved)
    bar = max(float(np.abs(a - b)[:, ~ex].max()) for a, b, ex in refs[name][1])
    err = max(float(np.abs(got[i] - b)[:, ~ex].max()) for i, (a, b, ex) in enumerate(refs[name][1]))
    print(f"{name} interleaved={interleaved}: max |kernel - ref64| = {err:.3g}, max |ref32 - ref64| = {bar:.3g}")
    assert all(ex.mean() <= R.EXCUSED_CAP for _, _, ex in refs[name][1])
    assert np.isfinite(got).all() and err <= MARGIN * bar, (err, bar)


def test_one_launch_without_contrast_two_with_it_and_a_broken_promise_is_loud():
    """`spatial`, and `all` records whose order holds no contrast op, take the one-launch route (no workspace); the C entry point
    writes NaN over a region whose record holds a contrast op when the caller said none does"""
    imgs = R.fixture("sq16")
    P = TA.TensorRegionParams
    no_contrast = [P(order=(TA.OP_HUE, TA.OP_BRIGHTNESS, TA.OP_SATURATION), brightness=R.f32(1.05), saturation=R.f32(0.93), hue=R.f32(-0.07),
                     theta=R._theta(21.0))] * 3
    got = run(imgs, no_contrast, False)
    for i in range(3):
        b, ix, iy = R.ref64(imgs[i], no_contrast[i])
        keep = ~R.excused(ix, iy, (16, 16))
        assert np.abs(got[i] - b)[:, keep].max() <= MARGIN * max(np.abs(R.ref32(imgs[i], no_contrast[i]) - b)[:, keep].max(), 2.0 ** -22)
    x = torch.from_numpy(imgs).to(DEV)
    recs = [P(), P(order=(TA.OP_CONTRAST,), contrast=R.f32(1.05)), P(hflip=True)]
    rec = TA.pack_tensor_records(recs).to(DEV)
    out = torch.empty((3, 3, 16, 16), dtype=torch.float32, device=DEV)
    N.call("hipt_augment_tensor", N.ptr(x), 1, 3, 16, 16, N.ptr(rec), N.ptr(out), None, 0, N.stream_ptr(torch.device(DEV)))
    out = out.cpu().numpy()
    assert np.isnan(out[1]).all() and np.array_equal(out[0], R.ref32(imgs[0], recs[0])) and np.array_equal(out[2], R.ref32(imgs[2], recs[2]))


def test_same_bits_again_and_alone():
    for name in ("sq16", "ns32x48"):
        imgs = R.fixture(name)
        n, H, W = R.FIXTURES[name]
        aug = TA.TensorAugment("all", 3)
        x = torch.from_numpy(imgs).to(DEV)
        a, b = aug(x, "slide", 1, 0), aug(x, "slide", 1, 0)
        assert torch.equal(a, b)
        alone = torch.cat([aug(x[i:i + 1], "slide", 1, i) for i in range(n)])
        assert torch.equal(a, alone)
        assert torch.equal(aug(x.permute(0, 3, 1, 2).contiguous(), "slide", 1, 0), a)   # the layout of the input does not matter


@pytest.mark.parametrize("interleaved", [False, True])
def test_regions_are_isolated_from_their_neighbours(interleaved):
    """every region sits between guard regions of 255: turned, translated and shrunk, no output pixel may carry a guard's value
    ((1 - mean) / std), and the region's output is what it is without the guards"""
    imgs = np.minimum(R.fixture("ns32x48"), 254)   # (no 255 of their own)
    P = TA.TensorRegionParams
    recs = [P(theta=R._theta(90.0)), P(theta=R._theta(-63.0, (5, -3), 0.9)), P(vflip=True, theta=R._theta(45.0, (-5, 3), 0.9))]
    guard = np.full_like(imgs[0], 255)
    batch = np.stack([guard, imgs[0], guard, imgs[1], guard, imgs[2], guard])
    got = run(batch, [P(), recs[0], P(), recs[1], P(), recs[2], P()], interleaved)
    alone = run(imgs, recs, interleaved)
    white = ((torch.ones(3) - torch.tensor(R.MEAN)) / torch.tensor(R.STD)).numpy()
    for k in range(3):
        assert np.array_equal(got[1 + 2 * k], alone[k])
        for c in range(3):
            assert not (got[1 + 2 * k, c] == white[c]).any()
            assert (got[2 * k, c] == white[c]).all()


def test_out_is_honoured_and_empty_batches_do_not_launch():
    imgs = R.fixture("sq16")
    recs = R.drawn_records("all", "sq16")
    x = torch.from_numpy(imgs).to(DEV)
    want = TA.augment_tensor(x, recs)
    out = torch.full((3, 3, 16, 16), float("nan"), device=DEV)
    assert TA.augment_tensor(x, recs, out=out) is out and torch.equal(out, want)
    odd = torch.full((3 * 3 * 16 * 16 + 1,), float("nan"), device=DEV)[1:].view(3, 3, 16, 16)   # 4-byte aligned only: the scalar stores
    assert TA.augment_tensor(x, recs, out=odd) is odd and torch.equal(odd, want)
    before = N.calls
    for bad in (torch.empty((3, 16, 16, 3), device=DEV), torch.empty((3, 3, 16, 16), dtype=torch.float64, device=DEV),
                torch.empty((3, 3, 16, 16)), torch.empty((2, 3, 16, 16), device=DEV)):
        with pytest.raises(ValueError, match="out must be"):
            TA.augment_tensor(x, recs, out=bad)
    alias = torch.empty((3 * 3 * 16 * 16,), dtype=torch.float32, device=DEV)
    xin = alias.view(torch.uint8)[:3 * 16 * 16 * 3].view(3, 16, 16, 3)
    with pytest.raises(ValueError, match="not the input"):
        TA.augment_tensor(xin, recs, out=alias.view(3, 3, 16, 16))
    empty = TA.augment_tensor(x[:0], [])
    assert empty.shape == (0, 3, 16, 16) and empty.dtype == torch.float32 and N.calls == before
    # other normalisation constants reach the kernel
    got = TA.augment_tensor(x, [TA.TensorRegionParams()] * 3, mean=(0.5, 0.25, 0.0), std=(0.5, 2.0, 1.0)).cpu()
    t = x.cpu().permute(0, 3, 1, 2).float().div(255)   # (on the host: torch's device division by a scalar multiplies by 1 / 255)
    assert torch.equal(got, (t - torch.tensor([0.5, 0.25, 0.0]).view(1, 3, 1, 1)) / torch.tensor([0.5, 2.0, 1.0]).view(1, 3, 1, 1))


def test_extract_slide_augmented_end_to_end(tmp_path):
    import resnet18_ref
    from hipt_abmil_atec23_amd import resnet18 as r18
    from hipt_abmil_atec23_amd.feature_store import extract_slide, extract_slide_augmented, load_coords
    m = r18.resnet18_baseline()
    m.load_state_dict(resnet18_ref.state_dict(), strict=False)
    m.fc = torch.nn.Sequential()
    m = m.eval().to(DEV)
    n, n_augs = 4, 2
    rng = np.random.default_rng(77)
    regs = [torch.from_numpy(rng.integers(0, 256, (1, 32, 32, 3), dtype=np.uint8)).to(DEV) for _ in range(n)]
    coords = [torch.tensor([[32 * i, 5 * i]], dtype=torch.int64) for i in range(n)]
    plain = torch.load(extract_slide(m, list(zip(regs, coords)), str(tmp_path / "plain"), "s", coalesce=4))
    files = {}
    for co in (1, 8):
        d = str(tmp_path / f"co{co}")
        paths = extract_slide_augmented(m, list(zip(regs, coords)), d, "s", "all", n_augs, seed=5, coalesce=co)
        assert [os.path.basename(p) for p in paths] == ["s.pt", "saug1.pt", "saug2.pt"]
        files[co] = [torch.load(p) for p in paths]
        for sid in ("s", "saug1", "saug2"):
            assert np.array_equal(load_coords(d, sid), torch.cat(coords).numpy())
    assert torch.equal(files[8][0], plain)
    for a, b in zip(files[1], files[8]):
        assert torch.equal(a, b)
    with torch.no_grad():
        x = torch.cat(regs)
        for k in range(1, n_augs + 1):
            params = TA.draw_tensor_region_params("all", 5, "s", k, 0, n, 32, 32)
            want = torch.cat([m(TA.augment_tensor(x[i:i + 1], params[i:i + 1])) for i in range(n)]).float().cpu()
            assert torch.equal(files[8][k], want), k
            assert not torch.equal(files[8][k], plain)
    paths = extract_slide_augmented(m, list(zip(regs, coords)), str(tmp_path / "sp"), "s", "spatial", 1, seed=5, include_original=False)
    assert [os.path.basename(p) for p in paths] == ["saug1.pt"] and torch.load(paths[0]).shape == plain.shape
