"""GPU tests of the patch-level heat-maps (csrc/patch_heatmap.hip through hipt_abmil_atec23_amd.patch_heatmap).
Every comparison is exact, byte for byte, against the numpy restatement tests/patch_heatmap_ref.py, which crops with Pillow,
upscales, ranks with scipy and slices as the reference does.  Inputs are seeded; a case's restatement is made once and shared.

Without the kernel every test here fails: the module and the entry point do not exist."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import patch_heatmap_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t):
    return t.detach().cpu().numpy()


def colormap(name):
    import matplotlib

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    if name == "half_jet":
        return HH.half_jet()                                   # 1024 entries
    if name == "two":
        return matplotlib.colormaps["coolwarm"].resampled(2)   # 2 entries
    return matplotlib.colormaps[name]                          # 256 entries


# name: (P, nh, offset, colormap, alpha, maps, pixels whose score equals the threshold)
# The threshold is the score of pixel (128, 128) of patch 0, head 0 -- an attained value, so those pixels take the wrapping
# hm + inverse sum.  The counts are the restatement's own (case() asserts them): with ties in the maps every token (pair) that
# repeats the value adds its area, and a rank attained in patch 0 is attained in the other patches too (every map has 256 values);
# the constant map scores one value on all 65 536 pixels.
CASES = {
    "three patches, six heads, offset 16": (3, 6, 16, "coolwarm", 0.5, "ties", 3328),
    "offset 0, table of 2, alpha 0": (1, 1, 0, "two", 0.0, "ties", 256),
    "offset 5, table of 1024, alpha 1": (1, 6, 5, "half_jet", 1.0, "ties", 512),
    "offset 255, random maps": (3, 1, 255, "coolwarm", 0.5, "random", 768),
    "offset 256: nothing overlaps": (1, 1, 256, "coolwarm", 0.3, "ties", 768),
    "constant map": (1, 1, 16, "coolwarm", 0.5, "constant", 65536),
}
_memo = {}


def maps_of(kind, p, nh, seed):
    if kind == "ties":
        return PR.synthetic_maps(p, nh, seed)
    if kind == "random":
        return np.random.default_rng(seed).random((p, 2, nh, 256), dtype=np.float32) + np.float32(0.001)
    return np.full((p, 2, nh, 256), 0.25, dtype=np.float32)


def case(name):
    """The inputs of a case, the threshold picked from the restatement's own scores, and the restatement's pictures (made once)."""
    if name not in _memo:
        p, nh, offset, cm, alpha, kind, equal = CASES[name]
        a256, patches = maps_of(kind, p, nh, 7 + len(name)), PR.synthetic_patches(p, 3 + len(name))
        how = dict(offset=offset, alpha=alpha)
        thr = float(PR.score(a256[0, 0, 0], a256[0, 1, 0], offset)[128, 128])
        want = [PR.pictures(a256[i], patches[i], cmap=colormap(cm), threshold=thr, **how) for i in range(p)]
        scores = np.stack([w["score"] for w in want])
        hit = scores == thr
        assert int(hit.sum()) == equal, (name, int(hit.sum()))
        if kind != "constant":
            assert (scores < thr).any() and (scores > thr).any()
        # the restatement itself wraps there: neither the patch nor the blend, their uint8 sum
        th = np.stack([w["256th"] for w in want])
        base = np.broadcast_to(patches[:, None], th.shape)
        assert (th[hit] != base[hit]).any() and (th[hit].astype(np.int32) < base[hit].astype(np.int32)).any()
        _memo[name] = (a256, patches, cm, thr, how, {k: np.stack([w[k] for w in want]) for k in ("256", "256th")})
    return _memo[name]


def dev(a):
    import torch
    return torch.from_numpy(a).to(DEV)


def same(got, want):
    import torch
    return got.dtype == torch.uint8 and tuple(got.shape) == want.shape and torch.equal(got, dev(want))


MAIN = "three patches, six heads, offset 16"


@pytest.mark.parametrize("name", list(CASES), ids=[c.split(":")[0].split(",")[0] for c in CASES])
def test_pictures_are_the_restatements_byte_for_byte(name):
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256, patches, cm, thr, how, want = case(name)
    before = N.calls
    got = PH.compose_patch_heatmaps(dev(a256), dev(patches), cmap=colormap(cm), threshold=thr, **how)
    assert N.calls == before + 2   # one rank launch, one render launch
    assert set(got) == {"256", "256th"} and all(v.is_cuda for v in got.values())
    for k in got:
        assert same(got[k], want[k]), (k, int((host(got[k]) != want[k]).sum()))
    # a table handed in as an array, and numpy for the patches, are the same pictures
    again = PH.compose_patch_heatmaps(dev(a256), patches, cmap=HH.colour_table_n(colormap(cm)), threshold=thr, **how)
    assert all(same(again[k], want[k]) for k in want)
    # without a threshold there is one picture
    plain = PH.compose_patch_heatmaps(dev(a256), dev(patches), cmap=colormap(cm), **how)
    assert set(plain) == {"256"} and same(plain["256"], want["256"])


def test_a_threshold_of_095_is_the_restatements_picture():
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256, patches, cm, _, how, _ = case("offset 5, table of 1024, alpha 1")
    want = np.stack([PR.pictures(a256[0], patches[0], cmap=colormap(cm), threshold=0.95, **how)["256th"]])
    got = PH.compose_patch_heatmaps(dev(a256), dev(patches), cmap=colormap(cm), threshold=0.95, which=("256th",), **how)
    assert set(got) == {"256th"} and same(got["256th"], want)


@pytest.mark.parametrize("cols", [3, 4, 1])
def test_mosaics_are_get_concat_images_with_unused_tiles_zero(cols):
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256, patches, cm, thr, how, want = case(MAIN)
    got = PH.compose_patch_heatmaps(dev(a256), dev(patches), cmap=cm, threshold=thr, concat=True, cols=cols, **how)
    for k in ("256", "256th"):
        mosaic = np.stack([PR.mosaic(want[k][p], cols) for p in range(3)])
        assert mosaic.shape == (3, -(-6 // cols) * 256, cols * 256, 3)
        assert same(got[k], mosaic), (k, cols)
    if cols == 4:   # two tiles of the second row hold no head
        assert not host(got["256"])[:, 256:, 512:].any() and not host(got["256th"])[:, 256:, 512:].any()


def test_out_buffers_are_reused_and_one_picture_leaves_the_other_alone():
    import torch

    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256, patches, cm, thr, how, want = case(MAIN)
    shape, canary, gap = want["256"].shape, 0xA5, 256
    size = int(np.prod(shape))
    arena = torch.full((2 * size + 3 * gap,), canary, dtype=torch.uint8, device=DEV)
    out = {"256": arena[gap:gap + size].view(shape), "256th": arena[2 * gap + size:2 * gap + 2 * size].view(shape)}
    args = (dev(a256), dev(patches))
    got = PH.compose_patch_heatmaps(*args, cmap=cm, threshold=thr, which=("256th",), out=out, **how)
    assert set(got) == {"256th"} and got["256th"].data_ptr() == out["256th"].data_ptr()
    flat = host(arena)
    assert np.array_equal(flat[2 * gap + size:2 * gap + 2 * size].reshape(shape), want["256th"])
    assert (flat[:2 * gap + size] == canary).all() and (flat[2 * gap + 2 * size:] == canary).all()   # the other buffer and every gap
    got = PH.compose_patch_heatmaps(*args, cmap=cm, which=("256",), out=out, **how)
    assert set(got) == {"256"} and same(out["256"], want["256"]) and same(out["256th"], want["256th"])
    for _ in range(2):   # both, into the same buffers again
        out["256"].zero_()
        out["256th"].zero_()
        got = PH.compose_patch_heatmaps(*args, cmap=cm, threshold=thr, out=out, **how)
        assert all(got[k].data_ptr() == out[k].data_ptr() and same(out[k], want[k]) for k in want)
    flat = host(arena)
    assert (flat[:gap] == canary).all() and (flat[gap + size:2 * gap + size] == canary).all() and (flat[2 * gap + 2 * size:] == canary).all()
    with pytest.raises(ValueError, match="out\\['256'\\]"):
        PH.compose_patch_heatmaps(*args, cmap=cm, out={"256": out["256"][:2]}, **how)
    with pytest.raises(ValueError, match="out\\['256'\\]"):
        PH.compose_patch_heatmaps(*args, cmap=cm, out={"256": out["256"].cpu()}, **how)
    with pytest.raises(ValueError, match="one buffer"):
        PH.compose_patch_heatmaps(*args, cmap=cm, threshold=thr, out={"256": out["256"], "256th": out["256"]}, **how)


def test_a_patchs_pictures_do_not_depend_on_the_batch_or_its_place_in_it():
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256, patches, cm, thr, how, want = case(MAIN)
    alone = PH.compose_patch_heatmaps(dev(a256[1:2]), dev(patches[1:2]), cmap=cm, threshold=thr, **how)
    assert all(same(alone[k], want[k][1:2]) for k in want)
    order = [2, 0, 1, 1]
    moved = PH.compose_patch_heatmaps(dev(a256[order]), dev(patches[order]), cmap=cm, threshold=thr, **how)
    assert all(same(moved[k], want[k][order]) for k in want)


def test_the_launches_are_capturable_and_replay_the_same_bytes():
    import torch

    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256, patches, cm, thr, how, want = case(MAIN)
    args = (dev(a256), dev(patches))
    warm = PH.compose_patch_heatmaps(*args, cmap=cm, threshold=thr, **how)   # (the colour table reaches the device here, once)
    out = {k: torch.zeros_like(v) for k, v in warm.items()}
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
    before = N.calls
    with torch.cuda.graph(graph, stream=stream):
        got = PH.compose_patch_heatmaps(*args, cmap=cm, threshold=thr, out=out, **how)
    assert N.calls == before + 2   # the rank launch and the render launch, neither of them run yet
    for _ in range(2):
        for v in out.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert all(same(got[k], want[k]) for k in want)


# ------------------------------------------------------------------------------------------------------------------------------
# end to end, synthetic ViT weights
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hipt():
    from hipt_abmil_atec23_amd import HIPT_4K, synth
    m = HIPT_4K(None, None, DEV, DEV)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def two_patches():
    from hipt_abmil_atec23_amd import synth
    return synth.hash_u8_np((2, 256, 256, 3), 33)


@pytest.fixture(scope="module")
def raw_maps(hipt, two_patches):
    """a256 [2, 2, nh, 256] the long way: eval_transforms on the host, layer by layer, one get_last_selfattention_cls call."""
    import torch

    from hipt_abmil_atec23_amd import patch_heatmap as PH
    from hipt_abmil_atec23_amd.hipt_model_utils import eval_transforms
    layers = PH.shifted_patches(two_patches)
    x = torch.stack([eval_transforms()(layers[p, l]) for p in range(2) for l in range(2)]).to(DEV)
    with torch.no_grad():
        a = hipt.model256.get_last_selfattention_cls(x)
    assert tuple(a.shape) == (4, 6, 257)
    return a[:, :, 1:].reshape(2, 2, 6, 256).contiguous()


def test_patch_heatmaps_is_compose_of_the_attention_of_the_shifted_patches(hipt, two_patches, raw_maps):
    import torch
    from PIL import Image

    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a256 = PH.patch_attention_maps(hipt.model256, two_patches)
    assert a256.is_cuda and a256.dtype == torch.float32 and torch.equal(a256, raw_maps)
    thr = float(PR.score(host(raw_maps)[0, 0, 0], host(raw_maps)[0, 1, 0], 16)[100, 100])
    want = PH.compose_patch_heatmaps(raw_maps, dev(two_patches), threshold=thr)
    got = PH.patch_heatmaps(hipt.model256, two_patches, threshold=thr)
    assert set(got) == {"256", "256th"} and all(torch.equal(got[k], want[k]) for k in want)
    ref = PR.pictures(host(raw_maps)[1], two_patches[1], cmap=colormap("coolwarm"), threshold=thr)
    assert same(got["256"][1], ref["256"]) and same(got["256th"][1], ref["256th"])
    # one patch, as a PIL image, a device tensor or a list: the same pictures without / with the batch dimension
    one = PH.patch_heatmaps(hipt.model256, Image.fromarray(two_patches[1]), threshold=thr)
    assert all(tuple(one[k].shape) == (6, 256, 256, 3) and torch.equal(one[k], want[k][1]) for k in want)
    one = PH.patch_heatmaps(hipt.model256, dev(two_patches[0]), concat=True)
    assert set(one) == {"256"} and same(one["256"], PR.mosaic(host(want["256"][0]), 3))
    both = PH.patch_heatmaps(hipt.model256, [Image.fromarray(p) for p in two_patches], threshold=thr)
    assert all(torch.equal(both[k], want[k]) for k in want)


def test_create_functions_write_the_references_files(hipt, two_patches, raw_maps, tmp_path):
    from PIL import Image

    from hipt_abmil_atec23_amd import patch_heatmap as PH
    a = host(raw_maps)[0]
    thr = float(PR.score(a[0, 0], a[1, 0], 16)[100, 100])
    want = PR.pictures(a, two_patches[0], cmap=colormap("coolwarm"), threshold=thr)
    assert int((want["score"] == thr).sum()) >= 1
    files = PH.create_patch_heatmaps_indiv(Image.fromarray(two_patches[0]), hipt.model256, str(tmp_path), "p0", threshold=thr,
                                           device256="ignored")
    names = {"p0_256[%d].png" % i: want["256"][i] for i in range(6)}
    names.update({"p0_256th[%d].png" % i: want["256th"][i] for i in range(6)})
    assert sorted(os.listdir(tmp_path)) == sorted(names) and sorted(os.path.basename(f) for f in files) == sorted(names)
    files = PH.create_patch_heatmaps_concat(Image.fromarray(two_patches[0]), hipt.model256, str(tmp_path), "p0", threshold=thr)
    assert [os.path.basename(f) for f in files] == ["p0_256th.png", "p0_256hm.png"]
    names.update({"p0_256hm.png": PR.mosaic(want["256"], 3), "p0_256th.png": PR.mosaic(want["256th"], 3)})
    for name, img in names.items():
        assert np.array_equal(np.array(Image.open(tmp_path / name)), img), name


def test_concat_select_is_the_grid_of_hierarchical_heatmaps_own_pictures(hipt, tmp_path):
    from PIL import Image

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    from hipt_abmil_atec23_amd import synth
    region = synth.hash_u8_np((512, 768, 3), 21)
    hs, ws = 128, 192
    base = np.array(Image.fromarray(region).resize((ws, hs)))
    pics = {k: host(v) for k, v in HH.hierarchical_heatmaps(hipt, region, pairs=[(0, 2), (5, 2)]).items()}
    grid = np.concatenate([np.concatenate([base, pics["4k"][0], pics["4k"][5]], axis=1),
                           np.concatenate([pics["256"][2], pics["blend"][0], pics["blend"][1]], axis=1)])
    got = HH.hierarchical_heatmaps_concat_select(hipt, region)
    assert got.is_cuda and same(got, grid)
    # other heads, two rows of ViT-256 heads
    pairs = [(3, 1), (3, 4)]
    pics = {k: host(v) for k, v in HH.hierarchical_heatmaps(hipt, region, pairs=pairs, alpha=0.3).items()}
    grid = np.concatenate([np.concatenate([base, pics["4k"][3]], axis=1), np.concatenate([pics["256"][1], pics["blend"][0]], axis=1),
                           np.concatenate([pics["256"][4], pics["blend"][1]], axis=1)])
    assert same(HH.hierarchical_heatmaps_concat_select(hipt, region, heads4k=(3,), heads256=(1, 4), alpha=0.3), grid)
    path = HH.create_hierarchical_heatmaps_concat_select(Image.fromarray(region), hipt, str(tmp_path), "r0")
    assert os.path.basename(path) == "r0_heatmap.png" and os.listdir(tmp_path) == ["r0_heatmap.png"]
    assert np.array_equal(np.array(Image.open(path)), host(got))
