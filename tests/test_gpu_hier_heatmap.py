"""GPU tests of the hierarchical heat-maps (csrc/hier_heatmap.hip through hipt_abmil_atec23_amd.hier_heatmap).
Every comparison is exact: float64 ranks as their int64 views, pictures byte for byte, against the numpy restatement
tests/hier_heatmap_ref.py, which upscales, ranks with scipy and slices as the reference does.  Inputs are seeded.

Without the kernels every test here fails: the module, the entry points and the method do not exist."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hier_heatmap_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("4k", "256", "blend", "256th")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    return t.detach().cpu().numpy()


def colormap(name):
    import matplotlib

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    return HH.half_jet() if name == "half_jet" else matplotlib.colormaps[name]


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("f", [1, 4, 16])
def test_ranks_are_scipys_on_the_upscaled_vectors(f, ties):
    import torch

    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    before = N.calls
    shapes = ((1, 1), (3, 2), (7, 255), (5, 256), (2, 257), (1, 4096))
    for v, l in shapes:
        x = HR.rank_case(v, l, 10 * l + f, ties)
        if ties and l >= 255:
            assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
        want = HR.long_way_percentiles(x, f)
        got = HH.hier_ranks(torch.from_numpy(x).to(DEV), f)
        assert got.dtype == torch.float64 and tuple(got.shape) == (v, l)
        assert np.array_equal(bits(host(got)), bits(want)), (v, l, f, int((bits(host(got)) != bits(want)).sum()))
    assert N.calls == before + len(shapes)


# (grid, scale, offset, heads, colormap, w256, alpha, pairs)
CASES = {
    "1x1 scale 4: layers 3 and 4 absent": ((1, 1), 4, 128, 6, "coolwarm", 2, 0.5, None),
    "2x3 scale 4, offsets of 25 pixels": ((2, 3), 4, 100, 6, "half_jet", 1, 0.3, None),
    "3x2 scale 16: one pixel a token": ((3, 2), 16, 128, 6, "coolwarm", 1, 0.5, None),
    "16x16 scale 16: the reference's grid": ((16, 16), 16, 128, 6, "half_jet", 2, 0.3, None),
    "2x2 scale 1, two heads, one pair": ((2, 2), 1, 128, 2, "coolwarm", 2, 0.5, [(1, 0)]),
}
_memo = {}


def case(name):
    """The inputs of a case, the threshold picked from the restatement's own scores, and the restatement's pictures (made once)."""
    if name not in _memo:
        (w, h), scale, offset, nh, cm, w256, alpha, pairs = CASES[name]
        a256, a4k = HR.synthetic_maps(w, h, nh, 5 + len(name))
        b = 256 // scale
        base = np.random.default_rng(1).integers(0, 256, (w * b, h * b, 3), dtype=np.uint8)
        how = dict(offset=offset, scale=scale, alpha=alpha, w256=w256, pairs=pairs)
        sc = HR.scores(a256, a4k, w, h, offset, scale)[2][0]
        thr = float(sc[sc.shape[0] // 2, sc.shape[1] // 2])   # the score of a pixel: its whole token is exactly AT the threshold
        want = HR.pictures(a256, a4k, w, h, base, cmap=colormap(cm), threshold=thr, **how)
        equal = sum(int((s == thr).sum()) for s in want["score256"])
        assert equal > 0 and any((s < thr).any() and (s > thr).any() for s in want["score256"])
        _memo[name] = (a256, a4k, w, h, base, cm, thr, how, want)
    return _memo[name]


@pytest.mark.parametrize("name", list(CASES), ids=[c.split(":")[0].split(",")[0] for c in CASES])
def test_pictures_are_the_restatements_byte_for_byte(name):
    import torch

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k, w, h, base, cm, thr, how, want = case(name)
    got = HH.compose_heatmaps(torch.from_numpy(a256).to(DEV), torch.from_numpy(a4k).to(DEV), w, h, torch.from_numpy(base).to(DEV),
                              cmap=cm, threshold=thr, **how)
    assert set(got) == set(KEYS)
    for k in KEYS:
        g = host(got[k])
        assert g.dtype == np.uint8 and g.shape == want[k].shape, (k, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (k, int((g != want[k]).sum()))
    # a table handed in as an array, and numpy for the base image, are the same pictures
    again = HH.compose_heatmaps(torch.from_numpy(a256).to(DEV), torch.from_numpy(a4k).to(DEV), w, h, base, cmap=HH.colour_table_n(cm),
                                threshold=thr, which=("256th", "4k"), **{k: v for k, v in how.items() if k != "pairs"})
    assert set(again) == {"4k", "256th"} and all(np.array_equal(host(again[k]), want[k]) for k in again)


def test_threshold_of_exactly_095_counts_as_above():
    """mask[mask > thr] = 0.95 leaves a score equal to a threshold of 0.95 holding the very value that marks 'above'."""
    import torch

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k, w, h, base, cm, _, how, _ = case("1x1 scale 4: layers 3 and 4 absent")
    want = HR.pictures(a256, a4k, w, h, base, cmap=colormap(cm), threshold=0.95, **how)
    got = HH.compose_heatmaps(torch.from_numpy(a256).to(DEV), torch.from_numpy(a4k).to(DEV), w, h, base, cmap=cm, threshold=0.95,
                              which=("256th",), **how)
    assert np.array_equal(host(got["256th"]), want["256th"])


def test_absent_outputs_are_left_alone_and_nothing_is_written_past_an_output():
    import torch

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k, w, h, base, cm, thr, how, want = case("2x3 scale 4, offsets of 25 pixels")
    nh, (hs, ws, _) = a4k.shape[1], base.shape
    shapes = {"4k": (nh, hs, ws, 3), "256": (nh, hs, ws, 3), "blend": (nh * nh, hs, ws, 3), "256th": (nh, hs, ws, 3)}
    gap, canary = 256, 0xA5
    sizes = {k: int(np.prod(s)) for k, s in shapes.items()}
    arena = torch.full((sum(sizes.values()) + gap * (len(sizes) + 1),), canary, dtype=torch.uint8, device=DEV)
    out, spans, at = {}, {}, gap
    for k in KEYS:
        out[k], spans[k] = arena[at:at + sizes[k]].view(shapes[k]), (at, at + sizes[k])
        at += sizes[k] + gap
    args = (torch.from_numpy(a256).to(DEV), torch.from_numpy(a4k).to(DEV), w, h, torch.from_numpy(base).to(DEV))
    got = HH.compose_heatmaps(*args, cmap=cm, which=("blend",), out=out, **how)
    assert set(got) == {"blend"} and got["blend"].data_ptr() == out["blend"].data_ptr()
    flat = host(arena)
    lo, hi = spans["blend"]
    assert np.array_equal(flat[lo:hi].reshape(shapes["blend"]), want["blend"])
    rest = np.ones(flat.shape, dtype=bool)
    rest[lo:hi] = False
    assert (flat[rest] == canary).all()   # the three other buffers and every gap
    got = HH.compose_heatmaps(*args, cmap=cm, threshold=thr, which=KEYS, out=out, **how)
    flat = host(arena)
    rest[:] = True
    for k in KEYS:
        lo, hi = spans[k]
        assert np.array_equal(flat[lo:hi].reshape(shapes[k]), want[k]), k
        rest[lo:hi] = False
    assert (flat[rest] == canary).all()   # the gaps in front of, between and behind the outputs


def test_the_launches_are_capturable_and_replay_the_same_bytes():
    import torch

    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k, w, h, base, cm, thr, how, want = case("3x2 scale 16: one pixel a token")
    args = (torch.from_numpy(a256).to(DEV), torch.from_numpy(a4k).to(DEV), w, h, torch.from_numpy(base).to(DEV))
    warm = HH.compose_heatmaps(*args, cmap=cm, threshold=thr, **how)   # (the colour table reaches the device here, once)
    out = {k: torch.zeros_like(v) for k, v in warm.items()}
    torch.cuda.synchronize()
    stream, graph = torch.cuda.Stream(device=DEV), torch.cuda.CUDAGraph()
    before = N.calls
    with torch.cuda.graph(graph, stream=stream):
        got = HH.compose_heatmaps(*args, cmap=cm, threshold=thr, out=out, **how)
    assert N.calls == before + 3   # two rank launches and the render launch, none of them run yet
    for _ in range(2):
        for v in out.values():
            v.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for k in KEYS:
            assert np.array_equal(host(got[k]), want[k]), k


@pytest.fixture(scope="module")
def hipt():
    from hipt_abmil_atec23_amd import HIPT_4K, synth
    m = HIPT_4K(None, None, DEV, DEV)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    return m.eval().to(DEV)


@pytest.fixture(scope="module")
def region():
    from hipt_abmil_atec23_amd import synth
    return synth.hash_u8_np((512, 768, 3), 21)


@pytest.fixture(scope="module")
def raw_maps(hipt, region):
    import torch

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k = HH.region_attention_maps(hipt, HH.shifted_regions(torch.from_numpy(region).to(DEV)))
    assert a256.is_cuda and a4k.is_cuda and tuple(a256.shape) == (4, 6, 6, 256) and tuple(a4k.shape) == (4, 6, 6)
    return host(a256), host(a4k)


def test_region_attention_maps_are_the_scores_of_each_region_alone(hipt, region, raw_maps):
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k = raw_maps
    up256, up4k = HR.upscaled_maps(a256, a4k, 2, 3, 4)
    for r, shifted in enumerate(HH.shifted_regions(region)):
        _, want256, want4k = hipt._get_region_attention_scores(shifted, scale=4)
        assert np.array_equal(up256[r], want256) and np.array_equal(up4k[r], want4k), r


def test_hierarchical_heatmaps_end_to_end(hipt, region, raw_maps):
    from PIL import Image

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k = raw_maps
    base = np.array(Image.fromarray(region).resize((768 // 4, 512 // 4)))
    want = HR.pictures(a256, a4k, 2, 3, base, cmap=colormap("coolwarm"))
    got = HH.hierarchical_heatmaps(hipt, region)
    assert set(got) == {"4k", "256", "blend"} and all(v.is_cuda for v in got.values())
    for k in got:
        assert np.array_equal(host(got[k]), want[k]), k


def test_the_method_returns_the_references_three_lists(hipt, region):
    """The half-jet table, the 256 level weighing 1, PIL images out.  The method sees the region through tensorbatch2im
    (hipt_4k.py:185), whose truncation moves some bytes of a normalised image down by one: the restatement gets that region."""
    import torch
    from PIL import Image

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    from hipt_abmil_atec23_amd.hipt_model_utils import eval_transforms, tensorbatch2im
    x = eval_transforms()(region).unsqueeze(0)
    seen = tensorbatch2im(x)[0]
    a256, a4k = (host(t) for t in HH.region_attention_maps(hipt, HH.shifted_regions(torch.from_numpy(seen).to(DEV))))
    base = np.array(Image.fromarray(seen).resize((768 // 4, 512 // 4)))
    hm4k, hm256, hm4k_256 = hipt.get_region_attention_heatmaps(x)
    want = HR.pictures(a256, a4k, 2, 3, base, cmap=colormap("half_jet"), w256=1)
    assert (len(hm4k), len(hm256), len(hm4k_256)) == (6, 6, 36)
    for imgs, k in ((hm4k, "4k"), (hm256, "256"), (hm4k_256, "blend")):
        assert all(np.array_equal(np.array(img), want[k][i]) for i, img in enumerate(imgs)), k


def test_create_hierarchical_heatmaps_indiv_writes_the_references_files(hipt, region, raw_maps, tmp_path):
    from PIL import Image

    from hipt_abmil_atec23_amd import hier_heatmap as HH
    a256, a4k = raw_maps
    base = np.array(Image.fromarray(region).resize((768 // 4, 512 // 4)))
    sc = HR.scores(a256, a4k, 2, 3, 128, 4)[2][0]
    thr = float(sc[70, 90])
    want = HR.pictures(a256, a4k, 2, 3, base, cmap=colormap("coolwarm"), threshold=thr)
    files = HH.create_hierarchical_heatmaps_indiv(Image.fromarray(region), hipt, str(tmp_path), "r0", threshold=thr)
    names = {"r0_1024[%d].png" % j: want["4k"][j] for j in range(6)}
    names.update({"r0_256[%d].png" % i: want["256"][i] for i in range(6)})
    names.update({"r0_256th[%d].png" % i: want["256th"][i] for i in range(6)})
    names.update({"r0_factorized_4k[%d]_256[%d].png" % (j, i): want["blend"][j * 6 + i] for j in range(6) for i in range(6)})
    assert sorted(os.listdir(tmp_path)) == sorted(names) and sorted(os.path.basename(f) for f in files) == sorted(names)
    for name, img in names.items():
        assert np.array_equal(np.array(Image.open(tmp_path / name)), img), name
