"""CPU tests of the heat-map score ranks: the numpy restatement tests/heatmap_scores_ref.py against scipy itself, bit
for bit; the C ABI entry declared, exported and bound; the argument checks of the Python layer, which raise before any native call;
``sample_rois`` on numpy input against a literal restatement of the reference's function; the drop-in hook."""
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_scores_ref as S  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import heatmap as H  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def edge_cases():
    """(name, q, ref): ties, all-equal input, both zeros, infinities, denormals, float32-origin values, nref = 1, nq != nref."""
    rng = np.random.default_rng(5)
    den = np.array([5e-324, -5e-324, 2.0 ** -1060, 0.0, -0.0, 2.2250738585072014e-308, 1e-310, 1e-310])
    f32 = rng.standard_normal(300).astype(np.float32)
    return [
        ("random", rng.standard_normal(257), rng.standard_normal(1031)),
        ("ties", *S.case(300, 500, 1, True)),
        ("all equal", np.full(40, 0.3), np.full(77, 0.3)),
        ("zeros", np.array([0.0, -0.0, 1.0, -1.0]), np.array([-0.0, 0.0, 0.0, -0.0, 1.0])),
        ("infinities", np.array([-np.inf, np.inf, 0.0, 1e308]), np.array([np.inf, -np.inf, np.inf, 0.0, -1e308])),
        ("denormals", den[rng.permutation(len(den))], den),
        ("float32 origin", f32[:120].astype(np.float64), f32.astype(np.float64)),
        ("nref 1", np.array([-1.0, 0.5, 2.0]), np.array([0.5])),
        ("nq 1", np.array([0.1]), rng.integers(0, 5, 64) / 4.0),
        ("integers", rng.integers(0, 9, 1000).astype(np.float64), rng.integers(0, 9, 333).astype(np.float64)),
    ]


@pytest.mark.parametrize("name,q,ref", edge_cases(), ids=[c[0] for c in edge_cases()])
def test_restatement_is_scipy_bit_for_bit(name, q, ref):
    from scipy.stats import percentileofscore, rankdata   # (importable on the build machine: this test runs there)
    assert np.array_equal(bits(S.percentiles(q, ref, S.OF_SCORE)), bits(percentileofscore(ref, q)))
    for x in (q, ref):
        want = rankdata(x, "average") / len(x) * 100
        assert np.array_equal(bits(S.percentiles(x, x, S.RANKDATA)), bits(want))
        assert np.array_equal(bits(H.to_percentiles(x)), bits(want))   # the package's numpy route


def test_float32_storage_restatement_is_the_reference_loop():
    from scipy.stats import percentileofscore
    rng = np.random.default_rng(6)
    a = rng.standard_normal((50, 1)).astype(np.float32)
    ref = np.concatenate([rng.standard_normal(211), a[:7, 0].astype(np.float64)])
    want = a.copy()
    for i in range(len(want)):
        want[i] = percentileofscore(ref, want[i])
    got = S.score2percentile_loop_f32(a, ref)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))


def test_entry_point_is_declared_exported_and_bound_under_abi_6():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"\bint hipt_score_counts\(const double\* q, int64_t nq, const double\* ref, int64_t nref,\s*int mode, int32_t\* less, "
                     r"int32_t\* leq,\s*double\* pct, void\* stream\);", hdr)
    assert re.search(r"#define HIPT_ABI_VERSION 6\b", hdr) and N.ABI_VERSION == 6
    assert f"#define HIPT_PCT_REF_TILE {N.PCT_REF_TILE}\n" in hdr and f"#define HIPT_PCT_QUERIES_PER_WG {N.PCT_QUERIES_PER_WG}\n" in hdr
    assert re.search(r"HIPT_PCT_RANKDATA = 0, HIPT_PCT_OF_SCORE = 1", hdr) and (N.PCT_RANKDATA, N.PCT_OF_SCORE) == (0, 1)
    assert "hipt_score_counts" in N.SIGNATURES and len(N.SIGNATURES["hipt_score_counts"][1]) == 9
    lib = N.lib()
    assert hasattr(lib, "hipt_score_counts") and lib.hipt_abi_version() == 6
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert " percentile.hip " in mk and "FLAGS_percentile.hip = -ffp-contract=off" in mk


def test_empty_calls_and_bad_modes_through_the_c_abi():
    """Host-side decisions of the entry point, made before any launch: nq = 0 or nref = 0 is HIPT_OK with nothing touched (the
    pointers here are never followed); an unknown mode and nref >= 2^31 are refused."""
    lib = N.lib()
    fake = 1 << 20
    assert lib.hipt_score_counts(fake, 0, fake, 10, 0, fake, fake, fake, None) == 0
    assert lib.hipt_score_counts(fake, 10, fake, 0, 1, fake, fake, fake, None) == 0
    assert lib.hipt_score_counts(None, 0, None, 0, 0, None, None, None, None) == 0
    assert lib.hipt_score_counts(fake, 10, fake, 10, 2, fake, fake, fake, None) == -1
    assert lib.hipt_score_counts(fake, -1, fake, 10, 0, fake, fake, fake, None) == -1
    assert lib.hipt_score_counts(fake, 10, fake, 2 ** 31, 0, fake, fake, fake, None) == -4 and b"int32" in lib.hipt_last_error()
    assert lib.hipt_score_counts(fake, 10, fake, 10, 0, None, None, None, None) == -1   # no output asked for
    assert lib.hipt_score_counts(fake, 10, fake + 4, 10, 0, fake, fake, fake, None) == -1   # misaligned reference


def test_argument_checks_raise_before_any_native_call():
    good = np.linspace(0, 1, 9)
    nan = good.copy()
    nan[4] = np.nan
    before = N.calls
    for fn in (H.score_counts, H.score2percentile):
        with pytest.raises(ValueError, match="scores contain NaN"):
            fn(nan, good)
        with pytest.raises(ValueError, match="ref_scores contain NaN"):
            fn(good, nan)
        with pytest.raises(ValueError, match="ref_scores contain NaN"):
            fn(torch.from_numpy(good), torch.from_numpy(nan))
        with pytest.raises(ValueError, match="empty"):
            fn(good, np.zeros(0))
        with pytest.raises(ValueError, match="empty"):
            fn(torch.from_numpy(good), torch.zeros(0, dtype=torch.float64))
        with pytest.raises(ValueError, match="different devices"):
            fn(torch.from_numpy(good), torch.zeros(3, device="meta"))
    with pytest.raises(ValueError, match="NaN"):
        H.sample_rois(torch.from_numpy(nan), np.zeros((9, 2), dtype=np.int64))
    with pytest.raises(ValueError, match="NaN"):
        H.to_percentiles(torch.from_numpy(nan))
    with pytest.raises(ValueError, match="empty"):
        H.compute_from_batches(None, None, [], ref_scores=np.zeros(0))
    with pytest.raises(ValueError, match="NaN"):
        H.compute_from_batches(None, None, [], ref_scores=nan)
    with pytest.raises(NotImplementedError):
        H.sample_rois(good, np.zeros((9, 2), dtype=np.int64), mode="median")
    assert N.calls == before


def rois(seed=3, n=400):
    rng = np.random.default_rng(seed)
    scores = rng.integers(0, 60, n).astype(np.float64) / 7.0   # ties
    coords = np.stack([rng.integers(0, 50, n) * 256, rng.integers(0, 40, n) * 256], axis=1)
    return scores, coords


@pytest.mark.parametrize("box", [None, ((2560, 1024), (9000, 8000))], ids=["whole", "screened"])
@pytest.mark.parametrize("mode,kw", [("topk", {}), ("reverse_topk", {}), ("range_sample", dict(score_start=40.0, score_end=60.0)),
                                     ("range_sample", dict(score_start=44.0, score_end=48.0, k=50))])
def test_sample_rois_on_numpy_input_is_the_reference_function(mode, kw, box):
    scores, coords = rois()
    tl, br = box if box else (None, None)
    kw = dict(dict(k=7, seed=11), **kw)
    keep = scores.copy()
    want = S.sample_rois_ref(scores.reshape(-1, 1), coords, mode=mode, top_left=tl, bot_right=br, **kw)
    before = N.calls
    got = H.sample_rois(scores.reshape(-1, 1), coords, mode=mode, top_left=tl, bot_right=br, **kw)
    assert N.calls == before and np.array_equal(scores, keep)   # numpy ranks on the host path
    assert set(got) == {"sampled_coords", "sampled_scores"}
    assert len(want["sampled_scores"]) == min(kw["k"], len(want["sampled_scores"])) and len(want["sampled_scores"]) > 0
    assert np.array_equal(got["sampled_coords"], want["sampled_coords"])
    assert np.array_equal(bits(got["sampled_scores"]), bits(want["sampled_scores"]))


def test_sample_rois_empty_window_returns_the_last_patch_as_the_reference_does():
    scores, coords = rois()
    want = S.sample_rois_ref(scores, coords, mode="range_sample")   # the defaults 0.45 .. 0.55 lie below every percentile of 400 scores
    got = H.sample_rois(scores, coords, mode="range_sample")
    assert np.ndim(want["sampled_scores"]) == 0 and want["sampled_coords"].shape == (2,)
    assert np.array_equal(got["sampled_coords"], coords[-1]) and np.array_equal(got["sampled_coords"], want["sampled_coords"])
    assert float(got["sampled_scores"]) == float(want["sampled_scores"]) == float(H.to_percentiles(scores)[-1])


# ---- drop-in hook --------------------------------------------------------------------------------------------------------------
@pytest.fixture
def fake_wsi_utils(monkeypatch):
    """A stand-in for the reference's wsi_core.wsi_utils module (the real one needs h5py and cv2)."""
    pkg = types.ModuleType("wsi_core")
    pkg.__path__ = []
    mod = types.ModuleType("wsi_core.wsi_utils")
    mod.to_percentiles = lambda scores: "reference"
    mod.sample_rois = lambda scores, coords, **kw: "reference"
    mod.screen_coords = lambda *a: "reference"
    pkg.wsi_utils = mod
    monkeypatch.setitem(sys.modules, "wsi_core", pkg)
    monkeypatch.setitem(sys.modules, "wsi_core.wsi_utils", mod)
    return mod


def test_install_binds_the_score_functions_only_when_asked(fake_wsi_utils):
    from hipt_abmil_atec23_amd import dropin
    original = (fake_wsi_utils.to_percentiles, fake_wsi_utils.sample_rois, fake_wsi_utils.screen_coords)
    try:
        done = dropin.install()
        assert (fake_wsi_utils.to_percentiles, fake_wsi_utils.sample_rois) == original[:2] and not any("wsi_utils" in k for k in done)
        done = dropin.install(heatmap_scores=True)
        assert fake_wsi_utils.to_percentiles is H.to_percentiles and fake_wsi_utils.sample_rois is H.sample_rois
        assert fake_wsi_utils.screen_coords is original[2]
        assert done["wsi_core.wsi_utils.sample_rois"].endswith("heatmap.sample_rois")
        dropin.install(heatmap_scores=True)   # twice: the saved originals are not overwritten
    finally:
        dropin.uninstall()
    assert (fake_wsi_utils.to_percentiles, fake_wsi_utils.sample_rois, fake_wsi_utils.screen_coords) == original


def test_install_heatmap_scores_is_a_no_op_without_the_reference(monkeypatch):
    from hipt_abmil_atec23_amd import dropin
    monkeypatch.delitem(sys.modules, "wsi_core.wsi_utils", raising=False)
    monkeypatch.delitem(sys.modules, "wsi_core", raising=False)
    try:
        done = dropin.install(heatmap_scores=True)
        assert not any("wsi_utils" in k for k in done) and "wsi_core.wsi_utils" not in sys.modules
    finally:
        dropin.uninstall()


def test_public_names():
    import hipt_abmil_atec23_amd as amd
    for name in ("score_counts", "to_percentiles", "score2percentile", "sample_rois", "compute_from_batches"):
        assert getattr(amd, name) is getattr(H, name)
