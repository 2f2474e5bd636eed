"""DRAS-MIL sampling, host side (no GPU): tests/sampling_ref.py against the goldens written by the reference's own functions and
sklearn (tests/golden/make_golden_sampling.py), the package's host functions, the configuration, the drop-in and the ABI."""
import argparse
import os
import random
import re
import sys

import numpy as np
import pytest

from conftest import ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import sampling_ref as R  # noqa: E402

DRAW_SEED = 1234   # make_golden_sampling.py


def _draw_cases():
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_sampling as G
    return G.draw_cases()


# ---- sampling_ref vs the reference's outputs -------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,neighbors", R.UPDATE_CASES)
def test_ref_update_bit_equal_to_reference(mode, neighbors):
    g = golden("dras_update")
    w0, scores, ids, sampled = R.update_fixture()
    assert np.array_equal(w0, g["w0"]) and np.array_equal(scores, g["scores"]) and np.array_equal(ids, g["ids"])
    w = R.update_sampling_weights(w0, scores, sampled, ids, neighbors, power=0.15, normalise=False, sampling_update=mode)
    assert np.array_equal(w, g[f"w_{mode}_{neighbors}"])   # bit for bit: the same float64 operations in the same order
    assert np.array_equal(w0, g["w0"]), "the restated function must not write to its input"


def test_update_golden_covers_what_it_should():
    g = golden("dras_update")
    _, scores, ids, _ = R.update_fixture()
    assert (scores == 0).sum() == 1
    counts = np.bincount(ids.ravel())
    assert counts.max() >= 3                                    # repeated targets
    assert not np.array_equal(g["w_average_8"], g["w_average_5"]) and not np.array_equal(g["w_max_8"], g["w_max_5"])
    assert not np.array_equal(g["w_newest_8"], g["w0"])         # the zeroing happened
    z = g["w0"].copy()
    z[g["sampled"]] = 0
    assert np.array_equal(g["w_newest_8"], z)                   # ... and nothing else ('newest' never reaches the weights)
    # the 'average' result depends on the fold order: folding the rows backwards gives other bits
    w0, scores, ids, sampled = R.update_fixture()
    back = R.update_sampling_weights(w0, scores[::-1], sampled, ids[::-1], 8, normalise=False, sampling_update="average")
    assert not np.array_equal(back, g["w_average_8"])


@pytest.mark.parametrize("impl", ["ref", "package"])
def test_draws_equal_reference(impl):
    g = golden("dras_draws")
    if impl == "ref":
        fn = R.generate_sample_idxs
    else:
        from hipt_abmil_atec23_amd import sampling
        fn = sampling.generate_sample_idxs
    for name, kw in _draw_cases():
        np.random.seed(DRAW_SEED)
        random.seed(DRAW_SEED)
        got = [int(i) for i in fn(**kw)]
        assert got == [int(i) for i in g[name]], name
        assert len(set(got)) == len(got)


@pytest.mark.parametrize("dup", [False, True])
def test_ref_spatial_knn_vs_sklearn(dup):
    g = golden("dras_knn")
    tag = "spatial_dup" if dup else "spatial"
    c = R.spatial_fixture(dup)
    assert c.max() > 1e5 and float(c.max()) ** 2 > 2 ** 24 * 256   # squared distances beyond fp32's integers
    q = R.query_fixture(len(c), 100)
    ids, dist, d2 = R.knn_spatial(c, q, 64)
    assert np.array_equal(dist, g[tag + "_dist"])                   # sorted distances: exactly sklearn's
    untied = np.ones_like(d2, dtype=bool)
    untied[:, 1:] &= d2[:, 1:] != d2[:, :-1]
    untied[:, :-1] &= d2[:, :-1] != d2[:, 1:]
    nxt = R.knn_spatial(c, q, 65)[2][:, 64]
    untied[:, -1] &= d2[:, -1] != nxt
    assert untied.mean() > 0.02 and np.array_equal(ids[untied], g[tag + "_ids"].astype(np.int64)[untied])
    # the defined order: ties by index, self first unless a duplicate with a lower index exists
    assert np.all((d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (ids[:, 1:] > ids[:, :-1])))
    assert np.all(d2[:, 0] == 0) and np.all(ids[:, 0] <= q)


@pytest.mark.parametrize("n,d,seed", R.TEXTURAL_CASES)
def test_ref_textural_knn_vs_sklearn(n, d, seed):
    g = golden("dras_knn")
    X = R.textural_fixture(n, d, seed)
    q = R.query_fixture(n, 100)
    for k in (20, 64):
        ids, dist, d2 = R.knn_textural(X, q, k)
        excused = R.textural_excused(d2, k, R.textural_gamma(d))
        assert np.array_equal(ids[~excused], g[f"textural_{n}_{d}_ids"].astype(np.int64)[:, :k][~excused])
        np.testing.assert_allclose(dist, g[f"textural_{n}_{d}_dist"][:, :k], rtol=1e-12, atol=1e-12)


def test_textural_fixtures_keep_near_ties_under_one_percent():
    """The condition on the GPU test's inputs: positions whose neighbouring float64 distances are within 2 * gamma relative
    (where an fp32 kernel may return either index) are at most 1 % of all positions of the textural test.  Measured with the
    decaying-spectrum fixture: (5000,192) 0.10 % / 0.16 % (k = 20 / 64), (3000,1024) 0.30 % / 1.22 %, (777,384) 0.10 % / 0.22 %;
    0.44 % of all 25 200 positions.  (Isotropic uniform features give 1.2-4 %, 15-40 % and 2-9 % for every seed tried.)"""
    excused = total = 0
    for n, d, seed in R.TEXTURAL_CASES:
        d2 = R.knn_textural(R.textural_fixture(n, d, seed), R.query_fixture(n, 100), 64)[2]
        for k in (20, 64):
            e = R.textural_excused(d2[:, :k + 1], k, R.textural_gamma(d))
            print(f"({n},{d}) k={k}: {e.mean():.4%} near-ties")
            excused, total = excused + int(e.sum()), total + e.size
    assert excused <= 0.01 * total, f"{excused} of {total} positions are near-ties: change the seeds"


# ---- configuration / validation ----------------------------------------------------------------------------------------------
def test_sampling_config_defaults_and_from_args():
    from hipt_abmil_atec23_amd import SamplingConfig
    c = SamplingConfig()
    assert (c.samples_per_iteration, c.resampling_iterations, c.sampling_random, c.sampling_random_delta) == (100, 10, 0.2, 0.02)
    assert (c.sampling_neighbors, c.sampling_neighbors_delta, c.sampling_type, c.use_all_samples) == (20, 0, "spatial", False)
    assert (c.final_sample_size, c.retain_best_samples, c.initial_grid_sample, c.sampling_average) == (100, 100, False, False)
    assert (c.weight_smoothing, c.fully_random) == (0.15, False)
    ns = argparse.Namespace(samples_per_iteration=50, sampling_type="textural", sampling_average=True, weight_smoothing=0.3,
                            unrelated_flag=1, sampling=True)
    c = SamplingConfig.from_args(ns)
    assert (c.samples_per_iteration, c.sampling_type, c.sampling_average, c.weight_smoothing, c.resampling_iterations) == (50, "textural", True, 0.3, 10)


@pytest.mark.parametrize("kw", [dict(sampling_type="cubic"), dict(sampling_neighbors=65), dict(sampling_neighbors=0),
                                dict(samples_per_iteration=0), dict(weight_smoothing=0.0), dict(samples_per_iteration=5000),
                                dict(sampling_neighbors=8, sampling_neighbors_delta=1, resampling_iterations=10)])
def test_sampling_config_rejects(kw):
    from hipt_abmil_atec23_amd import SamplingConfig
    with pytest.raises(ValueError):
        SamplingConfig(**kw)


def test_argument_validation_without_a_device():
    import torch
    from hipt_abmil_atec23_amd import SamplingConfig, sampling
    with pytest.raises(RuntimeError, match="HIP device"):
        sampling.knn(torch.zeros((10, 2), dtype=torch.int64), [0], 3)
    with pytest.raises(ValueError, match="spatial or|'spatial' or"):
        sampling.prepare_points(torch.zeros((10, 2), dtype=torch.int64), "other")
    with pytest.raises(RuntimeError, match="HIP device"):
        sampling.update_sampling_weights(torch.zeros(4, dtype=torch.float64), torch.zeros(1), [0], torch.zeros((1, 2), dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="exactly one"):
        sampling.dras_eval_slide(None, np.zeros((5, 2), dtype=np.int64), SamplingConfig())
    with pytest.raises(ValueError, match="exactly one"):
        sampling.dras_eval_slide(None, np.zeros((5, 2), dtype=np.int64), SamplingConfig(), data=torch.zeros(5, 4), feature_fn=lambda i: None)
    with pytest.raises(ValueError, match="spatial only"):
        sampling.dras_eval_slide(None, np.zeros((5, 2), dtype=np.int64), SamplingConfig(sampling_type="textural"), feature_fn=lambda i: None)
    with pytest.raises(RuntimeError, match="HIP device"):
        sampling.dras_eval_slide(None, np.zeros((5, 2), dtype=np.int64), SamplingConfig(), data=torch.zeros(5, 4))


def test_ref_loop_invariants_and_shortcuts():
    """The restated loop over the CPU oracle: sizes, no repeats, the short-cut branches."""
    import torch
    from hipt_abmil_atec23_amd import SamplingConfig, synth
    from oracle import torch_cpu as T
    specs = synth.clam_param_specs((384, 128, 64))
    p = T.to_torch(synth.make_params_np(specs, 384))

    def model_fn(rows):
        lo, pr, yh, a, _ = T.clam_sb_forward(torch.as_tensor(rows), p)
        return lo.numpy(), pr.numpy(), yh.numpy(), a.numpy()
    n = 900
    data = synth.hash_uniform_np((n, 384), 5)
    coords = R.spatial_fixture()[:n]
    cfg = SamplingConfig(samples_per_iteration=40, resampling_iterations=4, final_sample_size=40, retain_best_samples=30, sampling_neighbors=8)
    np.random.seed(3)
    random.seed(3)
    r = R.dras_eval_slide(model_fn, coords, cfg, data)
    assert len(r["sample_idxs"]) == 40 and len(set(r["all_sample_idxs"])) == len(r["all_sample_idxs"]) == 4 * 40 + 10
    assert len(r["round_Y_prob"]) == 5 and np.all(r["weights"][r["all_sample_idxs"][:160]] == 0)
    full = R.dras_eval_slide(model_fn, coords[:150], cfg, data[:150])       # 150 < 4 * 40 + 40: the whole bag
    assert full["sample_idxs"] == list(range(150)) and np.array_equal(full["logits"], model_fn(data[:150])[0])
    rnd = R.dras_eval_slide(model_fn, coords, SamplingConfig(samples_per_iteration=40, fully_random=True), data)
    assert len(rnd["sample_idxs"]) == 40 and rnd["weights"] is None


# ---- drop-in -----------------------------------------------------------------------------------------------------------------
def test_dropin_sampling_registration():
    import hipt_abmil_atec23_amd as amd
    from hipt_abmil_atec23_amd import dropin, sampling
    had = {k: sys.modules.get(k) for k in ("utils", "utils.sampling_utils")}
    try:
        amd.install()
        assert "utils.sampling_utils" not in sys.modules or sys.modules.get("utils.sampling_utils") is had["utils.sampling_utils"]   # opt-in
        amd.install(sampling=True)
        import utils.sampling_utils as su
        assert su.generate_sample_idxs is sampling.generate_sample_idxs
        assert su.update_sampling_weights is sampling.update_sampling_weights_np
        if getattr(su, "__hipt_amd_stub__", False):
            with pytest.raises(RuntimeError, match="not importable"):
                su.plot_sampling("s", None, None)
    finally:
        dropin.uninstall()
    assert sys.modules.get("utils.sampling_utils") is had["utils.sampling_utils"]
    assert sys.modules.get("utils") is had["utils"]


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("hipt_knn", "hipt_knn_workspace_bytes", "hipt_sampling_update", "hipt_sampling_update_workspace_bytes")


def test_abi_declares_binds_and_exports_the_sampling_symbols():
    from hipt_abmil_atec23_amd import _native
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    declared = set(re.findall(r"\b(hipt_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared, f"{s} not declared in include/hipt_abmil.h"
        assert s in _native.SIGNATURES, f"{s} not bound in _native.py"
    for name in ("HIPT_KNN_SPATIAL = 0", "HIPT_KNN_TEXTURAL = 1", "HIPT_SAMPLING_MAX = 0", "HIPT_SAMPLING_NEWEST = 1", "HIPT_SAMPLING_AVERAGE = 2"):
        assert name in hdr
    assert (_native.KNN_SPATIAL, _native.KNN_TEXTURAL, _native.SAMPLING_MAX, _native.SAMPLING_NEWEST, _native.SAMPLING_AVERAGE) == (0, 1, 0, 1, 2)
    if not os.path.isfile(_native.LIB_PATH):
        pytest.fail(f"{_native.LIB_PATH} missing: build() has not run")
    lib = _native.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s), f"libhipt_abmil.so does not export {s}"
    # host-side queries need no device: the workspace functions and the k > N / envelope answers
    assert lib.hipt_knn_workspace_bytes(100000, 100, 20) > 0 and lib.hipt_knn_workspace_bytes(100000, 100, 20) % 256 == 0
    assert lib.hipt_knn_workspace_bytes(10, 4, 11) == 0 and lib.hipt_knn_workspace_bytes(100, 4, 65) == 0
    assert lib.hipt_knn_workspace_bytes(1 << 20, 4096, 64) <= 64 << 20
    assert lib.hipt_sampling_update_workspace_bytes(100000) >= 100000 * 20
