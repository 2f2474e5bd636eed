"""Bootstrapped evaluation metrics on the GPU: ``bootstrap_metrics`` (csrc/bootstrap.hip) against the goldens written by the
reference's own bootstrapping.py and against tests/bootstrap_ref.py at the kernel's limits; bitwise independence of chunking;
the error paths; ``bootstrap_eval_dir`` over the committed fold CSVs.

Bars, against the reference's values: accuracy bit-exact; AUC, F1, balanced accuracy |d| <= 1e-15 per replicate
(values in [0, 1], one ulp <= 1.1e-16; the exact ratios differ from sklearn's float64 pipeline by <= 2.22e-16 on all golden
replicates; one miscounted pair moves an AUC by >= 1 / (2 P N) ~ 2e-5); summaries |d| <= 4e-15."""
import os
import re
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import bootstrap_ref as R  # noqa: E402
from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import bootstrap as Bt  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PER_REPLICATE_BAR = 1e-15
SUMMARY_BAR = 4e-15
CASES = ["binary", "3class"]
EVAL_ROOT = os.path.join(GOLDEN, "bootstrap_eval", "eval_results")


def _case(name):
    g = golden("bootstrap_" + name)
    return g, g["Y"].astype(np.int64), g["Y_hat"].astype(np.int64), g["probs"], g["idxs"].astype(np.int64), int(g["K"])


def _stack(res):
    return np.stack([res.auc, res.f1, res.accuracy, res.balanced_accuracy], axis=1)


def _bits(res):
    return _stack(res).view(np.uint64)


@pytest.mark.parametrize("name", CASES)
def test_every_golden_replicate(name):
    g, Y, Y_hat, probs, idxs, K = _case(name)
    before = N.calls
    res = Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, device=DEV)
    assert N.calls > before, "the native library was not used"
    got, want = _stack(res), g["per_replicate"]
    assert got.shape == want.shape == (int(g["B"]), 4) and got.dtype == np.float64
    d = np.abs(got - want).max(axis=0)
    print(f"{name}: max|d| auc {d[0]:.3g} f1 {d[1]:.3g} accuracy {d[2]:.3g} balanced accuracy {d[3]:.3g}")
    assert np.array_equal(got[:, 2], want[:, 2]), "accuracy: bit-exact"
    assert np.isfinite(got).all() and d.max() <= PER_REPLICATE_BAR
    ds = np.abs(np.array(res.summary()) - g["summary"]).max()
    print(f"{name}: summaries max|d| {ds:.3g}")
    assert ds <= SUMMARY_BAR


@pytest.mark.parametrize("name", CASES)
def test_seeded_draws_reproduce_the_reference_and_chunking_changes_no_bit(name):
    g, Y, Y_hat, probs, idxs, K = _case(name)
    B = int(g["B"])
    given = _bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, device=DEV))
    for chunk in (1, 7, 64, B):
        np.random.seed(int(g["seed"]))
        drawn = Bt.bootstrap_metrics(Y, Y_hat, probs, B, chunk=chunk, device=DEV)
        assert np.array_equal(_bits(drawn), given), f"chunk={chunk}: seeded draws differ from the given indices' results"
        assert np.array_equal(_bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, chunk=chunk, device=DEV)), given)
    assert np.abs(_stack(drawn) - g["per_replicate"]).max() <= PER_REPLICATE_BAR


def test_position_in_the_call_changes_no_bit():
    g, Y, Y_hat, probs, idxs, K = _case("binary")
    a = _bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, device=DEV))
    perm = np.random.RandomState(0).permutation(len(idxs))
    b = _bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs[perm], chunk=37, device=DEV))
    assert np.array_equal(b, a[perm])


@pytest.mark.parametrize("n,K", [(Bt.MAX_N, Bt.MAX_CLASSES), (Bt.MAX_N, 2), (Bt.MAX_N - 1, 3), (257, Bt.MAX_CLASSES), (1000, 2)])
def test_at_the_limits_against_the_restatement(n, K):
    """n and K at the limits the header names, heavy ties (37 score levels), random labels: the scan runs over all four waves
    with 16 positions per thread."""
    Y, Y_hat, probs = R.limit_case(n, K)
    idxs = np.random.RandomState(n + K).randint(0, n, size=(6, n))
    idxs[5] = np.arange(n)   # the sample itself
    got = _stack(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, chunk=4, device=DEV))
    want = R.bootstrap_metrics_ref(Y, Y_hat, probs, idxs, K)
    d = np.abs(got - want).max(axis=0)
    print(f"n={n} K={K}: max|d| auc {d[0]:.3g} f1 {d[1]:.3g} accuracy {d[2]:.3g} balanced accuracy {d[3]:.3g}")
    assert np.array_equal(got[:, 2], want[:, 2])
    assert np.isfinite(got).all() and d.max() <= PER_REPLICATE_BAR


def test_small_and_odd_sizes():
    for n, K in ((2, 2), (3, 3), (63, 2), (64, 5), (65, 2), (255, 4), (256, 2), (257, 2), (513, 3)):
        Y, Y_hat, probs = R.limit_case(n, K, levels=5)
        idxs = np.concatenate([np.arange(n)[None], np.random.RandomState(n).randint(0, n, size=(8, n))])
        want = R.bootstrap_metrics_ref(Y, Y_hat, probs, idxs, K)
        ok = np.isfinite(want[:, 0])   # row 0, the sample itself, always is
        got = _stack(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs[ok], device=DEV))
        assert np.abs(got - want[ok]).max() <= PER_REPLICATE_BAR, (n, K)


def test_above_the_limits_is_refused_not_truncated():
    with pytest.raises(ValueError, match="limits"):
        Bt.bootstrap_metrics(*R.limit_case(Bt.MAX_N + 1, 2), 4, device=DEV)
    with pytest.raises(ValueError, match="limits"):
        Bt.bootstrap_metrics(*R.limit_case(64, Bt.MAX_CLASSES + 1), 4, device=DEV)
    # the library itself: an error code, and nothing is launched (the output keeps its sentinel)
    n = 64
    z = torch.zeros(n, dtype=torch.int32, device=DEV)
    out = torch.full((4, 4), -7.0, dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    for bad_n, bad_k, bad_b in ((Bt.MAX_N + 1, 2, 4), (n, Bt.MAX_CLASSES + 1, 4), (n, 2, Bt.MAX_REPLICATES + 1)):
        with pytest.raises(RuntimeError, match="limits"):
            N.call("hipt_bootstrap_metrics", N.ptr(z), N.ptr(z), N.ptr(z), N.ptr(z), bad_n, bad_k, N.ptr(z), bad_b, N.ptr(out), N.ptr(flags),
                   N.stream_ptr(DEV))
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and int(flags[0]) == 0


def test_degenerate_replicate_raises():
    g, Y, Y_hat, probs, idxs, K = _case("binary")
    bad = idxs[:9].copy()
    bad[4] = np.resize(np.flatnonzero(Y == 0), len(Y))   # a replicate without a positive
    bad[7] = np.resize(np.flatnonzero(Y == 1), len(Y))
    with pytest.raises(ValueError, match=r"Only one class present.*replicate 4 "):
        Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=bad, chunk=2, device=DEV)
    g3, Y3, Yh3, p3, idxs3, _ = _case("3class")
    bad3 = idxs3[:3].copy()
    bad3[2] = np.resize(np.flatnonzero(Y3 != 2), len(Y3))   # class 2 absent
    with pytest.raises(ValueError, match=r"replicate 2 "):
        Bt.bootstrap_metrics(Y3, Yh3, p3, idxs=bad3, device=DEV)
    # and the stream is usable afterwards
    assert np.abs(_stack(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs[:9], device=DEV)) - g["per_replicate"][:9]).max() <= PER_REPLICATE_BAR


def test_bad_indices_are_refused_on_the_host():
    g, Y, Y_hat, probs, idxs, K = _case("binary")
    bad = idxs[:2].copy()
    bad[1, 5] = len(Y)
    with pytest.raises(IndexError):
        Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=bad, device=DEV)


def test_second_call_gives_the_same_bits_and_other_streams_work():
    g, Y, Y_hat, probs, idxs, K = _case("3class")
    a = _bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, chunk=16, device=DEV))
    b = _bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, chunk=16, device=DEV))
    assert np.array_equal(a, b)
    s = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(s):
        c = _bits(Bt.bootstrap_metrics(Y, Y_hat, probs, idxs=idxs, chunk=16, device=DEV))
        t = torch.arange(10, device=DEV).sum()
    assert np.array_equal(a, c) and int(t) == 45


@pytest.mark.parametrize("name", CASES)
def test_eval_dir_reproduces_the_reference_run(name, tmp_path, capsys):
    g = golden("bootstrap_" + name)
    K = int(g["K"])
    np.random.seed(int(g["seed"]))
    df = Bt.bootstrap_eval_dir(name, bootstraps=int(g["B"]), run_repeats=1, folds=int(g["folds"]), num_classes=K,
                               eval_root=EVAL_ROOT, out_dir=str(tmp_path / "metric_results"), chunk=50, device=DEV)
    text = open(tmp_path / "metric_results" / f"{name}.csv").read()
    ref_text = str(g["written_csv"])
    num = r"[-+]?\d+\.\d+(?:e[-+]?\d+)?"
    got = np.array([float(x) for x in re.findall(num, text)])
    want = np.array([float(x) for x in re.findall(num, ref_text)])
    s = g["summary"]
    assert np.array_equal(want, [s[0], s[2], s[3], s[1], s[4], s[6], s[7], s[5]]), "the reference's row order"
    assert got.shape == (8,) and np.abs(got - want).max() <= SUMMARY_BAR
    assert re.sub(num, "#", text) == re.sub(num, "#", ref_text), "same frame around the numbers"
    assert df.shape == (8, 1)
    out = capsys.readouterr().out
    assert "confusion matrix (predicted x axis, true y axis)" in out and "average ce loss:" in out
    assert ("F1 mean:" in out) if K == 2 else ("Macro F1 mean:" in out)
    assert str(g["confusion"]) in out
