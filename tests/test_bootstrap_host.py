"""Bootstrapped evaluation metrics, host side (no GPU): tests/bootstrap_ref.py against the goldens written by the reference's
own bootstrapping.py (tests/golden/make_golden_bootstrap.py), the seeded draws, the package's host preparation, its CSV reader
and writer, the degenerate-replicate error and the ABI.

Bars: accuracy bit-exact; AUC, F1 and balanced accuracy |d| <= 1e-15 per replicate against sklearn's values
(the correctly rounded exact ratios differ from sklearn's float64 pipeline by at most 2.22e-16 on the 360 golden replicates;
one miscounted pair moves an AUC by >= 1 / (2 P N) ~ 2e-5); summaries |d| <= 4e-15."""
import io
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

sys.path.insert(0, os.path.join(ROOT, "tests"))
import bootstrap_ref as R  # noqa: E402

PER_REPLICATE_BAR = 1e-15
SUMMARY_BAR = 4e-15
CASES = ["binary", "3class"]
EVAL_ROOT = os.path.join(GOLDEN, "bootstrap_eval", "eval_results")


def _case(name):
    g = golden("bootstrap_" + name)
    return g, g["Y"].astype(np.int64), g["Y_hat"].astype(np.int64), g["probs"], g["idxs"].astype(np.int64), int(g["K"])


# ---- the restatement against the reference's outputs -----------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_ref_matches_every_golden_replicate(name):
    g, Y, Y_hat, probs, idxs, K = _case(name)
    want = g["per_replicate"]
    assert want.shape == (int(g["B"]), 4) and idxs.shape == (int(g["B"]), len(Y)) and np.isfinite(want).all()
    got = R.bootstrap_metrics_ref(Y, Y_hat, probs, idxs, K)
    d = np.abs(got - want).max(axis=0)
    print(f"{name}: max|d| auc {d[0]:.3g} f1 {d[1]:.3g} accuracy {d[2]:.3g} balanced accuracy {d[3]:.3g}")
    assert np.array_equal(got[:, 2], want[:, 2]), "accuracy is an integer over n in both: bit-exact"
    assert d.max() <= PER_REPLICATE_BAR
    ds = np.abs(R.summary(got) - g["summary"]).max()
    print(f"{name}: summaries max|d| {ds:.3g}")
    assert ds <= SUMMARY_BAR


@pytest.mark.parametrize("name", CASES)
def test_golden_summary_is_mean_and_std_of_its_replicates(name):
    g = golden("bootstrap_" + name)
    assert np.array_equal(R.summary(g["per_replicate"]), g["summary"])


def test_goldens_cover_what_they_should():
    g, Y, _, probs, idxs, _ = _case("binary")
    assert len(Y) == 285 and int(g["B"]) == 300 and int(g["seed"]) == 123
    assert len(np.unique(probs)) < len(probs) // 2, "two-decimal p_1: many ties"
    assert 0.4 < Y.mean() < 0.6
    pos, neg = probs[Y == 1], probs[Y == 0]
    assert (pos[:, None] == neg[None, :]).sum() > 100, "ties between positives and negatives, where the AUC's tie term counts"
    g3, Y3, _, p3, _, K3 = _case("3class")
    assert len(Y3) == 150 and int(g3["B"]) == 60 and int(g3["seed"]) == 5 and K3 == 3 and p3.shape == (150, 3)
    assert np.allclose(p3.sum(axis=1), 1.0)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("chunk", [1, 7, 64, None])
def test_stored_indices_are_the_seeded_randint_stream(name, chunk):
    g, Y, _, _, idxs, _ = _case(name)
    n, B = len(Y), int(g["B"])
    chunk = B if chunk is None else chunk
    np.random.seed(int(g["seed"]))
    drawn = np.concatenate([np.random.randint(0, n, size=(min(chunk, B - b), n)) for b in range(0, B, chunk)])
    assert np.array_equal(drawn, idxs)


def test_randint_stream_is_the_references_choice_stream():
    np.random.seed(11)
    a = np.stack([np.random.choice(range(285), 285) for _ in range(40)])
    np.random.seed(11)
    assert np.array_equal(a, np.random.randint(0, 285, size=(40, 285)))


@pytest.mark.parametrize("K", [2, 4])
def test_ref_auc_equals_pairwise_brute_force(K):
    Y, Y_hat, probs = R.limit_case(90, K, seed=3, levels=9)
    rng = np.random.RandomState(4)
    idxs = rng.randint(0, 90, size=(25, 90))
    got = R.bootstrap_metrics_ref(Y, Y_hat, probs, idxs, K)
    for b, row in enumerate(idxs):
        if K == 2:
            want = R.pairwise_auc(Y, probs, row, 1)
        else:
            want = sum(R.pairwise_auc(Y, probs[:, c], row, c) for c in range(K)) / K
        assert abs(got[b, 0] - want) <= 1e-15, (b, got[b, 0], want)


def test_ref_marks_degenerate_replicates():
    Y, Y_hat, probs = R.limit_case(20, 2, seed=1)
    only_neg = np.flatnonzero(Y == 0)
    row = np.resize(only_neg, 20)
    m = R.replicate_metrics(Y, Y_hat, probs, row, 2)
    assert np.isnan(m[0]) and all(np.isfinite(m[1:]))


# ---- the package's host side -------------------------------------------------------------------------------------------------
def _host_eval(Y, Y_hat, order, tie, K, idx):
    """What the kernel computes from the prepared arrays, restated with Python integers (checks prepare_scores' contract:
    the order, and [lo, hi) of every position's tie group)."""
    n = len(Y)
    cnt = np.bincount(idx, minlength=n)
    auc = []
    for c in range(order.shape[0]):
        label = 1 if K == 2 else c
        neg = np.array([0 if Y[j] == label else cnt[j] for j in order[c]])
        E = np.concatenate([[0], np.cumsum(neg)])
        num = sum(int(cnt[j]) * int(E[tie[c][p] & 0xffff] + E[tie[c][p] >> 16]) for p, j in enumerate(order[c]) if Y[j] == label)
        P = int(cnt[Y == label].sum())
        auc.append(num / (2 * P * (n - P)))
    return sum(auc) / len(auc)


@pytest.mark.parametrize("name", CASES)
def test_prepare_scores_contract(name):
    from hipt_abmil_atec23_amd import bootstrap as Bt
    g, Y, Y_hat, probs, idxs, K = _case(name)
    y32, yh32, order, tie, k = Bt.prepare_scores(Y, Y_hat, probs)
    n = len(Y)
    C = 1 if K == 2 else K
    assert k == K and order.shape == tie.shape == (C, n) and order.dtype == tie.dtype == y32.dtype == yh32.dtype == np.int32
    for c in range(C):
        s = (probs if K == 2 else probs[:, c])[order[c]]
        assert sorted(order[c]) == list(range(n)) and (np.diff(s) >= 0).all()
        lo, hi = tie[c] & 0xffff, tie[c] >> 16
        for p in range(n):
            assert lo[p] <= p < hi[p] and (s[lo[p]:hi[p]] == s[p]).all()
            assert (lo[p] == 0 or s[lo[p] - 1] < s[p]) and (hi[p] == n or s[hi[p]] > s[p])
    for b in range(0, len(idxs), 17):
        assert abs(_host_eval(Y, Y_hat, order, tie, K, idxs[b]) - g["per_replicate"][b, 0]) <= PER_REPLICATE_BAR


def test_prepare_scores_rejects_what_the_kernel_cannot_take():
    from hipt_abmil_atec23_amd import bootstrap as Bt
    Y, Y_hat, probs = R.limit_case(50, 2)
    with pytest.raises(ValueError, match="class ids"):
        Bt.prepare_scores(Y + 1, Y_hat, probs)
    with pytest.raises(ValueError, match="NaN"):
        Bt.prepare_scores(Y, Y_hat, np.where(np.arange(50) == 3, np.nan, probs))
    with pytest.raises(ValueError, match="limits"):
        Bt.prepare_scores(*R.limit_case(Bt.MAX_N + 1, 2))
    with pytest.raises(ValueError, match="limits"):
        Bt.prepare_scores(*R.limit_case(100, Bt.MAX_CLASSES + 1))
    with pytest.raises(ValueError):
        Bt.prepare_scores(Y, Y_hat[:-1], probs)


def test_degenerate_replicate_raises_value_error():
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import bootstrap as Bt
    out = np.full((5, 4), 0.5)
    res = Bt._finish(out.copy(), 0)
    assert res.auc.shape == (5,) and res.auc.flags["C_CONTIGUOUS"]
    out[3, 0] = np.nan
    with pytest.raises(ValueError, match=r"Only one class present.*replicate 3 "):
        Bt._finish(out, N.BOOTSTRAP_DEGENERATE)
    with pytest.raises(ValueError):   # never NaN silently, whatever the flag word says
        Bt._finish(out, 0)
    with pytest.raises(RuntimeError):
        Bt._finish(np.full((5, 4), 0.5), N.BOOTSTRAP_BAD_INPUT)


def test_cpu_only_call_raises():
    import torch
    from hipt_abmil_atec23_amd import bootstrap as Bt
    Y, Y_hat, probs = R.limit_case(50, 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        Bt.bootstrap_metrics(Y, Y_hat, probs, 3, device="cpu")
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError, match="HIP device"):
            Bt.bootstrap_metrics(Y, Y_hat, probs, 3)


@pytest.mark.parametrize("name", CASES)
def test_summary_and_frame_from_given_replicates(name):
    """The result object's summary() and the written frame, from the reference's own per-replicate values: the same
    np.mean / np.std and the same DataFrame construction give the reference's CSV text byte for byte."""
    from hipt_abmil_atec23_amd import bootstrap as Bt
    g = golden("bootstrap_" + name)
    res = Bt._finish(g["per_replicate"].copy(), 0)
    s = res.summary()
    assert len(s) == 8 and np.array_equal(np.array(s), g["summary"])
    df = Bt.metric_frame([s])
    assert df.shape == (8, 1)
    buf = io.StringIO()
    df.to_csv(buf, index=False)
    import pandas as pd
    assert pd.read_csv(io.StringIO(buf.getvalue())).to_csv(index=False) == str(g["written_csv"])
    # row order of the file: AUC, accuracy, balanced accuracy, F1 (means), then the sds in the same order
    assert [row[0][0] for row in df.values] == [s[0], s[2], s[3], s[1], s[4], s[6], s[7], s[5]]
    two = Bt.metric_frame([s, s])
    assert two.shape == (8, 1) and two.iloc[0, 0] == [s[0], s[0]]


@pytest.mark.parametrize("name", CASES)
def test_reader_pools_the_folds_as_the_reference(name):
    from hipt_abmil_atec23_amd import bootstrap as Bt
    g, Y, Y_hat, probs, _, K = _case(name)
    y, yh, p, losses = Bt.read_eval_run(name, 0, run_repeats=1, folds=int(g["folds"]), num_classes=K, eval_root=EVAL_ROOT)
    assert np.array_equal(y, Y) and np.array_equal(yh, Y_hat) and np.array_equal(p, probs)
    assert np.mean(losses) == float(g["mean_loss"])
    assert np.array_equal(Bt.confusion_matrix(y, yh, K), g["confusion"])


def test_reader_run_repeats_and_multiclass_over_several_folds(tmp_path):
    """EVAL_<name>_run<r>/ directories for several repeats, and a K > 2 run pooled over more than one fold (which the
    reference's DataFrame.append can no longer do): row-wise concatenation."""
    import pandas as pd
    from hipt_abmil_atec23_amd import bootstrap as Bt
    Y, Y_hat, probs = R.synthetic_multiclass(seed=9, rows=40)
    root = tmp_path / "eval_results"
    (root / "EVAL_m").mkdir(parents=True)
    pd.DataFrame({"loss": [0.5, 0.7]}).to_csv(root / "EVAL_m" / "summary.csv", index=False)
    for r in range(2):
        (root / f"EVAL_m_run{r}").mkdir()
        for f in range(2):
            sl = slice(20 * f, 20 * f + 20)
            rows = {"slide_id": [f"s{i}" for i in range(20)], "Y": np.roll(Y, r)[sl], "Y_hat": Y_hat[sl]}
            rows.update({f"p_{c}": probs[sl, c] for c in range(3)})
            pd.DataFrame(rows).to_csv(root / f"EVAL_m_run{r}" / f"fold_{f}.csv", index=False)
    for r in range(2):
        y, yh, p, losses = Bt.read_eval_run("m", r, run_repeats=2, folds=2, num_classes=3, eval_root=str(root))
        assert np.array_equal(y, np.roll(Y, r)) and np.array_equal(yh, Y_hat) and losses == [0.5, 0.7]
        # pandas' default float parser (the one the reference reads with) is not round-trip exact: last-digit differences
        assert p.shape == probs.shape and np.abs(p - probs).max() < 1e-15


def test_cli_flags():
    from hipt_abmil_atec23_amd import bootstrap as Bt
    a = Bt.make_parser().parse_args(["--model_names", "a,b", "--data_csv", "x.csv"])
    assert (a.bootstraps, a.run_repeats, a.folds, a.num_classes, a.plot_roc_curves) == (100000, 10, 10, 2, False)
    with pytest.raises(SystemExit):
        Bt.main(["--model_names", "a", "--plot_roc_curves"])


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_binds_the_new_symbol():
    import ctypes as C
    from hipt_abmil_atec23_amd import _native as N
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    assert re.search(r"\bint\s+hipt_bootstrap_metrics\s*\(", hdr)
    assert re.search(r"#define\s+HIPT_ABI_VERSION\s+6\b", hdr) and N.ABI_VERSION == 6
    res, args = N.SIGNATURES["hipt_bootstrap_metrics"]
    decl = re.search(r"int\s+hipt_bootstrap_metrics\s*\(([^)]*)\)", hdr).group(1)
    assert res is C.c_int and len(args) == len(decl.split(",")) == 11
    for macro, val in (("HIPT_BOOTSTRAP_MAX_N", N.BOOTSTRAP_MAX_N), ("HIPT_BOOTSTRAP_MAX_CLASSES", N.BOOTSTRAP_MAX_CLASSES)):
        assert int(re.search(rf"#define\s+{macro}\s+(\d+)", hdr).group(1)) == val
    assert N.BOOTSTRAP_MAX_N >= 4096 and N.BOOTSTRAP_MAX_CLASSES >= 8
    assert f"HIPT_BOOTSTRAP_DEGENERATE = {N.BOOTSTRAP_DEGENERATE}" in hdr and f"HIPT_BOOTSTRAP_BAD_INPUT = {N.BOOTSTRAP_BAD_INPUT}" in hdr
    src = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert "bootstrap.hip" in src and "FLAGS_bootstrap.hip = -ffp-contract=off" in src


def test_package_exports_lazily():
    import hipt_abmil_atec23_amd as amd
    from hipt_abmil_atec23_amd import bootstrap as Bt
    assert amd.bootstrap_metrics is Bt.bootstrap_metrics and amd.bootstrap_eval_dir is Bt.bootstrap_eval_dir
