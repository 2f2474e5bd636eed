"""Host tests of tests/clam_wide_mb_ref.py, the fp64 reference of the wide-head multi-bag CLAM_MB forward: with the rounding switched
off it is ``clam_mb_ref.clam_mb_forward``; its branch k is tests/clam_wide_ref.py (the one-branch wide reference) run with branch k's
``wc``, ``bc`` and classifier; and for the seed, shapes, branch counts and row counts of tests/test_gpu_clam_wide_mb.py every bag's two
largest reference logits lie further apart than four times the logits bar of its dtype, so no bag is left out of the ``Y_hat``
comparison there.  The GPU test's constants are read from its source (importing it would need its device)."""
import ast
import os

import numpy as np
import pytest

import clam_bags_util as U
import clam_mb_ref as R
import clam_wide_mb_ref as WM
import clam_wide_ref as WR
from conftest import ROOT

TOL = 1e-12
ROWS = (1, 2, 33, 65, 129)


def gpu_test_constants():
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_clam_wide_mb.py")).read())
    want, out = ("ROWS", "CASES", "SEED", "MEASURED"), {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in want:
            out[node.targets[0].id] = ast.literal_eval(node.value)
    assert set(out) == set(want)
    return out


def close(a, b):
    return a.shape == b.shape and float(np.abs(a - b).max()) <= TOL


@pytest.mark.parametrize("size,K", [((128, 256, 64), 2), ((128, 512, 256), 3), ((64, 512, 384), 4)])
def test_without_rounding_it_is_the_clam_mb_restatement(size, K):
    p = U.params64(size, K, True, False)
    for b in WR.bags_host(size[0], 5, ROWS):
        h = b.double().numpy()
        got, want = WM.forward(h, p, round_h1=False), R.clam_mb_forward(h, p)
        for k in ("A_raw", "M", "logits", "Y_prob"):
            assert close(got[k], want[k]), k
        assert np.array_equal(got["Y_hat"], want["Y_hat"])


@pytest.mark.parametrize("size,K", [((128, 256, 64), 2), ((128, 512, 256), 3), ((64, 512, 384), 4)])
def test_a_branch_is_the_one_branch_wide_reference(size, K):
    p = U.params64(size, K, True, True)
    g = 2
    for b in WR.bags_host(size[0], 6, ROWS):
        h = b.bfloat16().double().numpy()
        got = WM.forward(h, p)
        for k in range(K):
            pk = {n: v for n, v in p.items() if not n.startswith("classifiers.") and "attention_c" not in n}
            pk[f"attention_net.{g}.attention_c.weight"] = p[f"attention_net.{g}.attention_c.weight"][k:k + 1]
            pk[f"attention_net.{g}.attention_c.bias"] = p[f"attention_net.{g}.attention_c.bias"][k:k + 1]
            pk["classifiers.weight"], pk["classifiers.bias"] = p[f"classifiers.{k}.weight"], p[f"classifiers.{k}.bias"]
            one = WR.forward(h, pk)
            assert close(got["A_raw"][k:k + 1], one["A_raw"]) and close(got["M"][k:k + 1], one["M"])
            assert close(got["logits"][:, k:k + 1], one["logits"])


def test_rounding_h1_for_the_gate_changes_the_scores_and_not_the_pooled_operand():
    size, K = (128, 256, 64), 2
    p = U.params64(size, K, True, True)
    h = WR.bags_host(128, 6, (1,))[0].bfloat16().double().numpy()       # one row: M[k] = h1 whatever the scores are
    a, b = WM.forward(h, p, round_h1=True), WM.forward(h, p, round_h1=False)
    assert float(np.abs(a["A_raw"] - b["A_raw"]).max()) > 1e-6
    assert close(a["M"], b["M"])


def test_every_bag_of_the_gpu_test_is_decided_beyond_four_times_the_logits_bar():
    c = gpu_test_constants()
    for dtype, rounded in (("fp32", False), ("bf16", True)):
        bar = 2.0 * c["MEASURED"][dtype]["logits"][1]
        if dtype == "fp32":
            bar = min(bar, 1e-4)
        assert bar > 0.0, "the measured loop error of the GPU test is pinned"
        gaps = [WM.logit_gap(r) for size, K in c["CASES"] for r in WM.reference(tuple(size), c["SEED"], tuple(c["ROWS"]), K, rounded, True)]
        assert len(gaps) == len(c["CASES"]) * len(c["ROWS"])
        print(f"{dtype}: smallest gap {min(gaps):.3e}, logits bar {bar:.3e}")
        assert min(gaps) > 4.0 * bar, (dtype, min(gaps), bar)
