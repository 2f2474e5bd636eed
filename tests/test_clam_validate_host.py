"""Host tests of the validation pass over many bags (``evaluate.validate_split``, ``forward_bags(..., label=, instance_eval=True)``) and of
the numpy restatement of ``CLAM_MB.forward`` the GPU tests measure against (tests/clam_mb_ref.py).  No GPU: the models live on the CPU,
where ``forward_bags`` loops over ``forward``."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import clam_mb_ref as R
from conftest import golden
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N
from hipt_abmil_atec23_amd import synth
from hipt_abmil_atec23_amd.evaluate import ValidationResult, validate_split

TOL = 1e-4  # the CLAM bar of tests/test_oracle_vs_golden.py
SIZE = (64, 32, 16)
ROWS = (8, 40, 17, 9, 33)
NEW_SYMBOLS = ("hipt_clam_mb_bags_supported", "hipt_clam_mb_bags_workspace_bytes", "hipt_clam_mb_forward_bags", "hipt_topk_segments")


def md(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max())


def test_restatement_against_the_reference_modules_outputs():
    g = golden("clam_mb_hipt_big_n333")
    p = synth.make_params_np(synth.clam_param_specs((192, 128, 64), n_classes=3, multi=True), 193)
    r = R.clam_mb_forward(synth.hash_uniform_np((333, 192), 25), p)
    for k in ("A_raw", "M", "logits", "Y_prob"):
        assert r[k].shape == g[k].shape and md(r[k], g[k]) < TOL, (k, md(r[k], g[k]))
    assert np.array_equal(r["Y_hat"], g["Y_hat"])


def test_restatement_instance_branch_is_the_oracles_for_one_branch():
    """With one branch the instance loop is CLAM_SB's, which the oracle has (and pins against the reference's golden files)."""
    from oracle import hipt_oracle as O
    p = synth.make_params_np(synth.clam_param_specs(SIZE, n_classes=2), 7)
    h = synth.hash_uniform_np((40, SIZE[0]), 3).astype(np.float64)
    p = {k: v.astype(np.float64) for k, v in p.items()}
    for subtyping in (False, True):
        o = O.clam_sb_forward(h, p, label=1, instance_eval=True, subtyping=subtyping)
        h1 = np.maximum(O.linear(h, p["attention_net.0.weight"], p["attention_net.0.bias"]), 0)
        r = R.instance_branch(O.softmax(o["A_raw"], axis=1), h1, p, 1, 8, subtyping, False)
        assert abs(r["instance_loss"] - o["instance_loss"]) < 1e-12
        assert all(np.array_equal(a, b) for a, b in zip(r["inst_ids"], o["inst_ids"]))


def make(cls, n_classes, subtyping):
    m = cls(size_arg=list(SIZE), n_classes=n_classes, subtyping=subtyping)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(SIZE, n_classes=n_classes, multi=cls is CLAM_MB), 5), strict=True)
    return m.eval()


def split(n_classes, seed=11):
    bags = list(torch.from_numpy(synth.hash_uniform_np((sum(ROWS), SIZE[0]), seed)).split(list(ROWS), dim=0))
    return bags, [b % n_classes for b in range(len(ROWS))]


def per_slide_loop(model, bags, labels, n_classes):
    """validate_clam's loop (utils/core_utils.py:521-548), one ``forward(bag, label=, instance_eval=True)`` per slide, with the counting
    rules of Accuracy_Logger.log / log_batch."""
    acc = [{"count": 0, "correct": 0} for _ in range(n_classes)]
    inst = [{"count": 0, "correct": 0} for _ in range(n_classes)]
    prob, labs = np.zeros((len(bags), n_classes)), np.zeros(len(bags))
    val_loss = val_error = val_inst_loss = 0.0
    model.eval()
    with torch.no_grad():
        for i, (bag, l) in enumerate(zip(bags, labels)):
            label = torch.tensor([l], device=bag.device)
            logits, y_prob, y_hat, _, d = model(bag, label=label, instance_eval=True)
            acc[l]["count"] += 1
            acc[l]["correct"] += int(int(y_hat) == l)
            val_loss += F.cross_entropy(logits, label).item()
            val_inst_loss += d["instance_loss"].item()
            p, t = np.array(d["inst_preds"]).astype(int), np.array(d["inst_labels"]).astype(int)
            for c in np.unique(t):
                inst[c]["count"] += int((t == c).sum())
                inst[c]["correct"] += int((p[t == c] == t[t == c]).sum())
            prob[i], labs[i] = y_prob.cpu().numpy(), l
            val_error += 1.0 - float(y_hat.float().eq(label.float()).float().mean().item())
    n = len(bags)
    return ValidationResult(prob=prob, labels=labs, val_loss=val_loss / n, val_error=val_error / n, acc=acc,
                            val_inst_loss=val_inst_loss / n, inst_count=n, inst=inst)


def assert_same(a, b, exact_loss=False):
    assert a.prob.dtype == np.float64 and a.prob.tobytes() == b.prob.tobytes() and a.labels.tobytes() == b.labels.tobytes()
    assert a.acc == b.acc and a.inst == b.inst and a.inst_count == b.inst_count and a.val_error == b.val_error
    if exact_loss:
        assert a.val_loss == b.val_loss and a.val_inst_loss == b.val_inst_loss
    else:
        assert abs(a.val_loss - b.val_loss) <= 1e-6 * abs(b.val_loss)
        assert abs(a.val_inst_loss - b.val_inst_loss) <= 1e-6 * abs(b.val_inst_loss)


@pytest.mark.parametrize("cls", [CLAM_SB, CLAM_MB])
@pytest.mark.parametrize("subtyping", [False, True])
@pytest.mark.parametrize("n_classes", [2, 3])
def test_validate_split_is_the_per_slide_loop(cls, subtyping, n_classes):
    m = make(cls, n_classes, subtyping)
    bags, labels = split(n_classes)
    want = per_slide_loop(m, bags, labels, n_classes)
    got = validate_split(m, bags, labels, n_classes)
    assert m.bags_route == "per_bag"
    assert_same(got, want)
    assert sum(d["count"] for d in got.inst) == len(bags) * 8 * ((n_classes + 1) if subtyping else 2)
    if cls is CLAM_MB:
        assert "bags_one_call" not in m.__dict__ and CLAM_MB.bags_one_call is False   # restored
    # a loader of (bag, label) pairs, and the independence of the chunking
    for cut in (1, 41, 1 << 16):
        assert_same(validate_split(m, list(zip(bags, [torch.tensor([l]) for l in labels])), None, n_classes, max_rows_per_call=cut), got, True)


def test_forward_bags_default_arguments_are_unchanged():
    m = make(CLAM_SB, 2, False)
    bags, _ = split(2)
    logits, y_prob, y_hat, a_raw, res = m.forward_bags(bags)
    assert res == {} and logits.shape == (5, 2) and y_hat.shape == (5, 1) and [tuple(a.shape) for a in a_raw] == [(1, n) for n in ROWS]
    res = m.forward_bags(bags, label=[0, 1, 0, 1, 0], instance_eval=True, return_features=True)[4]
    assert set(res) == {"features", "instance_loss", "inst_preds", "inst_labels"}
    assert res["instance_loss"].shape == (5,) and len(res["inst_preds"]) == 5 and all(p.shape == (16,) for p in res["inst_preds"])
    for form in (np.array([0, 1, 0, 1, 0]), torch.tensor([0, 1, 0, 1, 0])):
        again = m.forward_bags(bags, label=form, instance_eval=True)[4]
        assert torch.equal(again["instance_loss"], res["instance_loss"])


def test_a_bag_shorter_than_k_sample_is_an_error():
    m = make(CLAM_SB, 2, False)
    bags, labels = split(2)
    bags[2] = bags[2][:7]
    with pytest.raises(RuntimeError, match="selected index k out of range: k_sample=8 > 7 rows"):
        m.forward_bags(bags, label=labels, instance_eval=True)
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        validate_split(m, bags, labels, 2)
    with pytest.raises(ValueError, match="5 bags but 4 labels"):
        m.forward_bags(bags[:2] + bags[3:] + bags[:1], label=labels[:4], instance_eval=True)
    with pytest.raises(ValueError, match="needs the B class ids"):
        m.forward_bags(bags[:2], instance_eval=True)


def test_abi_header_and_binding_list_the_new_symbols():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "hipt_abmil.h")).read()
    declared = set(re.findall(r"\b(hipt_[a-z0-9_]+)\s*\(", hdr))
    for s in NEW_SYMBOLS:
        assert s in declared and s in N.SIGNATURES, s
    assert re.search(r"#define\s+HIPT_ABI_VERSION\s+6\b", hdr) and N.ABI_VERSION == 6


def test_install_validation_is_optional(monkeypatch):
    """``install(validation=True)`` binds ``utils.core_utils.validate_clam`` where that module imports and restores it on uninstall."""
    import sys
    import types

    from hipt_abmil_atec23_amd import dropin
    pkg, mod = types.ModuleType("utils"), types.ModuleType("utils.core_utils")
    pkg.__path__ = []
    mod.validate_clam = original = lambda *a, **k: None
    monkeypatch.setitem(sys.modules, "utils", pkg)
    monkeypatch.setitem(sys.modules, "utils.core_utils", mod)
    try:
        assert "utils.core_utils.validate_clam" not in dropin.install()
        assert mod.validate_clam is original
        assert "utils.core_utils.validate_clam" in dropin.install(validation=True)
        assert getattr(mod.validate_clam, "__hipt_amd__", False)
    finally:
        dropin.uninstall()
    assert mod.validate_clam is original
