"""Host tests (no GPU) of the multi-bag CLAM_SB call: the envelope of ``hipt_clam_bags_supported``; the Python layer checks the offsets
before any native call; and ``evaluate_split`` repeats the arithmetic of the reference's ``summary()`` (utils/eval_utils.py:115-179)
whatever the chunking.  What the form shares with the other five (symbols, argument errors, workspace sizes) is stated in
tests/clam_bags_util.py and run here on this form's cases."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from clam_bags_util import ARGUMENT_CASES, W, check_argument_error, check_attention_only_needs_no_pooled_outputs, check_outside, check_workspace_grows
from hipt_abmil_atec23_amd import CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd.evaluate import chunk_bags, evaluate_split

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks


def weights(dtype=N.HIPT_F32, s0=384, s1=128, s2=64, n_classes=2):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_classes, n_att=1)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def test_supported_is_the_fused_envelope():
    lib = N.lib()
    yes = [(N.HIPT_F32, 384, 128, 64), (N.HIPT_F32, 192, 64, 32), (N.HIPT_F32, 192, 32, 16), (N.HIPT_BF16, 384, 128, 64), (N.HIPT_BF16, 192, 64, 32)]
    no = [(N.HIPT_F32, 1024, 512, 256), (N.HIPT_BF16, 192, 32, 16), (N.HIPT_F32, 200, 128, 64), (N.HIPT_BF16, 96, 64, 32), (N.HIPT_F32, 192, 8, 4)]
    assert [lib.hipt_clam_bags_supported(C.byref(weights(*a))) for a in yes] == [1] * len(yes)
    assert [lib.hipt_clam_bags_supported(C.byref(weights(*a))) for a in no] == [0] * len(no)
    assert lib.hipt_clam_bags_supported(None) == 0


# ---- the checks every form shares (tests/clam_bags_util.py), on this form's cases ----
def test_workspace_grows_with_bags_and_rows():
    check_workspace_grows("sb", W(384, 128, 64))


@pytest.mark.parametrize("case,kw", ARGUMENT_CASES)
def test_argument_errors_come_back_before_any_device_work(case, kw):
    check_argument_error("sb", case, kw)


def test_attention_only_needs_no_pooled_outputs_and_other_widths_are_unsupported():
    check_attention_only_needs_no_pooled_outputs("sb")
    check_outside("sb", [W(1024, 512, 256), W(192, 32, 16, dtype=N.HIPT_BF16)])


# ---- the Python layer ----
@pytest.mark.parametrize("offsets,rows,what", [([0, 5, 3, 9], 9, "decrease"), ([0, 3, 3, 9], 9, "empty"), ([0, 3, 8, 10], 9, "end at 10"),
                                               ([1, 3, 9], 9, "starting at 0"), ([0], 0, "B\\+1")])
def test_python_checks_the_offsets_before_any_native_call(offsets, rows, what):
    m = CLAM_SB(size_arg="hipt_medium").eval()
    before = N.calls
    with pytest.raises(ValueError, match=what):
        Fn.check_offsets(offsets, rows)
    with pytest.raises(ValueError, match=what):
        m.forward_bags((torch.zeros(rows, 192), offsets))
    with pytest.raises(ValueError, match=what):
        m.forward_bags((torch.zeros(rows, 192), torch.tensor(offsets)))
    assert N.calls == before
    assert Fn.check_offsets([0, 3, 9], 9) == (0, 3, 9) and Fn.check_offsets(torch.tensor([0, 9]), 9) == (0, 9)


def test_forward_bags_rejects_bad_bags_and_training_with_autograd():
    m = CLAM_SB(size_arg="hipt_medium")
    with pytest.raises(ValueError, match="bag 1"):
        m.eval().forward_bags([torch.zeros(3, 192), torch.zeros(0, 192)])
    with pytest.raises(ValueError, match="bag 0"):
        m.forward_bags([torch.zeros(3, 191)])
    with pytest.raises(ValueError, match="no bags"):
        m.forward_bags([])
    m.train()
    with pytest.raises(RuntimeError, match="inference only.*forward\\(h\\)"):
        m.forward_bags([torch.zeros(3, 192)])
    with torch.no_grad():   # nothing to differentiate: served, with dropout off, and the mode left as it was
        out = m.forward_bags([torch.zeros(3, 192), torch.ones(2, 192)])
    assert m.training and m.bags_route == "per_bag" and out[0].shape == (2, 2) and [a.shape for a in out[3]] == [(1, 3), (1, 2)]


def test_cpu_route_loops_over_forward_with_the_same_structure():
    torch.manual_seed(0)
    m = CLAM_SB(size_arg="hipt_medium", dropout=0.25).eval()
    assert m.bags_route is None
    bags = [torch.randn(n, 192) for n in (1, 5, 3)]
    logits, y_prob, y_hat, a_raw, res = m.forward_bags(bags, return_features=True)
    pair = m.forward_bags((torch.cat(bags), [0, 1, 6, 9]), return_features=True)
    assert m.bags_route == "per_bag" and res["features"].shape == (3, 64)
    for b, bag in enumerate(bags):
        l1, p1, h1, a1, r1 = m(bag, return_features=True)
        assert torch.equal(logits[b:b + 1], l1) and torch.equal(y_prob[b:b + 1], p1) and torch.equal(y_hat[b:b + 1], h1)
        assert torch.equal(a_raw[b], a1) and torch.equal(res["features"][b:b + 1], r1["features"])
        assert torch.equal(pair[0][b:b + 1], l1) and torch.equal(pair[3][b], a1)


# ---- evaluate_split against a plain restatement of summary()'s arithmetic --------------------------------------------------------
class Stub:
    """A model whose logits are written in its bags: row 0, columns 0..C-1."""

    def __init__(self, C):
        self.C, self.calls = C, []

    def forward_bags(self, bags):
        self.calls.append([b.shape[0] for b in bags])
        logits = torch.stack([b[0, :self.C] for b in bags]).float()
        return logits, torch.softmax(logits, dim=1), torch.topk(logits, 1, dim=1)[1], [None] * len(bags), {}


def plain_summary(logits, labels, C, loss_fn):
    """utils/eval_utils.py:115-150 on given per-slide logits, one slide at a time."""
    data = [{"count": 0, "correct": 0} for _ in range(C)]
    n = len(labels)
    probs, preds, err, loss = np.zeros((n, C)), np.zeros(n), 0.0, 0.0
    for i in range(n):
        lg, lab = logits[i:i + 1], torch.tensor([labels[i]])
        y_hat = torch.topk(lg, 1, dim=1)[1]
        data[labels[i]]["count"] += 1
        data[labels[i]]["correct"] += int(int(y_hat) == labels[i])
        probs[i] = torch.softmax(lg, dim=1).numpy()
        preds[i] = y_hat.item()
        loss += loss_fn(lg, lab).item()
        err += 1.0 - y_hat.float().eq(lab.float()).float().mean().item()
    return probs, preds, err / n, loss / n, data


@pytest.mark.parametrize("C", [2, 3])
@pytest.mark.parametrize("custom_loss", [False, True])
def test_evaluate_split_is_summary_whatever_the_chunking(C, custom_loss):
    g = torch.Generator().manual_seed(5)
    rows = [3, 1, 40, 7, 129, 2, 64, 5, 300, 11]
    labels = [int(v) for v in torch.randint(0, C, (len(rows),), generator=g)]
    labels[0], labels[1] = 0, C - 1
    bags = [torch.randn(n, 8, generator=g) * 3 for n in rows]
    loss_fn = (lambda lg, lab: F.multi_margin_loss(lg, lab)) if custom_loss else None
    want = plain_summary(torch.stack([b[0, :C] for b in bags]), labels, C, loss_fn or F.cross_entropy)
    results = []
    for cap in (1 << 16, 130, 48, 1):
        stub = Stub(C)
        r = evaluate_split(stub, bags, labels, C, loss_fn, max_rows_per_call=cap)
        assert [n for call in stub.calls for n in call] == rows
        assert all(sum(call) <= cap or len(call) == 1 for call in stub.calls)
        results.append(r)
        assert r.all_probs.dtype == np.float64 and np.array_equal(r.all_probs, want[0]) and np.array_equal(r.all_preds, want[1])
        assert np.array_equal(r.all_labels, np.asarray(labels, dtype=np.float64))
        assert r.error == want[2] and math.isclose(r.loss, want[3], rel_tol=1e-12) and r.acc == want[4]
        assert r.class_accuracy(0)[1:] == (want[4][0]["correct"], want[4][0]["count"])
    assert len(results[0].all_probs) == len(rows)
    for r in results[1:]:
        assert r.all_probs.tobytes() == results[0].all_probs.tobytes() and r.loss == results[0].loss and r.error == results[0].error
    # a loader of (bag, label) pairs, labels as tensors
    r = evaluate_split(Stub(C), [(b.unsqueeze(0), torch.tensor([l])) for b, l in zip(bags, labels)], None, C, loss_fn, max_rows_per_call=100)
    assert r.all_probs.tobytes() == results[0].all_probs.tobytes() and r.acc == want[4]


def test_chunks_are_consecutive_and_bounded():
    assert chunk_bags([3, 5, 1, 9, 2], 6) == [range(0, 1), range(1, 3), range(3, 4), range(4, 5)]
    assert chunk_bags([3, 5, 1], 100) == [range(0, 3)]
    with pytest.raises(ValueError):
        chunk_bags([1], 0)
