"""MIL_fc / MIL_fc_mc without a GPU: the reference's state-dict keys, routes, the CPU route against tests/mil_ref.py, what raises, the C
ABI's three symbols and envelope, the shim, and the margin condition of every index case tests/test_gpu_mil.py uses."""
import ctypes as C_
import os
import re

import numpy as np
import pytest
import torch

import mil_ref as R
from hipt_abmil_atec23_amd import MIL_fc, MIL_fc_mc, _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("hipt_mil_forward_bags", "hipt_mil_bags_workspace_bytes", "hipt_mil_bags_supported")


def test_state_dict_keys_are_the_references():
    k = lambda m: list(m.state_dict())
    assert k(MIL_fc()) == ["classifier.0.weight", "classifier.0.bias", "classifier.2.weight", "classifier.2.bias"]
    assert k(MIL_fc(dropout=True)) == ["classifier.0.weight", "classifier.0.bias", "classifier.3.weight", "classifier.3.bias"]
    for d in (False, True):
        assert k(MIL_fc_mc(n_classes=3, dropout=d)) == ["fc.0.weight", "fc.0.bias"] + [f"classifiers.{c}.{n}" for c in range(3) for n in ("weight", "bias")]
    m = MIL_fc(dropout=True)
    assert m.top_k == 1 and m.size_dict == {"small": [1024, 512]} and isinstance(m.classifier[2], torch.nn.Dropout) and m.classifier[2].p == 0.25
    assert MIL_fc_mc(n_classes=4).n_classes == 4 and hasattr(MIL_fc_mc(n_classes=3), "relocate")


@pytest.mark.parametrize("C,dropout", [(2, False), (2, True), (3, False), (3, True)])
def test_strict_load_and_cpu_route_against_the_reference(C, dropout):
    p = R.weights(C)
    m = MIL_fc_mc(n_classes=C, dropout=dropout) if C > 2 else MIL_fc(dropout=dropout)
    m.load_state_dict(R.state_dict(p, C > 2, dropout), strict=True)
    m.eval()
    x = R.bag(65, 65, 32, p, C > 2)
    h = torch.from_numpy(x)
    assert m.route(h) == "torch" and m.train().route(h) == "torch"
    m.eval()
    with torch.no_grad():
        top, Y_prob, Y_hat, y_probs, res = m(h, return_features=True)
    ref = R.forward(x, p, C > 2, False)
    for got, want, bound in ((y_probs, ref["y_probs"], ref["e_p"]), (top, ref["top_instance"], ref["e_l"][ref["idx"]][None]),
                             (Y_prob, ref["Y_prob"], ref["e_p"][ref["idx"]][None]), (res["features"], ref["features"], ref["e_h"][ref["idx"]][None])):
        assert tuple(got.shape) == want.shape and (np.abs(got.double().numpy() - want) <= bound).all()
    assert int(Y_hat) == ref["Y_hat"] and Y_hat.dtype == torch.int64 and tuple(Y_hat.shape) == ((1,) if C > 2 else (1, 1))
    out = m.forward_bags([h, h[:5]], return_features=True)
    assert m.bags_route == "per_bag" and tuple(out[2].shape) == (2, 1) and torch.equal(out[0][:1], top) and tuple(out[4]["features"].shape) == (2, 512)


def test_what_raises():
    with pytest.raises(ValueError):
        MIL_fc(top_k=2)
    with pytest.raises(ValueError):
        MIL_fc_mc(n_classes=3, top_k=3)
    with pytest.raises(AssertionError):
        MIL_fc(n_classes=3)
    with pytest.raises(AssertionError):
        MIL_fc_mc(n_classes=2)
    for bad in ("big", [1024, 128], [1000, 512], [1024, 512, 256]):
        with pytest.raises(ValueError):
            MIL_fc(size_arg=bad)
    assert MIL_fc(size_arg=[512, 256])._sizes == (512, 256)
    m = MIL_fc().eval()
    with pytest.raises(ValueError):
        m.forward_bags([torch.zeros(3, 1024), torch.zeros(0, 1024)])
    with pytest.raises(ValueError):
        m.forward_bags((torch.zeros(3, 1024), [0, 3, 3]))


def test_abi_symbols_and_envelope():
    lib = N.lib()
    assert lib.hipt_abi_version() == 6 == N.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    for s in SYMBOLS:
        assert s in N.SIGNATURES and hasattr(lib, s) and re.search(rf"\b{s}\s*\(", hdr)
    def w(dtype, s0, s1, C, multi):
        v = N.MilWeights()
        v.dtype, v.s0, v.s1, v.n_classes, v.multi_class = dtype, s0, s1, C, multi
        return v
    ok = lambda *a: lib.hipt_mil_bags_supported(C_.byref(w(*a)))
    assert ok(N.HIPT_F32, 1024, 512, 2, 0) and ok(N.HIPT_BF16, 1024, 512, 2, 0) and ok(N.HIPT_BF16, 1024, 512, 8, 1) and ok(N.HIPT_F32, 32, 256, 3, 1)
    assert ok(N.HIPT_BF16, 64, 256, 2, 1)
    assert not ok(N.HIPT_BF16, 32, 256, 2, 0) and not ok(N.HIPT_F32, 1024, 128, 2, 0) and not ok(N.HIPT_F32, 1024, 512, 9, 1)
    assert not ok(N.HIPT_F32, 1024, 512, 1, 1) and not ok(N.HIPT_F32, 1024, 512, 3, 0) and not ok(2, 1024, 512, 2, 0) and not ok(N.HIPT_F32, 0, 512, 2, 0)
    good = w(N.HIPT_BF16, 1024, 512, 3, 1)
    assert lib.hipt_mil_bags_workspace_bytes(C_.byref(good), 3, 1000) > 0
    assert lib.hipt_mil_bags_workspace_bytes(C_.byref(good), 3, 2) == 0 and lib.hipt_mil_bags_workspace_bytes(C_.byref(good), 0, 10) == 0   # an empty bag; no bag
    # argument errors come before any launch: null pointers on a machine without a GPU
    assert lib.hipt_mil_forward_bags(C_.byref(good), None, None, 1, 1, None, None, None, None, None, None, None, 0, None) == -1


def test_shim_and_package_export_the_classes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("shim_model_mil", os.path.join(ROOT, "shims", "models", "model_mil.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.MIL_fc is MIL_fc and mod.MIL_fc_mc is MIL_fc_mc
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bmil\.hip\b", mk, re.M) and "FLAGS_mil.hip = -ffp-contract=off" in mk


@pytest.mark.parametrize("C", [2, 3, 8])
def test_margin_condition_of_every_gpu_index_case(C):
    p = R.weights(C)
    for name, n, planted in R.cases():
        x = R.bag(n, n, planted, p, C > 2)
        for bf16 in (False, True):
            ref = R.forward(x, p, C > 2, bf16)
            gap, bar = R.margin(ref, C > 2)
            assert ref["idx"] == planted and gap > bar, (name, bf16, ref["idx"], gap, bar)
    for n, seed, row in ((4, 5, 2),):   # the planted row of the tie tests
        assert R.forward(R.bag(n, seed, row, p, C > 2), p, C > 2)["idx"] == row


@pytest.mark.parametrize("C", [2, 3])
def test_reference_against_the_golden_of_the_reference_module(C, golden_loader):
    """tests/golden/mil_reference.npz: the reference's own models/model_mil.py on the CPU (tools/record_mil_golden.py).  Its fp32 results lie
    within the derived bounds of the fp64 restatement, its index and class are ours; the weights are drawn again and their checksum compared."""
    g = golden_loader("mil_reference")
    p = R.weights(C)
    assert R.checksum(p) == float(g[f"c{C}_checksum"])
    n, planted = int(g["n_rows"]), int(g["planted"])
    x = R.bag(n, n, planted, p, C > 2)
    assert float(np.asarray(x, np.float64).sum()) == float(g[f"c{C}_bag_checksum"])
    ref = R.forward(x, p, C > 2, False)
    i = ref["idx"]
    assert i == planted and int(np.asarray(g[f"c{C}_Y_hat"]).reshape(-1)[0]) == ref["Y_hat"]
    assert (np.abs(g[f"c{C}_y_probs"] - ref["y_probs"]) <= ref["e_p"]).all()
    assert (np.abs(g[f"c{C}_top_instance"] - ref["top_instance"]) <= ref["e_l"][i]).all()
    assert (np.abs(g[f"c{C}_Y_prob"] - ref["Y_prob"]) <= ref["e_p"][i]).all()
