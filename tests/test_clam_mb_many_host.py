"""Host tests (no GPU) of the multi-bag CLAM_MB call for 5 to 8 branches (csrc/abmil_bags_mb8.hip): its source is built;
``hipt_clam_mb_many_bags_supported`` answers yes for exactly the widths of ``abmil_tile::visit_width`` x K in {5, 6, 7, 8} with K classes;
the workspace is the sum of the three carves; a refusal names the branch range; the forms that existed before answer as they did (what
the form shares with the other five -- symbols, argument errors, the switches, the routing -- is in tests/test_clam_bags_forms_host.py);
and for the seed, shapes, branch counts and row counts of tests/test_gpu_clam_mb_many.py every bag's two largest reference logits lie
further apart than four times the logits bar of its dtype.  All pointers here are fake addresses."""
import ast
import ctypes as C
import os

import pytest
import torch

import clam_bags_util as U
import clam_mb_ref as R
from clam_wide_mb_ref import logit_gap
from clam_wide_ref import bags_host
from conftest import ROOT
from hipt_abmil_atec23_amd import CLAM_MB, _native as N

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks
E_BADARG, E_UNSUPPORTED = -1, -4
PREFIX = "clam_mb_forward_bags_many: "
F32, BF16 = N.HIPT_F32, N.HIPT_BF16
# abmil_tile::visit_width: (dtype, S1, S2)
TABLE = {(dt, s1, s2) for dt in (F32, BF16) for s1 in (128, 64) for s2 in (64, 32, 16)} | {(F32, 32, s2) for s2 in (64, 32, 16)}


def weights(dtype=F32, s0=384, s1=128, s2=64, n_att=5, n_classes=None):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_att if n_classes is None else n_classes, n_att=n_att)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def forward(lib, w, B=7, rows=1000, nbytes=None, attention_only=0):
    if nbytes is None:
        nbytes = lib.hipt_clam_mb_many_bags_workspace_bytes(C.byref(w), B, rows)
    return lib.hipt_clam_mb_forward_bags_many(C.byref(w), FAKE, FAKE, B, rows, attention_only, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, nbytes, None)


def test_the_kernel_source_is_in_the_makefile():
    assert "abmil_bags_mb8.hip" in open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()


def test_supported_is_the_width_table_times_five_to_eight_branches():
    lib = N.lib()
    sup = lambda *a, **kw: lib.hipt_clam_mb_many_bags_supported(C.byref(weights(*a, **kw)))
    for dt in (F32, BF16):
        for s1 in (8, 16, 32, 64, 128, 256, 512):          # narrow, mid and wide widths
            for s2 in (4, 8, 16, 32, 64, 256, 384):
                for K in (1, 2, 4, 5, 6, 7, 8, 9):
                    assert sup(dt, 384, s1, s2, K) == int((dt, s1, s2) in TABLE and 5 <= K <= 8), (dt, s1, s2, K)
    for s2 in (64, 32, 16):
        assert sup(F32, 384, 32, s2, 5) == 1 and sup(BF16, 384, 32, s2, 5) == 0     # (32, .) is fp32 only
    for K, C_ in ((5, 6), (6, 5), (8, 1), (5, 2), (7, 8)):
        assert sup(F32, 384, 128, 64, K, n_classes=C_) == 0, (K, C_)               # n_att != n_classes
    assert sup(F32, 96, 128, 64) == 1 and sup(BF16, 96, 128, 64) == 0              # S0: a multiple of 32 (fp32) / 64 (bf16)
    assert sup(F32, 100, 128, 64) == 0 and sup(F32, 0, 128, 64) == 0
    assert sup(2, 384, 128, 64) == 0                                               # no such dtype
    assert lib.hipt_clam_mb_many_bags_supported(None) == 0


@pytest.mark.parametrize("dt,s1,s2,K", [(F32, 128, 64, 5), (BF16, 128, 64, 8), (BF16, 64, 16, 7), (F32, 32, 16, 6)])
def test_workspace_is_the_sum_of_its_three_carves(dt, s1, s2, K):
    """unit table [units x 16 B] | tile_start [B + 1 ints] | partials [units x K x (2 + S1) floats], each rounded up to 256 bytes;
    units = ceil(rows / 128) + B."""
    lib = N.lib()
    w = weights(dt, 384, s1, s2, K)
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    size = lambda B, rows: lib.hipt_clam_mb_many_bags_workspace_bytes(C.byref(w), B, rows)   # noqa: E731
    for B, rows in ((1, 1), (1, 129), (7, 1000), (64, 14_400), (3, 100_000)):
        units = (rows + 127) // 128 + B
        assert size(B, rows) == al(units * 16) + al(4 * (B + 1)) + al(4 * units * K * (2 + s1)), (B, rows)
    assert size(0, 10) == 0 and size(5, 4) == 0 and size(-1, 10) == 0
    assert lib.hipt_clam_mb_many_bags_workspace_bytes(None, 7, 1000) == 0
    for bad in (weights(dt, 384, s1, s2, 4), weights(dt, 384, s1, s2, 9), weights(dt, 384, s1, s2, 1), weights(dt, 1024, 512, 256, K),
                weights(dt, 384, 16, 8, K), weights(dt, 384, s1, s2, K, n_classes=K + 1)):
        assert lib.hipt_clam_mb_many_bags_workspace_bytes(C.byref(bad), 7, 1000) == 0


def test_a_refusal_names_the_branch_range():
    lib = N.lib()
    for w in (weights(F32, 384, 128, 64, 4), weights(F32, 384, 128, 64, 9), weights(F32, 1024, 512, 256, 5), weights(BF16, 384, 32, 16, 5),
              weights(F32, 384, 128, 64, 5, n_classes=6)):
        assert forward(lib, w, nbytes=1 << 24) == E_UNSUPPORTED
        msg = lib.hipt_last_error().decode()
        assert msg.startswith(PREFIX) and "5 <= branches <= 8" in msg and f"[{w.s0},{w.s1},{w.s2}]" in msg, msg
    w = weights()
    short = lib.hipt_clam_mb_many_bags_workspace_bytes(C.byref(w), 7, 1000) - 1
    assert forward(lib, w, nbytes=short) == E_BADARG and lib.hipt_last_error().decode().startswith(PREFIX)
    assert forward(lib, w, B=0, nbytes=1 << 20) == E_BADARG and lib.hipt_last_error().decode().startswith(PREFIX)


def test_bags_form_needs_both_switches_and_the_predicate(monkeypatch):
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    m = CLAM_MB(size_arg=[64, 128, 64], n_classes=5).eval()
    asked = []
    monkeypatch.setattr(m, "_pack_stacked", lambda device: asked.append(device) or weights(F32, 64, 128, 64, 5))
    assert m._bags_form(dev) is None and asked == []            # the defaults never reach the library
    m.bags_many = True                                          # bags_many alone: still the loop
    assert m._bags_form(dev) is None and asked == []
    m.bags_one_call, m.bags_many = True, False                  # bags_one_call alone: the K <= 4 form says no, the loop
    assert m._bags_form(dev) is None
    m.bags_many = True
    w, form = m._bags_form(dev)
    assert form == "mb_many" and w.n_att == 5
    monkeypatch.setattr(m, "_pack_stacked", lambda device: weights(F32, 64, 128, 64, 3))     # K = 3 keeps the form it had
    assert m._bags_form(dev)[1] == "mb"
    monkeypatch.setattr(m, "_pack_stacked", lambda device: weights(F32, 64, 512, 256, 5))    # K = 5 at a wide head: out of scope
    m.bags_wide = True
    assert m._bags_form(dev) is None


def test_the_other_forms_answer_as_before():
    lib = N.lib()
    for dt in (F32, BF16):
        for K in (5, 6, 7, 8):
            w = weights(dt, 384, 128, 64, K)
            assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 0 and lib.hipt_clam_mb_bags_workspace_bytes(C.byref(w), 7, 1000) == 0
            assert lib.hipt_clam_mb_wide_bags_supported(C.byref(weights(dt, 1024, 512, 256, K))) == 0
            assert lib.hipt_clam_mb_supported(C.byref(w)) == 0
            assert lib.hipt_clam_bags_supported(C.byref(w)) == 1        # the one-branch form does not read n_att
        for K in (2, 3, 4):
            w = weights(dt, 384, 128, 64, K)
            assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 1 and lib.hipt_clam_mb_many_bags_supported(C.byref(w)) == 0
    w = weights(F32, 384, 128, 64, 5)
    rc = lib.hipt_clam_mb_forward_bags(C.byref(w), FAKE, FAKE, 7, 1000, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 24, None)
    assert rc == E_UNSUPPORTED and lib.hipt_last_error().decode().startswith("clam_mb_forward_bags: ")


def gpu_test_constants():
    """ROWS, CASES, SEED and MEASURED of the GPU test, read from its source (importing it would need its device)"""
    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_clam_mb_many.py")).read())
    want, out = ("ROWS", "CASES", "SEED", "MEASURED"), {}
    for node in tree.body:
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and getattr(node.targets[0], "id", None) in want:
            out[node.targets[0].id] = ast.literal_eval(node.value)
    assert set(out) == set(want)
    return out


def test_every_bag_of_the_gpu_test_is_decided_beyond_four_times_the_logits_bar():
    """SEED was chosen here, from the fp64 reference alone: of seeds 21..32 the one with the largest smallest gap (1.96e-2)."""
    c = gpu_test_constants()
    assert c["ROWS"] == (1, 2, 15, 17, 127, 128, 129, 300)
    assert c["CASES"] == [((64, 128, 64), 5), ((64, 128, 64), 8), ((192, 128, 64), 6), ((128, 64, 16), 7), ((64, 32, 16), 5)]
    for dtype, rounded in (("fp32", False), ("bf16", True)):
        bar = 2.0 * c["MEASURED"][dtype]["logits"][1]
        if dtype == "fp32":
            bar = min(bar, 1e-4)
        assert bar > 0.0, "the measured loop error of the GPU test is pinned"
        gaps = []
        for size, K in c["CASES"]:
            if rounded and size[1] == 32:
                continue                                   # (32, .) is fp32 only
            p = U.params64(tuple(size), K, True, rounded)
            for b in bags_host(size[0], c["SEED"], tuple(c["ROWS"])):     # bit-equal to the device's bags
                gaps.append(logit_gap(R.clam_mb_forward((b.bfloat16() if rounded else b).double().numpy(), p)))
        assert len(gaps) == (len(c["CASES"]) - int(rounded)) * len(c["ROWS"])
        print(f"{dtype}: smallest gap {min(gaps):.3e}, logits bar {bar:.3e}")
        assert min(gaps) > 4.0 * bar, (dtype, min(gaps), bar)
