"""GPU tests (-m gpu) of the ragged multi-bag CLAM_MB forward for 5 to 8 branches (csrc/abmil_bags_mb8.hip,
``hipt_clam_mb_forward_bags_many``; ``CLAM_MB`` with ``bags_one_call`` and ``bags_many`` both set).

Weights and bags are made as in tests/test_gpu_clam_wide_mb.py.  The row counts of a call are ``ROWS`` (719 rows, 11 work units): bags
of one and two rows, bags one row short of and one row past a 16-row MFMA block, bags that end before, on and after a 128-row unit, and
a bag of 300 rows = 3 units.  ``CASES``: K = 5 and K = 8 at [64, 128, 64], K = 6 at hipt_big's [192, 128, 64], K = 7 at [128, 64, 16]
and K = 5 at the fp32-only [64, 32, 16].

The bars.  Reference: ``clam_bags_util.reference(..., multi=True)`` (fp64, tests/clam_mb_ref.py; in bf16 mode on the bf16-rounded bag,
W1, Wa and Wb).  Per dtype and output, the worst |error| over CASES of the loop of ``forward`` calls on the same bags -- the route these
models take without this kernel -- was measured on one MI355X (MEASURED[dtype][output][1]; [0] is this kernel's figure in the same
run); the bar is twice the loop's figure, the factor covering the different fold order, and in fp32 never above the project's 1e-4.
SEED was chosen on the host from the fp64 reference alone: of seeds 21..32 the one whose smallest gap between a bag's two largest
reference logits, over CASES, both rounding modes and all bags, is largest (1.96e-2); tests/test_clam_mb_many_host.py holds that gap
against 4x the logits bars.  Each test prints its figures before it asserts.

What this form shares with the others is stated once in tests/clam_bags_util.py; graph capture, the two input forms and either
switch off run from tests/test_gpu_clam_forms.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import clam_bags_util as U
from clam_bags_util import DEV, OUTS, TOL, as_out, bits, errors, md, run_loop
from clam_wide_mb_ref import logit_gap
from hipt_abmil_atec23_amd import CLAM_MB, _native as N, synth
from hipt_abmil_atec23_amd.evaluate import validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 15, 17, 127, 128, 129, 300)
assert ROWS == U.FORMS["mb_many"].rows
CASES = [((64, 128, 64), 5), ((64, 128, 64), 8), ((192, 128, 64), 6), ((128, 64, 16), 7), ((64, 32, 16), 5)]
PARITY = [(s, K, dt) for dt in ("fp32", "bf16") for s, K in CASES if not (dt == "bf16" and s[1] == 32)]   # (32, .) is fp32 only
SEED = 29
# worst |error| per output over CASES against the fp64 reference, measured: (this kernel, the loop of forward calls)
MEASURED = {
    "fp32": {"A_raw": (1.354e-6, 1.354e-6), "M": (5.238e-7, 5.238e-7), "logits": (4.425e-7, 4.425e-7), "Y_prob": (5.870e-8, 5.718e-8)},
    "bf16": {"A_raw": (9.497e-3, 9.497e-3), "M": (1.356e-3, 3.129e-3), "logits": (6.367e-4, 1.611e-3), "Y_prob": (1.078e-4, 2.366e-4)},
}
BARS = {dt: {k: (min(2.0 * v[1], TOL) if dt == "fp32" else 2.0 * v[1]) for k, v in d.items()} for dt, d in MEASURED.items()}


make = functools.partial(U.model, "mb_many")


def bags_of(s0, seed=SEED, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def run_bags(m, bags, **kw):
    return U.run_form(m, "mb_many", bags, **kw)


def parity_figures(size, K, dtype):
    """(this kernel's worst errors, the loop's, bags with another Y_hat, the reference's logit gaps, the call's outputs)"""
    m = make(size, dtype, K)
    bags = bags_of(size[0])
    refs = U.reference(size, SEED, ROWS, dtype == "bf16", K, True)
    loop, _ = errors(run_loop(m, bags), refs, True)
    before = N.calls
    out = run_bags(m, bags)
    assert N.calls == before + 1, "one native call for the whole set"
    worst, wrong = errors(out, refs, True)
    return worst, loop, wrong, [logit_gap(r) for r in refs], out


# ---------------------------------------------------------------- 1. parity against the fp64 reference, and the route
@pytest.mark.parametrize("size,K,dtype", PARITY)
def test_parity_per_bag(size, K, dtype):
    w = make(size, dtype, K)._pack_stacked(torch.device(DEV))
    lib = N.lib()
    assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 0 and lib.hipt_clam_mb_many_bags_supported(C.byref(w)) == 1
    worst, loop, wrong, gaps, out = parity_figures(size, K, dtype)
    assert out["logits"].shape == (len(ROWS), K) and out["Y_prob"].shape == (len(ROWS), K)
    assert out["Y_hat"].shape == (len(ROWS), 1) and out["Y_hat"].dtype == torch.int64
    assert out["M"].shape == (len(ROWS), K, size[1])
    assert [tuple(a.shape) for a in out["A_raw"]] == [(K, n) for n in ROWS]
    print(f"mb many forward_bags {dtype} {size} K={K}: " + ", ".join(f"{k} {worst[k]:.3e} (per-bag loop {loop[k]:.3e})" for k in OUTS))
    print(f"  smallest reference logit gap {min(gaps):.3e}")
    bars = BARS[dtype]
    if dtype == "fp32":
        assert max(bars.values()) <= TOL
    for k in OUTS:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])
    assert min(gaps) > 4.0 * bars["logits"], (min(gaps), bars["logits"])   # every bag's class is decided beyond the logit bar
    assert wrong == []                                                     # no bag left out


# ---------------------------------------------------------------- 2. a branch has the bits the K <= 4 kernel gives it
def subset_model(m, size, dtype, lo, hi):
    """A CLAM_MB of hi - lo classes from branches [lo, hi) of ``m``: its rows of attention_c, its bag and instance classifiers; fc1,
    attention_a and attention_b shared"""
    sd, sub = m.state_dict(), {}
    for name, v in sd.items():
        head, _, rest = name.partition(".")
        if "attention_c" in name:
            sub[name] = v[lo:hi].clone()
        elif head in ("classifiers", "instance_classifiers"):
            i, _, tail = rest.partition(".")
            if lo <= int(i) < hi:
                sub[f"{head}.{int(i) - lo}.{tail}"] = v.clone()
        else:
            sub[name] = v.clone()
    s = CLAM_MB(size_arg=list(size), n_classes=hi - lo)
    s.load_state_dict(sub, strict=True)
    s.relocate()
    s.bags_one_call = True
    return s.eval().set_compute_dtype(dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K,groups", [((192, 128, 64), 6, ((0, 4), (4, 6))), ((64, 128, 64), 8, ((0, 4), (4, 8))),
                                           ((128, 64, 16), 7, ((0, 4), (4, 7), (2, 6)))])
def test_a_branch_has_the_bits_of_the_k_le_4_kernel(size, K, groups, dtype):
    m = make(size, dtype, K)
    bags = bags_of(size[0])
    full = run_bags(m, bags)
    A = torch.cat(list(full["A_raw"]), dim=1)                      # [K, rows]
    for lo, hi in groups:
        s = subset_model(m, size, dtype, lo, hi)
        w = s._pack_stacked(torch.device(DEV))
        assert N.lib().hipt_clam_mb_bags_supported(C.byref(w)) == 1 and s._bags_form(torch.device(DEV))[1] == "mb"
        sub = as_out(s.forward_bags(list(bags), return_features=True))
        assert s.bags_route == "bags"
        As = torch.cat(list(sub["A_raw"]), dim=1)
        for k in range(lo, hi):
            assert bits(A[k]) == bits(As[k - lo]), f"A_raw of branch {k} (group {lo}:{hi})"
            assert bits(full["M"][:, k]) == bits(sub["M"][:, k - lo]), f"M of branch {k} (group {lo}:{hi})"
            assert bits(full["logits"][:, k]) == bits(sub["logits"][:, k - lo]), f"logits of branch {k} (group {lo}:{hi})"


# ---------------------------------------------------------------- the checks every form shares (clam_bags_util), on this form's cases
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", U.FORMS["mb_many"].invariance)
def test_a_bag_does_not_see_its_neighbours(size, K, dtype, monkeypatch):
    U.check_neighbours("mb_many", size, K, dtype, monkeypatch)      # (the small grid: all 11 units on ONE workgroup)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", [((64, 128, 64), 8), ((128, 64, 16), 7)])
def test_attention_only_writes_a_raw_alone_and_nothing_leaves_its_buffer(size, K, dtype):
    U.check_attention_only("mb_many", size, K, dtype)
    U.check_fences("mb_many", size, K, dtype)


# ---------------------------------------------------------------- 3. validation of a split
def test_validate_split_in_one_call_agrees_with_the_loop():
    size, K = (64, 128, 64), 5
    m = CLAM_MB(size_arg=list(size), n_classes=K, k_sample=2)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=K, multi=True), size[0]), strict=True)
    m.relocate()
    m.eval().set_compute_dtype("fp32")
    rows = (2, 15, 17, 40, 127, 128, 129, 300)
    assert min(rows) >= m.k_sample == 2
    bags = bags_of(size[0], 23, rows)
    labels = [b % K for b in range(len(rows))]
    before = N.calls
    v1 = validate_split(m, bags, labels, K, many_one_call=True)
    calls = N.calls - before
    assert m.bags_route == "bags" and "bags_many" not in m.__dict__ and "bags_one_call" not in m.__dict__
    v0 = validate_split(m, bags, labels, K, many_one_call=False)
    assert m.bags_route == "per_bag" and N.calls - before - calls > calls
    bars = BARS["fp32"]
    print(f"validate_split mb many: prob {md(v1.prob, v0.prob):.3e} (bar {bars['Y_prob']:.3e}), loss {abs(v1.val_loss - v0.val_loss):.3e}, "
          f"instance loss {abs(v1.val_inst_loss - v0.val_inst_loss):.3e} (bar {bars['logits']:.3e}); native calls {calls}")
    assert md(v1.prob, v0.prob) <= bars["Y_prob"]
    assert abs(v1.val_loss - v0.val_loss) <= bars["logits"] and abs(v1.val_inst_loss - v0.val_inst_loss) <= bars["logits"]
    assert v1.val_error == v0.val_error
    assert v1.acc == v0.acc and v1.inst == v0.inst and v1.inst_count == v0.inst_count == len(rows)
    assert v1.labels.tobytes() == v0.labels.tobytes()
    assert np.array_equal(v1.prob.argmax(axis=1), v0.prob.argmax(axis=1))
