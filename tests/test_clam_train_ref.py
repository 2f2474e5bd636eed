"""CPU tests of tests/clam_train_ref.py, and the home of the bars the GPU tests of the CLAM training step use.

* `restated` (the backward by hand) equals `truth` (fp64 autograd of the oracle) to 1e-10 on every tensor;
* the NOISE FLOOR: the fp32 CPU oracle against `truth`, rel-L2 per tensor, the maximum over the cases of a group (FLOOR below,
  re-measured here; DESIGN.md 5 has the table).  BARS = 8 x FLOOR: the kernels add in another order at the same precision (16 column-group
  partials, serial column sums over N, fp32 atomics for long bags).  No bar comes from what a kernel produced;
* the inputs of every case meet the conditions the comparison stands on (top-k gaps, rows selected twice, the edge family's reach);
* every wrong-kernel variant lands >= 3 x beyond a bar in a case designed for it (clam_train_ref.VARIANT_CASES)."""
import pytest
import torch

import clam_train_ref as R

MARGIN = 8.0
# worst rel-L2 of the fp32 oracle against the fp64 one over the cases of the group, per kind of tensor (clam_train_ref.KINDS)
FLOOR = {
    "short": dict(logits=1.09e-06, A_raw=4.55e-07, M=3.53e-07, loss=1.39e-07, W1=8.17e-07, b1=6.28e-07, Wa=8.05e-07, ba=3.96e-06, Wb=8.29e-07,
                  bb=6.80e-07, wc=7.97e-07, bc=3.39e-05, wcls=3.92e-07, bcls=2.44e-07, winst=4.02e-07, binst=7.89e-07, bag=8.20e-07),
    "long": dict(logits=1.94e-07, A_raw=3.58e-07, M=1.32e-07, loss=5.60e-08, W1=6.32e-07, b1=2.03e-07, Wa=7.21e-07, ba=2.54e-06, Wb=8.52e-07,
                 bb=8.36e-07, wc=7.79e-07, bc=1.27e-05, wcls=2.03e-07, bcls=1.27e-07, winst=2.43e-07, binst=2.80e-07, bag=7.09e-07),
    "edge": dict(logits=1.00e-05, A_raw=8.21e-07, M=4.86e-06, loss=2.20e-06, W1=9.38e-06, b1=9.27e-06, Wa=9.39e-06, ba=9.39e-06, Wb=8.50e-06,
                 bb=8.51e-06, wc=8.64e-06, bc=5.18e-06, wcls=1.05e-05, bcls=4.10e-07, winst=3.10e-07, binst=4.89e-07, bag=9.53e-06),
}
BARS = {g: {k: MARGIN * v for k, v in d.items()} for g, d in FLOOR.items()}
# (bc under the extended loss is sum_n cA[k, n] -- ~0.3 / sqrt(N) -- plus a sum of N terms of dA that cancels to zero: its floor grows with
#  N and the 4 096-row case sets the short group's.  Under the plain loss the true value is zero and the bar is absolute: R.abs_bar.)
MIN_GAP = 1e-4          # k-th minus (k+1)-th score of every top-k: ~100 x A_raw's floor, the ids cannot flip between fp32 and fp64
FLOOR_SLACK = 1.5       # the fp32 oracle's own summation order moves with the BLAS and its thread count

_cache = {}


def case_data(name):
    """(inputs, truth) of a case, computed once"""
    if name not in _cache:
        inp = R.inputs(R.BY_NAME[name])
        _cache[name] = (inp, R.truth(inp))
    return _cache[name]


def test_case_list_covers_what_it_is_meant_to():
    assert 20 <= len(R.CASES) <= 30 and len(R.BY_NAME) == len(R.CASES)
    assert {c.size for c in R.CASES} == {R.BIG, R.TINY, R.SMALL, R.ODD, R.DEF}
    assert {1, 15, 16, 17, 100, 4096, 4097, 8200} <= {c.n for c in R.CASES}
    assert {c.C for c in R.CASES if c.multi} >= {3, 5, 8} and {c.C for c in R.CASES if not c.multi} >= {2, 5}
    assert {(c.sub, c.inst) for c in R.CASES} >= {(True, True), (False, True), (False, False)}
    assert sum(not c.ext for c in R.CASES) == 1
    assert {(c.size, c.n) for c in R.CASES if c.drop} >= {(R.BIG, 17), (R.BIG, 4097)} and any(c.drop and c.size == R.ODD for c in R.CASES)
    edge = {(c.size, c.n, c.C if c.multi else 1) for c in R.CASES if c.family == "edge"}
    assert {(R.BIG, 100, 1), (R.ODD, 37, 5)} <= edge and any(s == R.BIG and n == 4097 for s, n, _ in edge)
    assert set(R.VARIANT_CASES) == set(R.VARIANTS) and all(n in R.BY_NAME for v in R.VARIANT_CASES.values() for n in v)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_restated_backward_equals_autograd_truth(name):
    """with and without masks, cA / cM and the instance branch, every group: 1e-10 rel-L2 on every output and gradient, d bag included"""
    inp, (out, grads, aux) = case_data(name)
    ro, rg = R.restated(inp)
    assert set(rg) == set(grads) and "bag" in rg
    for k, (kind, v, absolute) in R.errors(ro, rg, out, grads, inp).items():
        assert v < 1e-10, (name, k, v)  # (rel-L2; the max abs of a tensor whose true gradient is zero)
    if inp.case.inst:
        assert abs(ro["instance_loss"] - out["instance_loss"]) < 1e-12 and (ro["inst_preds"] == out["inst_preds"]).all()


def test_restated_without_masks_and_external_terms():
    """the dropout case again with its masks, its cA / cM or both taken away"""
    base = R.inputs(R.BY_NAME["odd_n37_mb5_drop"])
    for masks, ext in ((None, True), (base.masks, False), (None, False)):
        inp = R.Inputs(base.case, base.p, base.bag, masks, base.cA if ext else None, base.cM if ext else None, base.label)
        out, grads, aux = R.truth(inp)
        for k, (kind, v, absolute) in R.errors(*R.restated(inp), out, grads, inp).items():
            assert v < 1e-10, (masks is None, ext, k, v)


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_input_conditions(name):
    inp, _ = case_data(name)
    c = inp.case
    cond = R.conditions(inp)
    assert cond["min_gap"] >= MIN_GAP, cond
    assert cond["min_abs_z1"] >= R.RELU_MARGIN, cond
    if name in R.SELECTED_TWICE:
        assert cond["selected_twice"] >= 1, cond
    if c.family == "edge":
        assert 0.3 <= cond["h1_zero"] <= 0.7 and cond["gate_beyond_15"] >= 0.02 and cond["gate_max"] >= 30 and cond["p_max"] >= 0.5, cond
        assert 30 <= cond["A_span"] <= 45, cond
    if c.drop:
        assert all(0.15 < float((m == 0).float().mean()) < 0.35 for m in inp.masks)


def test_noise_floor_is_what_the_bars_were_made_of():
    """the fp32 oracle against the fp64 one, per case and tensor: no case above its group's committed floor, and every group's worst
    tensor within FLOOR_SLACK of it (a floor that went stale would leave the bars looser than 8 x)"""
    seen = {g: {} for g in FLOOR}
    for c in R.CASES:
        inp, (out, grads, aux) = case_data(c.name)
        fo, fg, _ = R.autograd_step(inp, torch.float32)
        g = R.group_of(c)
        for name, (kind, v, absolute) in R.errors(fo, fg, out, grads, inp).items():
            if absolute:
                assert v < R.abs_bar(aux) / 8, (c.name, name, v)  # (the fp32 oracle itself sits far inside the absolute bar)
                continue
            assert v <= FLOOR_SLACK * FLOOR[g][kind], (c.name, name, v, FLOOR[g][kind])
            seen[g][kind] = max(seen[g].get(kind, 0.0), v)
    for g in FLOOR:
        print(f"\n{g}: " + ", ".join(f"{k}={seen[g][k]:.2e}" for k in R.KINDS))
        assert set(seen[g]) == set(R.KINDS)
        worst = max(R.KINDS, key=lambda k: FLOOR[g][k])
        assert seen[g][worst] >= FLOOR[g][worst] / FLOOR_SLACK, (g, worst, seen[g][worst])


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_every_variant_clears_a_bar_threefold(variant):
    for name in R.VARIANT_CASES[variant]:
        inp, (out, grads, aux) = case_data(name)
        vo, vg = R.restated(inp, variant)
        worst, at = R.worst_ratio(R.errors(vo, vg, out, grads, inp), BARS[R.group_of(inp.case)], aux)
        print(f"{variant} in {name}: {worst:.3g} x the bar of {at}")
        assert worst >= 3.0, (variant, name, worst, at)
