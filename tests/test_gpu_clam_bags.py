"""GPU tests (-m gpu) of the ragged multi-bag CLAM_SB forward (csrc/abmil_bags.hip, ``CLAM_SB.forward_bags``).

The row counts of a call are ``ROWS`` (1 687 rows, 17 work units; the last bag alone is 1 000 rows = 8 tiles): bags of one and two
rows between larger ones, a bag that ends one row short of a 128-row tile, one that fills a tile exactly and one that runs one row
past it, so that bag boundaries fall before, on and after the boundaries a tiling of the concatenated rows would have.  ``B = 1``
runs with 129 rows (a full tile and a one-row tile).  What this form shares with the others is stated
once in tests/clam_bags_util.py; graph capture and the two input forms run from tests/test_gpu_clam_forms.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import clam_bags_util as U
from clam_bags_util import DEV, OUTS, TOL, assert_same_bits, bits, errors, md, per_bag
from conftest import golden
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N
from hipt_abmil_atec23_amd import synth
from hipt_abmil_atec23_amd.evaluate import evaluate_split

pytestmark = pytest.mark.gpu
ROWS = [1, 127, 128, 129, 300, 2, 1000]

# bf16: worst |error| per output of the PER-BAG path (CLAM_SB.forward -> hipt_clam_sb_forward, whose code this change does not touch)
# against the fp64 oracle on the bf16-rounded bag and bf16-rounded W1 / Wa / Wb, over the seven bags of ROWS (seed 21) -- measured
# on an MI355X with measure_bf16("per_bag", size).  The bar of the multi-bag path is TWICE the per-bag figure.
#   [384,128,64]: per bag (the weight-stationary streaming kernel, abmil32.hip)  A_raw 8.822e-3  M 5.308e-4  logits 3.040e-4  Y_prob 1.145e-4
#                 forward_bags                                                   A_raw 8.822e-3  M 5.308e-4  logits 3.040e-4  Y_prob 1.144e-4
#   [192, 64,32]: per bag (the fused kernel, abmil.hip)                          A_raw 8.596e-3  M 5.417e-3  logits 1.739e-3  Y_prob 6.051e-4
#                 forward_bags                                                   A_raw 8.596e-3  M 5.843e-4  logits 3.535e-4  Y_prob 5.495e-5
# A_raw is the same arithmetic on both paths.  M: the multi-bag tile pass pools fp32 softmax weights against an fp32 copy of h1 in
# both dtypes (as the streaming kernel does); the fused per-bag kernel pools its bf16 h1 image, hence its larger figures at [192,64,32].
BF16_PER_BAG = {
    (384, 128, 64): {"A_raw": 8.823e-3, "M": 5.309e-4, "logits": 3.040e-4, "Y_prob": 1.145e-4},
    (192, 64, 32): {"A_raw": 8.596e-3, "M": 5.417e-3, "logits": 1.739e-3, "Y_prob": 6.051e-4},
}
BF16_SEED = 21


make = U.make


def bags_of(s0, seed, rows=tuple(ROWS)):
    return U.bags_of(s0, seed, rows)


def reference(size, seed, rounded=False, rows=tuple(ROWS)):
    return U.reference(size, seed, rows, rounded)


def run_bags(m, bags):
    return U.run_form(m, "sb", bags)


# ---------------------------------------------------------------- 1. fp32 parity
@pytest.mark.parametrize("size", [(384, 128, 64), (192, 64, 32)])
@pytest.mark.parametrize("rows", [tuple(ROWS), (129,)])
def test_fp32_parity_per_bag(size, rows):
    m = make(size)
    before = N.calls
    out = run_bags(m, bags_of(size[0], 3, rows))
    assert N.calls == before + 1, "one native call for the whole set"
    assert out["logits"].shape == (len(rows), 2) and out["Y_hat"].shape == (len(rows), 1) and out["Y_hat"].dtype == torch.int64
    assert [tuple(a.shape) for a in out["A_raw"]] == [(1, n) for n in rows]
    worst, wrong = errors(out, reference(size, 3, False, rows))
    print(f"forward_bags fp32 {size} rows {rows}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst
    assert wrong == []


def test_fp32_parity_s1_32_through_the_binding():
    size, rows = (192, 32, 16), tuple(ROWS)
    m = make(size)
    w = m._pack(torch.device(DEV))
    assert N.lib().hipt_clam_bags_supported(C.byref(w)) == 1
    bags = bags_of(192, 5, rows)
    (A_raw, M, logits, Y_prob, Y_hat), _, off = U.direct("sb", w, bags, rows)
    out = {"A_raw": [A_raw[off.host[b]:off.host[b + 1]].view(1, -1) for b in range(len(rows))], "M": M, "logits": logits, "Y_prob": Y_prob,
           "Y_hat": Y_hat.view(-1, 1)}
    worst, wrong = errors(out, reference(size, 5, False, rows))
    print(f"clam_sb_forward_bags fp32 {size}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()) and wrong == [], (worst, wrong)


@pytest.mark.parametrize("size,names", [((384, 128, 64), {1: ("clam_384_n1", 1, 12), 3: ("clam_384_n777", 777, 11)}),
                                        ((192, 128, 64), {2: ("clam_hipt_big_n500", 500, 5)})])
def test_fp32_golden_bags_among_others(size, names):
    """The reference's own outputs (tests/golden) for bags that share a call with other bags."""
    m = make(size)
    bags = list(bags_of(size[0], 7, (300, 129, 2, 127, 64)))
    for pos, (_, n, seed) in names.items():
        bags[pos] = synth.hash_uniform_torch((n, size[0]), seed, device=DEV)
    out = run_bags(m, bags)
    for pos, (name, n, _) in names.items():
        g, got = golden(name), per_bag(out, pos)
        for k in OUTS:
            assert md(got[k], g[k]) <= TOL, (name, k, md(got[k], g[k]))
        assert np.array_equal(got["Y_hat"].cpu().numpy(), g["Y_hat"])


# ---------------------------------------------------------------- 2. the split function
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_evaluate_split_does_not_depend_on_the_chunking(dtype):
    m = make((384, 128, 64), dtype)
    bags = bags_of(384, 9)
    labels = [0, 1, 1, 0, 1, 0, 1]
    a = evaluate_split(m, bags, labels, 2, max_rows_per_call=1 << 16)
    assert m.bags_route == "bags"
    b = evaluate_split(m, bags, labels, 2, max_rows_per_call=300)
    for x, y in ((a.all_probs, b.all_probs), (a.all_labels, b.all_labels), (a.all_preds, b.all_preds)):
        assert x.tobytes() == y.tobytes()
    assert a.error == b.error and a.loss == b.loss and a.acc == b.acc


# ---------------------------------------------------------------- 2b. one tile routine for both kernels
@pytest.mark.parametrize("size,dtype", [((384, 128, 64), "fp32"), ((192, 64, 32), "fp32"), ((192, 64, 32), "bf16")])
def test_tile_is_the_fused_kernels_tile(size, dtype):
    """abmil_bags_kernel and abmil_fused_kernel run the same tile arithmetic on the geometry of csrc/abmil_tile.h, so A_raw of
    ``forward_bags`` is A_raw of per-bag ``forward`` bit for bit.  In fp32 a bag of one tile agrees in every output: the tile's
    running state is that tile's partial, and both combines then do the same arithmetic on one partial."""
    m = make(size, dtype)
    rows = (1, 127, 128, 129, 300)
    bags = bags_of(size[0], 17, rows)
    out = run_bags(m, bags)
    N.profile_enable(True)
    try:
        with torch.no_grad():
            single = [m(b, return_features=True) for b in bags]
        torch.cuda.synchronize()
        counts = {k: c for k, (_, c) in N.profile_read().items()}
    finally:
        N.profile_enable(False)
    # the streaming kernel (abmil32) counts as abmil_fused WITHOUT a combine launch; the generic route launches neither
    if counts.get("abmil_fused") != len(rows) or counts.get("abmil_combine") != len(rows):
        pytest.skip(f"forward did not take abmil_fused_kernel + abmil_combine_kernel here: {counts}")
    for b, (n, (logits, y_prob, y_hat, a_raw, res)) in enumerate(zip(rows, single)):
        got = per_bag(out, b)
        assert bits(got["A_raw"]) == bits(a_raw), f"A_raw of the {n}-row bag"
        if dtype == "fp32" and n <= 128:
            one = {"A_raw": a_raw, "M": res["features"].reshape(got["M"].shape), "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}
            assert_same_bits(got, one, f"{n}-row bag")


# ---------------------------------------------------------------- 3. bf16 parity
def measure_bf16(route, size):
    m = make(size, "bf16")
    bags = bags_of(size[0], BF16_SEED)
    out = run_bags(m, bags) if route == "bags" else U.run_loop(m, bags)
    refs = reference(size, BF16_SEED, True)
    worst, wrong = errors(out, refs)
    return worst, wrong, refs


@pytest.mark.parametrize("size", [(384, 128, 64), (192, 64, 32)])
def test_bf16_parity_per_bag(size):
    worst, wrong, refs = measure_bf16("bags", size)
    bars = {k: 2.0 * v for k, v in BF16_PER_BAG[size].items()}
    print(f"forward_bags bf16 {size}: " + ", ".join(f"{k} {worst[k]:.3e} (bar {bars[k]:.3e})" for k in OUTS))
    for k in OUTS:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])
    # Y_hat only where the reference's two largest logits are further apart than the logit bar; at most one bag is left out
    gaps = [float(np.diff(np.sort(r["logits"].reshape(-1))[-2:])[0]) for r in refs]
    decided = [b for b, gap in enumerate(gaps) if gap > bars["logits"]]
    assert len(decided) >= len(ROWS) - 1, gaps
    assert [b for b in wrong if b in decided] == []


# ---------------------------------------------------------------- 4. fallback route
@pytest.mark.parametrize("cls,size", [(CLAM_SB, (1024, 512, 256)), (CLAM_MB, (192, 128, 64))])
def test_other_configurations_loop_over_forward(cls, size):
    m = make(size, "fp32", cls)
    bags = bags_of(size[0], 13, (1, 129, 300))
    logits, y_prob, y_hat, a_raw, res = m.forward_bags(list(bags), return_features=True)
    assert m.bags_route == "per_bag"
    assert logits.shape == (3, 2) and y_prob.shape == (3, 2) and y_hat.shape == (3, 1) and len(a_raw) == 3
    for b, bag in enumerate(bags):
        with torch.no_grad():   # the inference kernels, as forward_bags runs them (with gradients enabled forward() trains)
            l1, p1, h1, a1, r1 = m(bag, return_features=True)
        assert bits(logits[b:b + 1]) == bits(l1) and bits(y_prob[b:b + 1]) == bits(p1) and bits(y_hat[b:b + 1]) == bits(h1)
        assert bits(a_raw[b]) == bits(a1) and bits(res["features"][b]) == bits(r1["features"].reshape(res["features"][b].shape))
    att = m.forward_bags(list(bags), attention_only=True)
    assert [bits(a) for a in att] == [bits(a) for a in a_raw]


# ---------------------------------------------------------------- the checks every form shares (clam_bags_util), on this form's cases
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_bag_does_not_see_its_neighbours(dtype, monkeypatch):
    U.check_neighbours("sb", (384, 128, 64), 2, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attention_only_writes_a_raw_alone(dtype):
    U.check_attention_only("sb", (384, 128, 64), 2, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_outputs_and_workspace_stay_inside_their_buffers(dtype):
    U.check_fences("sb", (384, 128, 64), 2, dtype)
