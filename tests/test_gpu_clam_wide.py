"""GPU tests (-m gpu) of the ragged multi-bag CLAM_SB forward for the wide heads (csrc/abmil_wide.hip,
``hipt_clam_sb_forward_bags_wide``, ``CLAM_SB.bags_wide``).

Weights and bags are made as in tests/test_gpu_clam_bags.py.  The row counts of a call are ``ROWS`` (1 979 rows, 22 work units):
bags of one and two rows, bags one row short of and one row past the kernel's sub-tiles (32 rows in fp32, 64 in bf16), bags that end
before, on and after a 128-row unit, and a bag of 1 100 rows = 9 units, so that the combine's ``t + 8`` stride has a second term.

The bars.  fp32: the worst |error| against the fp64 oracle over the four shapes and the outputs A_raw, M, logits, Y_prob, measured on
one MI355X, was MEASURED_FP32_NEW for this kernel and MEASURED_FP32_LOOP for the loop of ``forward`` calls on the same bags (the
parent commit's route); FP32_BAR is twice the larger, and stays below the project's fp32 bar of 1e-4.  bf16: the same two
measurements against tests/clam_wide_ref.py (fp64; bag, W1, Wa, Wb rounded to bf16, h1 rounded to bf16 for the gate only), per
output; BF16_BARS is twice the larger per output.  Each test prints its figures before it asserts.

What this form shares with the others is stated once in tests/clam_bags_util.py; graph capture, the two input forms and the default
switch run from tests/test_gpu_clam_forms.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import clam_bags_util as U
import clam_wide_ref as WR
from clam_bags_util import DEV, OUTS, TOL, errors, md, run_loop
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 31, 33, 63, 65, 127, 128, 129, 300, 1100)
assert ROWS == U.FORMS["wide"].rows
ROWS_I = (8, 31, 33, 63, 65, 127, 128, 129, 300, 1100)      # the instance branch needs k_sample = 8 rows per bag
SHAPES = [(128, 256, 64), (128, 512, 256), (1024, 512, 384), (1024, 512, 256)]
# worst |error| over SHAPES and OUTS against the fp64 oracle, fp32 mode (seed 3), measured: (this kernel, the loop of forward calls)
MEASURED_FP32_NEW, MEASURED_FP32_LOOP = 3.338e-6, 3.338e-6      # both at (1024, 512, 384), A_raw; bar 6.676e-6
FP32_BAR = 2.0 * max(MEASURED_FP32_NEW, MEASURED_FP32_LOOP)
# bf16: the seed of the bags, chosen on the host from the fp64 reference of tests/clam_wide_ref.py alone: of seeds 21..28 the one whose
# smallest gap between a bag's two reference logits, over the four shapes and eleven bags, is largest (9.2e-2)
BF16_SEED = 22
# worst |error| per output over SHAPES against tests/clam_wide_ref.py, bf16 mode, measured: (this kernel, the loop of forward calls)
MEASURED_BF16 = {"A_raw": (1.421e-3, 1.421e-3), "M": (1.438e-4, 1.438e-4), "logits": (2.471e-5, 2.467e-5), "Y_prob": (8.918e-6, 8.948e-6)}
BF16_BARS = {k: 2.0 * max(v) for k, v in MEASURED_BF16.items()}


make = functools.partial(U.model, "wide")


def bags_of(s0, seed, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def run_wide(m, bags, **kw):
    return U.run_form(m, "wide", bags, **kw)


def decided(refs, bar):
    """bags whose two reference logits lie further apart than the bar"""
    return [b for b, r in enumerate(refs) if float(np.diff(np.sort(r["logits"].reshape(-1))[-2:])[0]) > bar]


# ---------------------------------------------------------------- 1. fp32 parity
@pytest.mark.parametrize("size", SHAPES)
def test_fp32_parity_per_bag(size):
    m = make(size)
    w = m._pack(torch.device(DEV))
    assert N.lib().hipt_clam_bags_supported(C.byref(w)) == 0 and N.lib().hipt_clam_wide_bags_supported(C.byref(w)) == 1
    bags = bags_of(size[0], 3)
    refs = U.reference(size, 3, ROWS)
    loop, _ = errors(run_loop(m, bags), refs)
    before = N.calls
    out = run_wide(m, bags)
    assert N.calls == before + 1, "one native call for the whole set"
    assert out["logits"].shape == (len(ROWS), 2) and out["Y_hat"].shape == (len(ROWS), 1) and out["Y_hat"].dtype == torch.int64
    assert out["M"].shape == (len(ROWS), size[1])
    assert [tuple(a.shape) for a in out["A_raw"]] == [(1, n) for n in ROWS]
    worst, wrong = errors(out, refs)
    print(f"wide forward_bags fp32 {size}: " + ", ".join(f"{k} {worst[k]:.3e} (per-bag loop {loop[k]:.3e})" for k in OUTS))
    assert FP32_BAR <= TOL
    assert all(v <= FP32_BAR for v in worst.values()), (worst, FP32_BAR)
    assert [b for b in wrong if b in decided(refs, FP32_BAR)] == []


# ---------------------------------------------------------------- 2. bf16 parity
@pytest.mark.parametrize("size", SHAPES)
def test_bf16_parity_per_bag(size):
    """Reference: tests/clam_wide_ref.py.  The bar per output is BF16_BARS (the header)."""
    m = make(size, "bf16")
    bags = bags_of(size[0], BF16_SEED)
    refs = WR.reference(size, BF16_SEED, ROWS)
    loop, _ = errors(run_loop(m, bags), refs)
    worst, wrong = errors(run_wide(m, bags), refs)
    print(f"wide forward_bags bf16 {size}: " + ", ".join(f"{k} {worst[k]:.3e} (per-bag loop {loop[k]:.3e})" for k in OUTS))
    gaps = [float(np.diff(np.sort(r["logits"].reshape(-1))[-2:])[0]) for r in refs]
    print(f"  smallest reference logit gap {min(gaps):.3e}")
    for k in OUTS:
        assert worst[k] <= BF16_BARS[k], (k, worst[k], BF16_BARS[k])
    assert min(gaps) > BF16_BARS["logits"], (min(gaps), BF16_BARS["logits"])   # every bag's class is decided beyond the logit bar
    assert wrong == []


# ---------------------------------------------------------------- 3. the instance branch
@pytest.mark.parametrize("subtyping", [False, True])
def test_instance_branch_is_the_per_bag_chain(subtyping):
    size, k = (128, 256, 64), 8
    m = make(size, "fp32", subtyping=subtyping)
    bags = bags_of(128, 23, ROWS_I)
    labels = [b % 2 for b in range(len(ROWS_I))]
    run_wide(m, bags[:1])   # the weight image exists
    before = N.calls
    out = run_wide(m, bags, label=labels, instance_eval=True)
    assert N.calls == before + 3, "forward, segmented top-k, gather"
    res = out["res"]
    w = m._pack(torch.device(DEV))
    st = N.stream_ptr(torch.device(DEV))
    for b, bag in enumerate(bags):
        a = out["A_raw"][b].contiguous()
        ids = torch.empty((1, 2, k), dtype=torch.int64, device=DEV)
        N.call("hipt_topk_rows", N.ptr(a), 1, bag.shape[0], k, N.ptr(ids), st)
        rows = torch.empty((1, 2, k, size[1]), dtype=torch.float32, device=DEV)
        x = bag.contiguous()
        N.call("hipt_clam_gather_h1", C.byref(w), N.ptr(x), N.ptr(ids), 2 * k, N.ptr(rows), st)
        torch.cuda.synchronize()
        with torch.no_grad():
            one = m._instance_branch(lambda r: (rows[r, 0], rows[r, 1]), torch.tensor([labels[b]], device=DEV))
        assert np.array_equal(res["inst_preds"][b], one["inst_preds"]) and np.array_equal(res["inst_labels"][b], one["inst_labels"])
        want = float(one["instance_loss"])
        assert abs(float(res["instance_loss"][b]) - want) <= 1e-6 * abs(want), (b, float(res["instance_loss"][b]), want)


# ---------------------------------------------------------------- 4. the split functions
def test_split_functions_on_the_device():
    m = make((128, 256, 64), "fp32", subtyping=True)
    bags = bags_of(128, 23, ROWS_I)
    labels = [b % 2 for b in range(len(ROWS_I))]
    e1 = evaluate_split(m, bags, labels, 2, max_rows_per_call=1 << 16, wide_one_call=True)
    assert m.bags_route == "bags" and "bags_wide" not in m.__dict__
    e2 = evaluate_split(m, bags, labels, 2, max_rows_per_call=300, wide_one_call=True)
    for x, y in ((e1.all_probs, e2.all_probs), (e1.all_labels, e2.all_labels), (e1.all_preds, e2.all_preds)):
        assert x.tobytes() == y.tobytes()
    assert e1.error == e2.error and e1.loss == e2.loss and e1.acc == e2.acc
    v1 = validate_split(m, bags, labels, 2, max_rows_per_call=1 << 16, wide_one_call=True)
    assert m.bags_route == "bags" and "bags_wide" not in m.__dict__
    v2 = validate_split(m, bags, labels, 2, max_rows_per_call=300, wide_one_call=True)
    assert v1.prob.tobytes() == v2.prob.tobytes() and v1.labels.tobytes() == v2.labels.tobytes()
    assert (v1.val_loss, v1.val_error, v1.val_inst_loss, v1.inst_count, v1.acc, v1.inst) == (v2.val_loss, v2.val_error, v2.val_inst_loss, v2.inst_count, v2.acc, v2.inst)
    assert e1.all_probs.tobytes() == v1.prob.tobytes()
    # against the loop over forward: the default
    e0 = evaluate_split(m, bags, labels, 2)
    assert m.bags_route == "per_bag"
    v0 = validate_split(m, bags, labels, 2)
    assert m.bags_route == "per_bag"
    print(f"split functions: evaluate {md(e1.all_probs, e0.all_probs):.3e}, validate {md(v1.prob, v0.prob):.3e} (bar {FP32_BAR:.3e})")
    assert md(e1.all_probs, e0.all_probs) <= FP32_BAR and md(v1.prob, v0.prob) <= FP32_BAR
    assert e1.acc == e0.acc and v1.acc == v0.acc and v1.inst == v0.inst and v1.inst_count == v0.inst_count
    assert np.array_equal(e1.all_preds, e0.all_preds)


# ---------------------------------------------------------------- the checks every form shares (clam_bags_util), on this form's cases
ROWS_PAST = (129, 64, 257)                                  # the call's last bag ends one row past a unit
SMALL = [(128, 256, 64), (128, 512, 256)]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", SMALL + [(1024, 512, 384)])
def test_a_bag_does_not_see_its_neighbours(size, dtype, monkeypatch):
    U.check_neighbours("wide", size, 2, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", SMALL)
def test_attention_only_writes_a_raw_alone(size, dtype):
    U.check_attention_only("wide", size, 2, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,rows", [((128, 256, 64), ROWS), ((128, 512, 256), ROWS), ((128, 512, 384), ROWS_PAST)])
def test_outputs_and_workspace_stay_inside_their_buffers(size, rows, dtype):
    U.check_fences("wide", size, 2, dtype, rows)
