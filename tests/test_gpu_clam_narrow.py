"""GPU tests (-m gpu) of the ragged multi-bag CLAM_SB forward for the narrow heads (csrc/abmil_narrow.hip,
``hipt_clam_sb_forward_bags_narrow``, ``CLAM_SB.bags_narrow``).

Weights and bags are made as in tests/test_gpu_clam_bags.py.  The row counts of a call are ``ROWS`` (1 851 rows, 19 work units):
bags of one and two rows, bags one row short of and one row past a 32-row wave block, bags that end before, on and after a 128-row
tile, and a bag of 1 100 rows = 9 tiles, so that the combine's ``t + 8`` stride has a second term.  What this form shares with the
others is stated once in tests/clam_bags_util.py; graph capture, the two input forms and the default switch run from
tests/test_gpu_clam_forms.py."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import clam_bags_util as U
from clam_bags_util import DEV, OUTS, TOL, bits, errors, md, per_bag, run_loop
from conftest import golden
from hipt_abmil_atec23_amd import CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd import synth
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 31, 33, 127, 128, 129, 300, 1100)
assert ROWS == U.FORMS["narrow"].rows
ROWS_I = (8, 31, 33, 127, 128, 129, 300, 1100)      # the instance branch needs k_sample = 8 rows per bag
SHAPES = [(192, 16, 8), (192, 8, 4), (512, 32, 8), (1024, 32, 8)]
SHAPES_BF16 = SHAPES + [(192, 32, 16)]
# bf16: the seed of the bags, chosen on the host from the fp64 reference (bf16-rounded bag, W1, Wa, Wb) alone: of seeds 21..28 the
# one whose smallest gap between a bag's two reference logits, over the five shapes and nine bags, is largest (5.7e-2)
BF16_SEED = 26


make = functools.partial(U.model, "narrow")


def bags_of(s0, seed, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def reference(size, seed, rounded=False, rows=ROWS):
    return U.reference(size, seed, rows, rounded)


def run_narrow(m, bags, **kw):
    return U.run_form(m, "narrow", bags, **kw)


# ---------------------------------------------------------------- 1. fp32 parity
@pytest.mark.parametrize("size", SHAPES)
def test_fp32_parity_per_bag(size):
    m = make(size)
    w = m._pack(torch.device(DEV))
    assert N.lib().hipt_clam_bags_supported(C.byref(w)) == 0 and N.lib().hipt_clam_narrow_bags_supported(C.byref(w)) == 1
    before = N.calls
    out = run_narrow(m, bags_of(size[0], 3))
    assert N.calls == before + 1, "one native call for the whole set"
    assert out["logits"].shape == (len(ROWS), 2) and out["Y_hat"].shape == (len(ROWS), 1) and out["Y_hat"].dtype == torch.int64
    assert out["M"].shape == (len(ROWS), size[1])
    assert [tuple(a.shape) for a in out["A_raw"]] == [(1, n) for n in ROWS]
    worst, wrong = errors(out, reference(size, 3))
    print(f"narrow forward_bags fp32 {size}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst
    assert wrong == []


# ---------------------------------------------------------------- 2. the reference's own bag among others
def test_fp32_golden_bag_among_others():
    """The reference module's outputs (tests/golden) for its hipt_smallest bag, sharing a call with other bags; the instance branch's
    top-k ids from the scores of this call."""
    name, size, base, n, seed, k = "clam_hipt_smallest_n100", (192, 8, 4), 8, 100, 6, 4
    g = golden(name)
    m = CLAM_SB(gate=True, size_arg="hipt_smallest", k_sample=k, n_classes=2, subtyping=True)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size), base), strict=True)
    m.relocate()
    m.eval()
    rows = (300, 129, 100, 4, 127)
    bags = list(bags_of(192, 7, rows))
    pos = 2
    bags[pos] = synth.hash_uniform_torch((n, 192), seed, device=DEV)
    out = run_narrow(m, bags)
    got = per_bag(out, pos)
    for key in OUTS:
        assert md(got[key], g[key]) <= TOL, (key, md(got[key], g[key]))
    assert np.array_equal(got["Y_hat"].cpu().numpy(), g["Y_hat"])
    off = Fn.BagOffsets(np.cumsum([0, *rows]), sum(rows), torch.device(DEV))
    ids, gids = Fn.topk_segments(torch.cat(out["A_raw"], dim=1).reshape(-1).contiguous(), off, k)
    torch.cuda.synchronize()
    same = lambda got, want: np.array_equal(np.sort(got.cpu().numpy()), np.sort(np.asarray(want).reshape(-1)))   # as sets: the order within the k is each top-k's own
    assert same(ids[pos, 0, 0], g["top_p"]) and same(ids[pos, 0, 1], g["top_n"])
    assert np.array_equal(gids[pos].cpu().numpy(), ids[pos].cpu().numpy() + off.host[pos])


# ---------------------------------------------------------------- 3. bf16 parity
@pytest.mark.parametrize("size", SHAPES_BF16)
def test_bf16_parity_per_bag(size):
    """Reference: the fp64 oracle on the bf16-rounded bag and bf16-rounded W1 / Wa / Wb.  The bar per output is TWICE the worst error of
    the per-bag ``forward`` loop (the generic path: the same rounding model) on the same bags, measured here."""
    m = make(size, "bf16")
    bags = bags_of(size[0], BF16_SEED)
    refs = reference(size, BF16_SEED, True)
    loop, loop_wrong = errors(run_loop(m, bags), refs)
    worst, wrong = errors(run_narrow(m, bags), refs)
    bars = {k: 2.0 * v for k, v in loop.items()}
    print(f"narrow forward_bags bf16 {size}: " + ", ".join(f"{k} {worst[k]:.3e} (per-bag loop {loop[k]:.3e})" for k in OUTS))
    for k in OUTS:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])
    gaps = [float(np.diff(np.sort(r["logits"].reshape(-1))[-2:])[0]) for r in refs]
    assert min(gaps) > bars["logits"], (min(gaps), bars["logits"])   # every bag's class is decided beyond the logit bar
    assert wrong == []


# ---------------------------------------------------------------- 4. the width both kernels have
def test_fp32_s1_32_s2_16_agrees_with_the_wide_call():
    size = (192, 32, 16)
    w = make(size)._pack(torch.device(DEV))
    assert N.lib().hipt_clam_bags_supported(C.byref(w)) == 1 and N.lib().hipt_clam_narrow_bags_supported(C.byref(w)) == 1
    bags = bags_of(192, 5)
    a, _, _ = U.direct("narrow", w, bags, ROWS)
    b, _, _ = U.direct("sb", w, bags, ROWS)
    torch.cuda.synchronize()
    for name, x, y in zip(OUTS, a[:4], b[:4]):
        assert md(x, y.cpu().numpy()) <= 1e-5, (name, md(x, y.cpu().numpy()))
    assert bits(a[4]) == bits(b[4])
    # forward_bags keeps the existing kernel for it, switch or not
    m = make(size)
    out = run_narrow(m, bags)
    assert bits(torch.cat(out["A_raw"], dim=1).reshape(-1)) == bits(b[0]) and bits(out["M"]) == bits(b[1])


# ---------------------------------------------------------------- 5. the instance branch and the split functions
@pytest.mark.parametrize("subtyping", [False, True])
def test_instance_branch_is_the_per_bag_chain(subtyping):
    size, k = (192, 16, 8), 8
    m = make(size, "fp32", subtyping=subtyping)
    bags = bags_of(192, 23, ROWS_I)
    labels = [b % 2 for b in range(len(ROWS_I))]
    run_narrow(m, bags[:1])   # the weight image exists
    before = N.calls
    out = run_narrow(m, bags, label=labels, instance_eval=True)
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


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_split_functions_on_the_device(dtype):
    m = make((192, 16, 8), dtype, subtyping=True)
    bags = bags_of(192, 23, ROWS_I)
    labels = [b % 2 for b in range(len(ROWS_I))]
    e1 = evaluate_split(m, bags, labels, 2, max_rows_per_call=1 << 16)
    assert m.bags_route == "bags" and "bags_narrow" not in m.__dict__
    e2 = evaluate_split(m, bags, labels, 2, max_rows_per_call=300)
    for x, y in ((e1.all_probs, e2.all_probs), (e1.all_labels, e2.all_labels), (e1.all_preds, e2.all_preds)):
        assert x.tobytes() == y.tobytes()
    assert e1.error == e2.error and e1.loss == e2.loss and e1.acc == e2.acc
    v1 = validate_split(m, bags, labels, 2, max_rows_per_call=1 << 16)
    assert m.bags_route == "bags" and "bags_narrow" not in m.__dict__
    v2 = validate_split(m, bags, labels, 2, max_rows_per_call=300)
    assert v1.prob.tobytes() == v2.prob.tobytes() and v1.labels.tobytes() == v2.labels.tobytes()
    assert (v1.val_loss, v1.val_error, v1.val_inst_loss, v1.inst_count, v1.acc, v1.inst) == (v2.val_loss, v2.val_error, v2.val_inst_loss, v2.inst_count, v2.acc, v2.inst)
    assert e1.all_probs.tobytes() == v1.prob.tobytes()
    if dtype == "fp32":     # against the loop over forward
        e0 = evaluate_split(m, bags, labels, 2, narrow_one_call=False)
        assert m.bags_route == "per_bag"
        v0 = validate_split(m, bags, labels, 2, narrow_one_call=False)
        assert m.bags_route == "per_bag"
        assert md(e1.all_probs, e0.all_probs) <= TOL and md(v1.prob, v0.prob) <= TOL
        assert e1.acc == e0.acc and v1.acc == v0.acc and v1.inst == v0.inst and v1.inst_count == v0.inst_count
        assert np.array_equal(e1.all_preds, e0.all_preds)


# ---------------------------------------------------------------- the checks every form shares (clam_bags_util), on this form's cases
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(192, 16, 8), (192, 8, 4), (1024, 32, 8)])
def test_a_bag_does_not_see_its_neighbours(size, dtype, monkeypatch):
    U.check_neighbours("narrow", size, 2, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(192, 16, 8), (192, 8, 4)])
def test_attention_only_writes_a_raw_alone(size, dtype):
    U.check_attention_only("narrow", size, 2, dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(192, 8, 4), (192, 16, 8), (512, 32, 8)])
def test_outputs_and_workspace_stay_inside_their_buffers(size, dtype):
    U.check_fences("narrow", size, 2, dtype)
