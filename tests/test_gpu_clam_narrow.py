"""GPU tests (-m gpu) of the ragged multi-bag CLAM_SB forward for the narrow heads (csrc/abmil_narrow.hip,
``hipt_clam_sb_forward_bags_narrow``, ``CLAM_SB.bags_narrow``).

Weights and bags are made as in tests/test_gpu_clam_bags.py.  The row counts of a call are ``ROWS`` (1 851 rows, 19 work units):
bags of one and two rows, bags one row short of and one row past a 32-row wave block, bags that end before, on and after a 128-row
tile, and a bag of 1 100 rows = 9 tiles, so that the combine's ``t + 8`` stride has a second term."""
import ctypes as C

import numpy as np
import pytest
import torch

import clam_bags_util as U
from clam_bags_util import DEV, FENCE, FILL, OUTS, TOL, assert_same_bits, bits, errors, md, per_bag
from conftest import golden
from hipt_abmil_atec23_amd import CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd import synth
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 31, 33, 127, 128, 129, 300, 1100)
ROWS_I = (8, 31, 33, 127, 128, 129, 300, 1100)      # the instance branch needs k_sample = 8 rows per bag
SHAPES = [(192, 16, 8), (192, 8, 4), (512, 32, 8), (1024, 32, 8)]
SHAPES_BF16 = SHAPES + [(192, 32, 16)]
# bf16: the seed of the bags, chosen on the host from the fp64 reference (bf16-rounded bag, W1, Wa, Wb) alone: of seeds 21..28 the
# one whose smallest gap between a bag's two reference logits, over the five shapes and nine bags, is largest (5.7e-2)
BF16_SEED = 26


def make(size, dtype="fp32", subtyping=False):
    return U.make(size, dtype, CLAM_SB, 2, subtyping)


def bags_of(s0, seed, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def reference(size, seed, rounded=False, rows=ROWS):
    return U.reference(size, seed, rows, rounded)


def run_narrow(m, bags, **kw):
    """forward_bags with the switch set, on the one-call route"""
    m.bags_narrow = True
    try:
        logits, y_prob, y_hat, a_raw, res = m.forward_bags(list(bags), return_features=True, **kw)
        assert m.bags_route == "bags"
    finally:
        del m.bags_narrow
    torch.cuda.synchronize()
    return {"A_raw": a_raw, "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat, "res": res}


def run_loop(m, bags):
    with torch.no_grad():   # (with gradients enabled forward() takes the fp32 training kernels)
        outs = [m(b, return_features=True) for b in bags]
    torch.cuda.synchronize()
    return {"A_raw": [o[3] for o in outs], "M": torch.cat([o[4]["features"] for o in outs]), "logits": torch.cat([o[0] for o in outs]),
            "Y_prob": torch.cat([o[1] for o in outs]), "Y_hat": torch.cat([o[2] for o in outs])}


def direct(w, bags, rows, narrow=True, **kw):
    cat = Fn.as_compute(torch.cat(list(bags), dim=0), w.dtype)
    off = Fn.BagOffsets(np.cumsum([0, *rows]), cat.shape[0], cat.device)
    call = Fn.clam_sb_forward_bags_narrow if narrow else Fn.clam_sb_forward_bags
    return call(w, cat, off, **kw), cat, off


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


# ---------------------------------------------------------------- 4. bitwise independence
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(192, 16, 8), (192, 8, 4), (1024, 32, 8)])
def test_a_bag_does_not_see_its_neighbours(size, dtype, monkeypatch):
    m = make(size, dtype)
    bags = bags_of(size[0], 9)
    full = run_narrow(m, bags)
    rev = run_narrow(m, bags[::-1])
    monkeypatch.setenv("HIPT_BAGS_MAX_WG", "3")     # 19 units over 3 workgroups instead of one each
    few = run_narrow(m, bags)
    monkeypatch.delenv("HIPT_BAGS_MAX_WG")
    B = len(bags)
    for b in range(B):
        assert_same_bits(per_bag(full, b), per_bag(run_narrow(m, [bags[b]]), 0), f"bag {b} alone")
        assert_same_bits(per_bag(full, b), per_bag(rev, B - 1 - b), f"bag {b} reversed order")
        assert_same_bits(per_bag(full, b), per_bag(few, b), f"bag {b} small grid")


# ---------------------------------------------------------------- 5. the width both kernels have
def test_fp32_s1_32_s2_16_agrees_with_the_wide_call():
    size = (192, 32, 16)
    w = make(size)._pack(torch.device(DEV))
    assert N.lib().hipt_clam_bags_supported(C.byref(w)) == 1 and N.lib().hipt_clam_narrow_bags_supported(C.byref(w)) == 1
    bags = bags_of(192, 5)
    a, _, _ = direct(w, bags, ROWS, narrow=True)
    b, _, _ = direct(w, bags, ROWS, narrow=False)
    torch.cuda.synchronize()
    for name, x, y in zip(OUTS, a[:4], b[:4]):
        assert md(x, y.cpu().numpy()) <= 1e-5, (name, md(x, y.cpu().numpy()))
    assert bits(a[4]) == bits(b[4])
    # forward_bags keeps the existing kernel for it, switch or not
    m = make(size)
    out = run_narrow(m, bags)
    assert bits(torch.cat(out["A_raw"], dim=1).reshape(-1)) == bits(b[0]) and bits(out["M"]) == bits(b[1])


# ---------------------------------------------------------------- 6. attention_only
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(192, 16, 8), (192, 8, 4)])
def test_attention_only_writes_a_raw_alone(size, dtype):
    m = make(size, dtype)
    bags = bags_of(size[0], 9)
    full = run_narrow(m, bags)
    m.bags_narrow = True
    try:
        views = m.forward_bags(list(bags), attention_only=True)
        assert m.bags_route == "bags"
    finally:
        del m.bags_narrow
    assert [bits(v) for v in views] == [bits(a) for a in full["A_raw"]]
    w = m._pack(torch.device(DEV))
    B = len(ROWS)
    sent = lambda *shape: torch.full(shape, -7.25, dtype=torch.float32, device=DEV)
    out = (sent(sum(ROWS)), sent(B, size[1]), sent(B, 2), sent(B, 2), torch.full((B,), -7, dtype=torch.int64, device=DEV))
    direct(w, bags, ROWS, attention_only=True, out=out)
    torch.cuda.synchronize()
    assert bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])
    assert all(bool((t == -7.25).all()) for t in out[1:4]) and bool((out[4] == -7).all())


# ---------------------------------------------------------------- 7. guard bytes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", [(192, 8, 4), (192, 16, 8), (512, 32, 8)])
def test_outputs_and_workspace_stay_inside_their_buffers(size, dtype):
    m = make(size, dtype)
    w = m._pack(torch.device(DEV))
    bags = bags_of(size[0], 9)
    B, rows, S1 = len(ROWS), sum(ROWS), size[1]
    need = N.lib().hipt_clam_narrow_bags_workspace_bytes(C.byref(w), B, rows)
    assert need > 0 and need % 256 == 0
    fenced = []

    def buf(nbytes, dt=torch.uint8):
        raw = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        fenced.append((raw, nbytes))
        return raw[FENCE:FENCE + nbytes].view(dt)

    out = (buf(rows * 4, torch.float32), buf(B * S1 * 4, torch.float32).view(B, S1), buf(B * 2 * 4, torch.float32).view(B, 2),
           buf(B * 2 * 4, torch.float32).view(B, 2), buf(B * 8, torch.int64))
    direct(w, bags, ROWS, out=out, ws=buf(need))
    torch.cuda.synchronize()
    for raw, n in fenced:
        assert bool((raw[:FENCE] == FILL).all()) and bool((raw[FENCE + n:] == FILL).all()), "a write outside a buffer"
    full = run_narrow(m, bags)
    assert bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])
    assert bits(out[1]) == bits(full["M"]) and bits(out[2]) == bits(full["logits"]) and bits(out[3]) == bits(full["Y_prob"])
    assert bits(out[4]) == bits(full["Y_hat"])


# ---------------------------------------------------------------- 8. graph capture
def test_one_call_is_captured_and_replayed():
    size = (192, 16, 8)
    m = make(size)
    static = torch.cat(bags_of(192, 9), dim=0).clone()
    off = Fn.BagOffsets(np.cumsum([0, *ROWS]), static.shape[0], static.device)   # checked and uploaded BEFORE the capture
    m.bags_narrow = True
    try:
        call = lambda: m.forward_bags((static, off), return_features=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                    # weight image, workspace and per-device kernel setup exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            logits, y_prob, y_hat, a_raw, res = call()
        assert m.bags_route == "bags"
    finally:
        del m.bags_narrow
    for seed in (31, 32):
        static.copy_(torch.cat(bags_of(192, seed), dim=0))
        g.replay()
        torch.cuda.synchronize()
        got = {"A_raw": torch.cat(a_raw, dim=1), "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}
        eager = run_narrow(m, bags_of(192, seed))
        eager["A_raw"] = torch.cat(eager["A_raw"], dim=1)
        assert_same_bits(got, eager, f"replay on seed {seed}")


# ---------------------------------------------------------------- 9. the instance branch and the split functions
@pytest.mark.parametrize("subtyping", [False, True])
def test_instance_branch_is_the_per_bag_chain(subtyping):
    size, k = (192, 16, 8), 8
    m = make(size, "fp32", subtyping)
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
    m = make((192, 16, 8), dtype, True)
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


# ---------------------------------------------------------------- 10. default behaviour
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_default_forward_bags_still_loops_with_the_bits_of_forward(dtype):
    m = CLAM_SB(size_arg="hipt_smaller")
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs((192, 16, 8)), 192), strict=True)
    m.relocate()
    m.eval().set_compute_dtype(dtype)
    assert m.bags_narrow is False
    bags = bags_of(192, 13, (1, 129, 300))
    logits, y_prob, y_hat, a_raw, res = m.forward_bags(list(bags), return_features=True)
    assert m.bags_route == "per_bag"
    for b, bag in enumerate(bags):
        with torch.no_grad():
            l1, p1, h1, a1, r1 = m(bag, return_features=True)
        assert bits(logits[b:b + 1]) == bits(l1) and bits(y_prob[b:b + 1]) == bits(p1) and bits(y_hat[b:b + 1]) == bits(h1)
        assert bits(a_raw[b]) == bits(a1) and bits(res["features"][b]) == bits(r1["features"].reshape(res["features"][b].shape))
