"""GPU tests (-m gpu) of the ragged multi-bag CLAM_SB forward for the wide heads (csrc/abmil_wide.hip,
``hipt_clam_sb_forward_bags_wide``, ``CLAM_SB.bags_wide``).

Weights and bags are made as in tests/test_gpu_clam_bags.py.  The row counts of a call are ``ROWS`` (1 979 rows, 22 work units):
bags of one and two rows, bags one row short of and one row past the kernel's sub-tiles (32 rows in fp32, 64 in bf16), bags that end
before, on and after a 128-row unit, and a bag of 1 100 rows = 9 units, so that the combine's ``t + 8`` stride has a second term.

The bars.  fp32: the worst |error| against the fp64 oracle over the four shapes and the outputs A_raw, M, logits, Y_prob, measured on
one MI355X, was MEASURED_FP32_NEW for this kernel and MEASURED_FP32_LOOP for the loop of ``forward`` calls on the same bags (the
parent commit's route); FP32_BAR is twice the larger, and stays below the project's fp32 bar of 1e-4.  bf16: the same two
measurements against tests/clam_wide_ref.py (fp64; bag, W1, Wa, Wb rounded to bf16, h1 rounded to bf16 for the gate only), per
output; BF16_BARS is twice the larger per output.  Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import clam_bags_util as U
import clam_wide_ref as WR
from clam_bags_util import DEV, FENCE, FILL, OUTS, TOL, assert_same_bits, bits, errors, md, per_bag
from hipt_abmil_atec23_amd import CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 31, 33, 63, 65, 127, 128, 129, 300, 1100)
ROWS_I = (8, 31, 33, 63, 65, 127, 128, 129, 300, 1100)      # the instance branch needs k_sample = 8 rows per bag
ROWS_PAST = (129, 64, 257)                                  # the call's last bag ends one row past a unit
SHAPES = [(128, 256, 64), (128, 512, 256), (1024, 512, 384), (1024, 512, 256)]
SMALL = [(128, 256, 64), (128, 512, 256)]
# worst |error| over SHAPES and OUTS against the fp64 oracle, fp32 mode (seed 3), measured: (this kernel, the loop of forward calls)
MEASURED_FP32_NEW, MEASURED_FP32_LOOP = 3.338e-6, 3.338e-6      # both at (1024, 512, 384), A_raw; bar 6.676e-6
FP32_BAR = 2.0 * max(MEASURED_FP32_NEW, MEASURED_FP32_LOOP)
# bf16: the seed of the bags, chosen on the host from the fp64 reference of tests/clam_wide_ref.py alone: of seeds 21..28 the one whose
# smallest gap between a bag's two reference logits, over the four shapes and eleven bags, is largest (9.2e-2)
BF16_SEED = 22
# worst |error| per output over SHAPES against tests/clam_wide_ref.py, bf16 mode, measured: (this kernel, the loop of forward calls)
MEASURED_BF16 = {"A_raw": (1.421e-3, 1.421e-3), "M": (1.438e-4, 1.438e-4), "logits": (2.471e-5, 2.467e-5), "Y_prob": (8.918e-6, 8.948e-6)}
BF16_BARS = {k: 2.0 * max(v) for k, v in MEASURED_BF16.items()}


def make(size, dtype="fp32", subtyping=False):
    return U.make(size, dtype, CLAM_SB, 2, subtyping)


def bags_of(s0, seed, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def run_wide(m, bags, **kw):
    """forward_bags with the switch set, on the one-call route"""
    m.bags_wide = True
    try:
        logits, y_prob, y_hat, a_raw, res = m.forward_bags(list(bags), return_features=True, **kw)
        assert m.bags_route == "bags"
    finally:
        del m.bags_wide
    torch.cuda.synchronize()
    return {"A_raw": a_raw, "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat, "res": res}


def run_loop(m, bags):
    with torch.no_grad():   # (with gradients enabled forward() takes the fp32 training kernels)
        outs = [m(b, return_features=True) for b in bags]
    torch.cuda.synchronize()
    return {"A_raw": [o[3] for o in outs], "M": torch.cat([o[4]["features"] for o in outs]), "logits": torch.cat([o[0] for o in outs]),
            "Y_prob": torch.cat([o[1] for o in outs]), "Y_hat": torch.cat([o[2] for o in outs])}


def direct(w, bags, rows, **kw):
    cat = Fn.as_compute(torch.cat(list(bags), dim=0), w.dtype)
    off = Fn.BagOffsets(np.cumsum([0, *rows]), cat.shape[0], cat.device)
    return Fn.clam_sb_forward_bags_wide(w, cat, off, **kw), cat, off


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


# ---------------------------------------------------------------- 3. bitwise independence
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", SMALL + [(1024, 512, 384)])
def test_a_bag_does_not_see_its_neighbours(size, dtype, monkeypatch):
    m = make(size, dtype)
    bags = bags_of(size[0], 9)
    full = run_wide(m, bags)
    rev = run_wide(m, bags[::-1])
    monkeypatch.setenv("HIPT_BAGS_MAX_WG", "3")     # 22 units over 3 workgroups instead of one each
    few = run_wide(m, bags)
    monkeypatch.delenv("HIPT_BAGS_MAX_WG")
    B = len(bags)
    mid = run_wide(m, [bags[(b + 1) % B] for b in range(B)])      # every bag one place earlier: the first goes last
    for b in range(B):
        assert_same_bits(per_bag(full, b), per_bag(run_wide(m, [bags[b]]), 0), f"bag {b} alone")
        assert_same_bits(per_bag(full, b), per_bag(rev, B - 1 - b), f"bag {b} reversed order")
        assert_same_bits(per_bag(full, b), per_bag(mid, (b - 1) % B), f"bag {b} shifted")
        assert_same_bits(per_bag(full, b), per_bag(few, b), f"bag {b} small grid")


# ---------------------------------------------------------------- 4. attention_only
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size", SMALL)
def test_attention_only_writes_a_raw_alone(size, dtype):
    m = make(size, dtype)
    bags = bags_of(size[0], 9)
    full = run_wide(m, bags)
    m.bags_wide = True
    try:
        views = m.forward_bags(list(bags), attention_only=True)
        assert m.bags_route == "bags"
    finally:
        del m.bags_wide
    assert [bits(v) for v in views] == [bits(a) for a in full["A_raw"]]
    w = m._pack(torch.device(DEV))
    B = len(ROWS)
    sent = lambda *shape: torch.full(shape, -7.25, dtype=torch.float32, device=DEV)
    out = (sent(sum(ROWS)), sent(B, size[1]), sent(B, 2), sent(B, 2), torch.full((B,), -7, dtype=torch.int64, device=DEV))
    direct(w, bags, ROWS, attention_only=True, out=out)
    torch.cuda.synchronize()
    assert bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])
    assert all(bool((t == -7.25).all()) for t in out[1:4]) and bool((out[4] == -7).all())


# ---------------------------------------------------------------- 5. guard bytes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,rows", [((128, 256, 64), ROWS), ((128, 512, 256), ROWS), ((128, 512, 384), ROWS_PAST)])
def test_outputs_and_workspace_stay_inside_their_buffers(size, rows, dtype):
    m = make(size, dtype)
    w = m._pack(torch.device(DEV))
    bags = bags_of(size[0], 9, rows)
    B, total, S1 = len(rows), sum(rows), size[1]
    need = N.lib().hipt_clam_wide_bags_workspace_bytes(C.byref(w), B, total)
    assert need > 0 and need % 256 == 0
    fenced = []

    def buf(nbytes, dt=torch.uint8):
        raw = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        fenced.append((raw, nbytes))
        return raw[FENCE:FENCE + nbytes].view(dt)

    out = (buf(total * 4, torch.float32), buf(B * S1 * 4, torch.float32).view(B, S1), buf(B * 2 * 4, torch.float32).view(B, 2),
           buf(B * 2 * 4, torch.float32).view(B, 2), buf(B * 8, torch.int64))
    ws = buf(need)
    direct(w, bags, rows, out=out, ws=ws)
    torch.cuda.synchronize()
    for raw, n in fenced:
        assert bool((raw[:FENCE] == FILL).all()) and bool((raw[FENCE + n:] == FILL).all()), "a write outside a buffer"
    full = run_wide(m, bags)
    assert bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])
    assert bits(out[1]) == bits(full["M"]) and bits(out[2]) == bits(full["logits"]) and bits(out[3]) == bits(full["Y_prob"])
    assert bits(out[4]) == bits(full["Y_hat"])
    # the workspace carries no state: a second call on the used workspace gives the same bits
    direct(w, bags, rows, out=out, ws=ws)
    torch.cuda.synchronize()
    assert bits(out[1]) == bits(full["M"]) and bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])


# ---------------------------------------------------------------- 6. graph capture
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_call_is_captured_and_replayed(dtype):
    size = (128, 512, 256)
    m = make(size, dtype)
    static = torch.cat(bags_of(128, 9), dim=0).clone()
    off = Fn.BagOffsets(np.cumsum([0, *ROWS]), static.shape[0], static.device)   # checked and uploaded BEFORE the capture
    m.bags_wide = True
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
        del m.bags_wide
    for seed in (31, 32):
        static.copy_(torch.cat(bags_of(128, seed), dim=0))
        g.replay()
        torch.cuda.synchronize()
        got = {"A_raw": torch.cat(a_raw, dim=1), "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}
        eager = run_wide(m, bags_of(128, seed))
        eager["A_raw"] = torch.cat(eager["A_raw"], dim=1)
        assert_same_bits(got, eager, f"replay on seed {seed}")


# ---------------------------------------------------------------- 7. the instance branch
@pytest.mark.parametrize("subtyping", [False, True])
def test_instance_branch_is_the_per_bag_chain(subtyping):
    size, k = (128, 256, 64), 8
    m = make(size, "fp32", subtyping)
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


# ---------------------------------------------------------------- 8. the split functions
def test_split_functions_on_the_device():
    m = make((128, 256, 64), "fp32", True)
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


# ---------------------------------------------------------------- 9. default behaviour
def test_default_forward_bags_still_loops_with_the_bits_of_forward():
    m = make((128, 256, 64))
    assert CLAM_SB.bags_wide is False and "bags_wide" not in m.__dict__
    bags = bags_of(128, 13, (1, 129, 300))
    logits, y_prob, y_hat, a_raw, res = m.forward_bags(list(bags), return_features=True)
    assert m.bags_route == "per_bag"
    for b, bag in enumerate(bags):
        with torch.no_grad():
            l1, p1, h1, a1, r1 = m(bag, return_features=True)
        assert bits(logits[b:b + 1]) == bits(l1) and bits(y_prob[b:b + 1]) == bits(p1) and bits(y_hat[b:b + 1]) == bits(h1)
        assert bits(a_raw[b]) == bits(a1) and bits(res["features"][b]) == bits(r1["features"].reshape(res["features"][b].shape))
