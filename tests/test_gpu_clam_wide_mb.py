"""GPU tests (-m gpu) of the ragged multi-bag CLAM_MB forward for the wide heads (csrc/abmil_wide_mb.hip,
``hipt_clam_mb_forward_bags_wide``; ``CLAM_MB`` with ``bags_one_call`` and ``bags_wide`` both set).

Weights and bags are made as in tests/test_gpu_clam_wide.py.  The row counts of a call are ``ROWS`` (879 rows, 12 work units): bags of
one and two rows, bags one row short of and one row past the kernel's sub-tiles (32 rows in fp32, 64 in bf16), bags that end before, on
and after a 128-row unit, and a bag of 300 rows = 3 units.  ``CASES``: K = 2 and K = 4 on every shape, K = 3 on (128, 512, 256).

The bars.  Reference: tests/clam_wide_mb_ref.py (fp64; in bf16 mode the bag, W1, Wa, Wb rounded to bf16 and h1 rounded to bf16 for the
gate only).  Per dtype and output, the worst |error| over CASES of the loop of ``forward`` calls on the same bags -- the route these
models took before this kernel -- was measured on one MI355X (MEASURED[dtype][output][1]; [0] is this kernel's figure in the same run);
the bar is twice the loop's figure, the factor covering the different fold order (sub-tile online softmax against the loop's), and in
fp32 never above the project's 1e-4.  SEED was chosen on the host from the fp64 reference alone: of seeds 21..32 the one whose smallest
gap between a bag's two largest reference logits, over CASES, both rounding modes and all bags, is largest (7.4e-2); the host test
tests/test_clam_wide_mb_ref.py holds that gap against 4x the logits bars.  Each test prints its figures before it asserts."""
import ctypes as C

import numpy as np
import pytest
import torch

import clam_bags_util as U
import clam_wide_mb_ref as WM
from clam_bags_util import DEV, FENCE, FILL, OUTS, TOL, assert_same_bits, bits, errors, md, per_bag
from hipt_abmil_atec23_amd import CLAM_MB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd.evaluate import validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 31, 33, 63, 65, 127, 128, 129, 300)
CASES = [((128, 256, 64), 2), ((128, 256, 64), 4), ((128, 512, 256), 2), ((128, 512, 256), 3), ((128, 512, 256), 4),
         ((1024, 512, 384), 2), ((1024, 512, 384), 4)]
INVARIANCE = [((128, 256, 64), 4), ((128, 512, 256), 3), ((1024, 512, 384), 2)]
SEED = 27
# worst |error| per output over CASES against tests/clam_wide_mb_ref.py, measured: (this kernel, the loop of forward calls)
MEASURED = {
    "fp32": {"A_raw": (2.862e-6, 2.977e-6), "M": (2.125e-6, 2.125e-6), "logits": (6.973e-7, 6.675e-7), "Y_prob": (2.014e-7, 1.229e-7)},
    "bf16": {"A_raw": (7.810e-4, 7.811e-4), "M": (1.338e-5, 1.338e-5), "logits": (2.150e-6, 2.082e-6), "Y_prob": (6.494e-7, 6.494e-7)},
}
BARS = {dt: {k: (min(2.0 * v[1], TOL) if dt == "fp32" else 2.0 * v[1]) for k, v in d.items()} for dt, d in MEASURED.items()}


def make(size, dtype="fp32", K=2):
    return U.make(size, dtype, CLAM_MB, K, False)


def bags_of(s0, seed=SEED, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def as_out(ret):
    logits, y_prob, y_hat, a_raw, res = ret
    return {"A_raw": a_raw, "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat, "res": res}


def run_wide(m, bags, **kw):
    """forward_bags with both switches set, on the one-call route"""
    m.bags_one_call = m.bags_wide = True
    try:
        pair = len(bags) == 2 and isinstance(bags[1], Fn.BagOffsets)      # (cat, offsets) instead of a sequence of bags
        ret = m.forward_bags(bags if pair else list(bags), return_features=True, **kw)
        assert m.bags_route == "bags"
    finally:
        del m.bags_one_call, m.bags_wide
    torch.cuda.synchronize()
    return as_out(ret)


def run_loop(m, bags):
    with torch.no_grad():   # (with gradients enabled forward() takes the fp32 training kernels)
        outs = [m(b, return_features=True) for b in bags]
    torch.cuda.synchronize()
    return {"A_raw": [o[3] for o in outs], "M": torch.stack([o[4]["features"] for o in outs]), "logits": torch.cat([o[0] for o in outs]),
            "Y_prob": torch.cat([o[1] for o in outs]), "Y_hat": torch.cat([o[2] for o in outs])}


def direct(w, bags, rows, **kw):
    cat = Fn.as_compute(torch.cat(list(bags), dim=0), w.dtype)
    off = Fn.BagOffsets(np.cumsum([0, *rows]), cat.shape[0], cat.device)
    return Fn.clam_mb_forward_bags_wide(w, cat, off, **kw), cat, off


def a_bits(views):
    """the [K, rows] score matrix of a call, from its per-bag views"""
    return bits(torch.cat(list(views), dim=1))


# ---------------------------------------------------------------- 1. parity against the fp64 reference, and the route
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", CASES)
def test_parity_per_bag(size, K, dtype):
    m = make(size, dtype, K)
    w = m._pack_stacked(torch.device(DEV))
    lib = N.lib()
    assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 0 and lib.hipt_clam_mb_wide_bags_supported(C.byref(w)) == 1
    bags = bags_of(size[0])
    refs = WM.reference(size, SEED, ROWS, K, dtype == "bf16")
    loop, _ = errors(run_loop(m, bags), refs, True)
    before = N.calls
    out = run_wide(m, bags)
    assert N.calls == before + 1, "one native call for the whole set"
    assert out["logits"].shape == (len(ROWS), K) and out["Y_prob"].shape == (len(ROWS), K)
    assert out["Y_hat"].shape == (len(ROWS), 1) and out["Y_hat"].dtype == torch.int64
    assert out["M"].shape == (len(ROWS), K, size[1])
    assert [tuple(a.shape) for a in out["A_raw"]] == [(K, n) for n in ROWS]
    worst, wrong = errors(out, refs, True)
    print(f"wide mb forward_bags {dtype} {size} K={K}: " + ", ".join(f"{k} {worst[k]:.3e} (per-bag loop {loop[k]:.3e})" for k in OUTS))
    gaps = [WM.logit_gap(r) for r in refs]
    print(f"  smallest reference logit gap {min(gaps):.3e}")
    bars = BARS[dtype]
    if dtype == "fp32":
        assert max(bars.values()) <= TOL
    for k in OUTS:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])
    assert min(gaps) > 4.0 * bars["logits"], (min(gaps), bars["logits"])   # every bag's class is decided beyond the logit bar
    assert wrong == []                                                     # no bag left out


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_either_switch_off_keeps_the_loop_and_its_bits(dtype):
    size, K = (128, 512, 256), 2
    m = make(size, dtype, K)
    assert CLAM_MB.bags_one_call is False and CLAM_MB.bags_wide is False
    bags = bags_of(size[0], 13, (1, 129, 300))
    want = run_loop(m, bags)
    for flags in ({}, {"bags_one_call": True}, {"bags_wide": True}):
        for k, v in flags.items():
            setattr(m, k, v)
        try:
            got = as_out(m.forward_bags(list(bags), return_features=True))
            assert m.bags_route == "per_bag", flags
        finally:
            for k in flags:
                delattr(m, k)
        assert a_bits(got["A_raw"]) == a_bits(want["A_raw"]), flags
        for k in ("M", "logits", "Y_prob", "Y_hat"):
            assert got[k].shape == want[k].shape and bits(got[k]) == bits(want[k]), (flags, k)


# ---------------------------------------------------------------- 2. bitwise independence
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", INVARIANCE)
def test_a_bag_does_not_see_its_neighbours(size, K, dtype, monkeypatch):
    m = make(size, dtype, K)
    bags = bags_of(size[0], 9)
    full = run_wide(m, bags)
    rev = run_wide(m, bags[::-1])
    monkeypatch.setenv("HIPT_BAGS_MAX_WG", "3")     # 12 units over 3 workgroups instead of one each
    few = run_wide(m, bags)
    monkeypatch.delenv("HIPT_BAGS_MAX_WG")
    B = len(bags)
    mid = run_wide(m, [bags[(b + 1) % B] for b in range(B)])      # every bag one place earlier: the first goes last
    for b in range(B):
        assert_same_bits(per_bag(full, b, True), per_bag(run_wide(m, [bags[b]]), 0, True), f"bag {b} alone")
        assert_same_bits(per_bag(full, b, True), per_bag(rev, B - 1 - b, True), f"bag {b} reversed order")
        assert_same_bits(per_bag(full, b, True), per_bag(mid, (b - 1) % B, True), f"bag {b} shifted")
        assert_same_bits(per_bag(full, b, True), per_bag(few, b, True), f"bag {b} small grid")


# ---------------------------------------------------------------- 3. the two input forms
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_list_and_concatenated_inputs_agree(dtype):
    size, K = (128, 512, 256), 3
    m = make(size, dtype, K)
    bags = bags_of(size[0], 9)
    full = run_wide(m, bags)
    cat = torch.cat(list(bags), dim=0)
    pair = run_wide(m, (cat, Fn.BagOffsets(np.cumsum([0, *ROWS]), cat.shape[0], cat.device)))
    for b in range(len(bags)):
        assert_same_bits(per_bag(full, b, True), per_bag(pair, b, True), f"bag {b}")


# ---------------------------------------------------------------- 4. attention_only and the buffers' edges
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", [((128, 256, 64), 2), ((128, 512, 256), 4)])
def test_attention_only_writes_a_raw_alone_and_nothing_leaves_its_buffer(size, K, dtype):
    m = make(size, dtype, K)
    bags = bags_of(size[0], 9)
    full = run_wide(m, bags)
    m.bags_one_call = m.bags_wide = True
    try:
        views = m.forward_bags(list(bags), attention_only=True)
        assert m.bags_route == "bags"
    finally:
        del m.bags_one_call, m.bags_wide
    assert [tuple(v.shape) for v in views] == [(K, n) for n in ROWS] and a_bits(views) == a_bits(full["A_raw"])
    w = m._pack_stacked(torch.device(DEV))
    B, total, S1 = len(ROWS), sum(ROWS), size[1]
    need = N.lib().hipt_clam_mb_wide_bags_workspace_bytes(C.byref(w), B, total)
    assert need > 0 and need % 256 == 0
    fenced = []

    def buf(nbytes, dt=torch.uint8):
        raw = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        fenced.append((raw, nbytes))
        return raw[FENCE:FENCE + nbytes].view(dt)

    def fences_hold():
        for raw, n in fenced:
            assert bool((raw[:FENCE] == FILL).all()) and bool((raw[FENCE + n:] == FILL).all()), "a write outside a buffer"

    out = (buf(K * total * 4, torch.float32).view(K, total), buf(B * K * S1 * 4, torch.float32).view(B, K, S1),
           buf(B * K * 4, torch.float32).view(B, K), buf(B * K * 4, torch.float32).view(B, K), buf(B * 8, torch.int64))
    ws = buf(need)
    direct(w, bags, ROWS, attention_only=True, out=out, ws=ws)
    torch.cuda.synchronize()
    fences_hold()
    assert bits(out[0]) == a_bits(full["A_raw"])
    assert all(bool((t.contiguous().view(torch.uint8) == FILL).all()) for t in out[1:]), "attention_only wrote a pooled output"
    direct(w, bags, ROWS, out=out, ws=ws)
    torch.cuda.synchronize()
    fences_hold()
    assert bits(out[0]) == a_bits(full["A_raw"]) and bits(out[1]) == bits(full["M"]) and bits(out[2]) == bits(full["logits"])
    assert bits(out[3]) == bits(full["Y_prob"]) and bits(out[4]) == bits(full["Y_hat"])
    # the workspace carries no state: a second call on the used workspace gives the same bits
    direct(w, bags, ROWS, out=out, ws=ws)
    torch.cuda.synchronize()
    assert bits(out[1]) == bits(full["M"]) and bits(out[0]) == a_bits(full["A_raw"])


# ---------------------------------------------------------------- 5. graph capture
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_one_call_is_captured_and_replayed(dtype):
    size, K = (128, 512, 256), 2
    m = make(size, dtype, K)
    static = torch.cat(bags_of(128, 9), dim=0).clone()
    off = Fn.BagOffsets(np.cumsum([0, *ROWS]), static.shape[0], static.device)   # checked and uploaded BEFORE the capture
    m.bags_one_call = m.bags_wide = True
    try:
        call = lambda: m.forward_bags((static, off), return_features=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                    # weight image, workspace and per-device kernel setup exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                     # one capture on a single stream
            logits, y_prob, y_hat, a_raw, res = call()
        assert m.bags_route == "bags"
    finally:
        del m.bags_one_call, m.bags_wide
    static.copy_(torch.cat(bags_of(128, 31), dim=0))
    g.replay()
    torch.cuda.synchronize()
    got = {"A_raw": torch.cat(a_raw, dim=1), "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}
    eager = run_wide(m, bags_of(128, 31))
    eager["A_raw"] = torch.cat(eager["A_raw"], dim=1)
    assert_same_bits(got, eager, "replay")


# ---------------------------------------------------------------- 6. validation of a split
def test_validate_split_in_one_call_agrees_with_the_loop():
    size, K = (128, 512, 256), 2
    m = make(size, "fp32", K)
    assert m.k_sample == 8
    rows = (20, 45, 64, 65, 100, 127, 128, 129, 200, 256, 257, 300)
    bags = bags_of(128, 23, rows)
    labels = [b % 2 for b in range(len(rows))]
    v1 = validate_split(m, bags, labels, K, wide_one_call=True)
    assert m.bags_route == "bags" and "bags_wide" not in m.__dict__ and "bags_one_call" not in m.__dict__
    v0 = validate_split(m, bags, labels, K, wide_one_call=True, mb_one_call=False)
    assert m.bags_route == "per_bag"
    print(f"validate_split wide mb: prob {md(v1.prob, v0.prob):.3e}, loss {abs(v1.val_loss - v0.val_loss):.3e}, "
          f"instance loss {abs(v1.val_inst_loss - v0.val_inst_loss):.3e} (bar {TOL:.1e})")
    assert md(v1.prob, v0.prob) <= TOL and abs(v1.val_loss - v0.val_loss) <= TOL and abs(v1.val_inst_loss - v0.val_inst_loss) <= TOL
    assert v1.val_error == v0.val_error
    assert v1.acc == v0.acc and v1.inst == v0.inst and v1.inst_count == v0.inst_count
    assert v1.labels.tobytes() == v0.labels.tobytes()
