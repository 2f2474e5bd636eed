"""GPU tests (-m gpu) of the ragged multi-bag CLAM_SB forward (csrc/abmil_bags.hip, ``CLAM_SB.forward_bags``).

The row counts of a call are ``ROWS`` (1 687 rows, 17 work units; the last bag alone is 1 000 rows = 8 tiles): bags of one and two
rows between larger ones, a bag that ends one row short of a 128-row tile, one that fills a tile exactly and one that runs one row
past it, so that bag boundaries fall before, on and after the boundaries a tiling of the concatenated rows would have.  ``B = 1``
runs with 129 rows (a full tile and a one-row tile)."""
import ctypes as C

import numpy as np
import pytest
import torch

import clam_bags_util as U
from clam_bags_util import DEV, FENCE, FILL, OUTS, TOL, assert_same_bits, bits, errors, md, per_bag
from conftest import golden
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
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
    logits, y_prob, y_hat, a_raw, res = m.forward_bags(list(bags), return_features=True)
    assert m.bags_route == "bags"
    torch.cuda.synchronize()
    return {"A_raw": a_raw, "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}


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
    cat = torch.cat(bags, dim=0)
    off = Fn.BagOffsets(np.cumsum([0, *rows]), cat.shape[0], cat.device)
    A_raw, M, logits, Y_prob, Y_hat = Fn.clam_sb_forward_bags(w, cat, off)
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


# ---------------------------------------------------------------- 2. bitwise batch invariance
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_bag_does_not_see_its_neighbours(dtype, monkeypatch):
    size = (384, 128, 64)
    m = make(size, dtype)
    bags = bags_of(384, 9)
    full = run_bags(m, bags)
    rev = run_bags(m, bags[::-1])
    monkeypatch.setenv("HIPT_BAGS_MAX_WG", "3")     # 17 units over 3 workgroups (6 + 6 + 5) instead of one each
    few = run_bags(m, bags)
    monkeypatch.delenv("HIPT_BAGS_MAX_WG")
    B = len(bags)
    for b in range(B):
        assert_same_bits(per_bag(full, b), per_bag(run_bags(m, [bags[b]]), 0), f"bag {b} alone")
        assert_same_bits(per_bag(full, b), per_bag(rev, B - 1 - b), f"bag {b} reversed order")
        assert_same_bits(per_bag(full, b), per_bag(few, b), f"bag {b} small grid")


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
    if route == "bags":
        out = run_bags(m, bags)
    else:
        with torch.no_grad():   # (with gradients enabled forward() takes the fp32 training kernels)
            outs = [m(b, return_features=True) for b in bags]
        out = {"A_raw": [o[3] for o in outs], "M": torch.cat([o[4]["features"] for o in outs]), "logits": torch.cat([o[0] for o in outs]),
               "Y_prob": torch.cat([o[1] for o in outs]), "Y_hat": torch.cat([o[2] for o in outs])}
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


# ---------------------------------------------------------------- 4. attention_only
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_attention_only_writes_a_raw_alone(dtype):
    size = (384, 128, 64)
    m = make(size, dtype)
    bags = bags_of(384, 9)
    full = run_bags(m, bags)
    views = m.forward_bags(list(bags), attention_only=True)
    assert [bits(v) for v in views] == [bits(a) for a in full["A_raw"]]
    w = m._pack(torch.device(DEV))
    cat = Fn.as_compute(torch.cat(bags, dim=0), w.dtype)
    off = Fn.BagOffsets(np.cumsum([0, *ROWS]), cat.shape[0], cat.device)
    B = len(ROWS)
    sent = lambda *shape: torch.full(shape, -7.25, dtype=torch.float32, device=DEV)
    out = (sent(cat.shape[0]), sent(B, 128), sent(B, 2), sent(B, 2), torch.full((B,), -7, dtype=torch.int64, device=DEV))
    Fn.clam_sb_forward_bags(w, cat, off, attention_only=True, out=out)
    torch.cuda.synchronize()
    assert bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])
    assert all(bool((t == -7.25).all()) for t in out[1:4]) and bool((out[4] == -7).all())


# ---------------------------------------------------------------- 5. fallback route
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


# ---------------------------------------------------------------- 6. graph capture
def test_one_call_is_captured_and_replayed():
    """The call is three launches on the capturing stream and nothing else (no copy, no synchronisation, no second stream), so the
    captured graph is a chain; replays on new contents of the same shape equal an eager call bit for bit."""
    size = (384, 128, 64)
    m = make(size)
    static = torch.cat(bags_of(384, 9), dim=0).clone()
    off = Fn.BagOffsets(np.cumsum([0, *ROWS]), static.shape[0], static.device)   # checked and uploaded BEFORE the capture
    call = lambda: m.forward_bags((static, off), return_features=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                        # weight image, workspace and per-device kernel setup exist before the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        logits, y_prob, y_hat, a_raw, res = call()
    for seed in (31, 32):
        fresh = torch.cat(bags_of(384, seed), dim=0)
        static.copy_(fresh)
        g.replay()
        torch.cuda.synchronize()
        got = {"A_raw": torch.cat(a_raw, dim=1), "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}
        eager = run_bags(m, bags_of(384, seed))
        eager["A_raw"] = torch.cat(eager["A_raw"], dim=1)
        assert_same_bits(got, eager, f"replay on seed {seed}")


# ---------------------------------------------------------------- 7. guard bytes
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_outputs_and_workspace_stay_inside_their_buffers(dtype):
    size = (384, 128, 64)
    m = make(size, dtype)
    w = m._pack(torch.device(DEV))
    bags = bags_of(384, 9)
    cat = Fn.as_compute(torch.cat(bags, dim=0), w.dtype)
    off = Fn.BagOffsets(np.cumsum([0, *ROWS]), cat.shape[0], cat.device)
    B, rows = len(ROWS), cat.shape[0]
    need = N.lib().hipt_clam_bags_workspace_bytes(C.byref(w), B, rows)
    assert need > 0 and need % 256 == 0
    fenced = []

    def buf(nbytes, dt=torch.uint8):
        raw = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        fenced.append((raw, nbytes))
        return raw[FENCE:FENCE + nbytes].view(dt)

    out = (buf(rows * 4, torch.float32), buf(B * 128 * 4, torch.float32).view(B, 128), buf(B * 2 * 4, torch.float32).view(B, 2),
           buf(B * 2 * 4, torch.float32).view(B, 2), buf(B * 8, torch.int64))
    Fn.clam_sb_forward_bags(w, cat, off, out=out, ws=buf(need))
    torch.cuda.synchronize()
    for raw, n in fenced:
        assert bool((raw[:FENCE] == FILL).all()) and bool((raw[FENCE + n:] == FILL).all()), "a write outside a buffer"
    full = run_bags(m, bags)
    assert bits(out[0]) == b"".join(bits(a) for a in full["A_raw"])
    assert bits(out[1]) == bits(full["M"]) and bits(out[2]) == bits(full["logits"]) and bits(out[3]) == bits(full["Y_prob"])
    assert bits(out[4]) == bits(full["Y_hat"])
