"""GPU tests (-m gpu) of the validation pass over many bags: the K-branch multi-bag forward (csrc/abmil_bags.hip,
``CLAM_MB.forward_bags`` with ``bags_one_call``), the segmented top-k (csrc/clam_train.hip), the instance branch batched over the bags
of a call and ``evaluate.validate_split``.

Forward tests run on ``ROWS`` (1 787 rows, 18 work units): bag boundaries before, on and after tile boundaries, and a last bag of
1 100 rows = 9 tiles, so that the combine's ``t + 8`` stride adds a second term to its first part.  Instance tests run on ``ROWS_I``
with ``k_sample = 8``: the 8-row bag selects every row twice.

bf16: worst |error| per output against the fp64 restatement (tests/clam_mb_ref.py) on the bf16-rounded bag and bf16-rounded W1 / Wa /
Wb, over the seven bags of ROWS (seed 21, K = 2), measured on an MI355X with ``measure_bf16(route, size)``.  The per-bag path is
``CLAM_MB.forward`` with ``bags_one_call = False`` (code this change does not touch); the bar of the one-call path is TWICE its figure.
  [384,128,64]: per bag (hipt_clam_mb_forward, the one-pass streaming kernel)    A_raw 9.171e-3  M 3.487e-3  logits 4.959e-4  Y_prob 1.059e-4
                forward_bags, one call                                          A_raw 9.172e-3  M 6.420e-4  logits 3.198e-4  Y_prob 8.939e-5
  [192, 64,32]: per bag (hipt_clam_sb_forward per branch, the fused kernel)      A_raw 9.077e-3  M 5.448e-3  logits 1.645e-3  Y_prob 1.666e-4
                forward_bags, one call                                          A_raw 9.077e-3  M 2.004e-3  logits 8.521e-4  Y_prob 7.673e-5
The smallest gap between the reference's two largest logits over the bags is 0.206 at [384,128,64] and 0.125 at [192,64,32], far above
the logit bars, so equality of Y_hat is a statement about the kernels; every Y_hat agrees.  M: both per-bag paths pool a bf16 image
of h1; the one-call path pools fp32 h1 (section 16's POOL32 path).

What the K-branch form shares with the others is stated once in tests/clam_bags_util.py; graph capture, the two input forms and the
default switch run from tests/test_gpu_clam_forms.py (form "mb").
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import clam_bags_util as U
import clam_mb_ref as R
from clam_bags_util import DEV, OUTS, TOL, bits, md
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd import synth
from hipt_abmil_atec23_amd.evaluate import validate_split
from oracle import hipt_oracle as O
from test_clam_validate_host import per_slide_loop

pytestmark = pytest.mark.gpu
ROWS = (1, 127, 128, 129, 300, 2, 1100)
ROWS_I = (8, 9, 127, 128, 129, 300)
SIZES = [(384, 128, 64), (192, 64, 32)]
BF16_SEED = 21
BF16_PER_BAG = {
    (384, 128, 64): {"A_raw": 9.172e-3, "M": 3.488e-3, "logits": 4.959e-4, "Y_prob": 1.059e-4},
    (192, 64, 32): {"A_raw": 9.077e-3, "M": 5.448e-3, "logits": 1.646e-3, "Y_prob": 1.667e-4},
}
INST_SEED = {CLAM_SB: 50, CLAM_MB: 50}   # seeds whose reference top-k gaps exceed GAP (checked on the CPU, asserted below)
GAP = 1e-3           # ten times the A_raw bar


def model_of(size, dtype="fp32", cls=CLAM_MB, n_classes=2, subtyping=False):
    return U.make(size, dtype, cls, n_classes, subtyping)


def params64(size, n_classes=2, multi=True, rounded=False):
    return U.params64(size, n_classes, multi, rounded)


def bags_of(s0, seed, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def reference(size, seed, n_classes=2, rounded=False, rows=ROWS):
    return U.reference(size, seed, rows, rounded, n_classes, True)


per_bag = functools.partial(U.per_bag, multi=True)
errors = functools.partial(U.errors, multi=True)


def run_bags(m, bags, **kw):
    return U.run_form(m, "mb" if m._multi else "sb", bags, **kw)


run_per_bag = U.run_loop     # (forward does not read bags_one_call: the per-bag path needs no switch)


# ---------------------------------------------------------------- 1. fp32 parity
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("K", [2, 3])
def test_fp32_parity_per_bag(size, K):
    m = model_of(size, "fp32", CLAM_MB, K)
    bags = bags_of(size[0], 3)
    run_bags(m, bags[:1])   # the weight image exists
    before = N.calls
    out = run_bags(m, bags)
    assert N.calls == before + 1, "one native call for the whole set"
    B = len(ROWS)
    assert out["logits"].shape == (B, K) and out["Y_hat"].shape == (B, 1) and out["Y_hat"].dtype == torch.int64 and out["M"].shape == (B, K, size[1])
    assert [tuple(a.shape) for a in out["A_raw"]] == [(K, n) for n in ROWS]
    worst, wrong = errors(out, reference(size, 3, K))
    print(f"CLAM_MB forward_bags fp32 {size} K={K}: " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert all(v <= TOL for v in worst.values()), worst
    assert wrong == []


# ---------------------------------------------------------------- 2. bf16 parity
def measure_bf16(route, size):
    m = model_of(size, "bf16")
    bags = bags_of(size[0], BF16_SEED)
    out = run_bags(m, bags) if route == "bags" else run_per_bag(m, bags)
    refs = reference(size, BF16_SEED, 2, True)
    worst, wrong = errors(out, refs)
    return worst, wrong, refs


@pytest.mark.parametrize("size", SIZES)
def test_bf16_parity_per_bag(size):
    worst, wrong, refs = measure_bf16("bags", size)
    gaps = [float(np.diff(np.sort(r["logits"].reshape(-1))[-2:])[0]) for r in refs]
    print(f"CLAM_MB forward_bags bf16 {size}: " + ", ".join(f"{k} {worst[k]:.3e}" for k in OUTS) + f"; smallest top-two logit gap {min(gaps):.3e}")
    bars = {k: 2.0 * v for k, v in BF16_PER_BAG[size].items()}
    for k in OUTS:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])
    # Y_hat where the reference's two largest logits are further apart than the logit bar; at most one bag is left out
    decided = [b for b, gap in enumerate(gaps) if gap > bars["logits"]]
    assert len(decided) >= len(ROWS) - 1, gaps
    assert [b for b in wrong if b in decided] == []


# ---------------------------------------------------------------- 3. a branch is the single-branch call with that branch's weights
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_branch_k_is_the_single_branch_call(size, dtype):
    m = model_of(size, dtype)
    bags = bags_of(size[0], 5)
    out = run_bags(m, bags)
    ws, _ = m._pack_branches(torch.device(DEV))
    a_all = torch.cat(out["A_raw"], dim=1)
    same = True
    for k, w in enumerate(ws):
        (A_raw, M, logits, _, _), _, _ = U.direct("sb", w, bags, ROWS)
        torch.cuda.synchronize()
        d = (md(a_all[k], A_raw.cpu().numpy()), md(out["M"][:, k], M.cpu().numpy()), md(out["logits"][:, k], logits.cpu().numpy()))
        same = same and bits(a_all[k]) == bits(A_raw) and bits(out["M"][:, k]) == bits(M) and bits(out["logits"][:, k]) == bits(logits.reshape(-1))
        assert max(d) <= 1e-5, (k, d)
    print(f"branch consistency {size} {dtype}: bit for bit equal = {same}")


# ---------------------------------------------------------------- 4. the checks every form shares (clam_bags_util), on form "mb"
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_a_bag_does_not_see_its_neighbours(dtype, monkeypatch):
    U.check_neighbours("mb", (384, 128, 64), 2, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("attention_only", [False, True])
def test_outputs_and_workspace_stay_inside_their_buffers(dtype, attention_only):
    (U.check_attention_only if attention_only else U.check_fences)("mb", (384, 128, 64), 2, dtype)


# ---------------------------------------------------------------- 5. segmented top-k
@pytest.mark.parametrize("K", [1, 2])
def test_topk_segments_is_topk_rows_per_bag(K):
    rows, k = (*ROWS_I, 20), 8
    A = synth.hash_uniform_torch((K, sum(rows)), 41 + K, device=DEV).contiguous()
    off = Fn.BagOffsets(np.cumsum([0, *rows]), sum(rows), A.device)
    A[:, off.host[-2]:] = 0.25                       # one row repeated: every score of the last bag is equal
    A[:, off.host[2]:off.host[2] + 5] = A[:, off.host[2] + 9:off.host[2] + 10]   # and a run of ties inside another
    ids, gids = Fn.topk_segments(A if K > 1 else A[0], off, k)
    torch.cuda.synchronize()
    assert ids.shape == (len(rows), K, 2, k) and ids.dtype == torch.int64
    for b, n in enumerate(rows):
        seg = A[:, off.host[b]:off.host[b + 1]].contiguous()
        one = torch.empty((K, 2, k), dtype=torch.int64, device=DEV)
        N.call("hipt_topk_rows", N.ptr(seg), K, n, k, N.ptr(one), N.stream_ptr(seg.device))
        torch.cuda.synchronize()
        assert bits(ids[b]) == bits(one), f"bag {b} ({n} rows)"
        assert bits(gids[b]) == bits(one + off.host[b])
    assert ids[-1, :, 0].tolist() == [list(range(k))] * K and ids[-1, :, 1].tolist() == [list(range(k))] * K   # ties: lowest index first
    assert sorted(ids[0, 0, 0].tolist()) == list(range(8)) and sorted(ids[0, 0, 1].tolist()) == list(range(8))   # the 8-row bag
    with pytest.raises(RuntimeError, match="selected index k out of range"):
        Fn.topk_segments(A, off, 9)


# ---------------------------------------------------------------- 6. the instance branch on the 'bags' route
def inst_labels(cls, n_classes=2):
    return [b % n_classes for b in range(len(ROWS_I))]


@pytest.mark.parametrize("cls", [CLAM_SB, CLAM_MB])
@pytest.mark.parametrize("subtyping", [False, True])
def test_instance_branch_is_the_per_bag_chain(cls, subtyping):
    size, k = (384, 128, 64), 8
    m = model_of(size, "fp32", cls, 2, subtyping)
    bags = bags_of(384, 23, ROWS_I)
    labels = inst_labels(cls)
    run_bags(m, bags[:1])   # the weight image exists
    before = N.calls
    out = run_bags(m, bags, label=labels, instance_eval=True)
    assert N.calls == before + 3, "forward, segmented top-k, gather"
    res = out["res"]
    w = m._pack_stacked(torch.device(DEV)) if cls is CLAM_MB else m._pack(torch.device(DEV))
    Ka = 2 if cls is CLAM_MB else 1
    st = N.stream_ptr(torch.device(DEV))
    cat = torch.cat(bags, dim=0).contiguous()
    off = np.cumsum([0, *ROWS_I])
    for b, bag in enumerate(bags):
        a = out["A_raw"][b].contiguous()
        ids = torch.empty((Ka, 2, k), dtype=torch.int64, device=DEV)
        N.call("hipt_topk_rows", N.ptr(a), Ka, bag.shape[0], k, N.ptr(ids), st)
        rows = torch.empty((Ka, 2, k, size[1]), dtype=torch.float32, device=DEV)
        x = bag.contiguous()
        N.call("hipt_clam_gather_h1", C.byref(w), N.ptr(x), N.ptr(ids), Ka * 2 * k, N.ptr(rows), st)
        grows = torch.empty_like(rows)
        gids = (ids + int(off[b])).contiguous()
        N.call("hipt_clam_gather_h1", C.byref(w), N.ptr(cat), N.ptr(gids), Ka * 2 * k, N.ptr(grows), st)
        torch.cuda.synchronize()
        assert bits(rows) == bits(grows), f"bag {b}: gathered rows"
        with torch.no_grad():
            one = m._instance_branch(lambda r: (rows[r, 0], rows[r, 1]), torch.tensor([labels[b]], device=DEV))
        assert np.array_equal(res["inst_preds"][b], one["inst_preds"]) and np.array_equal(res["inst_labels"][b], one["inst_labels"])
        want = float(one["instance_loss"])
        assert abs(float(res["instance_loss"][b]) - want) <= 1e-6 * abs(want), (b, float(res["instance_loss"][b]), want)


def inst_reference(cls, subtyping, seed):
    """fp64 reference of every bag of ROWS_I and the smallest gap at the k-th / (k+1)-th largest and smallest raw score of any branch."""
    size, k = (384, 128, 64), 8
    multi = cls is CLAM_MB
    p = params64(size, 2, multi)
    refs, gap = [], np.inf
    for bag, l in zip(bags_of(384, seed, ROWS_I), inst_labels(cls)):
        h = bag.double().cpu().numpy()
        if multi:
            r = R.clam_mb_forward(h, p, k, l, True, subtyping)
        else:
            r = O.clam_sb_forward(h, p)
            h1 = np.maximum(O.linear(h, p["attention_net.0.weight"], p["attention_net.0.bias"]), 0)
            r.update(R.instance_branch(O.softmax(r["A_raw"], axis=1), h1, p, l, k, subtyping, False))
        for a in r["A_raw"]:
            if a.shape[0] > k:
                s = np.sort(a)
                gap = min(gap, s[-k] - s[-k - 1], s[k] - s[k - 1])
        refs.append(r)
    return refs, float(gap)


@pytest.mark.parametrize("cls", [CLAM_SB, CLAM_MB])
@pytest.mark.parametrize("subtyping", [False, True])
def test_instance_branch_against_the_reference(cls, subtyping):
    seed = INST_SEED[cls]
    refs, gap = inst_reference(cls, subtyping, seed)
    assert gap > GAP, f"seed {seed}: the reference's own top-k is decided by {gap:.2e} only"
    m = model_of((384, 128, 64), "fp32", cls, 2, subtyping)
    bags = bags_of(384, seed, ROWS_I)
    out = run_bags(m, bags, label=inst_labels(cls), instance_eval=True)
    ids, _ = Fn.topk_segments(torch.cat(out["A_raw"], dim=1).contiguous(), Fn.BagOffsets(np.cumsum([0, *ROWS_I]), sum(ROWS_I), torch.device(DEV)), 8)
    ids = ids.cpu().numpy()
    for b, (r, l) in enumerate(zip(refs, inst_labels(cls))):
        assert md(out["A_raw"][b], r["A_raw"]) <= TOL
        j = 0
        for c in range(2):
            br = c if cls is CLAM_MB else 0
            if l == c:
                got = [set(ids[b, br, 0]), set(ids[b, br, 1])]
                want = [set(r["inst_ids"][j][:8]), set(r["inst_ids"][j][8:])]
            elif subtyping:
                got, want = [set(ids[b, br, 0])], [set(r["inst_ids"][j])]
            else:
                continue
            assert got == want, (b, c)
            j += 1
        assert np.array_equal(out["res"]["inst_labels"][b], r["inst_labels"])
        assert abs(float(out["res"]["instance_loss"][b]) - r["instance_loss"]) <= TOL


# ---------------------------------------------------------------- 7. validate_split on the device
@pytest.mark.parametrize("cls", [CLAM_SB, CLAM_MB])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_validate_split_on_the_device(cls, dtype):
    m = model_of((384, 128, 64), dtype, cls, 2, True)
    bags = bags_of(384, 23, ROWS_I)
    labels = inst_labels(cls)
    a = validate_split(m, bags, labels, 2, max_rows_per_call=1 << 16)
    assert m.bags_route == "bags"
    b = validate_split(m, bags, labels, 2, max_rows_per_call=300)
    for x, y in ((a.prob, b.prob), (a.labels, b.labels)):
        assert x.tobytes() == y.tobytes()
    assert (a.val_loss, a.val_error, a.val_inst_loss, a.inst_count, a.acc, a.inst) == (b.val_loss, b.val_error, b.val_inst_loss, b.inst_count, b.acc, b.inst)
    if dtype == "fp32":
        loop = per_slide_loop(m, bags, labels, 2)
        assert md(a.prob, loop.prob) <= TOL and a.labels.tobytes() == loop.labels.tobytes()
        assert a.acc == loop.acc and a.inst == loop.inst and a.inst_count == loop.inst_count
        assert abs(a.val_loss - loop.val_loss) <= TOL and abs(a.val_inst_loss - loop.val_inst_loss) <= TOL
