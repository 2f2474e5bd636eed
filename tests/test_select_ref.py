"""Host tests (no GPU) of tests/select_ref.py, DESIGN.md 37: the selection rule pinned to torch.topk on the CPU where torch is
determined, the NumPy restatement of topk_block against the rule, every wrong kernel caught on the family built for it and on no
family that lacks its trigger, the families' own claims, and the gather's reference, bound and wrong kernels."""
import numpy as np
import pytest
import torch

import select_ref as S

HOST_N, HOST_K = 600, 8     # every pair family exists, three elements per thread for some threads, k << N
SHAPES = ((HOST_N, HOST_K), (65, 8), (257, 64), (8, 8), (513, 1))


def _torch_ids(a, k, sign):
    return torch.topk(torch.from_numpy(S._signed(a, sign)), k)[1].numpy()


def test_the_issue_example():
    a = np.array([1, np.nan, 3, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    assert S.topk_order(a, 4, 1.0).tolist() == [1, 5, 3, 2]
    assert S.topk_order(a, 4, -1.0).tolist() == [1, 5, 4, 6]
    assert set(_torch_ids(a, 4, 1.0)) == {1, 5, 3, 2} and set(_torch_ids(a, 4, -1.0)[:3]) == {1, 5, 4} and _torch_ids(a, 4, -1.0)[3] in (6, 7)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_rule_is_torch_topk_where_torch_is_determined(family):
    for N, k in SHAPES:
        if not S.applies(family, N, k):
            continue
        for seed in (1, 2):
            a = S.family_row(family, N, k, seed)
            for sign in (1.0, -1.0):
                ref, got = S.topk_order(a, k, sign), _torch_ids(a, k, sign)
                key = S.order_key(S._signed(a, sign))
                assert np.array_equal(key[ref], key[got]), (family, N, k, sign)          # values at equal rank
                assert len(set(ref.tolist())) == k and ref.min() >= 0 and ref.max() < N
                nn = min(int(np.isnan(a).sum()), k)
                assert np.isnan(a[ref[:nn]]).all() and np.isnan(a[got[:nn]]).all()         # NaN leads both lists, here and in torch
                full = np.sort(key)[::-1]
                if k == N or full[k - 1] != full[k]:                                        # no tie across the boundary: one set
                    assert set(ref.tolist()) == set(got.tolist()), (family, N, k, sign)
                if family in ("distinct", "inf_once"):
                    assert np.array_equal(ref, got), (family, N, k, sign)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_emulated_topk_block_is_the_rule(family):
    """the kernel's structure in NumPy -- stride, tree, fold -- gives the rule at every edge length of the GPU tests"""
    for N in S.TOPK_N:
        for k in S.topk_ks(N):
            if S.applies(family, N, k):
                a = S.family_row(family, N, k, 3)
                for sign in (1.0, -1.0):
                    assert np.array_equal(S.emulate_topk(a, k, sign), S.topk_order(a, k, sign)), (family, N, k, sign)


def test_families_hold_what_they_claim():
    for N in S.TOPK_N:
        for k in S.topk_ks(N):
            for f in S.FAMILIES:
                if not S.applies(f, N, k):
                    continue
                a = S.family_row(f, N, k, 5)
                assert a.dtype == np.float32 and a.shape == (N,)
                base = f.rstrip("+-")
                if base in S.PAIRS:
                    i, j = S.PAIRS[base](N)
                    assert a[i] == a[j] and (a[i] == a.max() if f.endswith("+") else a[i] == a.min()) and (a == a[i]).sum() == 2
                if f == "all_equal":
                    assert (a == a[0]).all()
                if f == "two_valued":
                    assert len(np.unique(a)) == 2 and abs(int((a == a.max()).sum()) - N / 2) <= max(1, N // 4)
                if f in ("straddle_top", "straddle_bottom"):     # equal values at ranks k and k + 1, and nowhere else
                    o = S.topk_order(a, N, 1.0 if f == "straddle_top" else -1.0)
                    assert a[o[k - 1]] == a[o[k]] and len(np.unique(a)) == N - 1
                if f in S.TIE_FAMILIES and N >= 2 and not (f == "two_valued" and N == 2):
                    assert S.has_ties(a, k), (f, N, k)
                if f in ("distinct", "inf_once", "nan_one"):
                    assert not S.has_ties(a, k)
                if f == "zeros":
                    sb = np.signbit(a[a == 0])
                    assert sb.any() and (~sb).any() and (k < 2 or N < 4 or ((a > 0).any() and (a < 0).any())) and (a > 0).sum() < k
                if f == "inf_once":
                    assert np.isposinf(a).sum() == 1 and np.isneginf(a).sum() == 1
                if f == "inf_many":
                    assert np.isposinf(a).sum() >= 2 and np.isneginf(a).sum() >= 2
                if f.startswith("nan"):
                    nn = int(np.isnan(a).sum())
                    assert nn == {"nan_one": 1, "nan_few": N - k + 1, "nan_all": N}[f] and (f == "nan_one" or N - nn < k)
                    assert nn < 2 or (np.signbit(a[np.isnan(a)]).any() and (~np.signbit(a[np.isnan(a)])).any())
    i, j = S.PAIRS["pair256"](HOST_N)
    assert j - i == 256
    for N in (255, 512, 1025, HOST_N):        # the same lane of neighbouring waves, the earlier index in the earlier wave
        i, j = S.PAIRS["pair64"](N)
        assert j - i == 64 and (i % 256) // 64 + 1 == (j % 256) // 64 and i % 64 == j % 64
    i, j = S.PAIRS["pairx32"](HOST_N)
    assert i ^ 32 == j and i // 64 == j // 64


# variant -> the families on which it must differ from the rule, the first being the one built for it; on every other family it must
# agree.  The two structural mistakes are decided per row by select_ref.structure_trigger, which reads the trigger off the rule alone,
# so that the families with hashed positions are asserted as well; their lists name the families that hold the trigger by construction.
ALL_TIED = ("all_equal", "nan_all")
CATCHES = {
    "ties_highest": S.TIE_FAMILIES + ("zeros", "inf_many", "nan_few", "nan_all"),
    "nan_ineligible": ("nan_few", "nan_one", "nan_all"),
    "bottom_reversed": ("pair1-", "pair256-", "pair64-", "pairx32-", "pair_ends-", "straddle_bottom", "all_equal", "two_valued", "zeros", "inf_many",
                        "nan_one", "nan_few", "nan_all"),
    "neg_zero_less": ("zeros",),
    "stride_shadow": ("pair256+", "pair256-") + ALL_TIED,
    "fold_later_wave": ("pair64+", "pair64-", "pair_ends+", "pair_ends-") + ALL_TIED,
}
STRUCTURAL = ("stride_shadow", "fold_later_wave")
NEVER = ("distinct", "inf_once", "nan_one")     # no two equal keys: no structural mistake can show


@pytest.mark.parametrize("variant", S.TOPK_VARIANTS)
def test_wrong_topk_kernels_are_caught_on_their_families_only(variant):
    must = CATCHES[variant]
    assert set(must) <= set(S.FAMILIES)
    caught = []
    for f in S.FAMILIES:
        A = S.family_rows(f, 2, HOST_N, HOST_K, 11)
        ref, got = S.topk_rows(A, HOST_K), S.variant_topk_rows(variant, A, HOST_K)
        differs = not np.array_equal(ref, got)
        caught += [f] * differs
        if variant in STRUCTURAL:
            for r, row in enumerate(A):
                for s, sign in enumerate((1.0, -1.0)):
                    assert (not np.array_equal(ref[r, s], got[r, s])) == S.structure_trigger(variant, row, HOST_K, sign), (variant, f, r, sign)
            assert differs or f not in must, (variant, f)
            assert not (differs and f in NEVER), (variant, f)
        else:
            assert differs == (f in must), (variant, f)
    if variant == "stride_shadow":      # of the five pairs only the one a stride apart
        assert not {"pair64+", "pair64-", "pairx32+", "pairx32-", "pair1+", "pair1-", "pair_ends+", "pair_ends-"} & set(caught)
    if variant == "fold_later_wave":    # only the pairs in two waves
        assert not {"pair256+", "pair256-", "pairx32+", "pairx32-", "pair1+", "pair1-"} & set(caught)
    print(f"\n{variant}: differs on {caught}")
    if variant == "nan_ineligible":   # today's kernel: an id outside [0, N) -- what the GPU test's range assertion sees
        got = S.variant_topk_rows(variant, S.family_rows("nan_few", 1, HOST_N, HOST_K, 11), HOST_K)
        assert got.max() == S.NO_ID and got.max() >= HOST_N
        got = S.variant_topk_rows(variant, S.family_rows("nan_one", 1, HOST_N, HOST_K, 11), HOST_K)
        assert 0 <= got.min() and got.max() < HOST_N   # enough numbers left: wrong ids, all in range


SEG_ROWS = (1, 8, 7, 257, 64, 0, 300)


def seg_scores(K, row_stride, seed=31):
    rows = sum(SEG_ROWS)
    A = np.full((K, row_stride), np.nan, np.float32)
    A[:, :rows] = np.stack([S.distinct_row(rows, seed + r) for r in range(K)])
    return A, np.cumsum([0, *SEG_ROWS])


def test_segments_reference_and_its_wrong_kernels():
    rows = sum(SEG_ROWS)
    for K in (1, 2):
        for stride in (rows, rows + 13):
            A, off = seg_scores(K, stride)
            ids, gids = S.topk_segments(A, stride, off, K, 8)
            for b, n in enumerate(SEG_ROWS):
                if n < 8:
                    assert (ids[b] == -1).all() and (gids[b] == -1).all()
                else:
                    for r in range(K):
                        assert np.array_equal(ids[b, r], S.topk_rows(A[r, off[b]:off[b + 1]], 8)[0])
                    assert np.array_equal(gids[b], ids[b] + off[b])
            v = S.variant_topk_segments("branch_at_rows", A, stride, off, K, 8)
            assert (not np.array_equal(v[0], ids)) == (K > 1 and stride > rows), (K, stride)
            v = S.variant_topk_segments("gids_without_lo", A, stride, off, K, 8)
            assert np.array_equal(v[0], ids) and not np.array_equal(v[1], gids)
    one = np.array([0, 300])           # a single bag at row 0: the only place where gids without + lo are right
    A = S.distinct_row(300, 3)[None]
    assert np.array_equal(*S.variant_topk_segments("gids_without_lo", A, 300, one, 1, 8))
    bad = S.topk_segments(A, 300, np.array([-8, 0, 8, 400]), 1, 8)[0]     # offsets outside [0, row_stride]
    assert (bad[0] == -1).all() and (bad[1] >= 0).all() and (bad[2] == -1).all()


# ---------------------------------------------------------------- gather_h1
def emulate_gather(bag, w1, b1, idx, fused):
    """the kernel's chain in fp32: a = b1; a += x_k w_k, the product rounded on its own or inside an fma"""
    x = np.asarray(bag, np.float32)[idx]
    a = np.broadcast_to(np.asarray(b1, np.float32), (len(idx), w1.shape[0])).copy()
    for k in range(w1.shape[1]):
        p = x[:, k:k + 1].astype(np.float64) * w1[None, :, k].astype(np.float64)
        a = (a.astype(np.float64) + p).astype(np.float32) if fused else (a + p.astype(np.float32)).astype(np.float32)
    return np.maximum(a, np.float32(0)).astype(np.float64)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("head", S.GATHER_HEADS, ids=lambda h: f"{h[0]}x{h[1]}")
def test_gather_reference_bound_and_wrong_kernels(head, bf16):
    S0, S1 = head
    N, n_idx = 257, 40
    bag, w1, b1, cancel = S.gather_inputs(N, S0, S1, 40 + S1, bf16)
    idx = S.gather_idx(N, n_idx, 1)
    assert idx[0] == N - 1 and idx[-1] == 0 and idx[1] == idx[0] and (np.diff(idx) < 0).any() and idx.max() < N
    if bf16:
        assert np.array_equal(S.ops_ref.bf16_round(bag), bag) and np.array_equal(S.ops_ref.bf16_round(w1), w1)
    ref, bound = S.gather_h1(bag[:N], w1, b1, idx)
    cond, z = S.gather_condition(bag[:N], w1, b1, idx)
    sel_cancel = cancel[idx]
    assert sel_cancel.any() and (~sel_cancel).any()
    # cancelling rows: S / |y| >= 1e3 on at least half the columns of every such row (a column whose bias happens to dominate the residue
    # may fall below), and on the row's median
    assert ((cond[sel_cancel] >= 1e3).mean(axis=1) >= 0.5).all() and (np.median(cond[sel_cancel], axis=1) >= 1e3).all(), np.median(cond[sel_cancel], axis=1)
    assert ((z < 0).mean(axis=1) >= 0.25).sum() >= n_idx // 2                                            # a missing ReLU shows
    for fused in (False, True):
        r = S.ops_ref.ratio(emulate_gather(bag[:N], w1, b1, idx, fused), ref, bound)
        assert r.max() <= 1.0, (head, bf16, fused, r.max())
    worst = {}
    for name in S.GATHER_VARIANTS:
        r = S.ops_ref.ratio(S.gather_variant(name, bag, w1, b1, idx), ref, bound)
        worst[name] = float(r.max())
        assert r.max() >= 3.0, (name, head, bf16, r.max())
    print(f"\ngather {S0}x{S1} {'bf16' if bf16 else 'fp32'}: wrong kernels, worst |err| / bound " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


def test_gather_idx_edges():
    for N in S.GATHER_N:
        for n in S.GATHER_NIDX:
            idx = S.gather_idx(N, n, 2)
            assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < N and idx[0] == N - 1 and (n == 1 or (idx[-1] == 0 and idx[1] == N - 1))
