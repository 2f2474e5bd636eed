"""CPU side (NumPy) of the per-kernel tests of the CLAM instance branch -- the selection loop `topk_block` of csrc/clam_train.hip behind
hipt_topk_rows, hipt_topk_segments and the in-kernel top-k of hipt_clam_train_forward, and `gather_h1_kernel` of csrc/abmil.hip behind
hipt_clam_gather_h1 -- DESIGN.md 37.  The selection rule as one total order on fp32 values, the references built on it, a float64
reference of the gather with its derived per-element bound, wrong kernels written as references, and the input families.
tests/test_select_ref.py checks all of this without a GPU; tests/test_gpu_select_units.py holds the kernels to it."""
import numpy as np

import ops_ref
from hipt_abmil_atec23_amd import synth

U = ops_ref.U             # 2^-23, DESIGN.md 22
FLUSH = 2.0 ** -126       # the smallest normal fp32: a sum below it may be flushed
THREADS, WAVE = 256, 64   # topk_block: one workgroup of four waves
NAN_KEY = 1 << 31         # above the key of +inf (0x7f800000)
NO_ID = 0x7FFFFFFF        # what an iteration without a candidate leaves in `bi`


# =====================================================================================================================
# The rule
# =====================================================================================================================
def order_key(v, neg_zero_less=False):
    """int64 keys of fp32 values, monotone in the project's order: -inf < finite < +inf < NaN (either sign bit), -0.0 == +0.0.
    neg_zero_less: the raw sign-magnitude order, in which -0.0 sits one below +0.0 (a wrong kernel)"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    bits = v.view(np.int32).astype(np.int64)
    mag = bits & 0x7FFFFFFF
    key = np.where(bits >= 0, mag, -mag - (1 if neg_zero_less else 0))
    return np.where(np.isnan(v), NAN_KEY, key)


def _signed(a, sign):
    return (np.float32(sign) * np.ascontiguousarray(a, dtype=np.float32)).astype(np.float32)


def topk_order(a, k, sign=1.0):
    """the k ids of the rule on one row: key = sign * a descending, NaN above +inf, -0.0 == +0.0, equal keys (and NaNs among
    themselves) lowest index first"""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    assert 0 < k <= a.size
    return np.argsort(-order_key(_signed(a, sign)), kind="stable")[:k].astype(np.int64)


def topk_rows(A, k):
    """hipt_topk_rows: [rows, 2, k], the k largest then the k smallest of every row"""
    A = np.atleast_2d(np.asarray(A, np.float32))
    return np.stack([np.stack([topk_order(r, k, 1.0), topk_order(r, k, -1.0)]) for r in A])


def topk_segments(A, row_stride, offsets, K, k):
    """hipt_topk_segments: (ids, gids) [B, K, 2, k]; branch r of bag b is A.flat[r * row_stride + offsets[b] : ... + offsets[b + 1]].
    -1 everywhere for a bag with fewer than k rows, an empty bag or offsets outside [0, row_stride]"""
    flat = np.asarray(A, np.float32).reshape(-1)
    B = len(offsets) - 1
    ids = np.full((B, K, 2, k), -1, np.int64)
    gids = ids.copy()
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if not (lo >= 0 and hi > lo and hi <= row_stride and hi - lo >= k):
            continue
        for r in range(K):
            seg = flat[r * row_stride + lo:r * row_stride + hi]
            ids[b, r] = np.stack([topk_order(seg, k, 1.0), topk_order(seg, k, -1.0)])
        gids[b] = ids[b] + lo
    return ids, gids


# =====================================================================================================================
# topk_block in NumPy: the 256-thread stride, the wave tree, the four-wave fold -- and its wrong versions
# =====================================================================================================================
TOPK_VARIANTS = ("ties_highest", "nan_ineligible", "bottom_reversed", "neg_zero_less", "stride_shadow", "fold_later_wave")


def emulate_topk(a, k, sign=1.0, variant=None):
    """topk_block as the kernel runs it: k iterations; in each, thread t scans its elements t, t + 256, ... for the best eligible one
    (key descending, index ascending), a xor tree joins the 64 lanes of a wave, thread-uniform code folds the four waves; the winner
    is written and becomes the next iteration's threshold.  variant: one mistake of TOPK_VARIANTS (bottom_reversed is a mistake of
    the caller: variant_topk_rows)."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    N = a.size
    v = _signed(a, sign)
    key = order_key(v, neg_zero_less=variant == "neg_zero_less")
    if variant == "ties_highest":
        return np.lexsort((-np.arange(N), -key))[:k].astype(np.int64)
    usable = ~np.isnan(v) if variant == "nan_ineligible" else np.ones(N, bool)
    NONE = -(1 << 40)
    pad = -N % THREADS
    keyp = np.concatenate([key, np.full(pad, NONE, np.int64)]).reshape(-1, THREADS)      # [element of the thread, thread]
    idxp = np.arange(N + pad, dtype=np.int64).reshape(-1, THREADS)
    usep = np.concatenate([usable, np.zeros(pad, bool)]).reshape(-1, THREADS)
    # today's kernel starts at +inf, so that a NaN is above the first threshold and below nothing
    pk, pi = (order_key(np.float32(np.inf))[()] if variant == "nan_ineligible" else NAN_KEY), -1
    out = np.empty(k, np.int64)
    for it in range(k):
        elig = usep & ((keyp < pk) | ((keyp == pk) & (idxp > pi)))
        kk = np.where(elig, keyp, NONE)
        bk = kk.max(0)                                              # per thread
        hit = elig & (kk == bk)
        if variant == "stride_shadow":                              # `>=`: the later element of a thread replaces an equal one
            bi = np.where(hit, idxp, -1).max(0)
        else:
            bi = np.where(hit, idxp, NO_ID).min(0)
        bi = np.where(bk == NONE, NO_ID, bi)
        wk, wi = bk.reshape(4, WAVE), bi.reshape(4, WAVE)           # the tree is symmetric: best key, lowest index
        rk = wk.max(1)
        ri = np.where(wk == rk[:, None], wi, NO_ID).min(1)
        fk, fi = rk[0], ri[0]
        for q in range(1, 4):
            if rk[q] > fk or (rk[q] == fk and (ri[q] < fi or variant == "fold_later_wave")):   # (`>=`: the later wave wins a tie)
                fk, fi = rk[q], ri[q]
        out[it] = fi
        pk, pi = fk, fi
        if fk == NONE:                                              # bv = -inf, bi = NO_ID: nothing is eligible from here on
            out[it:] = NO_ID
            break
    return out


def structure_trigger(variant, a, k, sign):
    """whether the row holds what stride_shadow / fold_later_wave get wrong, read off the rule alone: walking the rule's list, a winner w
    for which another not yet selected element of the same key sits in w's thread (the thread then offers the later one and w is never
    offered) / in a later wave than w's (the fold ends on the last wave that holds the key).  Until the first such winner both run alike."""
    a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
    key, idx = order_key(_signed(a, sign)), np.arange(a.size)
    left = np.ones(a.size, bool)
    for w in topk_order(a, k, sign):
        left[w] = False
        same = left & (key == key[w])
        if variant == "stride_shadow" and (same & (idx % THREADS == w % THREADS)).any():
            return True
        if variant == "fold_later_wave" and (same & ((idx % THREADS) // WAVE > (w % THREADS) // WAVE)).any():
            return True
    return False


def variant_topk_rows(name, A, k):
    """hipt_topk_rows with one mistake -> [rows, 2, k]"""
    A = np.atleast_2d(np.asarray(A, np.float32))
    if name == "bottom_reversed":   # one descending order of the row, its tail read backwards
        full = [topk_order(r, r.size, 1.0) for r in A]
        return np.stack([np.stack([f[:k], f[::-1][:k]]) for f in full])
    return np.stack([np.stack([emulate_topk(r, k, 1.0, name), emulate_topk(r, k, -1.0, name)]) for r in A])


SEG_VARIANTS = ("branch_at_rows", "gids_without_lo")


def variant_topk_segments(name, A, row_stride, offsets, K, k):
    """hipt_topk_segments with one mistake; branch_at_rows: branch r read at r * rows (rows = offsets[-1]) instead of r * row_stride"""
    if name == "branch_at_rows":
        flat = np.asarray(A, np.float32).reshape(-1)
        rows = int(offsets[-1])
        moved = np.concatenate([flat[r * rows:r * rows + rows] for r in range(K)])
        return topk_segments(moved, rows, offsets, K, k)
    if name == "gids_without_lo":
        ids, _ = topk_segments(A, row_stride, offsets, K, k)
        return ids, ids.copy()
    raise KeyError(name)


# =====================================================================================================================
# Families of score rows
# =====================================================================================================================
# (i, j) of a tie pair at row length N: the same thread one stride apart; the same lane of two neighbouring waves, the earlier index in the
# earlier wave; the two ends of the tree's first step (lanes l, l ^ 32 of one wave); neighbours; the row's ends
PAIRS = {"pair256": lambda N: (N - 257, N - 1), "pair64": lambda N: ((N // 5) % 192, (N // 5) % 192 + 64),
         "pairx32": lambda N: tuple(sorted((37 % N, (37 % N) ^ 32))), "pair1": lambda N: (N // 2 - 1, N // 2), "pair_ends": lambda N: (0, N - 1)}
FAMILIES = ("distinct", "all_equal", "two_valued", *(p + s for p in PAIRS for s in ("+", "-")), "straddle_top", "straddle_bottom", "zeros",
            "inf_once", "inf_many", "nan_one", "nan_few", "nan_all")
TIE_FAMILIES = ("all_equal", "two_valued", *(p + s for p in PAIRS for s in ("+", "-")), "straddle_top", "straddle_bottom")
NEG_NAN = np.array([0xFFC00001], np.uint32).view(np.float32)[0]   # a NaN with the sign bit set and a payload
POS_NAN = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def distinct_row(N, seed):
    """hashed uniform values in (-1, 1), made distinct: a repeated value is replaced by one from a disjoint range"""
    a = synth.hash_uniform_np((N,), seed, 1.0)
    _, first = np.unique(a, return_index=True)
    dup = np.setdiff1d(np.arange(N), first)
    a[dup] = np.float32(2.0) + np.arange(len(dup), dtype=np.float32) * np.float32(2.0 ** -10)
    assert len(np.unique(a)) == N
    return a


def applies(family, N, k):
    """whether the family exists at this row length and k"""
    base = family.rstrip("+-")
    if base in PAIRS:
        i, j = PAIRS[base](N)
        return 0 <= i < j < N
    if family in ("straddle_top", "straddle_bottom"):
        return k < N
    if family == "two_valued":
        return N >= 2
    if family in ("inf_once", "zeros"):
        return N >= 2
    if family == "inf_many":
        return N >= 6
    return True


def family_row(family, N, k, seed):
    """one fp32 row of the family (see FAMILIES); applies(family, N, k) must hold"""
    assert applies(family, N, k), (family, N, k)
    a = distinct_row(N, seed)
    h = synth.hash_u32_np(N, seed + 1000)
    base = family.rstrip("+-")
    if family == "distinct":
        return a
    if family == "all_equal":
        return np.full(N, np.float32(0.25))
    if family == "two_valued":      # every other hashed entry, at least one of each, is the maximum
        hi = (h >> np.uint32(7)) % np.uint32(2) == 0
        hi[0], hi[N - 1] = True, False
        return np.where(hi, np.float32(0.75), np.float32(-0.5)).astype(np.float32)
    if base in PAIRS:               # the pair is the largest value ("+") or the smallest ("-")
        i, j = PAIRS[base](N)
        a[i] = a[j] = np.float32(3.0)
        return a if family.endswith("+") else -a
    if family in ("straddle_top", "straddle_bottom"):   # ranks k and k + 1 hold one value; the later index copies the earlier
        order = topk_order(a, N, 1.0 if family == "straddle_top" else -1.0)
        i, j = sorted((order[k - 1], order[k]))
        a[j] = a[i]
        return a
    if family == "zeros":           # +-0 by a hashed bit, and about k / 2 small numbers of either sign (denormals, the smallest normals):
        a = np.where((h >> np.uint32(9)) % np.uint32(2) == 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)   # both lists run into the zeros
        m = min(k // 2, (N - 2) // 2)
        where = np.argsort(h[1:N - 1], kind="stable")[:2 * m] + 1
        small = (np.arange(m, dtype=np.float64) + 1) * 2.0 ** -149
        small[1::2] += 2.0 ** -126
        a[where[:m]], a[where[m:]] = small.astype(np.float32), (-small).astype(np.float32)
        a[0], a[N - 1] = np.float32(-0.0), np.float32(0.0)
        return a
    if family == "inf_once":
        a[(N - 1) // 2], a[N - 1] = np.float32(np.inf), np.float32(-np.inf)
        return a
    if family == "inf_many":
        a[h % np.uint32(5) == 0] = np.float32(np.inf)
        a[h % np.uint32(5) == 1] = np.float32(-np.inf)
        a[0], a[1], a[N - 2], a[N - 1] = np.float32(-np.inf), np.float32(np.inf), np.float32(np.inf), np.float32(-np.inf)
        return a
    if family in ("nan_one", "nan_few", "nan_all"):    # both sign bits; nan_few leaves k - 1 numbers, nan_all none
        count = {"nan_one": 1, "nan_few": N - k + 1, "nan_all": N}[family]
        where = np.argsort(h, kind="stable")[:count]
        a[where] = np.where(np.arange(count) % 2 == 0, NEG_NAN, POS_NAN)
        return a
    raise KeyError(family)


def family_rows(family, rows, N, k, seed):
    return np.stack([family_row(family, N, k, seed + 17 * r) for r in range(rows)])


def has_ties(a, k):
    """whether either selected list of the row, or its boundary, holds two equal keys"""
    for sign in (1.0, -1.0):
        key = order_key(_signed(a, sign))
        top = np.sort(key)[::-1][:min(k + 1, a.size)]
        if (np.diff(top) == 0).any():
            return True
    return False


TOPK_N = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)


def topk_ks(N):
    return sorted({k for k in (1, 8, min(N, 64), N if N <= 257 else 1) if k <= N})


# =====================================================================================================================
# gather_h1
# =====================================================================================================================
def gather_h1(bag, w1, b1, idx):
    """ReLU(bag[idx] W1^T + b1) in float64 on the operands as the kernel reads them (fp32, or bf16-rounded values widened), and the
    bound of one serial fp32 chain a = b1; a += x_k w_k of S0 terms, fused or not, then ReLU (1-Lipschitz):
    |d| <= (S0 + 2) u (|b1| + sum_k |x_k w_k|) + 2^-126 -> (result, bound), [n_idx, S1] each"""
    x = np.asarray(bag, np.float64)[np.asarray(idx, np.int64)]
    w, b = np.asarray(w1, np.float64), np.asarray(b1, np.float64)
    S0 = w.shape[1]
    y = np.maximum(x @ w.T + b, 0.0)
    bound = (S0 + 2) * U * (np.abs(b) + np.abs(x) @ np.abs(w).T) + FLUSH
    return y, bound


def gather_condition(bag, w1, b1, idx):
    """S / |pre-activation| per element, and the pre-activation"""
    x = np.asarray(bag, np.float64)[np.asarray(idx, np.int64)]
    w, b = np.asarray(w1, np.float64), np.asarray(b1, np.float64)
    z = x @ w.T + b
    return (np.abs(b) + np.abs(x) @ np.abs(w).T) / np.abs(z), z


GATHER_VARIANTS = ("no_bias", "last_term", "next_row", "no_relu", "w1_stride_s1")


def gather_variant(name, bag_ext, w1, b1, idx):
    """a wrong gather in float64; bag_ext: the bag with the row that follows it in memory (next_row reads bag[idx + 1])"""
    idx = np.asarray(idx, np.int64)
    x = np.asarray(bag_ext, np.float64)
    w, b = np.asarray(w1, np.float64), np.asarray(b1, np.float64)
    S1, S0 = w.shape
    if name == "no_bias":
        return np.maximum(x[idx] @ w.T, 0.0)
    if name == "last_term":
        return np.maximum(x[idx, :S0 - 1] @ w[:, :S0 - 1].T + b, 0.0)
    if name == "next_row":
        return np.maximum(x[idx + 1] @ w.T + b, 0.0)
    if name == "no_relu":
        return x[idx] @ w.T + b
    if name == "w1_stride_s1":
        flat = w.reshape(-1)
        w2 = np.stack([flat[c * S1:c * S1 + S0] for c in range(S1)])
        return np.maximum(x[idx] @ w2.T + b, 0.0)
    raise KeyError(name)


# the heads the project ships (model_clam.SIZE_DICT): (S0, S1); S1 = 128: a partial round of the kernel's c += 256 loop, 256: one full
# round, 512: two; 8 / 16 / 32: the narrow heads of functional._BAGS_FORMS
GATHER_HEADS = ((384, 128), (192, 128), (1024, 512), (1024, 256), (192, 16), (192, 8), (1024, 32))
GATHER_N = (1, 2, 257)
GATHER_NIDX = (1, 16, 40)


def gather_inputs(N, S0, S1, seed, bf16):
    """bag [N + 1, S0] (the last row is what follows the bag in memory), W1 [S1, S0], b1 [S1], mask [N] of the cancelling rows: the
    construction of ops_ref.linear_inputs -- rows 0, 5, 10, ... and N - 2 are 65536 (z, -(1 - 2^-12) rot z) against a W1 whose second
    half repeats the first rotated, so that the sum cancels to 2^-12 of its terms; biases U(-0.5, 0.5), pre-activations of either sign"""
    a, w, bias, _, cancel = ops_ref.linear_inputs(N, S1, S0, seed, bf16)
    return a, w, bias, cancel


def gather_idx(N, n_idx, seed):
    """n_idx row ids: hashed (unsorted, with repeats once n_idx > N), row N - 1 first, and for n_idx > 1 a repeat of it second and row 0 last"""
    idx = (synth.hash_u32_np(n_idx, seed + 77) % np.uint32(N)).astype(np.int64)
    idx[0] = N - 1
    if n_idx > 1:
        idx[1], idx[-1] = N - 1, 0
    return idx
