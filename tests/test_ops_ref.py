"""Host tests of tests/ops_ref.py: the float64 references against torch, the NumPy emulation of each right kernel inside
its derived bound on every launch shape, every wrong kernel at least 3 x beyond it on the class it corrupts, and the input families'
own assertions.  No GPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ops_ref as R

EPS = 1e-6
CATCH = 3.0


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---------------------------------------------------------------------------------------------------------------------
# references against torch in float64
# ---------------------------------------------------------------------------------------------------------------------
def test_references_agree_with_torch_float64():
    x, w, b, _ = R.ln_inputs(9, 192, 3)
    t = lambda v: torch.from_numpy(np.asarray(v, np.float64))
    assert _rel(R.layernorm_ref(x, w, b, EPS), F.layer_norm(t(x), (192,), t(w), t(b), EPS).numpy()) < 1e-12
    a, wl, bias, r, _ = R.linear_inputs(21, 36, 96, 5, False, gelu=True, resid=True)
    a = a[:21]
    h = F.linear(t(a), t(wl), t(bias))
    assert _rel(R.linear_ref(a, wl, bias), h.numpy()) < 1e-12
    assert _rel(R.linear_ref(a, wl, bias, r, "gelu"), (F.gelu(h) + t(r)).numpy()) < 1e-12
    assert _rel(R.linear_ref(a, wl, bias, None, "relu"), F.relu(h).numpy()) < 1e-12
    for fam in ("ordinary", "spike_last"):
        qkv, _ = R.attn_inputs(2, 33, 3, 32, 7, fam, False)
        o, p = R.attention_ref(qkv, 3, 32 ** -0.5)
        q, k, v = (t(np.ascontiguousarray(z)) for z in R._split(qkv, 3))
        ot = F.scaled_dot_product_attention(q, k, v, scale=32 ** -0.5).permute(0, 2, 1, 3).reshape(2, 33, 96).numpy()
        pt = torch.softmax(q @ k.transpose(-1, -2) * 32 ** -0.5, -1).numpy()
        assert _rel(o, ot) < 1e-12 and _rel(p, pt) < 1e-12


def test_bf16_round_is_round_to_nearest_even():
    x = np.concatenate([np.float32(np.random.default_rng(0).standard_normal(4096) * 100), np.float32([1.00390625, 1.01171875, 0, -0.0])])
    assert np.array_equal(R.bf16_round(x), torch.from_numpy(x).bfloat16().float().numpy())


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def test_layernorm_families_reach_their_edges():
    x, w, b, cls = R.ln_inputs(257, 384, 11)
    kap = R.layernorm_kappa(x, EPS)
    assert kap[cls == 1].min() >= 100 and kap[cls == 0].max() < 2
    var = x.astype(np.float64).var(-1)
    assert 0.3 * EPS < var[cls == 2].min() and var[cls == 2].max() < 3 * EPS
    assert np.abs(x[cls == 3]).max() == 100 and w.min() == np.float32(0.05) and w.max() == 20
    for k in range(4):
        assert (cls == k).sum() >= 60


def test_layernorm_emulation_inside_bound_on_every_launch():
    peak = {}
    for i, (D, rows, smode, xoff, branch) in enumerate(R.LN_LAUNCHES):
        xs = R.ln_stride(D, smode)
        V = R.ln_vector_width(D, xs, D, xoff)
        assert f"V{V}" == branch
        x, w, b, cls = R.ln_inputs(rows, D, 100 + i)
        ref = R.layernorm_ref(x, w, b, EPS)
        for obf in (False, True):
            r = R.ratio(R.emulate_layernorm(x, w, b, EPS, V, obf), ref, R.layernorm_bound(x, w, b, EPS, obf))
            key = ("bf16" if obf else "fp32", branch)
            peak[key] = max(peak.get(key, 0.0), float(r.max()))
    print("\nlayernorm emulation, peak |err| / bound:", {f"{k[0]}/{k[1]}": round(v, 3) for k, v in peak.items()})
    assert set(b for _, b in peak) == {"V1", "V2"} and max(peak.values()) < 1.0


@pytest.mark.parametrize("name", R.LN_VARIANTS)
def test_layernorm_wrong_kernels_exceed_bound(name):
    D, rows = 384, 257
    x, w, b, cls = R.ln_inputs(rows, D, 11)
    pad = np.concatenate([x, np.full((rows, 1), 3.0, np.float32)], 1)  # x_stride = D + 1, a finite value in the gap
    ref = R.layernorm_ref(x, w, b, EPS)
    want = R.LN_CATCHES[name]
    sel = np.ones(rows, bool) if want is None else cls == R.LN_CLASSES.index(want)
    for obf in (False, True):
        got = R.rounded(R.layernorm_variant(name, x, w, b, EPS, pad), obf)
        r = R.ratio(got, ref, R.layernorm_bound(x, w, b, EPS, obf))[sel].max()
        print(f"\nlayernorm wrong kernel {name} ({'bf16' if obf else 'fp32'} out): {r:.3g} x bound on {want or 'all'} rows")
        assert r >= CATCH


# ---------------------------------------------------------------------------------------------------------------------
# Linear
# ---------------------------------------------------------------------------------------------------------------------
def _lin_case(M, Nn, K, seed, dtype, epi):
    flags, act, res, obf = R.EPILOGUES[epi]
    a, w, bias, r, cancel = R.linear_inputs(M, Nn, K, seed, dtype == R.BF16, gelu=act == "gelu", resid=res)
    return a, w, bias, r, cancel, act, (obf and dtype == R.BF16)


def test_linear_families_reach_their_edges():
    for dtype in (R.F32, R.BF16):
        a, w, bias, r, cancel, act, obf = _lin_case(273, 132, 192, 21, dtype, "gelu")
        h = R.linear_ref(a[:-1], w, bias)
        S = R.linear_terms(a[:-1], w, bias)
        assert cancel.sum() >= 50 and (S[cancel] / np.abs(h[cancel])).min() >= 1e3
        assert (S[~cancel] / np.abs(h[~cancel])).min() < 50
        tail, neg = float((np.abs(h) > 8).mean()), float(((h >= -8) & (h <= -2)).mean())
        print(f"\nlinear gelu family ({'bf16' if dtype else 'fp32'}): beyond |8| {tail:.3f}, in [-8, -2] {neg:.3f}")
        assert tail >= R.MIN_TAIL and neg >= R.MIN_NEG
        a, w, bias, r, cancel, act, obf = _lin_case(273, 132, 192, 21, dtype, "resid_f32")
        y, S = R.linear_ref(a[:-1], w, bias, r), R.linear_terms(a[:-1], w, bias, r)
        assert r is not None and (S[cancel] / np.abs(y[cancel])).min() >= 1e3


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["fp32", "bf16"])
def test_linear_emulation_inside_bound_on_every_launch(dtype):
    peak, seen = {}, set()
    for e, epi in enumerate(R.EPILOGUES):
        Ms, Ns, Ks = set(), set(), set()
        for i, (M, Nn, K, padded, branch) in enumerate(R.linear_launches(epi, dtype)):
            Ms.add(M), Ns.add(Nn), Ks.add(K), seen.add((epi, branch))
            a, w, bias, r, cancel, act, obf = _lin_case(M, Nn, K, 1000 * e + i, dtype, epi)
            a = a[:-1]
            pre = R.linear_ref(a, w, bias, r)  # (before the activation)
            assert (R.linear_terms(a, w, bias, r)[cancel] / np.abs(pre[cancel])).min() >= 1e3, (epi, M, Nn, K)
            got = R.emulate_linear(a, w, bias, r, act, obf, dtype == R.BF16)
            rt = R.ratio(got, R.linear_ref(a, w, bias, r, act), R.linear_bound(a, w, bias, r, act, obf))
            peak[epi] = max(peak.get(epi, 0.0), float(rt.max()))
        assert Ms == set(R.LIN_M) and Ns == set(R.LIN_N) and Ks == set(R.LIN_K[dtype]), epi
    print(f"\nlinear emulation ({'bf16' if dtype else 'fp32'}), peak |err| / bound per epilogue:", {k: round(v, 3) for k, v in peak.items()})
    assert seen == {(e, b) for e in R.EPILOGUES for b in ("ring", "guarded", "tiled")}
    assert max(peak.values()) < 1.0


@pytest.mark.parametrize("name", R.LINEAR_VARIANTS)
def test_linear_wrong_kernels_exceed_bound(name):
    for dtype in (R.F32, R.BF16):
        b16 = dtype == R.BF16
        gelu = name == "resid_before_gelu"
        resid = name in ("resid_before_gelu", "round_before_resid")
        outs = (False,) if resid else (False, True) if b16 else (False,)  # (RESID is instantiated with an fp32 output only)
        a, w, bias, r, cancel = R.linear_inputs(273, 132, 64 if name == "round_before_resid" else 192, 31, b16, gelu=gelu, resid=resid)
        act = "gelu" if gelu else "none"
        ref = R.linear_ref(a[:-1], w, bias, r, act)
        for obf in outs:
            bound = R.linear_bound(a[:-1], w, bias, r, act, obf)
            y, mask = R.linear_variant(name, a[:-1], w, bias, r, act, b16, a_next=a[-1])
            rt = R.ratio(R.rounded(y, obf), ref, bound)
            tag = f"linear wrong kernel {name} ({'bf16' if b16 else 'fp32'} operands, {'bf16' if obf else 'fp32'} out)"
            if name == "round_before_resid" and not b16:  # the accumulator already is the compute dtype: the right kernel
                print(f"\n{tag}: {rt.max():.3g} x bound (the right kernel here: held to the bound)")
                assert rt.max() < 1.0
                continue
            print(f"\n{tag}: {rt[mask].max():.3g} x bound on its class, {rt[~mask].max() if (~mask).any() else 0:.3g} outside")
            assert rt[mask].max() >= CATCH
            assert not (~mask).any() or rt[~mask].max() < 1.0


# ---------------------------------------------------------------------------------------------------------------------
# Attention
# ---------------------------------------------------------------------------------------------------------------------
def test_attention_families_reach_their_edges():
    for ntok in (17, 273):
        for fam in ("spike_first", "spike_last"):
            qkv, key = R.attn_inputs(2, ntok, 6, 64, 41, fam, True)
            assert key == (3 if fam == "spike_first" else ntok - 1) and (fam != "spike_last" or key % 16 == 0)
            rows = R.spike_rows(qkv, 6, 0.125, key)
            _, p = R.attention_ref(qkv, 6, 0.125)
            assert rows.mean() > 0.25 and rows.any(-1).all()           # in every head
            assert np.array_equal(p.argmax(-1) == key, rows) and np.percentile(p[rows][:, key], 75) > 0.99  # and mostly takes the row
            assert R.spike_rows(qkv, 6, 0.125, key, overflow=True).any()  # on some of them exp(s) overflows fp32 without the max
        qkv, _ = R.attn_inputs(2, ntok, 6, 64, 41, "flat_row", True)
        _, p = R.attention_ref(qkv, 6, 0.125)
        assert p[:, :, 1].max() / p[:, :, 1].min() < 1.05


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("dh", [32, 64])
def test_attention_emulation_inside_bound_on_every_launch(dh, bf16):
    peak = {}
    for i, (B, ntok, heads, fam) in enumerate(R.attention_launches(dh, bf16)):
        qkv, key = R.attn_inputs(B, ntok, heads, dh, 300 + i, fam, bf16)
        o, p = R.attention_ref(qkv, heads, dh ** -0.5)
        for kernel in ("attn", "attn64") if bf16 and dh == 64 and ntok > 256 else ("attn",):
            bo, bp = R.attention_bound(qkv, heads, dh ** -0.5, bf16, kernel)
            go, gp = R.emulate_attention(qkv, heads, dh ** -0.5, bf16, kernel)
            peak[kernel + "/out"] = max(peak.get(kernel + "/out", 0.0), float(R.ratio(go, o, bo).max()))
            peak[kernel + "/probs"] = max(peak.get(kernel + "/probs", 0.0), float(R.ratio(gp, p, bp).max()))
            assert float(np.abs(gp.sum(-1) - 1).max()) <= (ntok + 4) * R.U
    print(f"\nattention emulation (dh {dh}, {'bf16' if bf16 else 'fp32'}), peak |err| / bound:", {k: round(v, 3) for k, v in peak.items()})
    assert max(peak.values()) < 1.0


def test_attention_launch_list_reaches_every_branch():
    seen = set()
    for dh in (32, 64):
        for bf16 in (False, True):
            l = R.attention_launches(dh, bf16)
            assert {n for _, n, _, _ in l} == set(R.ATTN_NTOK)
            for B, ntok, heads, fam in l:
                for probs in (False, True):
                    seen.add(R.attention_branch(ntok, dh, B, heads, bf16, probs).rsplit("-", 1)[0])
    for k in ("attn", "attn64"):
        for t in ((2, 18) if k == "attn" else (17, 18)):
            for y in ("ysplit", "y1"):
                assert f"{k}-nkt{t}-{y}" in seen, (k, t, y)


@pytest.mark.parametrize("name", R.ATTN_VARIANTS)
def test_attention_wrong_kernels_exceed_bound(name):
    fam = R.ATTN_CATCHES[name]
    for bf16 in (False, True):
        for ntok, dh, heads in ((33, 64, 6), (273, 64, 6)) if name == "no_max" else ((17, 32, 2), (273, 64, 6)):
            qkv, key = R.attn_inputs(1, ntok, heads, dh, 51, fam, bf16)
            scale = dh ** -0.5
            o, p = R.attention_ref(qkv, heads, scale)
            bo, bp = R.attention_bound(qkv, heads, scale, bf16)
            vo, vp = R.attention_variant(name, qkv, heads, scale)
            ro = R.ratio(R.rounded(vo, bf16), o, bo)
            rp = R.ratio(np.asarray(vp, np.float32), p, bp)
            if name == "no_max":  # the rows whose maximum is the spiked key, with a score whose fp32 exponential overflows
                rows = R.spike_rows(qkv, heads, scale, key, overflow=True)
                assert rows.any()
                ro = ro.reshape(1, ntok, heads, dh).transpose(0, 2, 1, 3)[rows]
                rp = rp[rows]
            print(f"\nattention wrong kernel {name} ({'bf16' if bf16 else 'fp32'}, ntok {ntok}, dh {dh}): out {ro.max():.3g} x bound, probs {rp.max():.3g} x")
            assert ro.max() >= CATCH
            if name not in ("v_group_perm", "next_head_v"):  # (those leave the probabilities right)
                assert rp.max() >= CATCH
            else:
                assert rp.max() < 1.0
