"""The algebra behind the [CLS]-pruned last ViT-256 block without a K / V projection (csrc/cls_pool.hip).  CPU only, fp64 numpy.

With one query per (patch, head) -- q_h, bias included -- and xn_j the LayerNorm-1 rows of the patch:
    score_j = scale * q_h . (Wk_h xn_j + bk_h) = scale * (xn_j . u_h) + const,   u_h = Wk_h^T q_h
    o_h     = sum_j p_j (Wv_h xn_j + bv_h)     = Wv_h z_h + bv_h,                z_h = sum_j p_j xn_j
so K and V are never formed and bk is not needed at all.  Checked here on the synthetic weights of block 12:
  * the identity itself, to fp64 rounding (1e-10 relative);
  * the same with every operand rounded where the kernels round it -- bf16 xn and q (both routes), then u as a hi + lo bf16 pair of
    its fp32 value, bf16 p, bf16 z, bf16 o (new) against bf16 K, V, p, o (old: the fused kernel's [CLS]-only form) -- both against
    the unrounded fp64 result.  Measured here (8 patches a case; relative L2 of o, old / new with u as one bf16 / new with hi + lo):
        scores within +-6     4.0e-3 / 4.0e-3 / 3.4e-3   and   3.7e-3 / 3.4e-3 / 3.2e-3 (a second draw)
        scores within +-21    6.7e-3 / 6.4e-3 / 4.9e-3
        scores within +-150   1.8e-2 / 1.3e-2 / 8.2e-3
    The new route drops two bf16 roundings per element (K, V) for one (z) plus a 2^-17 one (u as a pair), and shares the bf16 q with
    the old one, so its error should not be the larger of the two; NEW <= 1.25 x OLD allows for the draw-to-draw variation of either
    figure (10 % between the two draws above).  A single bf16 u passes as well; the pair is what the kernel carries.
  * a large-logit case (the query scaled until the scores reach +-120, as the fused kernel's outlier cases have them), where
    exp() only works behind the max shift.
"""
import numpy as np
import pytest

from hipt_abmil_atec23_amd import synth

D, H, NTOK = 384, 6, 257
SCALE = 64 ** -0.5
FACTOR = 1.25  # new-route error <= FACTOR x old-route error (docstring)


def bf16(a):
    """Round to bfloat16 (nearest even), returned as float64."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return r.view(np.float32).astype(np.float64)


def f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


def hi_lo(a):
    a = f32(a)
    return bf16(a) + bf16(a - bf16(a))


def ident(a):
    return a


def rel(a, r):
    return float(np.linalg.norm(a - r) / np.linalg.norm(r))


@pytest.fixture(scope="module")
def blk12():
    p = synth.make_params_np(synth.vit_param_specs("vit256"), 256)
    pre = "blocks.11."
    W = bf16(p[pre + "attn.qkv.weight"])  # the bf16 matrices the kernels read
    b = p[pre + "attn.qkv.bias"].astype(np.float64)
    return dict(Wq=W[:D], Wk=W[D:2 * D], Wv=W[2 * D:], bq=b[:D], bk=b[D:2 * D], bv=b[2 * D:],
                g=p[pre + "norm1.weight"].astype(np.float64), beta=p[pre + "norm1.bias"].astype(np.float64))


def patches(w, n, seed):
    x = np.random.default_rng(seed).standard_normal((n, NTOK, D))
    x = (x - x.mean(-1, keepdims=True)) / x.std(-1, keepdims=True)
    return bf16(x * w["g"] + w["beta"])  # LayerNorm-1 rows as the bf16 image holds them


def reference_form(w, xn, q, r_kv=ident, r_p=ident):
    """project K, V; softmax; PV -- with K, V and the probabilities rounded by r_kv / r_p.  Returns (o, max |score|)."""
    K, V = r_kv(xn @ w["Wk"].T + w["bk"]), r_kv(xn @ w["Wv"].T + w["bv"])
    o, smax = np.zeros((xn.shape[0], D)), 0.0
    for h in range(H):
        sl = slice(64 * h, 64 * h + 64)
        s = np.einsum("nd,njd->nj", q[:, sl], K[:, :, sl]) * SCALE
        smax = max(smax, float(np.abs(s).max()))
        e = r_p(np.exp(s - s.max(-1, keepdims=True)))
        o[:, sl] = np.einsum("nj,njd->nd", e, V[:, :, sl]) / e.sum(-1, keepdims=True)
    return o, smax


def absorbed_form(w, xn, q, r_u=ident, r_p=ident, r_z=ident):
    o = np.zeros((xn.shape[0], D))
    for h in range(H):
        sl = slice(64 * h, 64 * h + 64)
        u = r_u(q[:, sl] @ w["Wk"][sl])                        # u_h = Wk_h^T q_h: no bk anywhere
        s = np.einsum("njc,nc->nj", xn, u) * SCALE
        e = r_p(np.exp(s - s.max(-1, keepdims=True)))
        z = r_z(np.einsum("nj,njc->nc", e, xn) / e.sum(-1, keepdims=True))
        o[:, sl] = z @ w["Wv"][sl].T + w["bv"][sl]
    return o


def query(w, xn, gain):
    return (xn[:, 0] @ w["Wq"].T + w["bq"]) * gain


@pytest.mark.parametrize("gain", [1.0, 4.0, 24.0])
def test_absorbed_form_is_the_reference_form_in_fp64(blk12, gain):
    xn = patches(blk12, 6, 11)
    q = query(blk12, xn, gain)
    o_ref, smax = reference_form(blk12, xn, q)
    err = rel(absorbed_form(blk12, xn, q), o_ref)
    print(f"gain {gain}: max |score| {smax:.1f}, absorbed vs reference form {err:.2e}")
    assert np.abs(blk12["bk"]).max() > 1e-3  # (a bias that would show if it did not cancel)
    assert err <= 1e-10


@pytest.mark.parametrize("gain,seed", [(1.0, 0), (1.0, 1), (4.0, 2), (24.0, 3)])
def test_rounding_points_of_the_new_route_cost_no_more_than_the_old_ones(blk12, gain, seed):
    xn = patches(blk12, 8, seed)
    q = query(blk12, xn, gain)
    o64, smax = reference_form(blk12, xn, q)
    qb = bf16(q)  # the Q rows leave their GEMM as bf16 on both routes
    old = rel(bf16(reference_form(blk12, xn, qb, bf16, bf16)[0]), o64)
    new1 = rel(bf16(absorbed_form(blk12, xn, qb, lambda a: bf16(f32(a)), bf16, bf16)), o64)
    new = rel(bf16(absorbed_form(blk12, xn, qb, hi_lo, bf16, bf16)), o64)
    print(f"gain {gain}: max |score| {smax:.1f}; old (bf16 q, K, V, p) {old:.3e}, new with one bf16 u {new1:.3e}, new (u hi + lo, bf16 p, z) {new:.3e}")
    if gain == 24.0:
        assert smax >= 100.0  # the large-logit case really is one
    assert new <= FACTOR * old
    assert new1 <= FACTOR * old


def test_large_logits_need_and_survive_the_max_shift(blk12):
    """Scores of about +-120: exp() of the raw scores overflows fp32 (e^89 is the limit), the shifted form stays exact."""
    xn = patches(blk12, 4, 5)
    q = query(blk12, xn, 24.0)
    o64, smax = reference_form(blk12, xn, q)
    assert 100.0 <= smax
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.exp(np.float32(smax)))
    o = absorbed_form(blk12, xn, bf16(q), hi_lo, lambda e: bf16(f32(e)), bf16)
    assert np.isfinite(o).all()
    assert rel(o, o64) < 3e-2  # (the bf16 query alone moves +-120 scores by 2^-9 * 120 = 0.2: this is not a precision bar)
