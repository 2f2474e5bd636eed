"""CPU tests of tests/vit_bf16_ref.py, the reference of the per-unit bf16 tests: the activation-image converters against the offset
formulas of csrc/kernels.h, the bf16 rounding helper against torch, and the emulation with its rounding points off against the
numpy oracle's block."""
import numpy as np
import torch

import vit_bf16_ref as R
from hipt_abmil_atec23_amd import synth
from oracle import hipt_oracle as O


def _expected_offsets(M, fp32):
    """offset of element (row, col) by the kernels.h formulas, [M, 384]"""
    row, col = np.meshgrid(np.arange(M), np.arange(384), indexing="ij")
    F, i = row // 16, row % 16
    k = col // 8  # 16-byte bf16 chunk = g + 4 c
    g, c = k % 4, k // 4
    lane = 16 * g + i
    if fp32:
        h, e = (col % 8) // 4, col % 4
        return F * 6144 + c * 512 + h * 256 + lane * 4 + e
    return F * 6144 + c * 512 + lane * 8 + col % 8


def test_activation_image_converters_match_kernels_h():
    for M in (16, 48, 257 * 16):
        ids = torch.arange(M * 384, dtype=torch.int64).view(M, 384)
        for fp32, to, back in ((False, R.to_image, R.from_image), (True, R.to_image_f32, R.from_image_f32)):
            img = to(ids).reshape(-1).numpy()
            off = _expected_offsets(M, fp32)
            assert np.array_equal(img[off], ids.numpy()), (M, fp32)  # element (row, col) lies where the formula says
            assert torch.equal(back(to(ids)), ids) and torch.equal(to(back(ids)), ids)
    # the two layouts are different permutations (a test that used one for the other would notice)
    ids = torch.arange(16 * 384).view(16, 384)
    assert not torch.equal(R.to_image(ids), R.to_image_f32(ids))


def test_bf16_rounding_helper_equals_torch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(200000, generator=g, dtype=torch.float64) * torch.logspace(-40, 38, 200000, dtype=torch.float64)
    u = torch.randint(0, 1 << 16, (4096,), generator=g, dtype=torch.int64)
    ties = ((u << 16) | 0x8000).to(torch.int64)  # exact halfway cases, both parities of the kept bit
    ties = (ties - ((ties >> 31) << 32)).to(torch.int32).view(torch.float32)
    special = torch.tensor([0.0, -0.0, 1e-45, -1e-45, 1.1754942e-38, 3.3895314e38, 3.4028235e38, float("inf"), -float("inf")])
    for t in (x.float(), ties, special):
        t = t[torch.isfinite(t) | torch.isinf(t)]
        want = t.bfloat16().float()
        assert torch.equal(R.bf16(t).view(torch.int32), want.view(torch.int32))
    assert torch.equal(R.bf16(x), x.float().bfloat16().double())
    assert torch.isnan(R.bf16(torch.tensor([float("nan")]))).all()


def _small_vit():
    specs = synth.vit_param_specs("vit256", depth=2)
    return synth.make_params_np(specs, 256)


def test_emulation_without_rounding_equals_oracle_block():
    p = _small_vit()
    nseq, ntok = 2, 33
    x = synth.hash_uniform_np((nseq, ntok, 384), 11, 2.0).astype(np.float64)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    want = O.block(x, p64, 0, 6)
    q = R.params_from_dict(p, 0, 6, rnd=False)
    got = R.block(torch.from_numpy(x).reshape(-1, 384), q, nseq, rnd=False).numpy().reshape(want.shape)
    assert np.linalg.norm(got - want) / np.linalg.norm(want) < 1e-12
    # the two units on their own: attention before proj, then the MLP unit with LN-1 of the next block
    xn = O.layer_norm(x, p64["blocks.0.norm1.weight"], p64["blocks.0.norm1.bias"])
    y, _ = O.attention(xn, p64, "blocks.0.attn.", 6)
    att = R.attention_unit(torch.from_numpy(xn).reshape(-1, 384), q, nseq, rnd=False)
    y_unit = att @ q["proj_w"].t() + q["proj_b"]
    assert float((y_unit - torch.from_numpy(y).reshape(-1, 384)).norm() / np.linalg.norm(y)) < 1e-12
    q1 = R.params_from_dict(p, 1, 6, rnd=False)
    xo, xn1 = R.mlp_unit(torch.from_numpy(x).reshape(-1, 384), att, q, q1, rnd=False)
    assert float((xo - torch.from_numpy(want).reshape(-1, 384)).norm() / np.linalg.norm(want)) < 1e-12
    xn1_want = O.layer_norm(want, p64["blocks.1.norm1.weight"], p64["blocks.1.norm1.bias"]).reshape(-1, 384)
    assert float((xn1 - torch.from_numpy(xn1_want)).norm() / np.linalg.norm(xn1_want)) < 1e-12


def test_emulation_rounding_points_are_live():
    """with rounding on, every rounding point moves the result by bf16-sized amounts, and the variants are distinct from it"""
    p = _small_vit()
    nseq, ntok = 2, 33
    x = torch.from_numpy(synth.hash_uniform_np((nseq * ntok, 384), 12, 2.0).astype(np.float64))
    q, q1 = R.params_from_dict(p, 0, 6), R.params_from_dict(p, 1, 6)
    exact = R.block(x, R.params_from_dict(p, 0, 6, rnd=False), nseq, rnd=False) - x
    emul = R.block(x, q, nseq) - x
    e = R.errors(emul, exact)["rel"]
    assert 1e-4 < e < 3e-2, e
    xn = R.bf16(R.layer_norm(x, q["ln1_w"], q["ln1_b"]))
    att = R.attention_unit(xn, q, nseq)
    base, xb = R.mlp_unit(x, att, q, q1)
    assert torch.equal(R.bf16(xb), xb) and torch.equal(R.bf16(att), att)
    for v in ("no_bproj", "b2_tile", "drop_chunk", "xn_block"):
        o, xv = R.mlp_unit(x, att, q, q1, variant=v, p_wrong=q)
        assert not (torch.equal(o, base) and torch.equal(xv, xb)), v
    for v in ("scale2", "mask_tile"):
        assert not torch.equal(R.attention_unit(xn, q, nseq, variant=v), att), v


# ---- the [CLS]-pruned last block: cls_block, its inputs and its noise floor ---------------------------------------------------------
_cls_cache = {}


def _cls_params(family):
    if ("p", family) not in _cls_cache:
        specs = synth.vit_param_specs("vit256")
        pn = synth.make_params_np(specs, 256) if family == "std" else synth.make_vit_outlier_params_np(specs, 256, 6)
        _cls_cache["p", family] = (R.params_from_dict(pn, 11, 6), R.params_from_dict(pn, 11, 6, rnd=False))
    return _cls_cache["p", family]


def _cls_case(family, nseq):
    if (family, nseq) not in _cls_cache:
        _cls_cache[family, nseq] = R.cls_inputs(_cls_params(family)[0], nseq, R.cls_seed(nseq), outlier_rows=family == "outlier")
    return _cls_cache[family, nseq]


def test_cls_block_without_rounding_equals_the_block_and_the_absorb_algebra():
    """rnd=False: every route is the [CLS] rows of R.block(rnd=False) to 1e-10, and test_cls_absorb_algebra's two forms on that
    file's own inputs"""
    import test_cls_absorb_algebra as A
    nseq = 6
    for family in ("std", "outlier"):
        _, pe = _cls_params(family)
        x = torch.from_numpy(synth.hash_uniform_np((nseq * 257, 384), 21, 2.0).astype(np.float64))
        xn = R.layer_norm(x, pe["ln1_w"], pe["ln1_b"])
        want = R.block(x, pe, nseq, rnd=False)[::257]
        att_want = R.attention_unit(xn, pe, nseq, rnd=False)[::257]
        for route in R.CLS_ROUTES:
            att, xc = R.cls_block(xn, x[::257], pe, nseq, route, rnd=False)
            assert float((att - att_want).norm() / att_want.norm()) < 1e-10, (family, route)
            assert float((xc - want).norm() / want.norm()) < 1e-10, (family, route)
    p, _ = _cls_params("std")
    W, b = p["qkv_w"].numpy(), p["qkv_b"].numpy()
    w = dict(Wq=W[:384], Wk=W[384:768], Wv=W[768:], bq=b[:384], bk=b[384:768], bv=b[768:], g=p["ln1_w"].numpy(), beta=p["ln1_b"].numpy())
    xn = A.patches(w, 6, 11)
    q = A.query(w, xn, 1.0)
    o_ref, o_abs = A.reference_form(w, xn, q)[0], A.absorbed_form(w, xn, q)
    for route in R.CLS_ROUTES:
        att = R.cls_block(torch.from_numpy(xn).reshape(-1, 384), torch.zeros(6, 384, dtype=torch.float64), p, 6, route, rnd=False)[0].numpy()
        assert A.rel(att, o_ref) < 1e-10 and A.rel(att, o_abs) < 1e-10, route


def test_cls_schedule_and_the_ordered_patches():
    """The schedule restatement covers tokens 0 .. 256 once, block 16 is wave 0's; the classes of cls_inputs reach their edges in head
    0: top row at token 256 / at the waves' first rows, strictly increasing block maxima (ascending), none raised after the first
    block (descending), equal rows; on the outlier inputs the largest |score| is beyond 30 (exp only works behind the shift)."""
    tok_blk, waves = R.cls_pool_schedule()
    blocks = sorted(b for w in waves for b in w)
    assert blocks == list(range(17)) and waves[0][-1] == 16 and all(16 not in w for w in waves[1:])
    assert torch.equal(torch.bincount(tok_blk), torch.tensor([16] * 16 + [1])) and int(tok_blk[256]) == 16
    g = R.fused_cls_groups()
    assert torch.equal(torch.bincount(g), torch.tensor([33] + [32] * 7)) and int(g[0]) == 0 and int(g[256]) == 7
    for family in ("std", "outlier"):
        for nseq in (16, 48):
            c = _cls_case(family, nseq)
            R.cls_assert_edges(c, _cls_params(family)[0], nseq, family)


# fp64 products against fp32 products of the same operands at the same rounding points: two equally valid evaluations of the
# emulation.  Their distance is what a kernel may differ by without being wrong (single bf16 flips of q / p / z / o / y1 and what they
# move); R.CLS_FLOOR records the largest value per (route, family, metric) over these cases, the bars of tests/test_gpu_cls_block_unit.py
# are R.CLS_BAR_FACTOR times it.
FLOOR_CASES = [(r, f, n) for f in ("std", "outlier") for n in (16, 48) for r in R.CLS_ROUTES] + [("absorb", f, 528) for f in ("std", "outlier")]


def test_cls_block_noise_floor():
    got = {}
    for route, family, nseq in FLOOR_CASES:
        c, p = _cls_case(family, nseq), _cls_params(family)[0]
        a64, x64 = R.cls_block(c["xn"], c["x_cls"], p, nseq, route)
        a32, x32 = R.cls_block(c["xn"], c["x_cls"], p, nseq, route, mm=torch.float32)
        assert torch.equal(R.bf16(a64), a64)
        e = R.cls_errors(a32, a64, x32, x64, c["x_cls"], c["classes"])
        print(f"floor {route} {family} nseq {nseq}: " + " ".join(f"{k} {e[k]:.2e}" for k in R.CLS_METRICS))
        cur = got.setdefault((route, family), dict.fromkeys(R.CLS_METRICS, 0.0))
        for k in R.CLS_METRICS:
            cur[k] = max(cur[k], e[k])
    for key, cur in got.items():
        print(f"floor {key}: " + " ".join(f"{k} {cur[k]:.2e}" for k in R.CLS_METRICS))
        for k in R.CLS_METRICS:
            # (single flips decide these values and fp32 products differ between BLAS builds: the table is held to a factor, not to digits)
            assert R.CLS_FLOOR[key][k] / 4 <= cur[k] <= R.CLS_FLOOR[key][k] * 2, (key, k, cur[k], R.CLS_FLOOR[key][k])


def test_cls_block_rounding_points_and_variants_are_live():
    c, p = _cls_case("std", 16), _cls_params("std")[0]
    pe = _cls_params("std")[1]
    exact = R.cls_block(c["xn"], c["x_cls"], pe, 16, "absorb", rnd=False)[0]
    outs = {}
    for route in R.CLS_ROUTES:
        att, xc = R.cls_block(c["xn"], c["x_cls"], p, 16, route)
        outs[route] = att
        assert 2e-4 < float((att - exact).norm() / exact.norm()) < 2e-2, route
        for v in R.CLS_VARIANTS[route]:
            av, xv = R.cls_block(c["xn"], c["x_cls"], p, 16, route, variant=v)
            assert not (torch.equal(av, att) and torch.equal(xv, xc)), (route, v)
    assert not torch.equal(outs["absorb"], outs["fused_cls"]) and not torch.equal(outs["fused_cls"], outs["two_kernel"])
