"""CPU tests of tests/vit_bf16_ref.py, the reference of the per-unit bf16 tests: the activation-image converters against the offset
formulas of csrc/kernels.h, the bf16 rounding helper against torch, and the emulation with its rounding points off against the
numpy oracle's block."""
import numpy as np
import pytest
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


# ---- the attention unit: attention_unit's routes, its schedule restatement, inputs, noise floor and variants ------------------------------
import math  # noqa: E402

_att_cache = {}


def _att_params(family, blk=3):
    if ("p", family, blk) not in _att_cache:
        specs = synth.vit_param_specs("vit256")
        pn = synth.make_params_np(specs, 256) if family == "std" else synth.make_vit_outlier_params_np(specs, 256, 6)
        _att_cache["p", family, blk] = (R.params_from_dict(pn, blk, 6), R.params_from_dict(pn, blk, 6, rnd=False))
    return _att_cache["p", family, blk]


def _att_case(family, nseq, blk=3):
    if (family, nseq, blk) not in _att_cache:
        _att_cache[family, nseq, blk] = R.att_inputs(_att_params(family, blk)[0], nseq, R.att_seed(nseq), outlier_rows=family == "outlier")
    return _att_cache[family, nseq, blk]


def _att_ref(family, nseq, route, blk=3):
    if ("ref", family, nseq, route, blk) not in _att_cache:
        _att_cache["ref", family, nseq, route, blk] = R.attention_unit(_att_case(family, nseq, blk)["xn"], _att_params(family, blk)[0], nseq, route=route)
    return _att_cache["ref", family, nseq, route, blk]


def _attention_unit_before_routes(xn, p, nseq, rnd=True, variant=None, seqs=32):
    """attention_unit as it stood before it learnt mm= and route= (kept word for word: R.block and the tests of tests/test_gpu_parity.py
    rest on these bits)"""
    r = R.bf16 if rnd else R._id
    M, Dm = xn.shape
    ntok = M // nseq
    H = p["heads"]
    dh = Dm // H
    out = []
    for s0 in range(0, nseq, seqs):
        ns = min(seqs, nseq - s0)
        x = xn[s0 * ntok:(s0 + ns) * ntok].double()
        qkv = r(x @ p["qkv_w"].t() + p["qkv_b"])
        qkv = qkv.view(ns, ntok, 3, H, dh).permute(2, 0, 3, 1, 4)
        sc = p["scale"] * (p["scale"] if variant == "scale2" else 1.0)
        s = (qkv[0] @ qkv[1].transpose(-1, -2)) * sc
        if variant == "mask_tile":
            s[..., 16:32] = -math.inf
        e = torch.exp(s - s.amax(-1, keepdim=True))
        l = e.sum(-1, keepdim=True)
        o = (r(e) @ qkv[2]) / l
        out.append(r(o.transpose(1, 2).reshape(ns * ntok, Dm)))
    return torch.cat(out)


def test_attention_unit_defaults_are_bit_unchanged_and_routes_without_rounding_are_plain_attention():
    p, pe = _att_params("std")
    for nseq, ntok, seqs in ((3, 257, 32), (3, 257, 2), (2, 33, 32)):
        xn = R.bf16(torch.from_numpy(synth.hash_uniform_np((nseq * ntok, 384), 31 + ntok, 2.0).astype(np.float64)))
        for rnd in (True, False):
            for v in (None, "scale2", "mask_tile"):
                want = _attention_unit_before_routes(xn, p, nseq, rnd=rnd, variant=v, seqs=seqs)
                got = R.attention_unit(xn, p, nseq, rnd=rnd, variant=v, seqs=seqs)
                assert torch.equal(got.view(torch.int64), want.view(torch.int64)), (nseq, ntok, seqs, rnd, v)
    # the two-kernel route IS that arithmetic; the fused one moves the [CLS] rows only
    c = _att_case("std", 16)
    base, two, fused = R.attention_unit(c["xn"], p, 16), _att_ref("std", 16, "two_kernel"), _att_ref("std", 16, "fused")
    assert torch.equal(base, two)
    rows = torch.ones(16 * 257, dtype=torch.bool)
    rows[::257] = False
    assert torch.equal(fused[rows], two[rows]) and not torch.equal(fused[~rows], two[~rows])
    # rnd=False: plain fp64 attention on either route
    xs = c["xn"].double()
    qkv = (xs @ pe["qkv_w"].t() + pe["qkv_b"]).view(16, 257, 3, 6, 64).permute(2, 0, 3, 1, 4)
    want = (torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) * pe["scale"], -1) @ qkv[2]).transpose(1, 2).reshape(16 * 257, 384)
    plain = {}
    for route in R.ATT_ROUTES:
        plain[route] = R.attention_unit(xs, pe, 16, rnd=False, route=route)
        assert float((plain[route] - want).norm() / want.norm()) < 1e-10, route
    # (the fused route's [CLS] rows came through the per-wave partials and their merge: the same numbers to 1e-10, not the same bits)
    assert torch.equal(plain["fused"][rows], plain["two_kernel"][rows]) and not torch.equal(plain["fused"][~rows], plain["two_kernel"][~rows])


def test_qkv_attn_schedule_restates_the_launcher():
    """Every (patch, head) is taken exactly once, by the workgroup and at the position the formulas of qkv_attention.hip:783-786 and
    unit_of (:176-181) give; at 256 CUs the smallest sizes with 1, 2 and 3 units on the busiest workgroup are 16, 48 and 96."""
    assert R.att_schedule_sizes(256) == (16, 48, 96)
    assert R.att_schedule_sizes(304) == (16, 64, 112)  # (38 workgroups per XCD)
    for ncu in (256, 304, 64, 4):
        for nseq in (16, 32, 48, 80, 96, 112, 528):
            s = R.qkv_attn_schedule(nseq, ncu)
            px, per = (nseq + 7) // 8, max(ncu // 8, 1)
            nslots = min(6 * px, per)
            assert bool((s["wg"] >= 0).all()) and int(s["wg"].max()) < 8 * nslots
            b, h = torch.meshgrid(torch.arange(nseq), torch.arange(6), indexing="ij")
            U = (b % px) * 6 + h  # the unit's number inside its XCD, head fastest
            assert torch.equal(s["wg"], b // px + 8 * (U % nslots)) and torch.equal(s["idx"], U // nslots)
            # a workgroup's units are numbered 0 .. count - 1, each once; prev / prev2 are the patches of the units before
            key = s["wg"] * 4096 + s["idx"]
            assert key.unique().numel() == nseq * 6
            for wg in s["wg"].unique().tolist()[:40]:
                m = s["wg"] == wg
                order = torch.argsort(s["idx"][m])
                assert s["idx"][m][order].tolist() == list(range(int(m.sum()))) and bool((s["count"][m] == int(m.sum())).all())
                pb = b[m][order].tolist()
                assert s["prev"][m][order].tolist() == [-1] + pb[:-1] and s["prev2"][m][order].tolist() == ([-1, -1] + pb[:-2])[:len(pb)]
            assert s["max_units"] == -(-6 * px // nslots)
            assert torch.equal(s["first"], s["idx"] == 0) and torch.equal(s["last"], s["idx"] == s["count"] - 1)
            assert not bool((s["carried"] & (s["first"] | s["last"])).any())
            assert bool((s["first"] | s["carried"] | s["last"]).all())
    s = R.qkv_attn_schedule(16, 256)
    assert bool((s["first"] & s["last"]).all())  # (one unit per workgroup)
    s = R.qkv_attn_schedule(96, 256)
    assert int(s["carried"].sum()) == 64 and int(s["first"].sum()) == 256 and int(s["last"].sum()) == 256


def test_attention_unit_inputs_reach_their_edges():
    assert torch.equal(R.fused_half0_keys()[:10], torch.tensor([1, 1, 1, 1, 1, 0, 0, 0, 0, 1], dtype=torch.bool)) and int(R.fused_half0_keys().sum()) == 129
    for family in ("std", "outlier"):
        for nseq in (16, 48, 96):
            c = _att_case(family, nseq)
            assert all(len(c["classes"][k]) >= 1 for k in R.ATT_CLASSES)
            e = R.att_assert_edges(c, _att_params(family)[0], nseq, family)
            print(f"edges {family} nseq {nseq}: " + " ".join(f"{k} {v:.3g}" for k, v in e.items()))


ATT_FLOOR_CASES = [(r, f, b, n) for f, b in (("std", 3), ("outlier", 3), ("outlier", 0)) for n in (16, 48, 96) for r in R.ATT_ROUTES]


def test_attention_unit_noise_floor():
    """fp64 products against fp32 products of the same operands at the same rounding points (see test_cls_block_noise_floor): R.ATT_FLOOR
    records the largest value per (route, family, metric) over these cases; block 0 of the outlier weights (the largest logits) has its own,
    taken with the fixed-order fp32 product (R.att_floor_key)."""
    got = {}
    for route, family, blk, nseq in ATT_FLOOR_CASES:
        c, p = _att_case(family, nseq, blk), _att_params(family, blk)[0]
        a64 = _att_ref(family, nseq, route, blk)
        fkey, mm = R.att_floor_key(family, blk)
        a32 = R.attention_unit(c["xn"], p, nseq, route=route, mm=mm)
        assert torch.equal(R.bf16(a64), a64)
        e = R.att_errors(a32, a64, nseq, c["classes"], R.qkv_attn_schedule(nseq, 256))
        print(f"floor {route} {family} block {blk} nseq {nseq}: " + " ".join(f"{k} {e[k]:.2e}" for k in R.ATT_METRICS))
        cur = got.setdefault((route, fkey), dict.fromkeys(R.ATT_METRICS, 0.0))
        for k in R.ATT_METRICS:
            cur[k] = max(cur[k], e[k])
    assert set(got) == set(R.ATT_FLOOR) and R.ATT_BAR_FACTOR == R.CLS_BAR_FACTOR
    for key, cur in got.items():
        print(f"floor {key}: " + " ".join(f"{k} {cur[k]:.2e}" for k in R.ATT_METRICS))
        for k in R.ATT_METRICS:
            # (single flips decide these values and fp32 products differ between BLAS builds: the table is held to a factor, not to digits)
            assert R.ATT_FLOOR[key][k] / 4 <= cur[k] <= R.ATT_FLOOR[key][k] * 2, (key, k, cur[k], R.ATT_FLOOR[key][k])


def test_attention_unit_variants_land_beyond_the_bars():
    """Every variant of R.ATT_VARIANTS[route] changes the output and lands >= 3 x beyond a bar (R.ATT_BAR_FACTOR x R.ATT_FLOOR): at 16
    patches, the two that need a workgroup with two / three units at 96.  R.ATT_NOT_PINNED may name (route, family, variant) where the
    mistake is arithmetically invisible; never a masking, bias-of-v or schedule variant."""
    must = {"pad_unmasked", "drop_cls_key", "drop_last_token", "no_bv", "stale_cls_row", "prev_patch_rows"}
    assert not any(v in must for _, _, v in R.ATT_NOT_PINNED)
    for family in ("std", "outlier"):
        p = _att_params(family)[0]
        for route in R.ATT_ROUTES:
            bar = {k: R.ATT_BAR_FACTOR * v for k, v in R.ATT_FLOOR[route, family].items()}
            for v in R.ATT_VARIANTS[route]:
                nseq = 96 if v in R.ATT_VARIANT_UNITS else 16
                sched = R.qkv_attn_schedule(nseq, 256)
                assert sched["max_units"] >= R.ATT_VARIANT_UNITS.get(v, 1)
                c, ref = _att_case(family, nseq), _att_ref(family, nseq, route)
                a = R.attention_unit(c["xn"], p, nseq, route=route, variant=v)
                assert not torch.equal(a, ref), (route, family, v)
                e = R.att_errors(a, ref, nseq, c["classes"], sched)
                k = max(R.ATT_METRICS, key=lambda k: e[k] / bar[k])
                pinned = (route, family, v) not in R.ATT_NOT_PINNED
                print(f"variant {route} {family} {v}: {e[k] / bar[k]:.3g} x the bar of {k}" + ("" if pinned else " (not pinned)"))
                assert e[k] / bar[k] >= 3.0 or not pinned, (route, family, v, k, e[k] / bar[k])
    with pytest.raises(ValueError):
        R.attention_unit(_att_case("std", 16)["xn"], _att_params("std")[0], 16, route="two_kernel", variant="no_merge_rescale")
