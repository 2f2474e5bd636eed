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
