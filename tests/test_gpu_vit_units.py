"""Per-unit bf16 parity of the fused proj + MLP kernel (csrc/mlp16.hip) through hipt_vit_mlp_unit, against the fp64 emulation of
tests/vit_bf16_ref.py (bf16 exactly where the kernel rounds, exact erf GELU): the BRANCH INCREMENT x_out - x_in and the LayerNorm-1
image xn_out, which the residual stream of the whole-network tests dilutes.  Every case also carries the reference's sensitivity
self-check (plausible wrong kernels land >= 3 x beyond the bar) and asserts that its inputs reach the edges they are meant to test.

Bars (2 x measured, printed with -s): rel-L2 of the increment and the largest rel-L2 of one 16-column output tile,
over all rows and over each row class; xn_out rel-L2.  The last test takes one whole block through every route of hipt_vit_blocks
(streaming chain, small call, HIPT_GENERIC, HIPT_NO_PROJ_FOLD, ViT-4K) against the same emulation, each route asserted from the
library's launch counts."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn as nn

import vit_bf16_ref as R
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 32  # rows of NaN behind every buffer the unit writes or reads
E_WORKSPACE, E_UNSUPPORTED = -2, -4

# bars: 2 x the largest measurement over the cases (printed per case).  All rows: rel-L2 3.43e-4, worst 16-column tile 3.48e-4 (standard
# weights; the edge weights 1.1e-4 / 1.4e-4).  One row class (a few dozen rows: fewer bf16 flips to average over; the near-constant rows'
# LayerNorm scales the fp32 rounding of x + b_proj by 1 / std ~ 1e3): worst tile 1.72e-3.  xn_out: 5.61e-4.
BAR_INC = {"rel": 6.8e-4, "tile": 6.9e-4}
BAR_CLASS = {"rel": 3.4e-3, "tile": 3.4e-3}
BAR_XN = 1.1e-3
# GELU coverage of the edge weights: fractions of fc1 pre-activations beyond |8| (gelu1s' clamp t <= 1 on h / 8) and in [-8, -2]
# (measured 0.040 ... 0.063 and 0.023 ... 0.026)
MIN_TAIL, MIN_NEG = 0.02, 0.015


def _specs(hidden, depth):
    return synth.vit_param_specs("vit256", depth=depth, mlp_ratio=hidden / 384)


def _edge_params(hidden, depth):
    """The outlier family (synth.apply_vit_outliers_np: LayerNorm gains 0.05 ... 20, residual channels at +-50 ... 100) with the fc1 rows
    of every eighth hidden unit scaled by 16 (pre-activations out to +-30 and beyond) and the proj / fc2 biases by 8 (a bias missing
    from one output tile is then far beyond the bar)."""
    p = synth.make_vit_outlier_params_np(_specs(hidden, depth), 256, 6)
    sel = synth.hash_u32_np(hidden, 901) % np.uint32(8) == 0
    for i in range(depth):
        p[f"blocks.{i}.mlp.fc1.weight"][sel] *= np.float32(16.0)
        p[f"blocks.{i}.mlp.fc1.bias"][sel] *= np.float32(16.0)
        p[f"blocks.{i}.attn.proj.bias"] *= np.float32(8.0)
        p[f"blocks.{i}.mlp.fc2.bias"] *= np.float32(8.0)
    return p


_models = {}


def model(family="std", hidden=1536, depth=12, dtype="bf16"):
    """(module, packed weights) of a bf16 ViT-256 with the given MLP width, cached per configuration"""
    key = (family, hidden, depth, dtype)
    if key not in _models:
        from hipt_abmil_atec23_amd.vision_transformer import VisionTransformer
        m = VisionTransformer(patch_size=16, embed_dim=384, depth=depth, num_heads=6, mlp_ratio=hidden / 384, qkv_bias=True,
                              norm_layer=partial(nn.LayerNorm, eps=1e-6))
        assert m.blocks[0].mlp.fc1.out_features == hidden
        if family == "std":
            m.load_state_dict(synth.make_state_dict(_specs(hidden, depth), 256))
        else:
            m.load_state_dict({k: torch.from_numpy(v) for k, v in _edge_params(hidden, depth).items()})
        m = m.eval().to(DEV).set_compute_dtype(dtype)
        pk = m._tokens(synth.hash_uniform_torch((1, 3, 256, 256), 2, device=DEV))[0]
        _models[key] = (m, pk)
    return _models[key]


def row_classes(M, nseq):
    """rows of the three edge classes: two in the first 128-row tile, two in the tail tile, and the [CLS] rows (s * 257) of every
    third sequence"""
    out = []
    for k in range(3):
        r = [1 + 2 * k, 2 + 2 * k, M - 1 - 2 * k, M - 2 - 2 * k] + [257 * s for s in range(k, nseq, 3)]
        out.append(torch.tensor(sorted(set(r)), dtype=torch.int64, device=DEV))
    return out


def inputs(M, nseq, seed, bp):
    """fp32 residual stream x and bf16 attention output att, ordinary O(1) rows, with the edge classes written into their rows:
    0: large common offset (mean 100, std 0.5: LayerNorm cancellation); 1: near-constant (variance ~1e-6 = eps: att = 0 and x + b_proj =
    1 + 1.7e-3 u, so the eps decides the output); 2: four residual channels at +-60 ... 100 (synth.apply_vit_outliers_np's magnitudes)"""
    x = synth.hash_uniform_torch((M, 384), seed, 2.0, device=DEV)
    att = synth.hash_uniform_torch((M, 384), seed + 1, 1.0, device=DEV).bfloat16()
    cls = row_classes(M, nseq)
    x[cls[0]] = synth.hash_uniform_torch((len(cls[0]), 384), seed + 2, 0.87, 100.0, device=DEV)
    x[cls[1]] = (1.0 - bp.float())[None] + synth.hash_uniform_torch((len(cls[1]), 384), seed + 3, 1.7e-3, device=DEV)
    att[cls[1]] = 0
    ch = torch.tensor([7, 100, 200, 333], device=DEV)
    x[cls[2][:, None], ch[None]] = torch.tensor([60.0, -75.0, 90.0, -100.0], device=DEV)
    return x, att, cls


def nan_rows(M, dtype):
    return torch.full((M + CANARY, 384), float("nan"), dtype=dtype, device=DEV)


def canaries_intact(buf, M):
    tail = buf[M:]
    bits = torch.full_like(tail, float("nan")).view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)
    return torch.equal(tail.view(bits.dtype), bits)


def run_mlp(pk, blk, x, att, nseq, xn_mode="sep", ws=None):
    """one hipt_vit_mlp_unit launch on images of x / att in NaN-fenced buffers -> (x_out row-major fp32, xn_out row-major bf16 or None,
    buffers for the canary checks)"""
    M = nseq * 257
    xb, ab = nan_rows(M, torch.float32), nan_rows(M, torch.bfloat16)
    xb[:M] = R.to_image_f32(x)
    ab[:M] = R.to_image(att)
    xnb = nan_rows(M, torch.bfloat16) if xn_mode == "sep" else (ab if xn_mode == "alias" else None)
    if ws is None:
        ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    before = N.calls
    N.call("hipt_vit_mlp_unit", pk.ref, blk, N.ptr(xb), N.ptr(ab), nseq, N.ptr(xnb), N.ptr(ws), ws.numel(), N.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert N.calls == before + 1
    xn = R.from_image(xnb[:M]) if xnb is not None else None
    return R.from_image_f32(xb[:M]), xn, (xb, ab, xnb)


def _fmt(e):
    return " ".join(f"{k} {v:.2e}" for k, v in e.items())


def check_against_reference(tag, m, blk, x, att, cls, nseq, xo, xn):
    """increment and xn_out against the emulation; the sensitivity variants against the bars"""
    depth = len(m.blocks)
    p = R.block_params(m, blk)
    p_next = R.block_params(m, blk + 1 if blk + 1 < depth else blk)
    p_wrong = R.block_params(m, blk if blk + 1 < depth else blk - 1)  # (a kernel reading the LN-1 of the wrong block)
    ref, xn_ref = R.mlp_unit(x, att, p, p_next)
    inc_ref, inc = ref - x.double(), xo.double() - x.double()
    e = R.errors(inc, inc_ref)
    e_xn = R.errors(xn, xn_ref)["rel"] if xn is not None else 0.0
    e_cls = [R.errors(inc[c], inc_ref[c]) for c in cls]
    print(f"\n{tag}: increment {_fmt(e)} (bars rel {BAR_INC['rel']:.1e} tile {BAR_INC['tile']:.1e}); xn_out rel {e_xn:.2e} (bar {BAR_XN:.1e}); "
          f"row classes offset / near-constant / outlier channels: " + " | ".join(_fmt(c) for c in e_cls) + f" (bars {BAR_CLASS['tile']:.1e})")
    assert bool(torch.isfinite(inc).all()), tag
    for k in ("rel", "tile"):
        assert e[k] < BAR_INC[k], (tag, k, e)
        for c in e_cls:
            assert c[k] < BAR_CLASS[k], (tag, k, e_cls)
    assert e_xn < BAR_XN, (tag, e_xn)
    # sensitivity: every wrong variant of the reference lands >= 3 x beyond a bar (over all rows or in one row class)
    for v in ("no_bproj", "b2_tile", "eps", "drop_chunk", "xn_block"):
        vo, vxn = R.mlp_unit(x, att, p, p_next, variant=v, p_wrong=p_wrong)
        if v == "xn_block":
            worst = R.errors(vxn, xn_ref)["rel"] / BAR_XN
        else:
            d = vo - x.double()
            worst = max(max(R.errors(d, inc_ref)[k] / BAR_INC[k], *(R.errors(d[c], inc_ref[c])[k] / BAR_CLASS[k] for c in cls)) for k in ("rel", "tile"))
        print(f"   variant {v}: {worst:.1f} x the bar")
        assert worst >= 3.0, (tag, v, worst)
    return p


# (nseq, block, family, hidden): M = 257 nseq, M mod 128 = 16, 48, 112, 0, 16, 0; 2 048 patches = the production launch (power_legs)
CASES = ([(n, 5, "std", 1536) for n in (16, 48, 112, 128, 528, 2048)] + [(48, 0, "std", 1536), (48, 11, "std", 1536)]
         + [(48, 3, "edge", h) for h in (256, 640, 768, 1152, 1536)] + [(528, 5, "edge", 1536)])


@pytest.mark.parametrize("nseq,blk,family,hidden", CASES)
def test_mlp_unit_vs_bf16_emulation(nseq, blk, family, hidden):
    """hipt_vit_mlp_unit against the fp64 emulation: the standard synthetic ViT-256 at blocks 0 / 5 / 11 (11: xn_out is LN-1 of the block
    itself) over call sizes whose last 128-row tile is partial or whole; the edge weights at every hidden width (2 ... 12 chunks of 128: odd
    counts end the A0 / B1 pipeline differently); NaN canaries past row M of every buffer stay untouched."""
    depth = 12 if family == "std" else 6
    m, pk = model(family, hidden, depth)
    M = nseq * 257
    x, att, cls = inputs(M, nseq, 1000 + nseq + blk, m.blocks[blk].attn.proj.bias.detach())
    xo, xn, bufs = run_mlp(pk, blk, x, att, nseq)
    for b in bufs:
        assert canaries_intact(b, M)
    tag = f"mlp unit {family} hidden {hidden} block {blk} nseq {nseq} (M mod 128 = {M % 128})"
    p = check_against_reference(tag, m, blk, x, att, cls, nseq, xo, xn)
    if family == "edge":  # the inputs reach the GELU's branches: beyond the clamp, and the negative lobe
        h = R.mlp_preact(x, att, p)
        tail, neg = float((h.abs() > 8).double().mean()), float(((h >= -8) & (h <= -2)).double().mean())
        print(f"   fc1 pre-activations: |h| max {float(h.abs().max()):.1f}; beyond |8| {tail:.3f} (min {MIN_TAIL}), in [-8, -2] {neg:.3f} (min {MIN_NEG})")
        assert tail >= MIN_TAIL and neg >= MIN_NEG


def test_mlp_unit_invariants():
    """Bits that must not move: xn_out NULL / separate / aliased to the attention image (the header allows it); a workspace of 0xFF
    and one reused for a second launch (the tile-queue counter is reset by the launcher's memset and by the kernel itself); a patch at
    another position inside a 128-row tile (16 patches alone vs the same 16 at offset 16 of a 48-patch call)."""
    m, pk = model()
    nseq, blk = 48, 4
    M = nseq * 257
    x, att, _ = inputs(M, nseq, 77, m.blocks[blk].attn.proj.bias.detach())
    xo, xn, _ = run_mlp(pk, blk, x, att, nseq)
    xo0, xn0, _ = run_mlp(pk, blk, x, att, nseq, "none")
    xo1, xn1, bufs = run_mlp(pk, blk, x, att, nseq, "alias")
    assert xn0 is None and torch.equal(xo0, xo) and torch.equal(xo1, xo) and torch.equal(xn1, xn)
    assert canaries_intact(bufs[1], M)
    ws = torch.full((256,), 0xFF, dtype=torch.uint8, device=DEV)
    xo2, xn2, _ = run_mlp(pk, blk, x, att, nseq, ws=ws)
    xo3, xn3, _ = run_mlp(pk, blk, x, att, nseq, ws=ws)
    assert torch.equal(xo2, xo) and torch.equal(xn2, xn) and torch.equal(xo3, xo) and torch.equal(xn3, xn)
    r16 = slice(16 * 257, 32 * 257)
    xs, xns, _ = run_mlp(pk, blk, x[r16].contiguous(), att[r16].contiguous(), 16)
    assert torch.equal(xs, xo[r16]) and torch.equal(xns, xn[r16])
    print(f"\nmlp unit invariants: xn_out NULL / separate / aliased, 0xFF and reused workspace, 16 patches at offset 0 vs 16: bit-identical")


def test_mlp_unit_refusals():
    """HIPT_E_UNSUPPORTED for widths outside hipt_mlp16_supported (128, 1664), nseq * 257 not a multiple of 16, fp32 weights;
    HIPT_E_WORKSPACE for a workspace under 256 bytes or not 256-aligned.  Nothing is launched: the buffers keep their bits."""
    lib = N.lib()
    st = N.stream_ptr(torch.device(DEV))
    nseq = 16
    M = nseq * 257
    xb, ab = torch.zeros(M, 384, device=DEV), torch.zeros(M, 384, dtype=torch.bfloat16, device=DEV)
    ws = torch.zeros(1024, dtype=torch.uint8, device=DEV)
    call = lambda pk, n=nseq, w=N.ptr(ws), nb=256: lib.hipt_vit_mlp_unit(pk.ref, 0, N.ptr(xb), N.ptr(ab), n, None, w, nb, st)
    for hidden in (128, 1664):
        assert call(model("std", hidden, 1)[1]) == E_UNSUPPORTED, hidden
    assert call(model("std", 1536, 1, "fp32")[1]) == E_UNSUPPORTED
    pk = model("std", 1536, 1)[1]
    assert call(pk, n=1) == E_UNSUPPORTED and call(pk, n=17) == E_UNSUPPORTED  # 257, 4 369 rows
    assert call(pk, nb=128) == E_WORKSPACE
    assert call(pk, w=C.c_void_p(ws.data_ptr() + 16)) == E_WORKSPACE
    assert call(pk, w=None) == E_WORKSPACE
    torch.cuda.synchronize()
    assert not bool(xb.any()) and not bool(ab.any())
    assert call(pk) == 0  # (the same arguments with a valid workspace run)
    torch.cuda.synchronize()
    assert bool(xb.any())


# ---- one block through every route: hipt_vit_blocks(b, b + 1) via VisionTransformer._blocks ----------------------------------------
# (route, model, nseq, environment, fold, profile counts of the one-block call).  hipt_vit_blocks hands the block row-major fp32 x (activation
# images and the fused QKV + attention kernel are the whole-forward calls' and the units' above): nseq 16 (whole 16-row fragments) and 27
# (not) take the LayerNorm-chained streaming kernels with proj folded into the fused MLP; nseq 3 (771 rows <= 1 088) the small-call path;
# HIPT_GENERIC=1 and HIPT_NO_PROJ_FOLD=1 a separate proj launch whose bf16 y1 the MLP kernel adds (fold False); ViT-4K (D = 192, dh = 32):
# nseq 2 the small-call path (every one-region ViT-4K forward), nseq 6 the streaming kernels with mlp.hip launch<3> (booked as vit4k_blocks).
SMALL = {"qkv_gemm": 1, "attention": 1, "proj_gemm": 1, "fc1_gemm": 1, "fc2_gemm": 1}
STREAM_NOFOLD = {"qkv_gemm": 1, "attention": 1, "proj_gemm": 1, "mlp_fused": 1}
# bars (rel-L2, worst 16-column tile) = 2 x measured: chain 16 7.98e-4 / 8.20e-4, chain 27 7.96e-4 / 8.15e-4, small call 6.24e-4 / 6.48e-4,
# generic 8.32e-4 / 8.58e-4, no proj fold 8.87e-4 / 9.14e-4, ViT-4K small call 1.12e-4 / 1.24e-4, ViT-4K launch<3> 5.12e-4 / 5.24e-4
ROUTES = [
    ("chain_16", "vit256", 16, {}, True, {"qkv_gemm": 1, "attention": 1, "mlp_fused": 1}, (1.5e-3, 1.6e-3)),
    ("chain_rowmajor_27", "vit256", 27, {}, True, {"qkv_gemm": 1, "attention": 1, "mlp_fused": 1}, (1.5e-3, 1.6e-3)),
    ("small_call_3", "vit256", 3, {}, True, SMALL, (1.2e-3, 1.2e-3)),
    ("generic_16", "vit256", 16, {"HIPT_GENERIC": "1"}, False, STREAM_NOFOLD, (1.6e-3, 1.7e-3)),
    ("no_proj_fold_16", "vit256", 16, {"HIPT_NO_PROJ_FOLD": "1"}, False, STREAM_NOFOLD, (1.7e-3, 1.8e-3)),
    ("vit4k_small_call_2", "vit4k", 2, {}, True, SMALL, (2.2e-4, 2.4e-4)),
    ("vit4k_launch3_6", "vit4k", 6, {}, False, {"vit4k_blocks": 4}, (1.0e-3, 1.0e-3)),
]
_routes_seen = {}


def _vit_for(kind):
    key = ("route", kind)
    if key not in _models:
        if kind == "vit256":
            _models[key] = model()
        else:
            from hipt_abmil_atec23_amd.vision_transformer4k import vit4k_xs
            m = vit4k_xs(num_classes=0)
            m.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
            m = m.eval().to(DEV).set_compute_dtype("bf16")
            pk = m._tokens(synth.hash_uniform_torch((1, 384, 16, 16), 4, device=DEV))[0]
            _models[key] = (m, pk)
    return _models[key]


@pytest.mark.parametrize("route,kind,nseq,env,fold,counts,bars", ROUTES, ids=[r[0] for r in ROUTES])
def test_one_block_per_route_vs_bf16_emulation(monkeypatch, route, kind, nseq, env, fold, counts, bars):
    """The block increment of hipt_vit_blocks(b, b + 1) against tests/vit_bf16_ref.block with the route's own rounding points, the
    route asserted from the library's per-category launch counts (a switch that silently did nothing would show other counts), the
    emulation with the route's fold setting closer than the other one (the y1 rounding point is live and placed right), and the
    sensitivity variants >= 3 x beyond the bar."""
    m, pk = _vit_for(kind)
    blk = 3
    Dm = m.embed_dim
    assert pk.w.ntok == 257 and Dm == (384 if kind == "vit256" else 192) and Dm // m.blocks[blk].attn.num_heads == (64 if kind == "vit256" else 32)
    x0 = synth.hash_uniform_torch((nseq, 257, Dm), 300 + nseq, 2.0, device=DEV)
    x = x0.clone()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        N.profile_enable(True)
        before = N.calls
        m._blocks(pk, x, blk, blk + 1)
        torch.cuda.synchronize()
        pr = N.profile_read()
        N.profile_enable(False)
    finally:
        for k in env:
            monkeypatch.delenv(k, raising=False)
    assert N.calls == before + 1
    bar = {"rel": bars[0], "tile": bars[1]}
    got = {k: c for k, (_, c) in pr.items()}
    print(f"\nroute {route}: profile counts {got}")
    assert got == counts, (route, got)
    _routes_seen[route] = x.clone()
    x0r, p = x0.view(-1, Dm), R.block_params(m, blk)
    inc = x.view(-1, Dm).double() - x0r.double()
    inc_ref = R.block(x0r, p, nseq, fold=fold) - x0r.double()
    e, e_other = R.errors(inc, inc_ref), R.errors(inc, R.block(x0r, p, nseq, fold=not fold) - x0r.double())
    print(f"   block increment vs its emulation (fold {fold}): {_fmt(e)} (bars rel {bar['rel']:.1e} tile {bar['tile']:.1e}); "
          f"vs the other fold setting: rel {e_other['rel']:.2e}")
    assert bool(torch.isfinite(inc).all())
    assert e["rel"] < bar["rel"] and e["tile"] < bar["tile"], (route, e)
    assert e["rel"] < e_other["rel"], (route, e, e_other)
    for v in ("no_bproj", "b2_tile", "drop_chunk", "scale2", "mask_tile"):
        d = R.block(x0r, p, nseq, fold=fold, variant=v) - x0r.double()
        worst = max(R.errors(d, inc_ref)[k] / bar[k] for k in ("rel", "tile"))
        print(f"   variant {v}: {worst:.1f} x the bar")
        assert worst >= 3.0, (route, v, worst)
    # the two switches of the 16-patch streaming call change its bits (each takes a route of its own)
    if route in ("generic_16", "no_proj_fold_16") and "chain_16" in _routes_seen:
        assert not torch.equal(x, _routes_seen["chain_16"])
    if route == "no_proj_fold_16" and "generic_16" in _routes_seen:
        assert not torch.equal(x, _routes_seen["generic_16"])
