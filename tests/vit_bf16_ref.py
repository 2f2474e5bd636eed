"""fp64 restatement of one ViT-256 block (vision_transformer.py:119-152) with the bf16 mode's rounding points made explicit: the
reference of the per-unit tests (tests/test_gpu_vit_units.py), and the activation-image converters those tests share.

Arithmetic is float64 on whatever device the inputs live on; a value is rounded to bf16 (``bf16``: round-to-nearest-even of its
fp32 value, what ``pack_bf16x2`` does, csrc/common.h:57) exactly where the kernels round it, and nowhere else.  ``rnd=False``
switches every rounding point off: the plain fp64 block (oracle/hipt_oracle.py), which the CPU tests hold it to.  GELU is the
exact erf form (nn.GELU()); the kernels' approximations (mlp_common.h gelu1s, |err| <= 2.6e-5) are part of what the tests
measure, not of the reference.

``variant`` names a plausible wrong kernel (the sensitivity self-checks of the unit tests): the reference with that one
mistake, which each test must reject at its bar."""
import math

import torch

LN_EPS = 1e-6
D, NTOK = 384, 257


# ---- bf16 rounding ----------------------------------------------------------------------
def bf16(t: torch.Tensor) -> torch.Tensor:
    """Round to bf16 (nearest, ties to even) and return in t's dtype: fp64 -> fp32 first (the kernels round fp32 values), then
    the upper 16 bits with the carry of the lower 16 (NaN stays NaN)."""
    f = t.float().contiguous()
    u = f.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    r = torch.where(torch.isnan(f), u | 0x400000, r) & 0xFFFF0000
    return (r - ((r >> 31) << 32)).to(torch.int32).view(torch.float32).to(t.dtype)


def _id(t):
    return t


# ---- activation images (csrc/kernels.h:74-80) -------------------------------------------------
# bf16: element (row 16 F + i, column 8 (g + 4 c) + e) at F * 6144 + c * 512 + (16 g + i) * 8 + e
# fp32: element (row 16 F + i, column 8 (g + 4 c) + 4 h + e) at F * 6144 + c * 512 + h * 256 + (16 g + i) * 4 + e
def to_image(x: torch.Tensor) -> torch.Tensor:
    """[M, 384] row-major -> the bf16 activation-image order (any dtype; M % 16 == 0)"""
    m = x.shape[0]
    return x.reshape(m // 16, 16, 12, 4, 8).permute(0, 2, 3, 1, 4).contiguous().view(m, D)


def from_image(img: torch.Tensor) -> torch.Tensor:
    m = img.shape[0]
    return img.reshape(m // 16, 12, 4, 16, 8).permute(0, 3, 1, 2, 4).contiguous().view(m, D)


def to_image_f32(x: torch.Tensor) -> torch.Tensor:
    """[M, 384] row-major -> the fp32 activation-image order (the residual stream hipt_vit_mlp_unit updates)"""
    m = x.shape[0]
    return x.reshape(m // 16, 16, 12, 4, 2, 4).permute(0, 2, 4, 3, 1, 5).contiguous().view(m, D)


def from_image_f32(img: torch.Tensor) -> torch.Tensor:
    m = img.shape[0]
    return img.reshape(m // 16, 12, 2, 4, 16, 4).permute(0, 4, 1, 3, 2, 5).contiguous().view(m, D)


# ---- weights --------------------------------------------------------------------------------
def block_params(model, i: int, device=None) -> dict:
    """fp64 tensors of block i of a ViT module: matrices as the bf16 the kernels read (hipt_vit_pack_weights packs the bf16 copy;
    the fused MLP's W1 / 8 and 8 W2 are exact rescalings of it), biases and LayerNorm affines as fp32 -> fp64."""
    b = model.blocks[i]
    dev = device if device is not None else b.mlp.fc1.weight.device
    m = lambda t: t.detach().to(dev).bfloat16().double()
    v = lambda t: t.detach().to(dev).double()
    return {"ln1_w": v(b.norm1.weight), "ln1_b": v(b.norm1.bias), "qkv_w": m(b.attn.qkv.weight), "qkv_b": v(b.attn.qkv.bias),
            "proj_w": m(b.attn.proj.weight), "proj_b": v(b.attn.proj.bias), "ln2_w": v(b.norm2.weight), "ln2_b": v(b.norm2.bias),
            "fc1_w": m(b.mlp.fc1.weight), "fc1_b": v(b.mlp.fc1.bias), "fc2_w": m(b.mlp.fc2.weight), "fc2_b": v(b.mlp.fc2.bias),
            "heads": b.attn.num_heads, "scale": float(b.attn.scale)}


def params_from_dict(p: dict, i: int, heads: int, device="cpu", rnd: bool = True) -> dict:
    """The same from a state dict / oracle parameter dict (numpy or torch, names blocks.{i}.*)"""
    t = lambda k: torch.as_tensor(p[f"blocks.{i}.{k}"]).to(device).double()
    m = (lambda k: bf16(t(k))) if rnd else t
    dh = t("norm1.weight").shape[0] // heads
    return {"ln1_w": t("norm1.weight"), "ln1_b": t("norm1.bias"), "qkv_w": m("attn.qkv.weight"), "qkv_b": t("attn.qkv.bias"),
            "proj_w": m("attn.proj.weight"), "proj_b": t("attn.proj.bias"), "ln2_w": t("norm2.weight"), "ln2_b": t("norm2.bias"),
            "fc1_w": m("mlp.fc1.weight"), "fc1_b": t("mlp.fc1.bias"), "fc2_w": m("mlp.fc2.weight"), "fc2_b": t("mlp.fc2.bias"),
            "heads": heads, "scale": dh ** -0.5}


# ---- the operations -----------------------------------------------------------------------------
def layer_norm(x, w, b, eps=LN_EPS):
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    return xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps) * w + b


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def mlp_preact(x, att, p, rnd=True):
    """fc1 pre-activations of the fused MLP for rows x / att (for the coverage assertions: where the GELU's branches are reached)"""
    r = bf16 if rnd else _id
    v = x.double() + att.double() @ p["proj_w"].t() + p["proj_b"]
    return r(layer_norm(v, p["ln2_w"], p["ln2_b"])) @ p["fc1_w"].t() + p["fc1_b"]


def mlp_unit(x, att, p, p_next=None, rnd=True, fold=True, eps=LN_EPS, variant=None, p_wrong=None, rows=65536):
    """hipt_vit_mlp_unit / the second half of Block.forward: x + att Wp^T + bp, then + fc2(GELU(fc1(LN2(.)))).  x fp32 / fp64 [M, 384]
    (the residual stream), att the attention output (bf16 values).  Returns (x_out, xn_out): xn_out = LayerNorm-1 of p_next (the next
    block, or the block itself after the last) of x_out, or None when p_next is None (variant "xn_block": of p_wrong instead).  fold=False: y1 = att Wp^T + bp is rounded to bf16
    before the residual add (the proj launch of HIPT_NO_PROJ_FOLD=1 and of the generic route writes y1 in bf16, seqgemm's output).
    Row blocks of `rows` keep the fp64 hidden tensor small at 2 048 patches."""
    r = bf16 if rnd else _id
    outs, xns = [], []
    for s in range(0, x.shape[0], rows):
        xs, ats = x[s:s + rows].double(), att[s:s + rows].double()
        y1 = ats @ p["proj_w"].t() + (0.0 if variant == "no_bproj" else p["proj_b"])
        v = xs + (y1 if fold else r(y1))
        ln2 = r(layer_norm(v, p["ln2_w"], p["ln2_b"], 1e-5 if variant == "eps" else eps))  # mlp16.hip:636 (row phase: LN-2 -> bf16 fc1 operand)
        h = ln2 @ p["fc1_w"].t() + p["fc1_b"]
        if variant == "drop_chunk":
            h[:, 128:256] = 0.0  # (GELU(0) = 0: hidden chunk 1 contributes nothing)
        g = r(gelu(h))  # mlp16.hip:327 (GELU'd fc1 accumulators -> bf16 fc2 operand)
        b2 = p["fc2_b"].clone()
        if variant == "b2_tile":
            b2[48:64] = 0.0  # (output tile 3 without its bias)
        xo = v + g @ p["fc2_w"].t() + b2
        outs.append(xo)
        if p_next is not None:
            q = p_wrong if variant == "xn_block" else p_next
            ln = q["ln1_w"], q["ln1_b"]
            xns.append(r(layer_norm(xo, *ln, eps)))  # mlp16.hip:781 (epilogue: LN-1 of the next block -> bf16 image)
    return torch.cat(outs), (torch.cat(xns) if p_next is not None else None)


def attention_unit(xn, p, nseq, rnd=True, variant=None, seqs=32):
    """hipt_vit_attention_unit: softmax(q k^T * scale) v per head from xn = LayerNorm-1(x) (bf16 values) [nseq * ntok, D] -> [nseq * ntok, D]
    before proj, with the kernels' rounding: q | k | v -> bf16, the UNNORMALISED probabilities exp(s - max) -> bf16 as the P V operand
    while the row sum l adds the unrounded ones, the 1 / l after P V, the output -> bf16.  Groups of `seqs` sequences."""
    r = bf16 if rnd else _id
    M, Dm = xn.shape
    ntok = M // nseq
    H = p["heads"]
    dh = Dm // H
    out = []
    for s0 in range(0, nseq, seqs):
        ns = min(seqs, nseq - s0)
        x = xn[s0 * ntok:(s0 + ns) * ntok].double()
        qkv = r(x @ p["qkv_w"].t() + p["qkv_b"])  # qkv_attention.hip:345-361 (fused) / the QKV GEMM's bf16 output (two kernels): q | k | v -> bf16
        qkv = qkv.view(ns, ntok, 3, H, dh).permute(2, 0, 3, 1, 4)
        sc = p["scale"] * (p["scale"] if variant == "scale2" else 1.0)
        s = (qkv[0] @ qkv[1].transpose(-1, -2)) * sc
        if variant == "mask_tile":
            s[..., 16:32] = -math.inf  # (key tile 1 masked)
        e = torch.exp(s - s.amax(-1, keepdim=True))
        l = e.sum(-1, keepdim=True)
        o = (r(e) @ qkv[2]) / l  # attention.hip:152 / qkv_attention.hip:680: P -> bf16 before normalisation; 1 / l at attention.hip:192 / qkv_attention.hip:707
        out.append(r(o.transpose(1, 2).reshape(ns * ntok, Dm)))  # qkv_attention.hip:707 / attention.hip:192: output -> bf16
    return torch.cat(out)


def block(x, p, nseq, rnd=True, fold=True, eps=LN_EPS, variant=None):
    """One whole block (Block.forward :146-152) on fp32 / fp64 x [nseq * ntok, D] (D = 384 or 192): LN-1 -> bf16 (every route hands the
    attention a bf16 LN-1 operand: the GEMM prologues' pack, gemm.hip:415, the layernorm kernel's bf16 output, mlp16.hip:781 of the block
    before), the attention unit, then the MLP unit; fold as in mlp_unit.  `variant` is one name of EITHER unit (no_bproj, b2_tile, eps,
    drop_chunk of mlp_unit; scale2, mask_tile of attention_unit): it is passed to both and the unit that does not know it ignores it."""
    r = bf16 if rnd else _id
    xn = r(layer_norm(x.double(), p["ln1_w"], p["ln1_b"], eps))
    att = attention_unit(xn, p, nseq, rnd=rnd, variant=variant)
    return mlp_unit(x, att, p, None, rnd=rnd, fold=fold, eps=eps, variant=variant)[0]


def errors(got: torch.Tensor, ref: torch.Tensor) -> dict:
    """rel-L2, the largest rel-L2 of one 16-column output tile (where a per-tile mistake shows undiluted) and max-abs / max |ref|"""
    d = got.double() - ref.double()
    ref = ref.double()
    nt = ref.shape[-1] // 16
    tiles = (d.reshape(-1, nt, 16).square().sum((0, 2)) / ref.reshape(-1, nt, 16).square().sum((0, 2))).sqrt()
    return {"rel": float(d.norm() / ref.norm()), "tile": float(tiles.max()), "max": float(d.abs().max() / ref.abs().max())}
