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


def _mm(a, b, mm=None):
    """a @ b in fp64, or with the product taken in dtype `mm` (the noise floor of the [CLS]-block tests: fp32 products of the same operands)"""
    return a @ b if mm is None else (a.to(mm) @ b.to(mm)).double()


def mlp_unit(x, att, p, p_next=None, rnd=True, fold=True, eps=LN_EPS, variant=None, p_wrong=None, rows=65536, mm=None):
    """hipt_vit_mlp_unit / the second half of Block.forward: x + att Wp^T + bp, then + fc2(GELU(fc1(LN2(.)))).  x fp32 / fp64 [M, 384]
    (the residual stream), att the attention output (bf16 values).  Returns (x_out, xn_out): xn_out = LayerNorm-1 of p_next (the next
    block, or the block itself after the last) of x_out, or None when p_next is None (variant "xn_block": of p_wrong instead).  fold=False: y1 = att Wp^T + bp is rounded to bf16
    before the residual add (the proj launch of HIPT_NO_PROJ_FOLD=1 and of the generic route writes y1 in bf16, seqgemm's output).
    Row blocks of `rows` keep the fp64 hidden tensor small at 2 048 patches.  mm: see _mm."""
    r = bf16 if rnd else _id
    outs, xns = [], []
    for s in range(0, x.shape[0], rows):
        xs, ats = x[s:s + rows].double(), att[s:s + rows].double()
        y1 = _mm(ats, p["proj_w"].t(), mm) + (0.0 if variant == "no_bproj" else p["proj_b"])
        v = xs + (y1 if fold else r(y1))
        ln2 = r(layer_norm(v, p["ln2_w"], p["ln2_b"], 1e-5 if variant == "eps" else eps))  # mlp16.hip:636 (row phase: LN-2 -> bf16 fc1 operand)
        h = _mm(ln2, p["fc1_w"].t(), mm) + p["fc1_b"]
        if variant == "drop_chunk":
            h[:, 128:256] = 0.0  # (GELU(0) = 0: hidden chunk 1 contributes nothing)
        g = r(gelu(h))  # mlp16.hip:327 (GELU'd fc1 accumulators -> bf16 fc2 operand)
        b2 = p["fc2_b"].clone()
        if variant == "b2_tile":
            b2[48:64] = 0.0  # (output tile 3 without its bias)
        xo = v + _mm(g, p["fc2_w"].t(), mm) + b2
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


# ---- the [CLS]-pruned last block (capi.hip, run_last_block_cls) ----------------------------------------------------------------------
CLS_ROUTES = ("absorb", "fused_cls", "two_kernel")  # default | HIPT_NO_CLS_ABSORB=1 | HIPT_NO_FUSED_ATTN=1
# plausible wrong kernels of the block; a route lists the ones that have a counterpart in its launch sequence (the two-kernel route has
# no per-wave merge, only the absorbed one carries u)
CLS_VARIANTS = {
    "absorb": ("scale2", "mask_tile", "drop_last_token", "no_bv", "no_merge_rescale", "wave0_four_blocks", "u_one_bf16", "no_bproj"),
    "fused_cls": ("scale2", "mask_tile", "drop_last_token", "no_bv", "no_merge_rescale", "wave0_four_blocks", "no_bproj"),
    "two_kernel": ("scale2", "mask_tile", "drop_last_token", "no_bv", "no_bproj"),
}
CLS_CLASSES = ("top256", "wave_first", "ascending", "descending", "equal", "plain")


def cls_pool_schedule():
    """cls_pool_kernel's schedule (cls_pool.hip:63, 76): (block of every token [257], the blocks of each wave in the order it takes
    them).  17 blocks of 16 tokens, the last holds token 256 alone; wave w owns blocks 4w .. 4w+3, wave 0 block 16 as well, last."""
    tok_blk = torch.arange(NTOK) // 16
    waves = [[4 * w + i for i in range(4)] + ([16] if w == 0 else []) for w in range(4)]
    return tok_blk, waves


def fused_cls_groups():
    """qkv_attention.hip's [CLS]-only form (:508-529): wave w of eight scores the [CLS] query against key tile w = tokens 32w+1 ..
    32w+32; the [CLS] key itself (tile 8, token 0) is wave 0's share.  -> wave of every token [257]"""
    g = (torch.arange(NTOK) - 1).clamp(min=0) // 32
    return g


def cls_running_max(s):
    """absorbed route: for scores s [..., 257] the running maximum m_blk(j) the kernel holds when it rounds p_j (the wave's maximum
    over its blocks up to and including the block of token j, cls_pool.hip:135), and the block maxima [..., 17]"""
    tok_blk, waves = cls_pool_schedule()
    pad = torch.full(s.shape[:-1] + (17 * 16 - NTOK,), -math.inf, dtype=s.dtype, device=s.device)
    bm = torch.cat([s, pad], -1).reshape(s.shape[:-1] + (17, 16)).amax(-1)
    run = torch.empty_like(bm)
    for blks in waves:
        run[..., blks] = torch.cummax(bm[..., blks], -1).values
    return run[..., tok_blk.to(s.device)], bm


def _cls_q(xc, p, r, mm):
    """the Q rows of the [CLS] tokens: every route's side GEMM writes them in bf16 (gemm.hip:89 / the seqgemm's bf16 output)"""
    Dm = xc.shape[-1]
    return r(_mm(xc, p["qkv_w"][:Dm].t(), mm) + p["qkv_b"][:Dm])


def cls_absorb_scores(xs, q, p, rnd=True, variant=None, mm=None):
    """scale * xn . u of the absorbed route for xs [n, 257, D] (fp64) and q [n, D]: u = fp32(q Wu^T) (gemm.hip:87, HIPT_EPI_OUT_F32)
    carried as a hi + lo bf16 pair (cls_pool.hip:91-102; u_one_bf16: hi alone) -> [n, H, 257]"""
    n, _, Dm = xs.shape
    H = p["heads"]
    dh = Dm // H
    wk = p["qkv_w"][Dm:2 * Dm].view(H, dh, Dm)
    u = _mm(q.view(n, H, 1, dh).transpose(0, 1), wk.unsqueeze(1), mm).transpose(0, 1).reshape(n, H, Dm)  # u_h = Wk_h^T q_h
    if rnd:
        u = u.float().double()
        hi = bf16(u)
        u = hi if variant == "u_one_bf16" else hi + bf16(u - hi)
    sc = p["scale"] * (p["scale"] if variant == "scale2" else 1.0)
    return _mm(u, xs.transpose(1, 2), mm) * sc  # cls_pool.hip:118-130


def cls_block(xn, x_cls, p, nseq, route, rnd=True, variant=None, mm=None, seqs=64):
    """hipt_vit_cls_block_unit: the last block for the [CLS] rows only.  xn [nseq * 257, D] = LayerNorm-1 of the block's input (bf16
    values), x_cls [nseq, D] the residual rows of the [CLS] tokens -> (att_rows [nseq, D] before proj, xc [nseq, D] the final
    residual rows).  fp64 with bf16 where the route rounds:

    absorb      q -> bf16; u -> fp32 -> hi + lo; score = scale * xn . u; the kernel's online softmax restated: with m_blk(j) the
                running maximum of token j's wave including j's block, M the patch maximum,
                    p_eff_j = bf16(exp(s_j - m_blk(j))) * exp(m_blk(j) - M)
                (cls_pool.hip:141 rounds, :146-149 rescale the wave's sum and pooled rows by exp(m_old - m_new) in fp32, :181-183
                weight the four partials by exp(m_w - M)); the row sum adds the ROUNDED values (:142); z = bf16(sum_j p_eff_j xn_j / L)
                (:185-186); o = bf16(z Wo^T + bv) (gemm.hip:89)
    fused_cls   q | k | v -> bf16 (qkv_attention.hip:346-359; the [CLS] row's from the side GEMM); wave g of eight takes its 32 keys
                (wave 0: + the [CLS] key) against ITS OWN maximum m_g: e_j = exp(scale (s_j - m_g)) (:538), the sum l_g adds the
                UNROUNDED e (:539), the P V operand is bf16(e) (:545); merge: weights exp(scale (m_g - M)) (:275-277); o = bf16(O / L) (:283)
    two_kernel  q | k | v -> bf16 (the seqgemm's output); one maximum, e = exp(s - m) and the P V sum in fp32 throughout -- P is NOT
                rounded (misc.hip:232, :257); o = bf16(O / l) (misc.hip:269)
    then on every route y1 = bf16(o Wp^T + bp) (gemm.hip:89) and the fused MLP without the fold on the compact rows (mlp_unit,
    fold=False: hipt_mlp_launch with y1, no image).  rnd=False: the plain fp64 block.  variant: one of CLS_VARIANTS[route]."""
    if variant is not None and variant not in CLS_VARIANTS[route]:
        raise ValueError(f"variant {variant} has no counterpart on route {route}")
    r = bf16 if rnd else _id
    Dm = xn.shape[-1]
    H = p["heads"]
    dh = Dm // H
    ntok = xn.shape[0] // nseq
    assert ntok == NTOK
    dev = xn.device
    bv = p["qkv_b"][2 * Dm:]
    sc2 = p["scale"] if variant == "scale2" else 1.0
    out = []
    for s0 in range(0, nseq, seqs):
        n = min(seqs, nseq - s0)
        xs = xn[s0 * ntok:(s0 + n) * ntok].double().view(n, ntok, Dm)
        q = _cls_q(xs[:, 0], p, r, mm)
        if route == "absorb":
            s = cls_absorb_scores(xs, q, p, rnd, variant, mm)
            if variant == "mask_tile":
                s[..., 16:32] = -math.inf  # (tokens 16 .. 31 masked)
            if variant == "drop_last_token":
                s[..., 256] = -math.inf  # (block 16 masked: 16 kb + 4 g + r < 256)
            M = s.amax(-1, keepdim=True)
            mb = cls_running_max(s)[0] if rnd else M.expand_as(s)
            pj = r(torch.exp(s - mb))  # cls_pool.hip:141
            wgt = pj * torch.exp(mb - M)
            if variant == "no_merge_rescale":  # (wave 2's partial enters the merge without exp(m_w - M))
                mw = s[..., 128:192].amax(-1, keepdim=True)
                wgt[..., 128:192] = pj[..., 128:192] * torch.exp(mb[..., 128:192] - mw)
            L = wgt.sum(-1, keepdim=True)  # :142-146: the sum of the rounded values
            if variant == "wave0_four_blocks":
                wgt = wgt.clone()
                wgt[..., 256] = 0.0  # (wave 0 pools four blocks: token 256 is in the row sum, its row never reaches Z)
            z = r(_mm(wgt, xs, mm) / L)  # :185-186
            wv = p["qkv_w"][2 * Dm:].view(H, dh, Dm)
            o = _mm(z.transpose(0, 1), wv.transpose(1, 2), mm).transpose(0, 1).reshape(n, Dm)  # o_h = Wv_h z_h
            att = r(o + (0.0 if variant == "no_bv" else bv))  # gemm.hip:89
        else:
            kv = _mm(xs.reshape(n * ntok, Dm), p["qkv_w"][Dm:].t(), mm) + p["qkv_b"][Dm:]
            if variant == "no_bv":
                kv[:, Dm:] -= bv
            kv = r(kv).view(n, ntok, 2, H, dh).permute(2, 0, 3, 1, 4)  # qkv_attention.hip:346-359 / the K | V GEMM's bf16 output
            s = _mm(q.view(n, H, 1, dh), kv[0].transpose(-1, -2), mm).squeeze(2) * (p["scale"] * sc2)
            if variant == "mask_tile":
                s[..., 16:32] = -math.inf
            if variant == "drop_last_token":
                s[..., 256] = -math.inf
            M = s.amax(-1, keepdim=True)
            if route == "fused_cls" and rnd:
                g = fused_cls_groups().to(dev)
                mg = torch.full(s.shape[:-1] + (8,), -math.inf, dtype=s.dtype, device=dev).scatter_reduce(-1, g.expand_as(s), s, "amax")
                mg = torch.where(torch.isinf(mg), M, mg)  # (a wave whose keys are all masked: the variants only)
                mt = mg[..., g]
                e = torch.exp(s - mt)  # qkv_attention.hip:538
                f = torch.exp(mt - M)  # :275
                if variant == "no_merge_rescale":
                    f = f.clone()
                    f[..., g == 2] = 1.0  # (wave 2's partial enters the merge unweighted)
                pe = r(e) * f  # :545
                L = (e * f).sum(-1, keepdim=True)  # :539: the unrounded values
                if variant == "wave0_four_blocks":
                    pe[..., 0] = 0.0  # (wave 0 without its extra share, the [CLS] key, in P V; still in the sum)
            else:
                pe = torch.exp(s - M)  # misc.hip:232: fp32, never rounded
                L = pe.sum(-1, keepdim=True)
                if variant == "wave0_four_blocks":
                    pe[..., 0] = 0.0
            o = _mm(pe.unsqueeze(2), kv[1], mm).squeeze(2) / L
            att = r(o.reshape(n, Dm))  # qkv_attention.hip:283 / misc.hip:269
        out.append(att)
    att = torch.cat(out)
    xc = mlp_unit(x_cls, att, p, None, rnd=rnd, fold=False, variant=variant if variant == "no_bproj" else None, mm=mm)[0]
    return att, xc


# ---- inputs of the [CLS]-block tests ------------------------------------------------------------------------------------------
def cls_inputs(p, nseq, seed, device="cpu", outlier_rows=False):
    """Residual stream x fp32 [nseq * 257, D] and xn = bf16(LayerNorm-1(x)) with the weights' own affine (LayerNorm-output
    statistics: the outlier family's gains 0.05 .. 20 are in them), patch i of class CLS_CLASSES[i % 6].  A class is a
    permutation of the non-[CLS] rows of its patch (q does not change) by the emulation's own head-0 scores of the absorbed route:
      top256      the top-scoring row at token 256 (block 16, wave 0's fifth block, raises the maximum last)
      wave_first  the four top-scoring rows at tokens 64, 128, 192 (the first row of waves 1 .. 3) and 1 (wave 0's is the [CLS] row)
      ascending   rows 1 .. 256 in ascending score order, the 16 top rows as the last rows of blocks 1 .. 16: every block raises its
                  wave's running maximum
      descending  in descending order: no block after a wave's first raises it
      equal       all 257 rows equal row 0: p = 1 everywhere, z is that row
      plain       as drawn
    outlier_rows: four residual channels at +-60 .. 100 in every row of every second patch (synth.apply_vit_outliers_np's magnitudes).
    -> dict x, xn (torch.bfloat16), x_cls [nseq, D] fp32, classes {name: patch indices}, s0 [nseq, 257] (head-0 scores, after)"""
    from hipt_abmil_atec23_amd import synth
    M = nseq * NTOK
    x = synth.hash_uniform_torch((M, D), seed, 2.0, device=device)
    if outlier_rows:
        ch = torch.tensor([7, 100, 200, 333], device=device)
        big = torch.tensor([60.0, -75.0, 90.0, -100.0], device=device)
        xv = x.view(nseq, NTOK, D)
        xv[1::2][:, :, ch] = big * (1.0 + 0.1 * xv[1::2][:, :, ch])
    x = x.view(nseq, NTOK, D)
    cls = torch.arange(nseq, device=device) % len(CLS_CLASSES)
    x[cls == 4] = x[cls == 4][:, :1].expand(-1, NTOK, -1).clone()

    def scores(xv):
        out = []
        for s0 in range(0, nseq, 64):
            xs = bf16(layer_norm(xv[s0:s0 + 64].double(), p["ln1_w"], p["ln1_b"]))
            out.append(cls_absorb_scores(xs, _cls_q(xs[:, 0], p, bf16, None), p)[:, 0])
        return torch.cat(out)

    s = scores(x)[:, 1:]  # non-[CLS] rows
    order = torch.argsort(s, -1)  # ascending
    perm = torch.arange(256, device=device).repeat(nseq, 1)  # new row 1 + j <- old row 1 + perm[j]
    # ascending: the 16 top rows close blocks 1 .. 16 in ascending order (tokens 31, 47, .. 255, 256), the other 240 fill the rest in
    # ascending order -- every block then raises the maximum even where the [CLS] row's own score is not the patch's lowest
    carrier = torch.tensor([16 * b + 14 for b in range(1, 16)] + [255], device=device)
    fill = torch.ones(256, dtype=torch.bool, device=device)
    fill[carrier] = False
    asc = torch.empty_like(order)
    asc[:, carrier] = order[:, 240:]
    asc[:, fill] = order[:, :240]
    perm[cls == 2] = asc[cls == 2]
    perm[cls == 3] = order[cls == 3].flip(-1)
    for c, dst in ((0, (255,)), (1, (63, 127, 191, 0))):
        for i in torch.nonzero(cls == c).flatten().tolist():
            for k, d in enumerate(dst):
                src = int(order[i, 255 - k])
                j = int(torch.nonzero(perm[i] == src).flatten()[0])
                perm[i, j], perm[i, d] = perm[i, d].clone(), perm[i, j].clone()
    rows = torch.cat([torch.zeros(nseq, 1, dtype=torch.int64, device=device), 1 + perm], 1)
    x = torch.gather(x, 1, rows[..., None].expand(-1, -1, D)).contiguous()
    xn = torch.empty(M, D, dtype=torch.bfloat16, device=device)
    for s0 in range(0, nseq, 64):
        blk = bf16(layer_norm(x[s0:s0 + 64].double(), p["ln1_w"], p["ln1_b"]))
        xn[s0 * NTOK:(s0 + blk.shape[0]) * NTOK] = blk.reshape(-1, D).bfloat16()
    classes = {name: torch.nonzero(cls == k).flatten() for k, name in enumerate(CLS_CLASSES)}
    return {"x": x.view(M, D), "xn": xn, "x_cls": x[:, 0].contiguous(), "classes": classes, "s0": scores(x)}


def cls_errors(att, att_ref, xc, xc_ref, x_cls, classes) -> dict:
    """The metrics of the [CLS]-block tests.  att rows: rel-L2, the worst head (64 columns), the worst patch class; the increment
    xc - x_cls: rel-L2, the worst 16-column tile (errors()), the worst patch class."""
    rl = lambda a, b: float((a - b).norm() / b.norm())
    a, ar = att.double(), att_ref.double()
    inc, incr = xc.double() - x_cls.double(), xc_ref.double() - x_cls.double()
    e = errors(inc, incr)
    out = {"att_rel": rl(a, ar), "att_head": max(rl(a[:, 64 * h:64 * h + 64], ar[:, 64 * h:64 * h + 64]) for h in range(a.shape[1] // 64)),
           "inc_rel": e["rel"], "inc_tile": e["tile"]}
    per = {k: (rl(a[i], ar[i]), rl(inc[i], incr[i])) for k, i in classes.items() if len(i)}
    out["att_class"] = max(v[0] for v in per.values())
    out["inc_class"] = max(v[1] for v in per.values())
    out["per_class"] = per
    return out


CLS_METRICS = ("att_rel", "att_head", "att_class", "inc_rel", "inc_tile", "inc_class")


def cls_seed(nseq):
    return 500 + nseq


def cls_assert_edges(c, p, nseq, family):
    """the inputs of a case reach the edges they are built for (head-0 scores of the absorbed route; all heads for the magnitude)"""
    s0, cl = c["s0"], c["classes"]
    _, bm = cls_running_max(s0)
    # top256: token 256 tops the rows that can move (1 .. 256) in every patch, and the whole patch unless the [CLS] row's own score does
    t = s0[cl["top256"]]
    assert bool((t[:, 1:].argmax(-1) == 255).all()) and int(t[0].argmax()) == 256 and float((t.argmax(-1) == 256).double().mean()) >= 0.75, "top256"
    top4 = torch.topk(s0[cl["wave_first"]][:, 1:], 4, -1).indices + 1
    assert bool((top4 == torch.tensor([64, 128, 192, 1], device=s0.device)).all()), "wave_first"
    # ascending: blocks 1 .. 16 raise the maximum in every patch; block 0 holds the [CLS] row, whose own score is among the patch's 16
    # largest in about one patch of 16, and block 1 cannot top it there: most patches, and the first one, have all 17 in order
    up = bm[cl["ascending"]].diff(dim=-1) > 0
    assert bool(up[:, 1:].all()) and bool(up[0].all()) and float(up.all(-1).double().mean()) >= 0.75, "ascending: every block raises the maximum"
    assert bool((bm[cl["descending"]][:, 1:].diff(dim=-1) < 0).all()), "descending"
    tok_blk, waves = cls_pool_schedule()
    for w in waves:  # (no block after a wave's first raises its running maximum)
        assert bool((bm[cl["descending"]][:, w[1:]] < bm[cl["descending"]][:, w[:1]]).all()), "descending"
    xe = c["xn"].view(nseq, NTOK, D)[cl["equal"]]
    assert bool((xe == xe[:, :1]).all()), "equal"
    if family == "outlier":
        smax = 0.0
        for s in range(0, nseq, 64):
            xs = c["xn"][s * NTOK:(s + 64) * NTOK].double().view(-1, NTOK, D)
            smax = max(smax, float(cls_absorb_scores(xs, _cls_q(xs[:, 0], p, bf16, None), p).abs().max()))
        assert smax > 30.0, smax
        return smax
    return None


# The noise floor of cls_block: the largest distance, per (route, family) and metric of cls_errors, between the emulation with fp64
# products and with fp32 products (tests/test_vit_bf16_ref.py, test_cls_block_noise_floor: 16 and 48 patches on every route, 528 on
# the absorbed one).  The bars of tests/test_gpu_cls_block_unit.py are CLS_BAR_FACTOR times these.
CLS_BAR_FACTOR = 4.0
CLS_FLOOR = {
    ('absorb', 'std'): {"att_rel": 9.62e-05, "att_head": 1.77e-04, "att_class": 4.14e-04, "inc_rel": 4.19e-04, "inc_tile": 5.68e-04, "inc_class": 9.99e-04},
    ('fused_cls', 'std'): {"att_rel": 5.43e-05, "att_head": 1.02e-04, "att_class": 2.86e-04, "inc_rel": 2.87e-04, "inc_tile": 3.45e-04, "inc_class": 6.93e-04},
    ('two_kernel', 'std'): {"att_rel": 4.36e-05, "att_head": 8.20e-05, "att_class": 2.05e-04, "inc_rel": 3.33e-04, "inc_tile": 4.27e-04, "inc_class": 6.35e-04},
    ('absorb', 'outlier'): {"att_rel": 1.39e-04, "att_head": 3.58e-04, "att_class": 4.72e-04, "inc_rel": 4.72e-04, "inc_tile": 9.85e-04, "inc_class": 8.68e-04},
    ('fused_cls', 'outlier'): {"att_rel": 8.34e-05, "att_head": 1.97e-04, "att_class": 1.99e-04, "inc_rel": 3.38e-04, "inc_tile": 9.08e-04, "inc_class": 6.84e-04},
    ('two_kernel', 'outlier'): {"att_rel": 8.90e-05, "att_head": 2.61e-04, "att_class": 1.63e-04, "inc_rel": 4.01e-04, "inc_tile": 8.99e-04, "inc_class": 7.09e-04},
}
