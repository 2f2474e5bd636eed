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
    """a @ b in fp64, or with the product taken in dtype `mm` (the noise floor of the [CLS]-block tests: fp32 products of the same operands).
    mm = "f32k16": fp32 accumulation in a FIXED order -- the sum over each run of 16 k (one MFMA k-step) is taken in fp64, which is exact
    for bf16 operands, rounded to fp32 and added to an fp32 accumulator run after run.  No BLAS summation order enters the result."""
    if mm is None:
        return a @ b
    if mm != "f32k16":
        return (a.to(mm) @ b.to(mm)).double()
    acc = None
    for k0 in range(0, a.shape[-1], 16):
        part = (a[..., k0:k0 + 16] @ b[..., k0:k0 + 16, :]).float()
        acc = part if acc is None else acc + part
    return acc.double()


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


# ---- the attention unit (capi.hip, hipt_vit_attention_unit) ----------------------------------------------------------------------
ATT_ROUTES = ("fused", "two_kernel")  # fused = 1: [CLS]-row gather + side GEMM + qkv_attn_kernel<0> | fused = 0: QKV GEMM (head-major) + attn64_kernel
# plausible wrong kernels; a route lists the ones that have a counterpart in its launch sequence (the work-unit schedule, the lane
# halves of the 32 x 32 score tiles, the V sub-images, key tile 8 and the [CLS] merge are the fused kernel's alone)
ATT_VARIANTS = {
    "fused": ("scale2", "mask_tile", "pad_unmasked", "drop_cls_key", "drop_last_token", "half_max", "no_bq", "no_bv", "v_dtile_swap",
              "head_bias_next", "stale_cls_row", "prev_patch_rows", "no_merge_rescale", "last_merge_dropped"),
    "two_kernel": ("scale2", "mask_tile", "pad_unmasked", "drop_last_token", "no_bq", "no_bv", "head_bias_next"),
}
# variants that need a workgroup with that many work units to differ from the emulation (qkv_attn_schedule()["max_units"])
ATT_VARIANT_UNITS = {"stale_cls_row": 3, "prev_patch_rows": 2}
ATT_PAD_KEYS = {"fused": 31, "two_kernel": 15}  # key tile 8 = the [CLS] key + 31 rows of padding | 17 tiles of 16 keys = 257 + 15


def qkv_attn_schedule(nseq, ncu=256):
    """qkv_attention.hip's static split (:783-786) and a workgroup's walk (unit_of, :176-181): XCD x owns patches [x px, (x + 1) px),
    px = ceil(nseq / 8); its units (patch, head), head fastest, go round nslots = min(6 px, ncu / 8) workgroups: workgroup (x, slot)
    takes units slot + nslots i, i = 0, 1, .. while they exist.  -> dict of [nseq, 6] tensors: wg (the workgroup id, x + 8 slot),
    idx (i), count (units of that workgroup), prev / prev2 (the patch of the workgroup's unit i - 1 / i - 2, -1 where there is
    none), first / carried / last (bool; a workgroup with one unit is first and last), and max_units (int)."""
    H = 6
    px = (nseq + 7) // 8
    nslots = min(px * H, max(ncu // 8, 1))
    o = {k: torch.full((nseq, H), -1, dtype=torch.int64) for k in ("wg", "idx", "count", "prev", "prev2")}
    for x in range(8):
        for slot in range(nslots):
            walk = []
            i = 0
            while True:
                U = slot + nslots * i
                bq, h = divmod(U, H)
                b = x * px + bq
                if not (bq < px and b < nseq):
                    break
                walk.append((b, h))
                i += 1
            for i, (b, h) in enumerate(walk):
                assert int(o["wg"][b, h]) == -1
                o["wg"][b, h], o["idx"][b, h], o["count"][b, h] = x + 8 * slot, i, len(walk)
                o["prev"][b, h] = walk[i - 1][0] if i >= 1 else -1
                o["prev2"][b, h] = walk[i - 2][0] if i >= 2 else -1
    o["first"] = o["idx"] == 0
    o["last"] = o["idx"] == o["count"] - 1
    o["carried"] = ~o["first"] & ~o["last"]
    o["max_units"] = int(o["count"].max())
    return o


def att_schedule_sizes(ncu=256, limit=4096):
    """the smallest nseq (multiples of 16: whole 16-row fragments) whose busiest workgroup takes 1, 2 and 3 work units"""
    out = {}
    for nseq in range(16, limit, 16):
        px = (nseq + 7) // 8
        nslots = min(px * 6, max(ncu // 8, 1))
        out.setdefault(-(-px * 6 // nslots), nseq)
        if all(k in out for k in (1, 2, 3)):
            return out[1], out[2], out[3]
    raise ValueError(ncu)


def fused_half0_keys():
    """qkv_attention.hip's score tiles S^T[key][query] are 32 x 32 accumulators: lane (r, hh) holds query r and the keys 8 (i >> 2) + 4 hh
    + (i & 3), i = 0 .. 15, of each tile (:84-85), the [CLS] key in register 0 of lane half 0 of tile 8 (:623).  -> bool [257]: the keys
    (tokens) of lane half 0; a row maximum needs the other half's through the shfl_xor 32 of :625 (:533 for the [CLS] query)"""
    t = torch.arange(NTOK)
    return (t == 0) | (((t - 1) % 8) < 4)


def _att_softmax_pv(s, v, r, mm, variant, npad):
    """rows of scaled scores s [.., nq, 257] against v [.., 257, dh]: one maximum per row, e = exp(s - m), the row sum l adds the
    UNROUNDED e, the P V operand is bf16(e), 1 / l after P V (attention2.hip:79-100, :113-116, :144; qkv_attention.hip:626-641, :681, :702-709)"""
    if variant == "half_max":
        m = s.masked_fill(~fused_half0_keys().to(s.device), -math.inf).amax(-1, keepdim=True)
    else:
        m = s.amax(-1, keepdim=True)
    if variant == "pad_unmasked":
        m = m.clamp(min=0.0)  # (the padding keys score 0)
    e = torch.exp(s - m)
    if variant == "half_max":
        e = e.float().double()  # (beyond the true maximum the fp32 exponential can overflow)
    l = e.sum(-1, keepdim=True)
    if variant == "pad_unmasked":
        l = l + npad * torch.exp(-m)  # (their value rows are zero: they dilute the row, nothing else)
    return _mm(r(e), v, mm) / l


def _att_fused_cls_row(s0, v, r, mm, variant):
    """the [CLS] query of the fused kernel: s0 [.., 257] its scaled scores, v [.., 257, dh] -> [.., dh].  cls_query (qkv_attention.hip:490-584):
    wave w of eight takes keys 1 + 32 w .. 32 w + 32, wave 0 the [CLS] key as well (:529); its own maximum m_w (:530-533), e = exp(s - m_w)
    (:538, :542), l_w adds the UNROUNDED e (:539, :543-544), the P V operand is bf16(e) (:545-546), (m_w, l_w, o_w) go to LDS in fp32
    (:571-579).  merge_cls (:256-284): f_w = exp(m_w - max m) (:275), L = sum f_w l_w (:276), o = sum f_w o_w (:277), bf16(o / L) (:283: 1 / L
    once, on the merged row; the caller rounds)."""
    dev = s0.device
    g = fused_cls_groups().to(dev)
    sm = s0.masked_fill(~fused_half0_keys().to(dev), -math.inf) if variant == "half_max" else s0
    mg = torch.full(s0.shape[:-1] + (8,), -math.inf, dtype=s0.dtype, device=dev).scatter_reduce(-1, g.expand_as(s0), sm, "amax")
    if variant == "pad_unmasked":  # (tile 8 is wave 0's share)
        mg[..., 0] = mg[..., 0].clamp(min=0.0)
    M = mg.amax(-1, keepdim=True)
    mg = torch.where(torch.isinf(mg), M, mg)  # (a wave whose keys are all masked: no variant here does that)
    e = torch.exp(s0 - mg[..., g])
    if variant == "half_max":
        e = e.float().double()
    fw = torch.ones_like(mg) if variant == "no_merge_rescale" else torch.exp(mg - M)
    f = fw[..., g]
    L = (e * f).sum(-1, keepdim=True)
    if variant == "pad_unmasked":
        L = L + ATT_PAD_KEYS["fused"] * torch.exp(-mg[..., :1]) * fw[..., :1]
    return _mm((r(e) * f).unsqueeze(-2), v, mm).squeeze(-2) / L


def attention_unit(xn, p, nseq, rnd=True, variant=None, seqs=32, mm=None, route=None, ncu=256):
    """hipt_vit_attention_unit: softmax(q k^T * scale) v per head from xn = LayerNorm-1(x) (bf16 values) [nseq * ntok, D] -> [nseq * ntok, D]
    before proj, with the kernels' rounding: q | k | v -> bf16, the UNNORMALISED probabilities exp(s - max) -> bf16 as the P V operand
    while the row sum l adds the unrounded ones, the 1 / l after P V, the output -> bf16.  Groups of `seqs` sequences.  mm: see _mm (the
    three products).

    route  None / "two_kernel": the arithmetic above on every row (QKV GEMM + attn64_kernel; None takes no route-specific variant).
           "fused": the same for tokens 1 .. 256 of a patch; the [CLS] query row is _att_fused_cls_row (per-wave partial softmaxes, each
           rounding P against the wave's own maximum, merged by one wave).  Its q comes from the side GEMM, bf16 like the rest (the
           seqgemm's bf16 output), so the scores are the same numbers on both routes.
    variant  one of ATT_VARIANTS[route] (scale2 / mask_tile on any route), the emulation with that one mistake:
           pad_unmasked     the padding keys of the last key tile (ATT_PAD_KEYS) take part with score 0 (qkv_attention.hip:622, :642 absent)
           drop_cls_key     key tile 8 ignored: key and value of token 0 missing
           drop_last_token  key 256 missing
           half_max         the maximum over the keys of lane half 0 only (fused_half0_keys; no shfl_xor 32): moves the result only through
                            the fp32 overflow of exp and the rounding of P
           no_bq, no_bv     that bias never added.  (no_bk is not a variant: q . bk is one constant per query row, which the softmax
                            removes -- the mistake is invisible to the unit)
           v_dtile_swap     the two 32-dim V sub-images of a head exchanged
           head_bias_next   head h projected with head h + 1's bias slice
           stale_cls_row    a workgroup's i-th work unit, i >= 2, takes the [CLS] k and v of its (i - 2)-th unit's patch (the `par` LDS slot
                            not refreshed, :435)
           prev_patch_rows  a carried unit (i >= 1) computes tokens 1 .. 256 from the previous unit's patch rows (the prefetch of :655-691
                            not consumed)
           no_merge_rescale the [CLS] merge without the exp(m_w - m) factors (:275)
           last_merge_dropped  the [CLS] row of the last unit of every workgroup never merged (:728): it stays 0
           The schedule variants follow qkv_attn_schedule(nseq, ncu)."""
    if route is not None and route not in ATT_ROUTES:
        raise ValueError(route)
    if route is not None and variant not in (None, "scale2", "mask_tile") and variant not in ATT_VARIANTS[route]:
        raise ValueError(f"variant {variant} has no counterpart on route {route}")
    if route is None and variant not in ("scale2", "mask_tile"):
        variant = None  # (block() hands every unit the variants of both: a name of the other unit's is ignored)
    r = bf16 if rnd else _id
    M, Dm = xn.shape
    ntok = M // nseq
    H = p["heads"]
    dh = Dm // H
    bias = p["qkv_b"]
    if variant in ("no_bq", "no_bv"):
        bias = bias.clone()
        (bias[:Dm] if variant == "no_bq" else bias[2 * Dm:]).zero_()
    elif variant == "head_bias_next":
        bias = bias.view(3, H, dh).roll(-1, 1).reshape(-1)

    def project(s0):
        ns = min(seqs, nseq - s0)
        x = xn[s0 * ntok:(s0 + ns) * ntok].double()
        qkv = r(_mm(x, p["qkv_w"].t(), mm) + bias)  # qkv_attention.hip:345-361 (fused) / the QKV GEMM's bf16 output (two kernels): q | k | v -> bf16
        return qkv.view(ns, ntok, 3, H, dh).permute(2, 0, 3, 1, 4)

    sched = qkv_attn_schedule(nseq, ncu) if variant in ("stale_cls_row", "prev_patch_rows", "last_merge_dropped") else None
    full = None
    if variant in ("stale_cls_row", "prev_patch_rows"):
        full = torch.cat([project(s0) for s0 in range(0, nseq, seqs)], 1).contiguous()  # [3, nseq, H, ntok, dh]
        prev = sched["prev" if variant == "prev_patch_rows" else "prev2"].to(xn.device)
        src = torch.where(prev >= 0, prev, torch.arange(nseq, device=xn.device)[:, None].expand(nseq, H))
        moved = full[:, src, torch.arange(H, device=xn.device)[None, :]]
        full = full.clone()
        if variant == "prev_patch_rows":
            full[:, :, :, 1:] = moved[:, :, :, 1:]
        else:
            full[1:, :, :, 0] = moved[1:, :, :, 0]
    out = []
    for s0 in range(0, nseq, seqs):
        ns = min(seqs, nseq - s0)
        qkv = project(s0) if full is None else full[:, s0:s0 + ns]
        v = qkv[2]
        if variant == "v_dtile_swap":
            v = torch.cat([v[..., dh // 2:], v[..., :dh // 2]], -1)
        sc = p["scale"] * (p["scale"] if variant == "scale2" else 1.0)
        s = _mm(qkv[0], qkv[1].transpose(-1, -2), mm) * sc
        if variant == "mask_tile":
            s[..., 16:32] = -math.inf  # (key tile 1 masked)
        elif variant == "drop_cls_key":
            s[..., 0] = -math.inf
        elif variant == "drop_last_token":
            s[..., ntok - 1] = -math.inf
        # attention.hip:152 / qkv_attention.hip:680: P -> bf16 before normalisation; 1 / l at attention.hip:192 / qkv_attention.hip:707
        o = _att_softmax_pv(s, v, r, mm, variant, ATT_PAD_KEYS.get(route, 0))
        if route == "fused":  # (rnd=False too: the partial-and-merge algebra must then be plain attention)
            o[:, :, 0] = _att_fused_cls_row(s[:, :, 0], v, r, mm, variant)
        if variant == "last_merge_dropped":
            o[:, :, 0] = torch.where(sched["last"][s0:s0 + ns].to(o.device)[..., None], torch.zeros_like(o[:, :, 0]), o[:, :, 0])
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


# ---- inputs, metrics and noise floor of the attention-unit tests (tests/test_gpu_attention_unit.py) --------------------------------------
# The spiked tokens: the [CLS] key (key tile 8, register 0 of lane half 0), tile 0 lane half 0, tile 0 lane half 1, the last key of
# tile 0, the first key of tile 1, the last key of the patch (fused_half0_keys: token 1 + 32 kt + j is in lane half (j % 8) >= 4).
ATT_SPIKES = (0, 1, 5, 32, 33, 256)
ATT_CLASSES = ("plain",) + tuple(f"spike{t}" for t in ATT_SPIKES) + ("equal", "near_equal")
ATT_SPIKE_FACTOR = 16.0  # (a power of two: exact in bf16)


def att_seed(nseq):
    return 700 + nseq


def att_inputs(p, nseq, seed, device="cpu", outlier_rows=False):
    """xn = bf16(LayerNorm-1(hash rows)) with the block's own affine (as cls_inputs; outlier_rows: its four residual channels at
    +-60 .. 100 in every row of the odd patches of the plain, equal and near_equal classes -- under them all queries of a patch share
    one direction, and a spiked key would be the maximum of all of them or of none), patch i of class ATT_CLASSES[i % 9]:
      plain       as drawn
      spike<t>    the xn row of token t x ATT_SPIKE_FACTOR: that key holds the running maximum of many queries, and as a query the row
                  has huge self-scores (its output row stays in the comparison)
      equal       all 257 rows equal row 0: p = 1 / 257 exactly, the output is the v row
      near_equal  row 0 with every element moved by -2 .. 2 bf16 ulps per row: a flat softmax with every key live
    -> dict xn (torch.bfloat16 [nseq * 257, 384]), classes {name: patch indices}"""
    from hipt_abmil_atec23_amd import synth
    M = nseq * NTOK
    x = synth.hash_uniform_torch((M, D), seed, 2.0, device=device)
    cls = torch.arange(nseq, device=device) % len(ATT_CLASSES)
    if outlier_rows:
        ch = torch.tensor([7, 100, 200, 333], device=device)
        big = torch.tensor([60.0, -75.0, 90.0, -100.0], device=device)
        spiked = (cls >= 1) & (cls <= len(ATT_SPIKES))
        odd = torch.nonzero((torch.arange(nseq, device=device) % 2 == 1) & ~spiked).flatten()
        xv = x.view(nseq, NTOK, D)
        xv[odd[:, None], :, ch] = (big * (1.0 + 0.1 * xv[odd][:, :, ch])).transpose(1, 2)
    xn = bf16(layer_norm(x.double(), p["ln1_w"], p["ln1_b"])).view(nseq, NTOK, D)
    for k, name in enumerate(ATT_CLASSES):
        i = torch.nonzero(cls == k).flatten()
        if name.startswith("spike"):
            xn[i, int(name[5:])] *= ATT_SPIKE_FACTOR
        elif name == "equal":
            xn[i] = xn[i][:, :1].expand(-1, NTOK, -1).clone()
        elif name == "near_equal" and len(i):
            bits = xn[i][:, :1].bfloat16().view(torch.int16).to(torch.int32).expand(-1, NTOK, -1)  # (sign-magnitude: +1 is one ulp up in magnitude)
            step = (synth.hash_uniform_torch((len(i), NTOK, D), seed + 1, 2.5, device=device)).round().to(torch.int32)
            step[:, 0] = 0
            mag = bits & 0x7FFF
            step = torch.where((mag > 16) & (mag < 0x7F00), step, torch.zeros_like(step))
            xn[i] = (bits + step).to(torch.int16).view(torch.bfloat16).double()
    classes = {name: torch.nonzero(cls == k).flatten() for k, name in enumerate(ATT_CLASSES)}
    return {"xn": xn.view(M, D).bfloat16(), "classes": classes}


def att_scores(xn, p, nseq, patches):
    """the emulation's own scaled scores [len(patches), H, 257, 257] of some patches (bf16 q and k)"""
    Dm, H = xn.shape[-1], p["heads"]
    x = xn.view(nseq, NTOK, Dm)[patches].double()
    qk = bf16(x @ p["qkv_w"][:2 * Dm].t() + p["qkv_b"][:2 * Dm]).view(len(patches), NTOK, 2, H, Dm // H).permute(2, 0, 3, 1, 4)
    return (qk[0] @ qk[1].transpose(-1, -2)) * p["scale"]


def att_assert_edges(c, p, nseq, family):
    """the inputs of a case reach the edges they are built for, by the emulation's own scores: in every spike patch and every head the
    spiked key is the row maximum of >= 25 % of the 257 queries, and some |score| of the patch is beyond 89 (exp overflows fp32 without
    the maximum subtracted); the equal patches' rows are bitwise equal; a near_equal row's scores spread by less than 1 (and its rows differ);
    outlier family: plain-patch scores beyond 30.  -> the figures, for printing"""
    xn, cl = c["xn"], c["classes"]
    out = {"spike_frac": 1.0, "spike_smax": math.inf}
    for t in ATT_SPIKES:
        s = att_scores(xn, p, nseq, cl[f"spike{t}"])
        frac = (s.argmax(-1) == t).double().mean(-1)  # [patches, H]
        smax = s.abs().amax((-1, -2, -3))  # per patch
        assert float(frac.min()) >= 0.25, (f"spike{t}", float(frac.min()))
        assert float(smax.min()) > 89.0, (f"spike{t}", float(smax.min()))
        out["spike_frac"], out["spike_smax"] = min(out["spike_frac"], float(frac.min())), min(out["spike_smax"], float(smax.min()))
    xe = xn.view(nseq, NTOK, -1)[cl["equal"]]
    assert bool((xe.view(torch.int16) == xe[:, :1].view(torch.int16)).all()), "equal"
    xq = xn.view(nseq, NTOK, -1)[cl["near_equal"]]
    assert not bool((xq[:, 1:] == xq[:, :1]).all(-1).any()), "near_equal: a row equals row 0"
    s = att_scores(xn, p, nseq, cl["near_equal"])
    out["near_equal_spread"] = float((s.amax(-1) - s.amin(-1)).max())
    assert out["near_equal_spread"] < 1.0, out["near_equal_spread"]
    out["plain_smax"] = float(att_scores(xn, p, nseq, cl["plain"]).abs().max())
    if family == "outlier":
        assert out["plain_smax"] > 30.0, out["plain_smax"]
    return out


ATT_METRICS = ("rows_rel", "cls_rel", "rows_head", "rows_wave", "rows_class", "cls_class", "rows_pos", "cls_pos")


def att_errors(got, ref, nseq, classes, sched) -> dict:
    """The metrics of the attention-unit tests, every one a rel-L2 ||got - ref|| / ||ref|| over a set of elements ([nseq * 257, 384]
    row-major; inf if got is not finite there):
      rows_rel / cls_rel      the rows other than [CLS] / the [CLS] rows
      rows_head               the worst head (64 columns) of the non-[CLS] rows
      rows_wave               the worst query wave (rows 1 + 32 w .. 32 w + 32 of every patch)
      rows_class / cls_class  the worst patch class
      rows_pos / cls_pos      the worst schedule position: the (patch, head) blocks that were their workgroup's first, carried or last unit
    and per_class, per_pos for printing."""
    H = sched["first"].shape[1]
    dev = got.device
    d2 = torch.nan_to_num((got.double() - ref.double()).square(), nan=math.inf, posinf=math.inf).view(nseq, NTOK, H, -1).sum(-1)
    r2 = ref.double().square().view(nseq, NTOK, H, -1).sum(-1)
    dr, rr = d2[:, 1:].reshape(nseq, 8, 32, H).sum(2), r2[:, 1:].reshape(nseq, 8, 32, H).sum(2)  # [patch, wave, head]
    dc, rc = d2[:, 0], r2[:, 0]  # [patch, head]
    rl = lambda a, b: float((a.sum() / b.sum()).sqrt())
    out = {"rows_rel": rl(dr, rr), "cls_rel": rl(dc, rc),
           "rows_head": max(rl(dr[..., h], rr[..., h]) for h in range(H)), "rows_wave": max(rl(dr[:, w], rr[:, w]) for w in range(8))}
    per = {k: (rl(dr[i], rr[i]), rl(dc[i], rc[i])) for k, i in classes.items() if len(i)}
    pos = {}
    for k in ("first", "carried", "last"):
        m = sched[k].to(dev)
        if bool(m.any()):
            mw = m[:, None, :].expand(-1, 8, -1)
            pos[k] = (rl(dr[mw], rr[mw]), rl(dc[m], rc[m]))
    out["rows_class"], out["cls_class"] = max(v[0] for v in per.values()), max(v[1] for v in per.values())
    out["rows_pos"], out["cls_pos"] = max(v[0] for v in pos.values()), max(v[1] for v in pos.values())
    out["per_class"], out["per_pos"] = per, pos
    return out


# The noise floor of attention_unit, as CLS_FLOOR: the largest distance, per (route, family) and metric of att_errors, between the
# emulation with fp64 products and with fp32 products on att_inputs at 16, 48 and 96 patches, the sizes of the GPU cases
# (tests/test_vit_bf16_ref.py, test_attention_unit_noise_floor).  The [CLS] metrics rest on nseq rows and a handful of bf16 flips: at 96
# patches they are up to 14 x what 16 and 48 show.  "std" / "outlier": block 3 of those weights, mm=torch.float32.  "outlier_b0": block 0
# of the outlier weights, whose logits reach 3e4 -- an fp32 product of a score is off by 1e-3 and more in absolute terms there, the
# summation order of the product decides the figure, and the floor is taken with the fixed-order product of _mm, mm="f32k16".  The bars
# of tests/test_gpu_attention_unit.py are ATT_BAR_FACTOR times these; no kernel measurement enters them.
ATT_BAR_FACTOR = CLS_BAR_FACTOR
ATT_FLOOR = {
    ('fused', 'std'): {"rows_rel": 1.03e-04, "cls_rel": 3.68e-05, "rows_head": 2.11e-04, "rows_wave": 1.27e-04, "rows_class": 2.06e-04, "cls_class": 1.55e-04, "rows_pos": 1.47e-04, "cls_pos": 5.28e-05},
    ('two_kernel', 'std'): {"rows_rel": 1.03e-04, "cls_rel": 4.12e-05, "rows_head": 2.11e-04, "rows_wave": 1.27e-04, "rows_class": 2.06e-04, "cls_class": 2.13e-04, "rows_pos": 1.47e-04, "cls_pos": 5.29e-05},
    ('fused', 'outlier'): {"rows_rel": 4.74e-05, "cls_rel": 2.72e-05, "rows_head": 7.99e-05, "rows_wave": 9.02e-05, "rows_class": 1.26e-04, "cls_class": 1.12e-04, "rows_pos": 5.69e-05, "cls_pos": 2.72e-05},
    ('two_kernel', 'outlier'): {"rows_rel": 4.74e-05, "cls_rel": 6.31e-06, "rows_head": 7.99e-05, "rows_wave": 9.02e-05, "rows_class": 1.26e-04, "cls_class": 1.51e-04, "rows_pos": 5.69e-05, "cls_pos": 7.07e-06},
    ('fused', 'outlier_b0'): {"rows_rel": 1.86e-04, "cls_rel": 9.18e-06, "rows_head": 4.91e-04, "rows_wave": 5.24e-04, "rows_class": 4.04e-04, "cls_class": 2.94e-04, "rows_pos": 1.86e-04, "cls_pos": 1.19e-05},
    ('two_kernel', 'outlier_b0'): {"rows_rel": 1.86e-04, "cls_rel": 1.00e-05, "rows_head": 4.91e-04, "rows_wave": 5.24e-04, "rows_class": 4.04e-04, "cls_class": 2.94e-04, "rows_pos": 1.86e-04, "cls_pos": 1.26e-05},
}


def att_floor_key(family, blk):
    """-> (the family key of ATT_FLOOR, the mm= its floor is taken with)"""
    return ("outlier_b0", "f32k16") if (family, blk) == ("outlier", 0) else (family, torch.float32)


# variants that stay below 3 x every bar on a (route, family) because the mistake is arithmetically invisible there
ATT_NOT_PINNED = set()
