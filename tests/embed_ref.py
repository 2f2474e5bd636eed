"""CPU side (float64) of the per-unit tests of the pixel-reading patch embedding (csrc/embed32.hip + misc.hip: cls_init_kernel /
cls_init_img_kernel) through hipt_vit_embed_unit -- DESIGN.md 30.  The patchify through a hipt_image_layout from the formula of
include/hipt_abmil.h, the operands as the kernel rounds them, the exact tokens x = a W^T + bias + pos[1 + t] with the per-element bound
of ops_ref.linear_bound, LayerNorm-1 of block 0 with ops_ref.layernorm_bound on this kernel's summation chain, an fp32 emulation of the
kernel, the wrong kernels written as references, the weight families and the case table.  tests/test_embed_ref.py checks all of this
without a GPU; tests/test_gpu_embed_unit.py holds the kernel to it."""
import math
from collections import namedtuple

import numpy as np
import torch

import ops_ref as P
from hipt_abmil_atec23_amd import synth

D, NTOK, K, TOK = 384, 257, 768, 256
F32, U8_CHW, U8_HWC = 0, 1, 2   # input_kind of hipt_vit_embed_unit
TILE = 128                      # token rows of one workgroup tile: 8 token rows of one patch
# roundings between an element and the mean (ops_ref.layernorm_bound's L).  embed32.hip, LNOUT: a lane adds its 192 values serially,
# one shfl_xor 32 joins the two lanes of a token, one division.  cls_init_img_kernel: 6 values per lane, the 6-step tree, the division
# -- ln_kernel's own D / 64 + 7.
LN_CHAIN_TOKENS = 192 + 1 + 1
LN_CHAIN_CLS = D // 64 + 6 + 1

Layout = namedtuple("Layout", "grid_w grid_h patch_h patch_w row_stride chan_stride batch_stride")


def plain_layout(w, h):
    """a batch [B, 3, w, h]: one patch per item (include/hipt_abmil.h)"""
    return Layout(1, 1, w, h, h, w * h, 3 * w * h)


def region_layout(W, H, row_stride=None, chan_stride=None):
    """[B, 3, W, H] cut into 256 x 256 patches; the strides of a window of a larger tensor where given"""
    rs = H if row_stride is None else row_stride
    cs = W * rs if chan_stride is None else chan_stride
    return Layout(W // 256, H // 256, 256, 256, rs, cs, 3 * cs)


# =====================================================================================================================
# Patchify: element indices of the 768 pixels of every token, k = (c, y, x) as Conv2d's weight.view(384, 768)
# =====================================================================================================================
def patch_index(lay, seq0, nseq, kind, variant=None):
    """int64 [nseq, 256, 768]: where pixel (c, y, x) of token (b, ty, tx) lies, in elements of the image tensor.  The header's formula:
    pixel(b, c, y, x) = img[(b / (gw gh)) batch_stride + c chan_stride + (((b / gh) % gw) patch_h + y) row_stride + (b % gh) patch_w + x];
    interleaved uint8: strides count pixels, a pixel is three consecutive bytes"""
    gw, gh = (lay.grid_h, lay.grid_w) if variant == "grid_swap" else (lay.grid_w, lay.grid_h)
    b = np.arange(seq0, seq0 + nseq, dtype=np.int64).reshape(-1, 1, 1, 1, 1, 1)
    ty = np.arange(16, dtype=np.int64).reshape(1, -1, 1, 1, 1, 1)
    tx = np.arange(16, dtype=np.int64).reshape(1, 1, -1, 1, 1, 1)
    c = np.arange(3, dtype=np.int64).reshape(1, 1, 1, -1, 1, 1)
    if variant == "swap_rb":
        c = 2 - c
    y = 16 * ty + np.arange(16, dtype=np.int64).reshape(1, 1, 1, 1, -1, 1)
    x = 16 * tx + np.arange(16, dtype=np.int64).reshape(1, 1, 1, 1, 1, -1)
    item = b // (gw * gh)
    inimg = (((b // gh) % gw) * lay.patch_h + y) * lay.row_stride + (b % gh) * lay.patch_w + x
    if kind == U8_HWC:
        idx = (item * (lay.batch_stride // 3) + inimg) * 3 + c
    else:
        idx = item * lay.batch_stride + c * lay.chan_stride + inimg
    return np.ascontiguousarray(np.broadcast_to(idx, (nseq, 16, 16, 3, 16, 16))).reshape(nseq, TOK, K)


def normalize_u8(p):
    """ToTensor + Normalize(0.5, 0.5) in fp32, the reference's two divisions (hipt_model_utils.py:113-118)"""
    return ((np.asarray(p).astype(np.float32) / np.float32(255.0) - np.float32(0.5)) / np.float32(0.5)).astype(np.float32)


def bf16_trunc(x):
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def operands(pix, kind, variant=None):
    """the gathered pixels [.., 768] as the MFMA reads them: bf16 values in float64"""
    v = np.asarray(pix, np.float32) if kind == F32 else normalize_u8(pix)
    a = (bf16_trunc(v) if variant == "trunc" else P.bf16_round(v)).astype(np.float64)
    if variant == "drop_row":      # the last pixel row of channel 2
        a = a.copy()
        a[..., 2 * 256 + 15 * 16:] = 0.0
    if variant == "stale_c0":      # channel 0 of tile n is the one fetched for tile n - 1 (tiles in call order)
        t = a.reshape(-1, TILE, K).copy()
        t[1:, :, :256] = t[:-1, :, :256].copy()
        a = t.reshape(a.shape)
    return a


def gather(storage, lay, seq0, nseq, kind, variant=None):
    """storage: the flat buffer `images` points into (numpy, fp32 or uint8) -> operands [nseq, 256, 768]"""
    flat, idx = np.asarray(storage).reshape(-1), patch_index(lay, seq0, nseq, kind, variant)
    if variant == "grid_swap":   # (a wrong address may leave the tensor: wrapped, it still reads wrong pixels)
        idx = idx % flat.size
    return operands(flat[idx], kind, variant)


# =====================================================================================================================
# Weights
# =====================================================================================================================
def interpolate_pos(pos_embed):
    """[1, 197, 384] -> [257, 384] fp32: the module's own call (vision_transformer.py:213-233) for a 256 x 256 patch"""
    pe = torch.as_tensor(np.asarray(pos_embed, np.float32))
    Np = pe.shape[1] - 1
    side = int(math.sqrt(Np))
    s = (16 + 0.1) / math.sqrt(Np)
    g = torch.nn.functional.interpolate(pe[:, 1:].reshape(1, side, side, D).permute(0, 3, 1, 2), scale_factor=(s, s), mode="bicubic")
    assert g.shape[-2:] == (16, 16)
    return torch.cat((pe[:, :1], g.permute(0, 2, 3, 1).reshape(1, -1, D)), dim=1)[0].contiguous().numpy()


# token classes of the edge family (token index t = 16 ty + tx; pos row 1 + t): the first and the last token row of both tiles of a patch
EDGE_CLASSES = ("offset", "near_const", "outlier_ch")
OUTLIER_CH = (7, 100, 200, 333)        # output columns in both halves of a token's lane pair ((col >> 2) & 1 = 1, 1, 0, 1)
OUTLIER_VAL = (60.0, -75.0, 90.0, -100.0)


def edge_tokens():
    """the three classes, and "debiased": token rows 3 and 12, whose pos rows take the embedding bias (with its four channels at +-400 ...
    800) out again -- ordinary O(0.3) rows with kappa ~ 1 under the outlier gains, where a LayerNorm output can be small against its two
    terms (what shows a divisor D - 1)"""
    tok = {name: np.array([16 * ty + tx for ty in (0, 7, 8, 15) for tx in (1 + k, 14 - k)]) for k, name in enumerate(EDGE_CLASSES)}
    tok["debiased"] = np.array([16 * ty + tx for ty in (3, 12) for tx in range(16)])
    return tok


def edge_reach(x, prm):
    """asserts, from the exact x [nseq, 257, 384] of the edge case with fp32 pixels, what each class is there for -> the figures"""
    tok = edge_tokens()
    kap = P.layernorm_kappa(x[:, 1 + tok["offset"]], prm["eps"])
    var = x[:, 1 + tok["near_const"]].var(-1)
    big = np.abs(x[:, 1 + tok["outlier_ch"]][..., list(OUTLIER_CH)])
    assert kap.min() >= 100.0, kap.min()                                                            # cancellation in the mean
    assert 0.1 * prm["eps"] <= var.min() and var.max() <= 10 * prm["eps"], (var.min(), var.max())   # eps decides the output
    assert big.min() >= 55.0 and big.max() <= 105.0, (big.min(), big.max())
    return {"kappa_offset_min": kap.min(), "var_near_const_min": var.min(), "var_near_const_max": var.max(), "outlier_min": big.min()}


def make_params(family="std", depth=2):
    """-> (state dict of a ViT-256 of `depth` blocks as numpy, the embedding's parameters).  std: synth's standard family.  edge: the
    outlier family (LayerNorm gains 0.05 ... 20, four embedding biases at +-50 ... 100) with the patch-embedding bias x 8 and the
    positional rows of edge_tokens() rewritten so that x = a W^T + bias + pos is: 100 + 0.87 u (+ a W^T: LayerNorm cancellation);
    1 + 1.7e-3 u exactly where the pixels are 0 (variance ~ eps); ordinary with four channels at +-60 ... 100; and the "debiased" rows
    of edge_tokens()."""
    specs = synth.vit_param_specs("vit256", depth=depth)
    sd = synth.make_params_np(specs, 256) if family == "std" else synth.make_vit_outlier_params_np(specs, 256, 6)
    pos = interpolate_pos(sd["pos_embed"])
    if family == "edge":
        sd["patch_embed.proj.bias"] = sd["patch_embed.proj.bias"] * np.float32(8.0)
        bias, tok = sd["patch_embed.proj.bias"], edge_tokens()
        r = 1 + tok["offset"]
        pos[r] = synth.hash_uniform_np((len(r), D), 911, 0.87, 100.0) - bias
        r = 1 + tok["near_const"]
        pos[r] = (np.float32(1.0) - bias)[None] + synth.hash_uniform_np((len(r), D), 912, 1.7e-3)
        r = 1 + tok["debiased"]
        pos[r] = pos[r] - bias
        r = 1 + tok["outlier_ch"]
        pos[np.ix_(r, OUTLIER_CH)] = np.asarray(OUTLIER_VAL, np.float32) - bias[list(OUTLIER_CH)]
    w = sd["patch_embed.proj.weight"].reshape(D, K)
    prm = {"w": w, "wb": P.bf16_round(w).astype(np.float64), "bias": sd["patch_embed.proj.bias"], "cls": sd["cls_token"].reshape(D),
           "pos": np.ascontiguousarray(pos, np.float32), "ln_w": sd["blocks.0.norm1.weight"], "ln_b": sd["blocks.0.norm1.bias"],
           "eps": float(np.float32(1e-6))}
    return sd, prm


# =====================================================================================================================
# The exact unit and its bounds
# =====================================================================================================================
def tokens_ref(a, prm, variant=None):
    """x [nseq, 257, 384] in float64: rows 1 + t = a W^T + bias + pos[1 + t], row 0 = cls + pos[0]"""
    nseq = a.shape[0]
    bias = prm["bias"].astype(np.float64)
    pos = prm["pos"].astype(np.float64)
    body = a.reshape(-1, K) @ prm["wb"].T + bias
    if variant == "bias_tile":     # no bias in output columns 32 O .. 32 O + 31, O = 5
        body[:, 160:192] -= bias[160:192]
    x = np.empty((nseq, NTOK, D))
    x[:, 1:] = body.reshape(nseq, TOK, D) + (pos[:TOK] if variant == "pos_shift" else pos[1:])
    x[:, 0] = prm["cls"].astype(np.float64) + pos[0]
    return x


def tokens_bound(a, prm):
    """rows 1 + t: ops_ref.linear_bound with K = 768 -- bf16 products exact in fp32, fp32 accumulation, then the two fp32 additions;
    row 0: one fp32 addition"""
    nseq = a.shape[0]
    a2 = a.reshape(-1, K)
    S = np.abs(a2) @ np.abs(prm["wb"]).T + np.abs(prm["bias"].astype(np.float64))
    S = S.reshape(nseq, TOK, D) + np.abs(prm["pos"][1:].astype(np.float64))
    b = np.empty((nseq, NTOK, D))
    b[:, 1:] = (K + 4) * P.U * S + P.TINY
    b[:, 0] = P.U * np.abs(prm["cls"].astype(np.float64) + prm["pos"][0].astype(np.float64)) + P.TINY
    return b


def xn_ref(x, prm, variant=None):
    """LayerNorm-1 of block 0 of the rows x [nseq, 257, 384] (the kernel's own fp32 x in the tests) in float64"""
    x = np.asarray(x, np.float64)
    w, b, eps = prm["ln_w"].astype(np.float64), prm["ln_b"].astype(np.float64), prm["eps"]
    if variant == "no_eps":
        return P.layernorm_variant("no_eps", x, w, b, eps)
    if variant == "div_dm1":
        return P.layernorm_variant("div_dm1", x, w, b, eps)
    if variant == "xn_before_pos":
        x = x.copy()
        x[:, 1:] -= prm["pos"][1:].astype(np.float64)
    return P.layernorm_ref(x, w, b, eps)


def xn_bound(x, prm):
    x = np.asarray(x, np.float64)
    b = np.empty(x.shape)
    b[:, 1:] = P.layernorm_bound(x[:, 1:], prm["ln_w"], prm["ln_b"], prm["eps"], True, chain=LN_CHAIN_TOKENS)
    b[:, :1] = P.layernorm_bound(x[:, :1], prm["ln_w"], prm["ln_b"], prm["eps"], True, chain=LN_CHAIN_CLS)
    return b


VARIANTS_X = ("trunc", "pos_shift", "bias_tile", "swap_rb", "grid_swap", "drop_row", "stale_c0")
VARIANTS_XN = ("no_eps", "div_dm1", "xn_before_pos")
# the case (CASES) on which each wrong kernel must land >= 3 x beyond its bound
CATCHES = {"trunc": "plain16", "pos_shift": "plain16", "bias_tile": "plain16", "swap_rb": "plain16", "grid_swap": "region2x4",
           "drop_row": "plain16", "stale_c0": "multi", "no_eps": "edge", "div_dm1": "edge", "xn_before_pos": "plain16"}


def variant_tokens(name, storage, lay, seq0, nseq, kind, prm):
    """x of a wrong kernel, float64"""
    av = name if name in ("trunc", "drop_row", "stale_c0", "swap_rb", "grid_swap") else None
    return tokens_ref(gather(storage, lay, seq0, nseq, kind, av), prm, name)


# =====================================================================================================================
# fp32 emulation of the kernel
# =====================================================================================================================
_f32 = lambda v: np.asarray(v, np.float64).astype(np.float32)


def emulate_tokens(a, prm):
    """embed32_kernel in NumPy: one MFMA k-step = the 16 pixels of one pixel row of one channel, accumulated in fp32 in the kernel's
    order (channel, pixel row); then (acc + bias) + pos in fp32.  -> x [nseq, 257, 384] float32"""
    nseq = a.shape[0]
    a2 = a.reshape(-1, K)
    acc = np.zeros((a2.shape[0], D), np.float32)
    for k in range(0, K, 16):
        acc = _f32(acc.astype(np.float64) + a2[:, k:k + 16] @ prm["wb"][:, k:k + 16].T)
    v = ((acc + prm["bias"]).astype(np.float32).reshape(nseq, TOK, D) + prm["pos"][1:]).astype(np.float32)
    x = np.empty((nseq, NTOK, D), np.float32)
    x[:, 1:] = v
    x[:, 0] = (prm["cls"] + prm["pos"][0]).astype(np.float32)
    return x


def _lane_columns():
    """[2, 192]: the output columns lane half h of a token holds, in the order it adds them: 32 O + 8 q + 4 h + e"""
    O, q, e = np.meshgrid(np.arange(12), np.arange(4), np.arange(4), indexing="ij")
    return np.stack([(32 * O + 8 * q + 4 * h + e).reshape(-1) for h in (0, 1)])


def emulate_xn(x32, prm):
    """the LNOUT epilogue (token rows) and cls_init_img_kernel ([CLS] rows) in NumPy fp32 -> bf16 values [nseq, 257, 384] in float64"""
    x32 = np.asarray(x32, np.float32)
    g, b, eps = prm["ln_w"].astype(np.float32), prm["ln_b"].astype(np.float32), np.float32(prm["eps"])
    out = np.empty(x32.shape)

    def finish(v, mean, var):
        rstd = (np.float32(1.0) / np.sqrt(((var / np.float32(D)).astype(np.float32) + eps).astype(np.float32))).astype(np.float32)
        n = ((v - mean).astype(np.float32) * rstd).astype(np.float32)
        return P.rounded(_f32(n.astype(np.float64) * g + b), True)   # one fma, then the bf16 store

    v = x32[:, 1:]
    cols = _lane_columns()
    s = np.zeros(v.shape[:2] + (2,), np.float32)
    for i in range(192):
        s = (s + v[..., cols[:, i]]).astype(np.float32)
    mean = ((s[..., 0] + s[..., 1]).astype(np.float32) / np.float32(D)).astype(np.float32)[..., None]
    q = np.zeros(v.shape[:2] + (2,), np.float64)
    for i in range(192):
        d = (v[..., cols[:, i]] - mean).astype(np.float32).astype(np.float64)
        q = _f32(d * d + q).astype(np.float64)
    var = (q[..., 0].astype(np.float32) + q[..., 1].astype(np.float32)).astype(np.float32)[..., None]
    out[:, 1:] = finish(v, mean, var)

    c = x32[:, 0].reshape(-1, 6, 64)   # lane l owns elements l + 64 j
    s = np.zeros((c.shape[0], 64), np.float32)
    for j in range(6):
        s = (s + c[:, j]).astype(np.float32)
    mean = (P._wave_sum32(s) / np.float32(D)).astype(np.float32)
    q = np.zeros((c.shape[0], 64), np.float64)
    for j in range(6):
        d = (c[:, j] - mean).astype(np.float32).astype(np.float64)
        q = _f32(d * d + q).astype(np.float64)
    var = P._wave_sum32(q.astype(np.float32))
    out[:, 0] = finish(x32[:, 0], mean, var)
    return out


# =====================================================================================================================
# Cases
# =====================================================================================================================
# name -> logical tensor [B, 3, W, H], layout ("plain" | "region" | "window"), seq0, nseq, input kinds, outputs ("img": fp32 image + xn
# image, "rows": row-major), weight family.  nseq None: set by the device (multi); the host runs it with 16.
Case = namedtuple("Case", "name shape layout seq0 nseq kinds outs family")
CASES = {c.name: c for c in (
    Case("plain16", (16, 3, 256, 256), "plain", 0, 16, (F32, U8_CHW, U8_HWC), ("img", "rows"), "std"),
    Case("rows5", (5, 3, 256, 256), "plain", 0, 5, (F32, U8_CHW, U8_HWC), ("rows",), "std"),
    Case("region2x4", (2, 3, 512, 1024), "region", 0, 16, (F32, U8_CHW, U8_HWC), ("img",), "std"),
    Case("second_half", (2, 3, 1024, 1024), "region", 16, 16, (F32, U8_HWC), ("img",), "std"),
    Case("cross_2x3", (2, 3, 512, 768), "region", 3, 7, (F32, U8_CHW), ("rows",), "std"),
    Case("window", (2, 3, 512, 512), "window", 1, 6, (F32, U8_CHW, U8_HWC), ("rows",), "std"),
    Case("edge", (16, 3, 256, 256), "plain", 0, 16, (F32, U8_CHW), ("img",), "edge"),
    Case("multi", None, "plain", 0, None, (U8_CHW, F32), ("img", "rows"), "std"),
)}
WINDOW_PAD_ROW, WINDOW_PAD_CHAN, WINDOW_LEAD = 8, 64, 32   # elements (pixels): multiples of 8, so of 4; the lead keeps 16-byte alignment
WHITE, BLACK = 1, 2                                       # patches of the edge case that are all 255 / all 0


def case_layout(case, shape):
    _, _, W, H = shape
    if case.layout == "plain":
        return plain_layout(W, H)
    if case.layout == "region":
        return region_layout(W, H)
    rs = H + WINDOW_PAD_ROW
    return region_layout(W, H, rs, W * rs + WINDOW_PAD_CHAN)


def case_pixels(case, nseq=None, seed=None):
    """the logical uint8 tensor [B, 3, W, H] of a case.  edge: patch WHITE all 255, patch BLACK all 0"""
    shape = case.shape if case.shape is not None else (nseq, 3, 256, 256)
    u8 = synth.hash_u8_np(shape, 5000 + sum(map(ord, case.name)) if seed is None else seed)
    if case.name == "edge":
        u8[WHITE], u8[BLACK] = 255, 0
    return u8


def to_float(case, u8):
    """the fp32 tensor of the same byte values by the reference's normalisation; edge: the tokens of the near-constant class are 0"""
    f = normalize_u8(u8)
    if case.name == "edge":
        for t in edge_tokens()["near_const"]:
            ty, tx = divmod(int(t), 16)
            f[:, :, 16 * ty:16 * ty + 16, 16 * tx:16 * tx + 16] = 0.0
    return f


def store(logical, kind, lay, lead=0, tail=0):
    """the flat buffer a logical tensor [B, 3, W, H] lives in under `lay` (fp32: NaN wherever no pixel lies; uint8: 0xA5), written
    plane by plane and row by row; `lead` elements (interleaved: pixels) in front of the image origin -> (buffer, offset of the origin
    in elements of the buffer)"""
    B, _, W, H = logical.shape
    px = 3 if kind == U8_HWC else 1
    n = lead * px + B * lay.batch_stride + tail
    if lead == 0 and tail == 0 and lay.row_stride == H and lay.chan_stride == W * H:   # a whole contiguous tensor
        return np.ascontiguousarray(logical.transpose(0, 2, 3, 1) if kind == U8_HWC else logical).reshape(-1), 0
    buf = np.full(n, np.nan, np.float32) if kind == F32 else np.full(n, 0xA5, np.uint8)
    for b in range(B):
        for c in range(3):
            for y in range(W):
                if kind == U8_HWC:
                    o = (lead + b * (lay.batch_stride // 3) + y * lay.row_stride) * 3 + c
                    buf[o:o + 3 * H:3] = logical[b, c, y]
                else:
                    o = lead + b * lay.batch_stride + c * lay.chan_stride + y * lay.row_stride
                    buf[o:o + H] = logical[b, c, y]
    return buf, lead * px


def build(case, kind, nseq=None, u8=None):
    """-> (buffer, origin offset in buffer elements, layout, seq0, nseq) of a case for one input kind"""
    if u8 is None:
        u8 = case_pixels(case, nseq)
    lay = case_layout(case, u8.shape)
    logical = to_float(case, u8) if kind == F32 else u8
    buf, off = store(logical, kind, lay, WINDOW_LEAD if case.layout == "window" else 0)
    return buf, off, lay, case.seq0, (case.nseq if case.nseq is not None else nseq)
