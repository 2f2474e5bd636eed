"""Fine-grained operators of the HIP library as torch-tensor functions.

These are the units the parity tests exercise and what the sub-modules
(``Attention``, ``Mlp``, ``PatchEmbed`` ...) call when used on their own; the whole-model
forwards go through the coarse entry points (one C call per ViT / region / bag).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import torch

from . import _native as N

_TORCH_DT = {N.HIPT_F32: torch.float32, N.HIPT_BF16: torch.bfloat16}
_workspaces = {}


def torch_dtype(code: int):
    return _TORCH_DT[code]


def workspace(device, nbytes: int, slot=0, zero: bool = False) -> torch.Tensor:
    """Grow-only per-device scratch (the library itself never allocates).  ``slot``: one scratch per concurrent use (a
    stream handle, a part index).  ``zero``: allocate zero-filled -- for scratch that carries the CLAM ticket block
    (include/hipt_abmil.h: zero before the first call, left zero by every call)."""
    key = (device.type, device.index, slot)
    ws = _workspaces.get(key)
    if ws is None or ws.numel() < nbytes:
        n = max(int(nbytes), 1 << 20)
        ws = torch.zeros(n, dtype=torch.uint8, device=device) if zero else torch.empty(n, dtype=torch.uint8, device=device)
        _workspaces[key] = ws
    return ws


def as_compute(t: torch.Tensor, code: int) -> torch.Tensor:
    """Contiguous copy/view of ``t`` in the compute dtype (weights and GEMM inputs)."""
    return t.detach().to(_TORCH_DT[code]).contiguous()


def f32c(t):
    return None if t is None else t.detach().float().contiguous()


def layernorm(x: torch.Tensor, weight, bias, eps: float = 1e-6, out_dtype: int = N.HIPT_F32) -> torch.Tensor:
    """nn.LayerNorm over the last dim (vision_transformer.py:138,142,195)."""
    N.require_cuda(x, "layernorm")
    x2 = x.detach().float().contiguous().view(-1, x.shape[-1])
    out = torch.empty(x2.shape, dtype=_TORCH_DT[out_dtype], device=x.device)
    N.call("hipt_layernorm", N.ptr(x2), x2.shape[1], N.ptr(f32c(weight)), N.ptr(f32c(bias)), N.ptr(out), out_dtype,
           x2.shape[1], x2.shape[0], x2.shape[1], float(eps), N.stream_ptr(x.device))
    return out.view(x.shape)


def linear(a: torch.Tensor, weight: torch.Tensor, bias=None, resid=None, gelu=False, relu=False,
           out_f32=True, dtype: int = N.HIPT_F32) -> torch.Tensor:
    """``epilogue(a @ weight.T + bias)`` (nn.Linear, vision_transformer.py:93-95,114,116)."""
    N.require_cuda(a, "linear")
    a2 = as_compute(a, dtype).view(-1, a.shape[-1])
    w = as_compute(weight, dtype)
    M, K = a2.shape
    Nn = w.shape[0]
    flags = (N.EPI_GELU if gelu else 0) | (N.EPI_RELU if relu else 0) | (N.EPI_OUT_F32 if out_f32 else 0)
    r = None
    if resid is not None:
        r = resid.detach().float().contiguous().view(M, Nn)
        flags |= N.EPI_RESID
    out = torch.empty((M, Nn), dtype=torch.float32 if out_f32 else _TORCH_DT[dtype], device=a.device)
    b = f32c(bias)
    N.call("hipt_linear", N.ptr(a2), K, N.ptr(w), K, N.ptr(b), N.ptr(r), N.ptr(out), Nn, M, Nn, K, dtype, flags,
           N.stream_ptr(a.device))
    return out.view(*a.shape[:-1], Nn)


def attention(qkv: torch.Tensor, num_heads: int, scale: float, dtype: int = N.HIPT_F32, return_probs: bool = False):
    """softmax(q k^T * scale) v from the fused qkv projection output [B, N, 3*C]
    (vision_transformer.py:122-128).  Returns (out [B,N,C], probs [B,H,N,N] or None)."""
    N.require_cuda(qkv, "attention")
    B, ntok, C3 = qkv.shape
    Cc = C3 // 3
    q = as_compute(qkv, dtype)
    out = torch.empty((B, ntok, Cc), dtype=_TORCH_DT[dtype], device=qkv.device)
    probs = torch.empty((B, num_heads, ntok, ntok), dtype=torch.float32, device=qkv.device) if return_probs else None
    N.call("hipt_attention", N.ptr(q), N.ptr(out), N.ptr(probs), B, ntok, num_heads, Cc // num_heads, float(scale), dtype,
           N.stream_ptr(qkv.device))
    return out, probs


# ---- CLAM on one bag (include/hipt_abmil.h: hipt_clam_sb_forward, hipt_clam_mb_forward) ----
# form -> (native call, its workspace size, workspace slot, shapes of (A_raw, M, logits) for n rows, does the call write Y_prob / Y_hat)
_FORMS = {
    "sb": ("hipt_clam_sb_forward", "hipt_clam_workspace_bytes", "clam", lambda w, n: ((1, n), (1, w.s1), (1, w.n_classes)), True),
    "mb": ("hipt_clam_mb_forward", "hipt_clam_mb_workspace_bytes", "clam_mb", lambda w, n: ((w.n_att, n), (w.n_att, w.s1), (1, w.n_att)), False),
}


def clam_forward(w, bag: torch.Tensor, attention_only: bool = False, out=None, ws=None, form: str = "sb"):
    """The single-bag CLAM forward in the form ``"sb"`` or ``"mb"`` (the ``K = w.n_att`` branches of a stacked weight image in one pass) on
    ``bag [n >= 1, S0]``, contiguous, on the device, in the dtype of the weight image ``w``: NOT checked here, ``CLAM_SB._infer`` has.
    Returns ``(A_raw, M, logits, Y_prob, Y_hat)``; ``"mb"`` has no ``Y_prob`` / ``Y_hat`` (None: softmax and argmax over the K logits are
    the caller's), ``attention_only`` only ``A_raw``.  ``out``: the five to write into instead of fresh buffers; ``w`` and ``out`` may be
    lists of equal length: one call per pair on one stream and workspace (``CLAM_MB`` branch by branch, into row views of shared outputs).
    ``ws``: a zeroed workspace instead of the stream's own (it carries the partials and the finish ticket, left at zero by every call)."""
    sym, ws_sym, slot, shapes, heads = _FORMS[form]
    dev, n, st = bag.device, bag.shape[0], N.stream_ptr(bag.device)
    if ws is None:
        ws = workspace(dev, getattr(N.lib(), ws_sym)(C.byref(w[0] if isinstance(w, list) else w), n), (slot, st.value), zero=True)
    if out is None:
        (a, m, l), e = shapes(w, n), torch.empty
        out = ((e(a, dtype=torch.float32, device=dev), None, None, None, None) if attention_only else
               (e(a, dtype=torch.float32, device=dev), e(m, dtype=torch.float32, device=dev), e(l, dtype=torch.float32, device=dev)) +
               ((e(l, dtype=torch.float32, device=dev), e((1, 1), dtype=torch.int64, device=dev)) if heads else (None, None)))
    for w, (A_raw, M, logits, Y_prob, Y_hat) in (zip(w, out) if isinstance(w, list) else ((w, out),)):
        own = (N.ptr(Y_prob), N.ptr(Y_hat)) if heads else ()
        N.call(sym, C.byref(w), N.ptr(bag), n, 1 if attention_only else 0, N.ptr(A_raw), N.ptr(M), N.ptr(logits), *own, N.ptr(ws), ws.numel(), st)
    return out


# ---- CLAM over many bags in one call (include/hipt_abmil.h: hipt_clam_sb_forward_bags and its narrow / CLAM_MB forms) ----
def check_offsets(offsets, rows: int) -> tuple:
    """The B+1 row offsets of a multi-bag call as a tuple of ints, or ``ValueError``: they start at 0, increase strictly (no
    empty bag) and end at ``rows``.  The library trusts what it is handed, so every upload goes through here first."""
    if isinstance(offsets, torch.Tensor):
        offsets = offsets.detach().cpu().tolist()
    off = tuple(int(v) for v in offsets)
    if len(off) < 2 or off[0] != 0:
        raise ValueError(f"bag offsets must be B+1 >= 2 numbers starting at 0, got {off[:4]}{'...' if len(off) > 4 else ''}")
    for b in range(len(off) - 1):
        if off[b + 1] < off[b]:
            raise ValueError(f"bag offsets decrease at bag {b}: {off[b]} -> {off[b + 1]}")
        if off[b + 1] == off[b]:
            raise ValueError(f"bag {b} is empty (offsets {off[b]} == {off[b + 1]}): every bag needs at least one row")
    if off[-1] != int(rows):
        raise ValueError(f"bag offsets end at {off[-1]} but the concatenated bags have {int(rows)} rows")
    return off


class BagOffsets:
    """Checked offsets of a multi-bag call: ``host`` (tuple of B+1 ints) and ``dev`` (the same, int64 on the device).  Make it
    once -- outside a graph capture: the upload is a host-to-device copy -- and hand it to every call over bags of these sizes."""
    __slots__ = ("host", "dev")

    def __init__(self, offsets, rows: int, device):
        self.host = check_offsets(offsets, rows)
        self.dev = torch.tensor(self.host, dtype=torch.int64, device=device)

    def __len__(self):
        return len(self.host) - 1


# One row per form of the multi-bag call, in routing priority (``CLAM_SB._bags_form`` walks the rows of the model's kind in this order and
# takes the first whose switches are all set on the model and whose predicate answers 1): the C entry point, its workspace size, its
# ``*_supported`` predicate, whether the outputs have the K-branch shapes, the model kind, the model switches the form needs, and the
# heads it serves (documentation: the predicate decides).
BagsForm = namedtuple("BagsForm", "name entry ws_bytes supported multi kind switches heads")
_BAGS_FORMS = {f.name: f for f in (
    BagsForm("sb", "hipt_clam_sb_forward_bags", "hipt_clam_bags_workspace_bytes", "hipt_clam_bags_supported", False, "CLAM_SB", (),
             "S1 in {128, 64}, in fp32 also 32, with S2 in {64, 32, 16}"),
    BagsForm("narrow", "hipt_clam_sb_forward_bags_narrow", "hipt_clam_narrow_bags_workspace_bytes", "hipt_clam_narrow_bags_supported", False, "CLAM_SB",
             ("bags_narrow",), "the narrow heads, (S1, S2) in {(8, 4), (16, 8), (32, 8), (32, 16)}"),
    BagsForm("wide", "hipt_clam_sb_forward_bags_wide", "hipt_clam_wide_bags_workspace_bytes", "hipt_clam_wide_bags_supported", False, "CLAM_SB",
             ("bags_wide",), "the wide heads, (S1, S2) in {(256, 64), (512, 256), (512, 384)}"),
    BagsForm("mb", "hipt_clam_mb_forward_bags", "hipt_clam_mb_bags_workspace_bytes", "hipt_clam_mb_bags_supported", True, "CLAM_MB",
             ("bags_one_call",), "2 to 4 branches at the widths of ``hipt_clam_sb_forward_bags``"),
    BagsForm("mb_many", "hipt_clam_mb_forward_bags_many", "hipt_clam_mb_many_bags_workspace_bytes", "hipt_clam_mb_many_bags_supported", True, "CLAM_MB",
             ("bags_one_call", "bags_many"), "5 to 8 branches at the widths of ``hipt_clam_sb_forward_bags``; branch ``k`` has the bits that "
             "``hipt_clam_mb_forward_bags`` gives it on weights made of a subset of the branches"),
    BagsForm("mb_wide", "hipt_clam_mb_forward_bags_wide", "hipt_clam_mb_wide_bags_workspace_bytes", "hipt_clam_mb_wide_bags_supported", True, "CLAM_MB",
             ("bags_one_call", "bags_wide"), "2 to 4 branches at the widths of ``hipt_clam_sb_forward_bags_wide``"),
)}
BAGS_FORMS_OF = {kind: tuple(f for f in _BAGS_FORMS.values() if f.kind == kind) for kind in ("CLAM_SB", "CLAM_MB")}  # a kind's rows, in routing order
BAGS_FORMS_K = tuple(f.name for f in _BAGS_FORMS.values() if f.multi)  # the forms with K = w.n_att rows of A_raw and K pooled vectors per bag


def bags_shapes(form: str, w, B: int, rows: int) -> tuple:
    """Shapes of ``(A_raw, M, logits / Y_prob)`` of a multi-bag call in ``form`` for B bags of ``rows`` rows in all; ``Y_hat`` is ``[B]``."""
    if _BAGS_FORMS[form].multi:
        return (w.n_att, rows), (B, w.n_att, w.s1), (B, w.n_att)
    return (rows,), (B, w.s1), (B, w.n_classes)


def clam_forward_bags(w, cat: torch.Tensor, offsets: BagOffsets, attention_only: bool = False, out=None, ws=None, form: str = "sb"):
    """The multi-bag CLAM forward in a form of ``_BAGS_FORMS`` (include/hipt_abmil.h) on ``cat [rows, S0]``, already
    in the dtype of the weight image ``w`` (an ``_native.ClamWeights``).  Returns ``(A_raw, M, logits, Y_prob, Y_hat)`` -- the last
    four ``None`` with ``attention_only``.  ``out`` / ``ws``: buffers to write into instead of fresh ones (tests: guard regions,
    sentinels)."""
    sym, ws_sym = _BAGS_FORMS[form].entry, _BAGS_FORMS[form].ws_bytes
    what = sym[len("hipt_"):]
    N.require_cuda(cat, what)
    dev, B, rows = cat.device, len(offsets), cat.shape[0]
    if cat.dim() != 2 or not cat.is_contiguous() or cat.dtype != _TORCH_DT[w.dtype] or cat.shape[1] != w.s0:
        raise ValueError(f"expected contiguous [rows, {w.s0}] bags in {_TORCH_DT[w.dtype]}, got {tuple(cat.shape)} {cat.dtype}")
    if offsets.host[-1] != rows:
        raise ValueError(f"bag offsets end at {offsets.host[-1]} but the concatenated bags have {rows} rows")
    N.same_device(what, dev, offsets.dev)
    st = N.stream_ptr(dev)
    if ws is None:
        ws = workspace(dev, getattr(N.lib(), ws_sym)(C.byref(w), B, rows), ("clam_bags", st.value))
    if out is None:
        e = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
        a, m, l = bags_shapes(form, w, B, rows)
        out = (e(a), None, None, None, None) if attention_only else (e(a), e(m), e(l), e(l), e((B,), torch.int64))
    A_raw, M, logits, Y_prob, Y_hat = out
    N.call(sym, C.byref(w), N.ptr(cat), N.ptr(offsets.dev), B, rows, 1 if attention_only else 0, N.ptr(A_raw), N.ptr(M), N.ptr(logits),
           N.ptr(Y_prob), N.ptr(Y_hat), N.ptr(ws), ws.numel(), st)
    return out


def _bags_wrapper(form: str):
    """``clam_forward_bags`` in one form, under the name of its entry point and with the form's heads and result shapes as its docstring"""
    f = _BAGS_FORMS[form]

    def call(w, cat: torch.Tensor, offsets: BagOffsets, attention_only: bool = False, out=None, ws=None):
        return clam_forward_bags(w, cat, offsets, attention_only, out, ws, form)

    shapes = ("``(A_raw [K, rows], M [B, K, S1], logits [B, K], Y_prob [B, K], Y_hat [B])`` for the ``K = w.n_att`` branches of a stacked ``CLAM_MB`` "
              "weight image; bag ``b`` is the columns ``[offsets[b], offsets[b+1])`` of ``A_raw``" if f.multi else
              "``(A_raw [rows], M [B, S1], logits [B, C], Y_prob [B, C], Y_hat [B])``")
    call.__name__ = call.__qualname__ = f.entry[len("hipt_"):]
    call.__doc__ = f"``{f.entry}`` for {f.heads} (``{f.supported}``; fp32 and bf16).  Returns {shapes}."
    return call


clam_sb_forward_bags = _bags_wrapper("sb")
clam_sb_forward_bags_narrow = _bags_wrapper("narrow")
clam_sb_forward_bags_wide = _bags_wrapper("wide")
clam_mb_forward_bags = _bags_wrapper("mb")
clam_mb_forward_bags_many = _bags_wrapper("mb_many")
clam_mb_forward_bags_wide = _bags_wrapper("mb_wide")


def topk_segments(A: torch.Tensor, offsets: BagOffsets, k: int, want_global: bool = True):
    """``hipt_topk_segments`` on the scores of a multi-bag call, ``A [rows]`` or ``[K, rows]`` fp32: ``(ids, global_ids)``, int64
    ``[B, K, 2, k]`` each -- per bag and branch the ids of the k largest and of the k smallest scores (ties: lowest index first),
    bag-local and as rows of the concatenated matrix (None unless ``want_global``).  A bag with fewer than ``k`` rows raises
    before anything is launched, with the text of ``torch.topk`` in ``forward``."""
    N.require_cuda(A, "topk_segments")
    A2 = A.reshape(1, -1) if A.dim() == 1 else A
    if A2.dim() != 2 or A2.dtype != torch.float32 or not A2.is_contiguous() or A2.shape[1] != offsets.host[-1]:
        raise ValueError(f"expected contiguous fp32 scores [K, {offsets.host[-1]}], got {tuple(A.shape)} {A.dtype}")
    for b in range(len(offsets)):
        n = offsets.host[b + 1] - offsets.host[b]
        if k > n:
            raise RuntimeError(f"selected index k out of range: k_sample={k} > {n} rows (torch.topk, model_clam.py:120)")
    N.same_device("topk_segments", A.device, offsets.dev)
    B, K = len(offsets), A2.shape[0]
    ids = torch.empty((B, K, 2, k), dtype=torch.int64, device=A.device)
    gids = torch.empty_like(ids) if want_global else None
    N.call("hipt_topk_segments", N.ptr(A2), A2.shape[1], N.ptr(offsets.dev), B, K, k, N.ptr(ids), N.ptr(gids), N.stream_ptr(A.device))
    return ids, gids
