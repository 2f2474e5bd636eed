"""Macenko stain normalisation of uint8 RGB images on the HIP library (csrc/macenko.hip).

The reference's ``--use_transforms macenko`` route (extract_features_fp.py:41-60) runs torchstain's
``MacenkoNormalizer(backend='torch')`` on every dataset item on the CPU.  Here a batch of resident uint8 images is fitted and
normalised on the device: ``macenko_fit`` gives each image's stain matrix ``HE``, its 99th-percentile concentrations ``maxC`` and
a ``status`` (0, or 1 = fallback: the image passes through unchanged, as the reference's ``except`` passes ``image / 255`` on);
``macenko_apply`` maps an image to a target; ``macenko_normalize`` does both on one stream without a host synchronisation.
The arithmetic is stated in include/hipt_abmil.h; percentiles are exact order statistics.

The reference's ``MacenkoNormalisation.__call__`` forgets its ``return``.  What it evidently means is implemented:
``norm.permute(2, 0, 1) / 255``, a ``[3, h, w]`` float in [0, 1] with NO mean / std normalisation after it --
``macenko_normalize(x, out_dtype=torch.float32)``.

torchstain is not part of this environment: agreement with its bytes is argued, not measured.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _frontend as F
from . import _native as N

HE_REF = ((0.5626, 0.2159), (0.7201, 0.8012), (0.4062, 0.5581))
MAXC_REF = (1.9705, 1.0308)


def _images(x, what: str) -> Tuple[torch.Tensor, bool, int, int, bool]:
    """(x as a batch, interleaved, h, w, batched); ValueError for anything but uint8 RGB [.., 3, h, w] / [.., h, w, 3]"""
    il, h, w = F.rgb_layout(what, x)
    batched = x.dim() == 4
    xb = x if batched else x[None]
    if xb.shape[0] < 1 or h * w < 1 or h * w >= 1 << 31:
        raise ValueError(f"{what}: {xb.shape[0]} images of {h} x {w} pixels (at least one, h * w below 2^31)")
    return xb, il, h, w, batched


def _check_params(what: str, Io, alpha, beta) -> Tuple[float, float, float]:
    try:
        Io, alpha, beta = float(Io), float(alpha), float(beta)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: Io / alpha / beta are numbers") from None
    if not (Io > 0 and Io < float("inf")):
        raise ValueError(f"{what}: Io = {Io} is not positive")
    if not 0 < alpha < 50:
        raise ValueError(f"{what}: alpha = {alpha} is outside (0, 50)")
    if not (beta >= 0 and beta < float("inf")):
        raise ValueError(f"{what}: beta = {beta} is negative")
    return Io, alpha, beta


def _check_target(what: str, target, dev):
    """(HE float32 [6] or None, maxC float32 [2] or None) on ``dev``; ``target`` is None or a (HE, maxC) pair of ONE image"""
    if target is None:
        return None, None
    try:
        he, mc = target
    except (TypeError, ValueError):
        raise ValueError(f"{what}: target is None or a (HE, maxC) pair") from None
    he, mc = torch.as_tensor(he), torch.as_tensor(mc)
    if he.numel() != 6 or tuple(he.shape[-2:]) != (3, 2) or mc.numel() != 2:
        raise ValueError(f"{what}: target is (HE [3, 2], maxC [2]) of one image, got {list(he.shape)} and {list(mc.shape)}")
    return he.to(device=dev, dtype=torch.float32).reshape(6).contiguous(), mc.to(device=dev, dtype=torch.float32).reshape(2).contiguous()


def _out_shape(what: str, out, x, xb, h, w, batched, out_dtype):
    """The result's shape; a given ``out`` is checked against it here, before the question for a device."""
    if out_dtype not in (torch.uint8, torch.float32):
        raise ValueError(f"{what}: out_dtype is torch.uint8 or torch.float32, got {out_dtype}")
    if out_dtype == torch.uint8:
        shape = tuple(x.shape)
    else:   # the reference route's tensor: planar whatever the input's layout
        shape = (xb.shape[0], 3, h, w) if batched else (3, h, w)
    if out is not None:
        F.check_out(what, out, shape, out_dtype, x.device, not_alias=(x,))
    return shape


def macenko_fit(x_u8, Io=240, alpha=1, beta=0.15, *, _aux=False):
    """``(HE float32 [R, 3, 2], maxC float32 [R, 2], status int32 [R])`` of every image of ``x_u8`` -- uint8 RGB on a HIP device,
    planar ``[R, 3, h, w]`` or interleaved ``[R, h, w, 3]``; one image (``[3, h, w]`` / ``[h, w, 3]``) gives ``R = 1`` -- as
    device tensors; nothing is copied to the host.  ``status`` 1 marks a fallback image (fewer than two tissue pixels, or a
    degenerate fit); its ``HE`` and ``maxC`` are zeros.  ``(HE[i], maxC[i])`` is a ``target`` for the other two functions:
    torchstain's ``normalizer.fit(target_image)``.  ValueError -- before any native call -- for float input, another shape, a
    CPU tensor, ``Io <= 0``, ``alpha`` outside (0, 50) or ``beta < 0``."""
    xb, il, h, w, _ = _images(x_u8, "macenko_fit")
    Io, alpha, beta = _check_params("macenko_fit", Io, alpha, beta)
    dev, r = F.resolve_device("macenko_fit", None, (xb,), exc=ValueError), int(xb.shape[0])
    src = xb.detach().contiguous()
    with torch.cuda.device(dev):
        he = torch.empty((r, 3, 2), dtype=torch.float32, device=dev)
        mc = torch.empty((r, 2), dtype=torch.float32, device=dev)
        st = torch.empty((r,), dtype=torch.int32, device=dev)
        aux = torch.empty((r, 16), dtype=torch.float32, device=dev) if _aux else None
        ws, need = F.scratch("hipt_macenko_workspace_bytes", r, h, w, dev=dev)
        N.call("hipt_macenko_fit", N.ptr(src), int(il), r, h, w, Io, alpha, beta, N.ptr(he), N.ptr(mc), N.ptr(st), N.ptr(aux), N.ptr(ws), need,
               N.stream_ptr(dev))
    return (he, mc, st, aux) if _aux else (he, mc, st)


def macenko_apply(x_u8, HE, maxC, status=None, target=None, out=None, out_dtype=torch.uint8, Io=240):
    """Every image of ``x_u8`` mapped from its own stains (``HE [R, 3, 2]``, ``maxC [R, 2]``, as ``macenko_fit`` returns them) to
    ``target`` -- ``None`` for torchstain's reference constants, or the ``(HE [3, 2], maxC [2])`` of one fitted image.  Images
    whose ``status`` is not 0 are copied through.  ``out_dtype=torch.uint8``: the input's shape and layout;
    ``torch.float32``: planar ``[R, 3, h, w]`` (``[3, h, w]`` for one image) equal to the uint8 result / 255."""
    xb, il, h, w, batched = _images(x_u8, "macenko_apply")
    Io, _, _ = _check_params("macenko_apply", Io, 1, 0)
    shape = _out_shape("macenko_apply", out, x_u8, xb, h, w, batched, out_dtype)
    r = int(xb.shape[0])
    if not torch.is_tensor(HE) or not torch.is_tensor(maxC) or HE.numel() != 6 * r or maxC.numel() != 2 * r:
        raise ValueError(f"macenko_apply: HE is [{r}, 3, 2] and maxC [{r}, 2], one per image")
    if status is not None and (not torch.is_tensor(status) or status.numel() != r):
        raise ValueError(f"macenko_apply: status is int32 [{r}]")
    dev = F.resolve_device("macenko_apply", None, (xb,), exc=ValueError)
    ref_he, ref_mc = _check_target("macenko_apply", target, dev)
    he = HE.to(device=dev, dtype=torch.float32).contiguous()
    mc = maxC.to(device=dev, dtype=torch.float32).contiguous()
    st = None if status is None else status.to(device=dev, dtype=torch.int32).contiguous()
    src = xb.detach().contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=dev)
        N.call("hipt_macenko_apply", N.ptr(src), int(il), r, h, w, Io, N.ptr(he), N.ptr(mc), N.ptr(st), N.ptr(ref_he), N.ptr(ref_mc),
               N.ptr(out), int(out_dtype == torch.float32), N.stream_ptr(dev))
    return out


def macenko_normalize(x_u8, Io=240, alpha=1, beta=0.15, target=None, out=None, out_dtype=torch.uint8, return_status=False):
    """``macenko_fit`` then ``macenko_apply`` in one native call: launches on the current stream only, no host
    synchronisation, so a call with a preallocated ``out`` can be captured into a graph.  Bit for bit what the two functions
    give one after the other.  Returns the normalised images (``out``, where given), with ``return_status=True`` the pair
    ``(images, status int32 [R])``.  Arguments as in the two functions."""
    xb, il, h, w, batched = _images(x_u8, "macenko_normalize")
    Io, alpha, beta = _check_params("macenko_normalize", Io, alpha, beta)
    shape = _out_shape("macenko_normalize", out, x_u8, xb, h, w, batched, out_dtype)
    dev, r = F.resolve_device("macenko_normalize", None, (xb,), exc=ValueError), int(xb.shape[0])
    ref_he, ref_mc = _check_target("macenko_normalize", target, dev)
    src = xb.detach().contiguous()
    with torch.cuda.device(dev):
        if out is None:
            out = torch.empty(shape, dtype=out_dtype, device=dev)
        st = torch.empty((r,), dtype=torch.int32, device=dev) if return_status else None
        ws, need = F.scratch("hipt_macenko_workspace_bytes", r, h, w, dev=dev)
        N.call("hipt_macenko_normalize", N.ptr(src), int(il), r, h, w, Io, alpha, beta, N.ptr(ref_he), N.ptr(ref_mc), N.ptr(out),
               int(out_dtype == torch.float32), None, None, N.ptr(st), N.ptr(ws), need, N.stream_ptr(dev))
    return (out, st) if return_status else out


def macenko_keys(x_u8, aux, Io=240, beta=0.15):
    """For tests: ``(keys float32 [R, 3, h * w], tissue uint8 [R, h * w])`` -- phi, C[0], C[1] of every pixel exactly as the
    select passes compute them from ``aux`` (``macenko_fit(..., _aux=True)[3]``)."""
    xb, il, h, w, _ = _images(x_u8, "macenko_keys")
    Io, _, beta = _check_params("macenko_keys", Io, 1, beta)
    dev, r = F.resolve_device("macenko_keys", None, (xb,), exc=ValueError), int(xb.shape[0])
    src = xb.detach().contiguous()
    aux = aux.to(device=dev, dtype=torch.float32).contiguous()
    with torch.cuda.device(dev):
        keys = torch.empty((r, 3, h * w), dtype=torch.float32, device=dev)
        tissue = torch.empty((r, h * w), dtype=torch.uint8, device=dev)
        N.call("hipt_macenko_keys", N.ptr(src), int(il), r, h, w, Io, beta, N.ptr(aux), N.ptr(keys), N.ptr(tissue), N.stream_ptr(dev))
    return keys, tissue


class MacenkoNormalizer:
    """torchstain's call surface for ``stains=False``: ``fit(target)``, then ``normalize(I) -> (norm, None, None)``.

    ``I`` is ``[3, h, w]`` with values 0..255, float or uint8, as the reference hands it over (``ToTensor`` then ``* 255``); it
    is rounded to uint8 and moved to ``device`` (default: the current HIP device) when it is not there.  ``norm`` is
    ``[h, w, 3]`` int32 on that device.  A fallback image comes back as its own bytes (torchstain raises there and the
    reference's ``except`` passes the image on).  ``stains=True`` (the separate H and E images) raises NotImplementedError."""

    def __init__(self, device=None):
        self.device = device
        self.target = None

    def _u8(self, I):
        if not torch.is_tensor(I) or I.dim() != 3 or I.shape[0] != 3:
            raise ValueError(f"MacenkoNormalizer: I is [3, h, w] with values 0..255, got {list(getattr(I, 'shape', []))}")
        dev = F.resolve_device("MacenkoNormalizer", self.device, (I,), exc=ValueError, staged=True)
        if I.dtype != torch.uint8:
            I = I.round().clamp(0, 255).to(torch.uint8)
        return I.to(dev)

    def fit(self, I, Io=240, alpha=1, beta=0.15):
        he, mc, status = macenko_fit(self._u8(I), Io, alpha, beta)
        if int(status[0]) != 0:
            raise ValueError("MacenkoNormalizer.fit: the target image has no stain plane (fewer than two tissue pixels, or degenerate)")
        self.target = (he[0], mc[0])
        return self

    def normalize(self, I, Io=240, alpha=1, beta=0.15, stains=False):
        if stains:
            raise NotImplementedError("MacenkoNormalizer.normalize: stains=True (the separate H and E images) is not implemented")
        out = macenko_normalize(self._u8(I), Io, alpha, beta, target=self.target)
        return out.permute(1, 2, 0).to(torch.int32), None, None


__all__ = ["macenko_fit", "macenko_apply", "macenko_normalize", "MacenkoNormalizer", "HE_REF", "MAXC_REF"]
