"""On-device ``all`` / ``spatial`` region augmentation (``--use_transforms all | spatial`` of ``extract_features_fp.py:63-82``).

The two policies of the reference's ResNet routes put ``ToTensor()`` first, so every step is torchvision's TENSOR code in
float32 -- not the PIL code of the ``HIPT_*`` policies (``augment.py``): flips, ``RandomAffine`` as a normalised grid read through
``grid_sample(mode='nearest')``, for ``all`` ``ColorJitter``'s float blends and float HSV round trip, then ``Normalize``.  The
random parameters of a region are drawn on the host exactly as ``augment.draw_params`` draws them (same helper, same order, one
generator per (seed, slide, k, region index)); the pixels are transformed by ``hipt_augment_tensor`` (csrc/tensor_augment.hip),
uint8 in -- planar ``[R,3,rows,cols]`` or interleaved ``[R,rows,cols,3]`` -- float32 planar ``[R,3,rows,cols]`` out, already
normalised: what the ResNet extractors and ``HIPT_4K`` take as float input.  DESIGN.md section 28 states the arithmetic.

torchvision is not part of this environment: agreement with its bytes is argued from its source, not measured.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from . import _frontend as F
from . import _native as N
from .augment import (AFFINE, HFLIP, OP_BRIGHTNESS, OP_CONTRAST, OP_HUE, OP_SATURATION, VFLIP, _jitter, draw_spec,  # noqa: F401
                      inverse_affine_matrix, region_seed)
from .resnet_custom import IMAGENET_MEAN, IMAGENET_STD

_AFFINE = dict(degrees=(-90.0, 90.0), translate=(0.1, 0.1), scale=(0.9, 1.1), shear=(-0.1, 0.1))
# policy name -> steps in the reference's order (extract_features_fp.py:63-82), in the form of augment.POLICIES
TENSOR_POLICIES = {
    "all": dict(flip=0.5, affine=_AFFINE, jitter=_jitter(0.1, 0.1, 0.1, 0.1)),
    "spatial": dict(flip=0.5, affine=_AFFINE),
}


class TensorAugmentParams(C.Structure):
    """mirror of ``hipt_tensor_augment_params`` (include/hipt_abmil.h)"""
    _fields_ = [("theta", C.c_float * 6), ("factor", C.c_float * 3), ("hue", C.c_float), ("flags", C.c_int32), ("n_ops", C.c_int32),
                ("ops", C.c_int32 * 4), ("mean", C.c_float * 3), ("std", C.c_float * 3), ("reserved", C.c_int32 * 2)]


@dataclass
class TensorRegionParams:
    """One region's drawn parameters (what torchvision's transforms would have drawn for it on a tensor)."""
    hflip: bool = False
    vflip: bool = False
    theta: Optional[Tuple[float, ...]] = None    # _get_inverse_affine_matrix about [0, 0] (6 doubles) or None
    order: Tuple[int, ...] = ()                  # colour ops that are on, in application order (OP_*)
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue: float = 0.0                             # torchvision hue_factor, added to h in [0, 1) modulo 1
    draws: dict = field(default_factory=dict)    # the raw draws (angle, translate, scale, shear, perm), for inspection

    def record(self, mean=IMAGENET_MEAN, std=IMAGENET_STD) -> TensorAugmentParams:
        p = TensorAugmentParams()
        p.flags = (HFLIP if self.hflip else 0) | (VFLIP if self.vflip else 0) | (AFFINE if self.theta is not None else 0)
        if self.theta is not None:
            for i, v in enumerate(self.theta):
                p.theta[i] = v                   # (ctypes rounds the double to float32, as torch.tensor(matrix, dtype=float32) does)
        p.factor[0], p.factor[1], p.factor[2] = self.brightness, self.contrast, self.saturation
        p.hue = self.hue
        p.n_ops = len(self.order)
        for i, op in enumerate(self.order):
            p.ops[i] = op
        for i in range(3):
            p.mean[i], p.std[i] = mean[i], std[i]
        return p


def draw_tensor_params(policy: str, generator: torch.Generator, rows: int, cols: int) -> TensorRegionParams:
    """Draw one region's parameters in torchvision's order (``augment.draw_spec``: flips, angle / tx / ty / scale / shear_x,
    then for ``all`` ``randperm(4)`` and b, c, s, h).  The matrix is ``_get_inverse_affine_matrix`` about ``[0, 0]``: the tensor path
    works in coordinates centred on the image."""
    if policy not in TENSOR_POLICIES:
        raise ValueError(f"unknown tensor augmentation policy {policy!r}; known: {sorted(TENSOR_POLICIES)}")
    p = draw_spec(TENSOR_POLICIES[policy], generator, rows, cols, TensorRegionParams())
    d = p.draws
    p.theta = tuple(inverse_affine_matrix([0.0, 0.0], d["angle"], [float(v) for v in d["translate"]], d["scale"], d["shear"]))
    return p


def draw_tensor_region_params(policy: str, seed: int, slide_id: str, k: int, first: int, count: int, rows: int,
                              cols: int) -> List[TensorRegionParams]:
    """parameters of regions first .. first+count-1 of a slide for augmentation k: one generator per region
    (``augment.region_seed``), so the draws do not depend on how the regions are batched"""
    out = []
    for i in range(first, first + count):
        g = torch.Generator()
        g.manual_seed(region_seed(seed, slide_id, k, i))
        out.append(draw_tensor_params(policy, g, rows, cols))
    return out


def _check_norm(mean, std) -> Tuple[Tuple[float, ...], Tuple[float, ...]]:
    try:
        mean, std = tuple(float(v) for v in mean), tuple(float(v) for v in std)
    except (TypeError, ValueError):
        raise ValueError("augment_tensor: mean / std are three numbers each") from None
    if len(mean) != 3 or len(std) != 3 or any(not abs(v) < float("inf") for v in mean + std) or any(v == 0 for v in std):
        raise ValueError(f"augment_tensor: mean / std are three finite numbers each, std not 0, got {mean} and {std}")
    return mean, std


def pack_tensor_records(params: Sequence[TensorRegionParams], mean=IMAGENET_MEAN, std=IMAGENET_STD) -> torch.Tensor:
    """the parameter records as a host uint8 tensor (pinned: the device copy is asynchronous)"""
    arr = (TensorAugmentParams * len(params))(*[p.record(mean, std) for p in params])
    host = torch.empty(C.sizeof(arr), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    C.memmove(host.data_ptr(), C.addressof(arr), C.sizeof(arr))
    return host


def augment_tensor(regions_u8: torch.Tensor, params: Sequence[TensorRegionParams], mean=IMAGENET_MEAN, std=IMAGENET_STD,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``regions_u8`` (uint8 on a HIP device, planar ``[R,3,rows,cols]`` or interleaved ``[R,rows,cols,3]``) with region i
    transformed by ``params[i]`` and normalised: float32 planar ``[R,3,rows,cols]``.  One launch, or two when a record holds a
    contrast op (its mean needs a pass of its own).  ValueError -- before any native call -- for a CPU tensor, a dtype other than
    uint8, a shape that is not a batch of RGB regions, the wrong number of records or an ``out`` that does not fit."""
    interleaved, rows, cols = F.rgb_layout("augment_tensor", regions_u8, dims=(4,))
    n = int(regions_u8.shape[0])
    if len(params) != n:
        raise ValueError(f"augment_tensor: {n} regions but {len(params)} parameter records")
    if rows < 1 or cols < 1 or rows * cols > 1 << 30:
        raise ValueError(f"augment_tensor: regions of {rows} x {cols} pixels (at least one, rows * cols at most 2^30)")
    mean, std = _check_norm(mean, std)
    dev = F.resolve_device("augment_tensor", None, (regions_u8,), exc=ValueError)   # (a CPU tensor is refused here)
    src = regions_u8.detach().contiguous()
    with torch.cuda.device(dev):
        dst = F.check_out("augment_tensor", out, (n, 3, rows, cols), torch.float32, dev, not_alias=(src,))
        if n == 0:
            return dst
        rec = pack_tensor_records(params, mean, std).to(dev, non_blocking=True)
        ws, need = None, 0
        if any(OP_CONTRAST in p.order for p in params):   # the mean of contrast: the two-pass route and its partial sums
            ws, need = F.scratch("hipt_augment_tensor_workspace_bytes", n, rows, cols, dev=dev)
        N.call("hipt_augment_tensor", N.ptr(src), int(interleaved), n, rows, cols, N.ptr(rec), N.ptr(dst), N.ptr(ws), need, N.stream_ptr(dev))
        cur = torch.cuda.current_stream(dev)
        for t in (src, rec) + (() if ws is None else (ws,)):  # (allocator: these stay alive until the kernel has read them)
            t.record_stream(cur)
    return dst


class TensorAugment:
    """``TensorAugment(policy, seed)(regions, slide_id, k, first)``: device uint8 batch -> augmented, normalised float32 planar
    batch, regions numbered ``first, first+1, ...`` within the slide (their parameters depend on that number, not on the batch)."""

    def __init__(self, policy: str, seed: int = 0, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        if policy not in TENSOR_POLICIES:
            raise ValueError(f"unknown tensor augmentation policy {policy!r}; known: {sorted(TENSOR_POLICIES)}")
        self.policy, self.seed = policy, int(seed)
        self.mean, self.std = _check_norm(mean, std)

    def params(self, slide_id: str, k: int, first: int, count: int, rows: int, cols: int) -> List[TensorRegionParams]:
        return draw_tensor_region_params(self.policy, self.seed, slide_id, k, first, count, rows, cols)

    def __call__(self, regions: torch.Tensor, slide_id: str = "", k: int = 1, first: int = 0) -> torch.Tensor:
        _, rows, cols = F.rgb_layout("TensorAugment", regions, dims=(4,))
        return augment_tensor(regions, self.params(slide_id, k, first, regions.shape[0], rows, cols), self.mean, self.std)
