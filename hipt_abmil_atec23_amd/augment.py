"""On-device ``HIPT_*`` region augmentation (the ``--use_transforms`` switch of ``extract_features_fp.py:89-136``).

The reference augments each region on the CPU with torchvision transforms on a PIL image before ``eval_transforms``.  Here
the random parameters of a region are drawn on the host, in torchvision's draw order, from a ``torch.Generator`` seeded per
(seed, slide, augmentation index k, region index in the slide); the pixels are then transformed on the device by ONE kernel
(``hipt_augment_regions``), uint8 in, uint8 out, planar ``[R,3,rows,cols]`` or interleaved ``[R,rows,cols,3]``.  The kernel is a
pure function of (region bytes, parameter record) and reproduces what torchvision + Pillow write for the same parameters
(DESIGN.md section 10 states the arithmetic).  Only raw RGB can be augmented faithfully: float input raises ``ValueError``.

In Pillow terms the width of a region is ``cols`` and its height ``rows``: HFlip reverses ``cols``, the affine's image size is
``[cols, rows]``.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import torch

from . import _frontend as F
from . import _native as N

HFLIP, VFLIP, AFFINE, BLUR = 1, 2, 4, 8                       # hipt_augment_params.flags
OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = 0, 1, 2, 3  # ColorJitter's fn_id


def _jitter(b, c, s, h):
    """ColorJitter's ranges (torchvision ``_check_input``): a factor of 0 is off (None: not drawn)."""
    rng = lambda v, centre: None if v == 0 else ((max(0.0, centre - v), centre + v) if centre == 1 else (-v, v))
    return (rng(b, 1), rng(c, 1), rng(s, 1), rng(h, 0))


# policy name -> steps in the reference's order (extract_features_fp.py:89-136); None = identity
POLICIES = {
    "HIPT": None,
    "none": None,
    "HIPT_augment": dict(flip=0.5, affine=dict(degrees=(-5.0, 5.0), translate=(0.025, 0.025), scale=(0.975, 1.025), shear=(-0.025, 0.025)),
                         jitter=_jitter(0.2, 0.2, 0.2, 0.2)),
    "HIPT_augment01": dict(flip=0.5, affine=dict(degrees=(-5.0, 5.0), translate=(0.025, 0.025), scale=(0.975, 1.025), shear=(-0.025, 0.025)),
                           jitter=_jitter(0.1, 0.1, 0.1, 0.1)),
    "HIPT_augment_colour": dict(flip=0.5, jitter=_jitter(0.2, 0.2, 0.2, 0.2)),
    "HIPT_wang": dict(flip=0.5, affine=dict(degrees=(-90.0, 90.0), translate=None, scale=None, shear=None), jitter=_jitter(0.125, 0.2, 0.2, 0)),
    "HIPT_blur": dict(blur=(7.0, 9.0)),
}


class AugmentParams(C.Structure):
    """mirror of ``hipt_augment_params`` (include/hipt_abmil.h)"""
    _fields_ = [("affine", C.c_double * 6), ("factor", C.c_float * 3), ("blur_w", C.c_float * 3), ("flags", C.c_int32),
                ("hue_shift", C.c_int32), ("n_ops", C.c_int32), ("ops", C.c_int32 * 4), ("reserved", C.c_int32)]


def inverse_affine_matrix(center, angle, translate, scale, shear) -> List[float]:
    """torchvision ``_get_inverse_affine_matrix`` (output pixel -> input pixel; Pillow's AFFINE data), in Python doubles"""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


def blur_weights(sigma: float) -> Tuple[float, float, float]:
    """torchvision ``_get_gaussian_kernel1d(3, sigma)`` in float32 (top, centre, bottom tap)"""
    x = torch.linspace(-1.0, 1.0, steps=3, dtype=torch.float32)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    return tuple(float(v) for v in (pdf / pdf.sum()))


@dataclass
class RegionParams:
    """One region's drawn parameters (what torchvision's transforms would have drawn for it)."""
    hflip: bool = False
    vflip: bool = False
    affine: Optional[Tuple[float, ...]] = None   # Pillow AFFINE data (6 doubles) or None
    order: Tuple[int, ...] = ()                  # colour ops that are on, in application order (OP_*)
    brightness: float = 1.0
    contrast: float = 1.0
    saturation: float = 1.0
    hue: float = 0.0                             # torchvision hue_factor
    blur_sigma: Optional[float] = None
    draws: dict = field(default_factory=dict)    # the raw draws (angle, translate, scale, shear, ...), for inspection

    @property
    def hue_shift(self) -> int:
        # adjust_hue: uint8(hue_factor * 255) added to H modulo 256; a negative factor wraps (-0.1 -> -25 -> 231)
        return int(math.trunc(self.hue * 255.0)) % 256

    def record(self) -> AugmentParams:
        p = AugmentParams()
        p.flags = (HFLIP if self.hflip else 0) | (VFLIP if self.vflip else 0) | (AFFINE if self.affine is not None else 0) | \
                  (BLUR if self.blur_sigma is not None else 0)
        if self.affine is not None:
            for i, v in enumerate(self.affine):
                p.affine[i] = v
        p.factor[0], p.factor[1], p.factor[2] = self.brightness, self.contrast, self.saturation
        if self.blur_sigma is not None:
            p.blur_w[0], p.blur_w[1], p.blur_w[2] = blur_weights(self.blur_sigma)
        p.hue_shift = self.hue_shift
        p.n_ops = len(self.order)
        for i, op in enumerate(self.order):
            p.ops[i] = op
        return p


def _uniform(g: torch.Generator, lo: float, hi: float) -> float:
    return float(torch.empty(1).uniform_(float(lo), float(hi), generator=g).item())


def draw_spec(spec: dict, generator: torch.Generator, rows: int, cols: int, p):
    """The draws of one region for ``spec`` (a value of ``POLICIES``, or of ``tensor_augment.TENSOR_POLICIES``) in torchvision's
    order, written into ``p`` (a ``RegionParams`` or anything with its flip and colour fields): flips (``rand(1) < p``, H then
    V); RandomAffine.get_params (angle, tx, ty, scale, shear_x: a draw only for an argument that is given) into
    ``p.draws`` -- the matrix is the caller's, it differs between the PIL and the tensor path; ColorJitter.get_params
    (``randperm(4)``, then b, c, s, h: a factor that is off is not drawn); GaussianBlur.get_params (sigma)."""
    g = generator
    if "flip" in spec:
        p.hflip = bool(torch.rand(1, generator=g) < spec["flip"])
        p.vflip = bool(torch.rand(1, generator=g) < spec["flip"])
    if "affine" in spec:
        a = spec["affine"]
        angle = _uniform(g, *a["degrees"])
        tx = ty = 0
        if a["translate"] is not None:
            max_dx, max_dy = float(a["translate"][0] * cols), float(a["translate"][1] * rows)  # img_size = [cols, rows]
            tx = int(round(_uniform(g, -max_dx, max_dx)))
            ty = int(round(_uniform(g, -max_dy, max_dy)))
        scale = _uniform(g, *a["scale"]) if a["scale"] is not None else 1.0
        shear_x = _uniform(g, *a["shear"]) if a["shear"] is not None else 0.0
        p.draws.update(angle=angle, translate=(tx, ty), scale=scale, shear=(shear_x, 0.0))
    if "jitter" in spec:
        perm = torch.randperm(4, generator=g).tolist()
        f = [None if r is None else _uniform(g, *r) for r in spec["jitter"]]
        p.order = tuple(op for op in perm if f[op] is not None)
        p.brightness = f[0] if f[0] is not None else 1.0
        p.contrast = f[1] if f[1] is not None else 1.0
        p.saturation = f[2] if f[2] is not None else 1.0
        p.hue = f[3] if f[3] is not None else 0.0
        p.draws.update(perm=tuple(perm))
    if "blur" in spec:
        if rows < 2:
            raise ValueError("HIPT_blur: reflect padding needs at least 2 rows")
        p.blur_sigma = _uniform(g, *spec["blur"])
    return p


def draw_params(policy: str, generator: torch.Generator, rows: int, cols: int) -> RegionParams:
    """Draw one region's parameters in torchvision's order (``draw_spec``); the affine is Pillow's AFFINE data about the image
    centre ``[cols / 2, rows / 2]``."""
    if policy not in POLICIES:
        raise ValueError(f"unknown augmentation policy {policy!r}; known: {sorted(POLICIES)}")
    spec = POLICIES[policy]
    p = RegionParams()
    if spec is None:
        return p
    draw_spec(spec, generator, rows, cols, p)
    if "affine" in spec:
        d = p.draws
        p.affine = tuple(inverse_affine_matrix([cols * 0.5, rows * 0.5], d["angle"], d["translate"], d["scale"], d["shear"]))
        _check_fixed(p.affine, rows, cols)
    return p


def _check_fixed(m, rows: int, cols: int) -> None:
    # Pillow samples in 16.16 fixed point only where all four corners map inside +-32768 (Geometry.c check_fixed); outside
    # that it falls back to a floating-point path the kernel does not implement
    for x, y in ((0, 0), (cols, rows), (0, rows), (cols, 0)):
        if not (abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0):
            raise ValueError(f"affine on a {rows}x{cols} region leaves Pillow's fixed-point envelope")


def region_seed(seed: int, slide_id: str, k: int, index: int) -> int:
    """Stable 63-bit seed of one region's generator: the first 8 bytes (little-endian) of BLAKE2b over
    ``"{seed}\\x1f{slide_id}\\x1f{k}\\x1f{index}"`` (UTF-8), top bit cleared.  Not Python's ``hash`` (salted per process)."""
    h = hashlib.blake2b(f"{int(seed)}\x1f{slide_id}\x1f{int(k)}\x1f{int(index)}".encode("utf-8"), digest_size=8).digest()
    return int.from_bytes(h, "little") & 0x7FFF_FFFF_FFFF_FFFF


def draw_region_params(policy: str, seed: int, slide_id: str, k: int, first: int, count: int, rows: int, cols: int) -> List[RegionParams]:
    """parameters of regions first .. first+count-1 of a slide for augmentation k: one generator per region, so the draws do
    not depend on how the regions are batched"""
    out = []
    for i in range(first, first + count):
        g = torch.Generator()
        g.manual_seed(region_seed(seed, slide_id, k, i))
        out.append(draw_params(policy, g, rows, cols))
    return out


def pack_records(params: Sequence[RegionParams]) -> torch.Tensor:
    """the parameter records as a host uint8 tensor (pinned: the device copy is asynchronous)"""
    arr = (AugmentParams * len(params))(*[p.record() for p in params])
    host = torch.empty(C.sizeof(arr), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
    C.memmove(host.data_ptr(), C.addressof(arr), C.sizeof(arr))
    return host


def augment_regions(regions_u8: torch.Tensor, params: Sequence[RegionParams], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``regions_u8`` (uint8 on a HIP device, planar or interleaved) with region i transformed by ``params[i]``; same layout."""
    interleaved, rows, cols = F.rgb_layout("augment_regions", regions_u8, dims=(4,))
    N.require_cuda(regions_u8, "augment_regions")
    n = regions_u8.shape[0]
    if len(params) != n:
        raise ValueError(f"{n} regions but {len(params)} parameter records")
    if any(p.blur_sigma is not None for p in params) and rows < 2:
        raise ValueError("blur: reflect padding needs at least 2 rows")
    src = regions_u8.contiguous()
    dev = src.device
    dst = F.check_out("augment_regions", out, src.shape, torch.uint8, dev, not_alias=(src,))   # (the kernel reads neighbours: never in place)
    if n == 0:
        return dst
    rec = pack_records(params).to(dev, non_blocking=True)
    ws, _ = F.scratch("hipt_augment_workspace_bytes", n, rows, cols, dev=dev)
    N.call("hipt_augment_regions", N.ptr(src), int(interleaved), n, rows, cols, N.ptr(rec), N.ptr(dst), N.ptr(ws), ws.numel(),
           N.stream_ptr(dev))
    cur = torch.cuda.current_stream(dev)
    for t in (src, rec, ws):  # (allocator: these stay alive until the kernel has read them)
        t.record_stream(cur)
    return dst


class RegionAugment:
    """``RegionAugment(policy, seed)(regions, slide_id, k, first)``: device uint8 batch -> augmented batch (same layout),
    regions numbered ``first, first+1, ...`` within the slide (their parameters depend on that number, not on the batch)."""

    def __init__(self, policy: str, seed: int = 0):
        if policy not in POLICIES:
            raise ValueError(f"unknown augmentation policy {policy!r}; known: {sorted(POLICIES)}")
        self.policy, self.seed = policy, int(seed)

    def params(self, slide_id: str, k: int, first: int, count: int, rows: int, cols: int) -> List[RegionParams]:
        return draw_region_params(self.policy, self.seed, slide_id, k, first, count, rows, cols)

    def __call__(self, regions: torch.Tensor, slide_id: str = "", k: int = 1, first: int = 0) -> torch.Tensor:
        _, rows, cols = F.rgb_layout("RegionAugment", regions, dims=(4,))
        return augment_regions(regions, self.params(slide_id, k, first, regions.shape[0], rows, cols))
