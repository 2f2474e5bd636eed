"""What every host-mirror module (the ViTs, ``ResNet_Baseline``, ``Attn_Net_Gated``, ``CLAM_SB`` / ``CLAM_MB``) shares:
the compute-dtype setting and the cache of device-side weight images.

A weight image is whatever a module's ``build`` makes for one device: ctypes structs plus the tensors they point into.  It is
the one place where this package hands addresses to the GPU, so its protocol exists once: the image is keyed by the dtype
code and ``(data_ptr, _version)`` of every weight tensor, goes stale only when that key changes, is built only after every
tensor was found on the device the kernels will run on, and is never pickled or deep-copied.
"""
from __future__ import annotations

import os
import warnings

import torch

from . import _native as N


def default_dtype() -> str:
    return os.environ.get("HIPT_AMD_DTYPE", "fp32")


class ComputeDtype:
    """``set_compute_dtype`` / ``compute_dtype``: ``'fp32'`` or ``'bf16'`` (``_compute_dtype``, set by the constructor)."""

    def set_compute_dtype(self, name: str):
        N.dtype_code(name)
        self._compute_dtype = "bf16" if name in ("bf16", "bfloat16") else "fp32"
        return self

    @property
    def compute_dtype(self) -> str:
        return self._compute_dtype


class WeightImageCache(ComputeDtype):
    """Mixin of an ``nn.Module`` (listed before it) whose forward runs on a device-side image of its weights."""

    _caches = ("_packed",)    # attributes holding device -> (key, value) caches: emptied by pickle / deepcopy
    _image_buffers = False    # do floating-point buffers enter the image (ResNet: the BatchNorm running statistics)?

    def _init_host(self):
        self._compute_dtype = default_dtype()
        for name in self._caches:  # _packed: device -> (key, image); nn.DataParallel replicas share these dicts (shallow __dict__ copy)
            setattr(self, name, {})
        self._warned_grad = False

    def __getstate__(self):
        d = self.__dict__.copy()
        for name in self._caches:
            d[name] = {}
        return d

    def _tensors(self):
        """The tensors that enter the image.  A ``nn.DataParallel`` replica has no ``parameters()`` (they are plain attributes
        there, torch/nn/parallel/replicate.py; the reference wraps its extractors so whenever it sees more than one GPU,
        extract_features_fp.py:217-218): take them from ``_former_parameters``."""
        ts = list(self.parameters())
        if not ts:
            ts = [t for m in self.modules() for t in getattr(m, "_former_parameters", {}).values() if t is not None]
        if self._image_buffers:
            ts += [b for b in self.buffers() if b.is_floating_point()]
        return ts

    def _version_key(self):
        return tuple((t.data_ptr(), t._version) for t in self._tensors())

    def _cached(self, device, key_extra, build):
        """The image for ``device``; ``build(dtype code)`` makes a new one when the dtype, ``key_extra`` or a weight changed.
        A hit needs no device check: an equal key names the very tensors that were checked when the image was built."""
        code = N.dtype_code(self._compute_dtype)
        key = (code, *key_extra, self._version_key())
        hit = self._packed.get(device)
        if hit is None or hit[0] != key:
            N.same_device(type(self).__name__, device, *self._tensors())  # e.g. relocate() never called: a clean error, not a GPU fault
            hit = (key, build(code))
            self._packed[device] = hit
        return hit[1]

    def _warn_no_grad_fn(self, message: str):
        """Said once per module: the inference forwards return tensors without ``grad_fn``."""
        if torch.is_grad_enabled() and not self._warned_grad and any(p.requires_grad for p in self.parameters()):
            warnings.warn(message, stacklevel=4)
            self._warned_grad = True
