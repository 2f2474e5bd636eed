"""What the Python front-end of a device op does before its native call, in one place: tell a tensor from an array, settle the
device, stage an input there, check ``out=``, allocate the scratch buffer, and the small checks several ops share.  Every refusal
here comes before any native call and before the device is touched.  ``what`` is the prefix of a message (the public function's
name, or the module's); where modules differ in the exception class of a refusal the caller hands the class in (``exc=``).
torch is imported inside the functions: importing a front-end does not import it."""
from __future__ import annotations

import numpy as np

from . import _native as N

NO_CPU = "hipt_abmil_atec23_amd runs only on a HIP device (there is deliberately no CPU path)"
_tables = {}   # (builder's name, colormap name) -> the host array; (builder's name, colormap name, device) -> its copy there


def is_tensor(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch" and hasattr(x, "data_ptr")


def as_array(a):
    return a if a is None or is_tensor(a) else np.asarray(a)


def _kind(dtype) -> str:
    return str(dtype).replace("torch.", "")


def check_int(what: str, name: str, v, lo=None, hi=None) -> int:
    """``int(v)`` of an integer (no bool, no float) in ``lo .. hi``; an end that is None is open."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or (lo is not None and v < lo) or (hi is not None and v > hi):
        span = "" if lo is None and hi is None else f" >= {lo}" if hi is None else f" <= {hi}" if lo is None else f" in {lo} .. {hi}"
        raise ValueError(f"{what}: {name} must be an integer{span} (integers only, and not a bool), got {v!r}")
    return int(v)


def check_image(what: str, name: str, a, shape, kinds) -> None:
    """``a`` (array or tensor; None passes) has ``shape`` and one of the dtypes named in ``kinds``."""
    if a is not None and (tuple(a.shape) != tuple(shape) or _kind(a.dtype) not in kinds):
        raise ValueError(f"{what}: {name} must be {kinds[0]} {list(shape)}, got {a.dtype} {list(a.shape)}")


def check_no_nan(what: str, **named) -> None:
    """``ValueError`` on a NaN; numpy arrays are looked at on the host, device tensors with one synchronisation, which is left
    out while the stream is being captured into a graph (the kernels then count a NaN as neither below nor above anything)."""
    import torch
    for name, a in named.items():
        if a is None:
            continue
        if is_tensor(a):
            if a.is_cuda and torch.cuda.is_current_stream_capturing():
                continue
            bad = bool(torch.isnan(a).any()) if a.numel() else False
        else:
            bad = bool(np.isnan(np.asarray(a, dtype=np.float64)).any())
        if bad:
            raise ValueError(f"{what}: {name} contain NaN")


def rgb_layout(what: str, x, dims=(3, 4)):
    """``(interleaved, h, w)`` of a uint8 RGB tensor, planar ``[.., 3, h, w]`` or interleaved ``[.., h, w, 3]``, with ``x.dim()`` in
    ``dims``.  ``[R, 3, h, 3]`` counts as planar (HIPT_4K's test)."""
    forms = "[3, h, w] / [h, w, 3] or a batch of either" if 3 in dims else "a batch, [R, 3, h, w] or [R, h, w, 3]"
    if not is_tensor(x):
        raise ValueError(f"{what}: x is a uint8 tensor, got {type(x).__name__}")
    if _kind(x.dtype) != "uint8":
        raise ValueError(f"{what} takes raw uint8 RGB images (got {x.dtype}): the reference works on the bytes, before eval_transforms, "
                         f"so normalised float input cannot be treated faithfully")
    s = (1,) * (4 - x.dim()) + tuple(int(v) for v in x.shape)
    if x.dim() in dims and s[3] == 3 and s[1] != 3:
        return True, s[1], s[2]
    if x.dim() in dims and s[1] == 3:
        return False, s[2], s[3]
    raise ValueError(f"{what}: x is uint8 RGB, {forms}, got {list(x.shape)}")


def resolve_device(what: str, device, tensors=(), *, exc=RuntimeError, staged=False):
    """The concrete ``cuda:N`` an op runs on: ``device`` where given, else that of the first device tensor of ``tensors``, else the
    current one; ``exc`` for anything but a HIP device (before ``torch.cuda`` is asked), for a missing HIP runtime, and for a tensor
    that lives elsewhere.  ``staged``: the caller copies every tensor to the result, so none is refused."""
    import torch
    refs = [t for t in tensors if is_tensor(t)]
    on_dev = [t for t in refs if t.is_cuda]
    dev = torch.device(device) if device is not None else (on_dev[0].device if on_dev else torch.device("cuda"))
    if dev.type != "cuda":
        raise exc(f"{what}: device {dev}; {NO_CPU}")
    if not on_dev and not torch.cuda.is_available():   # (a device tensor is proof of the runtime: the hot path does not ask)
        raise exc(f"{what}: no HIP device; {NO_CPU}")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    for t in () if staged else refs:
        if t.device != dev:
            raise exc(f"{what}: expected all tensors on {dev}, found one on {t.device} (move the inputs to the same HIP device; there "
                      f"is deliberately no CPU path)")
    return dev


def to_device(a, dev):
    """An array or tensor as a detached contiguous tensor on ``dev`` (bool: the same bytes as uint8); None stays None."""
    import torch
    if a is None:
        return None
    t = (a if is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))).detach().to(dev).contiguous()
    return t.view(torch.uint8) if t.dtype == torch.bool else t


def as_device_u8(what: str, x, device, *, dims: int, channels=None, exc=ValueError):
    """A picture ``x`` -- numpy array or tensor, uint8, ``dims`` axes beginning ``[H, W]``, the last one of ``channels`` where given --
    as a detached contiguous tensor on the device ``resolve_device`` settles for it."""
    if not isinstance(x, np.ndarray) and not is_tensor(x):
        raise ValueError(f"{what}: the input is a numpy array or a device tensor, got {type(x).__name__}")
    shape = [int(v) for v in x.shape]
    if _kind(x.dtype) != "uint8" or len(shape) != dims:
        raise ValueError(f"{what}: the input is uint8 with {dims} axes, got {x.dtype} {shape}")
    if channels is not None and shape[-1] not in channels:
        raise ValueError(f"{what}: the image is uint8 [H, W, C] with C one of {list(channels)}, got {shape}")
    if shape[0] < 1 or shape[1] < 1 or shape[0] * shape[1] >= 1 << 31:
        raise ValueError(f"{what}: {shape[0]} x {shape[1]} pixels (at least one, H * W below 2^31)")
    return to_device(x, resolve_device(what, device, (x,), exc=exc))


def check_out(what: str, out, shape, dtype, dev, *, not_alias=(), name="out"):
    """``out`` where given -- a contiguous ``dtype`` tensor of ``shape`` on ``dev`` that begins where none of ``not_alias`` does --
    else a new one."""
    import torch
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=dev)
    if (not is_tensor(out) or out.dtype != dtype or tuple(out.shape) != tuple(shape) or out.device != dev or not out.is_contiguous()
            or any(out.data_ptr() == t.data_ptr() for t in not_alias)):
        raise ValueError(f"{what}: {name} must be a contiguous {_kind(dtype)} {list(shape)} tensor on {dev}" + (", and not the input" if not_alias else ""))
    return out


def scratch(symbol: str, *dims, dev, floor=256):
    """``(buffer, need)``: ``need`` is what the library's ``symbol`` asks for ``dims``; the buffer is a fresh uint8 tensor of
    ``max(need, floor)`` bytes (new per call: safe on any stream under the caching allocator), or None where that is 0."""
    import torch
    need = int(getattr(N.lib(), symbol)(*dims))
    size = max(need, floor)
    return (torch.empty((size,), dtype=torch.uint8, device=dev) if size else None), need


def table_host(builder, cmap):
    """``builder(cmap)``, a host array; the table of a named colormap is built once per builder."""
    if not isinstance(cmap, str):
        return builder(cmap)
    key = (builder.__name__, cmap)
    if key not in _tables:
        _tables[key] = builder(cmap)
    return _tables[key]


def table_on(builder, cmap, host, dev):
    """``host`` (``table_host``'s, or the caller's own array or tensor) on ``dev``; a named colormap's table is copied there once, so
    that a later call can be captured into a graph."""
    if not isinstance(cmap, str):
        return to_device(host, dev)
    key = (builder.__name__, cmap, str(dev))
    if key not in _tables:
        _tables[key] = to_device(host, dev)
    return _tables[key]
