"""ResNet-50 baseline extractor: the reference's ``models/resnet_custom.py`` call surface on top of the gfx950 library.

``ResNet_Baseline`` / ``Bottleneck_Baseline`` / ``resnet50_baseline`` / ``load_pretrained_weights`` keep the reference's
constructor arguments, module names and state-dict keys (``conv1``, ``bn1``, ``layer{1,2,3}.{i}.{conv,bn}{1,2,3}``,
``layer{1,2,3}.0.downsample.{0,1}``, ``num_batches_tracked`` included), so a torchvision ``resnet50`` checkpoint loads with
``strict=False`` exactly as there (``layer4.*`` / ``fc.*`` unexpected, nothing missing).  The modules only HOLD
parameters: ``forward`` runs the whole truncated network -- stem, maxpool, layer1..layer3, average pool -- as HIP kernels
through ``libhipt_abmil.so`` (``hipt_resnet_forward``), eval-mode BatchNorm folded into the conv weights.  There is no
CPU path and no train-mode path (BatchNorm would need batch statistics).

Input: ``[B, 3, H, W]`` float, already normalised (the reference's ``eval_transforms``), or raw uint8 RGB, planar
``[B, 3, H, W]`` or interleaved ``[B, H, W, 3]``, normalised on the device with :meth:`ResNet_Baseline.set_input_normalization`
(ImageNet by default; ``(0.5, 0.5)`` for ``--use_transforms HIPT`` runs).  H and W: multiples of 16, at least 32.

``compute_dtype``: ``'fp32'`` (exact-fp32 MFMA) or ``'bf16'`` (bf16 operands and stored activations, fp32 accumulate);
``set_compute_dtype`` or the ``HIPT_AMD_DTYPE`` environment variable.
"""
from __future__ import annotations

import ctypes as C
import os
from urllib.parse import urlparse

import torch
import torch.nn as nn

from . import _native as N
from . import functional as Fn
from ._host import WeightImageCache

__all__ = ['ResNet_Baseline', 'Bottleneck_Baseline', 'resnet18_baseline', 'resnet50_baseline', 'load_pretrained_weights']

model_urls = {
    'resnet18': 'https://download.pytorch.org/models/resnet18-5c106cde.pth',
    'resnet34': 'https://download.pytorch.org/models/resnet34-333f7ec4.pth',
    'resnet50': 'https://download.pytorch.org/models/resnet50-19c8e357.pth',
    'resnet50_histo': 'https://dox.uliege.be/index.php/s/kvABLtVuMxW8iJy/download',
    'resnet101': 'https://download.pytorch.org/models/resnet101-5d3b4d8f.pth',
    'resnet152': 'https://download.pytorch.org/models/resnet152-b121ed2d.pth',
}

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _conv_bn_struct(conv: nn.Conv2d, bn: nn.BatchNorm2d, keep: list) -> N.ConvBN:
    def f(t):
        t = t.detach().float().contiguous()
        keep.append(t)
        return t.data_ptr()

    c = N.ConvBN()
    c.weight, c.bn_weight, c.bn_bias = f(conv.weight), f(bn.weight), f(bn.bias)
    c.bn_mean, c.bn_var = f(bn.running_mean), f(bn.running_var)
    c.cout, c.cin, c.kh, c.kw = conv.weight.shape
    c.bn_eps = float(bn.eps)
    return c


# ---- fine-grained units (NHWC tensors on a HIP device) -----------------------------------------------------------------
def pack_conv_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d, dtype: int = N.HIPT_F32):
    """(weight [cout, kp] in the compute dtype, bias [cout] fp32): ``bn(conv(.))`` in eval mode folded into one conv."""
    dev = conv.weight.device
    N.require_cuda(conv.weight, "pack_conv_bn")
    keep = []
    c = _conv_bn_struct(conv, bn, keep)
    nbytes = N.lib().hipt_conv_bn_packed_bytes(C.byref(c), dtype)
    if not nbytes:
        raise ValueError(f"pack_conv_bn: unsupported conv {tuple(conv.weight.shape)}")
    w = torch.empty(nbytes // (2 if dtype == N.HIPT_BF16 else 4), dtype=Fn.torch_dtype(dtype), device=dev).view(c.cout, -1)
    b = torch.empty(c.cout, dtype=torch.float32, device=dev)
    N.call("hipt_conv_bn_pack", C.byref(c), dtype, N.ptr(w), N.ptr(b), N.stream_ptr(dev))
    return w, b


def _conv2d(who: str, entry: str, x, w_packed, bias, kernel_size, stride, padding, resid, relu, dtype, *tile_rows):
    """The one body of :func:`conv2d_nhwc` (``hipt_conv2d``) and :func:`.resnet18.conv2d_nhwc_ex` (``hipt_conv2d_ex``, which
    takes the tile height before the stream)."""
    N.require_cuda(x, who)
    x = x.detach().to(Fn.torch_dtype(dtype)).contiguous()
    n, h, w, cin = x.shape
    cout = w_packed.shape[0]
    oh, ow = (h + 2 * padding - kernel_size) // stride + 1, (w + 2 * padding - kernel_size) // stride + 1
    out = torch.empty((n, oh, ow, cout), dtype=x.dtype, device=x.device)
    r = None if resid is None else resid.detach().to(x.dtype).contiguous()
    if r is not None and tuple(r.shape) != tuple(out.shape):
        raise ValueError(f"{who}: residual {tuple(r.shape)} does not match the output {tuple(out.shape)}")
    N.call(entry, N.ptr(x), n, h, w, cin, N.ptr(w_packed), N.ptr(bias), cout, kernel_size, kernel_size, stride, padding,
           N.ptr(r), int(relu), N.ptr(out), dtype, *tile_rows, N.stream_ptr(x.device))
    return out


def conv2d_nhwc(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, kernel_size: int, stride: int = 1, padding: int = 0,
                resid: torch.Tensor = None, relu: bool = False, dtype: int = N.HIPT_F32) -> torch.Tensor:
    """``relu?(conv2d(x) + bias (+ resid))`` on NHWC ``x [n, h, w, cin]`` with a packed weight (:func:`pack_conv_bn`); returns
    ``[n, oh, ow, cout]`` in the compute dtype."""
    return _conv2d("conv2d_nhwc", "hipt_conv2d", x, w_packed, bias, kernel_size, stride, padding, resid, relu, dtype)


def maxpool_nhwc(x: torch.Tensor, dtype: int = N.HIPT_F32) -> torch.Tensor:
    """``MaxPool2d(3, 2, 1)`` on NHWC ``x``."""
    N.require_cuda(x, "maxpool_nhwc")
    x = x.detach().to(Fn.torch_dtype(dtype)).contiguous()
    n, h, w, c = x.shape
    out = torch.empty((n, (h + 1) // 2, (w + 1) // 2, c), dtype=x.dtype, device=x.device)
    N.call("hipt_resnet_maxpool", N.ptr(x), n, h, w, c, N.ptr(out), dtype, N.stream_ptr(x.device))
    return out


def avgpool_nhwc(x: torch.Tensor, dtype: int = N.HIPT_F32) -> torch.Tensor:
    """``AdaptiveAvgPool2d(1)`` on NHWC ``x [n, h, w, c]`` -> ``[n, c]`` fp32."""
    N.require_cuda(x, "avgpool_nhwc")
    x = x.detach().to(Fn.torch_dtype(dtype)).contiguous()
    n, h, w, c = x.shape
    out = torch.empty((n, c), dtype=torch.float32, device=x.device)
    N.call("hipt_resnet_avgpool", N.ptr(x), n, h * w, c, N.ptr(out), dtype, N.stream_ptr(x.device))
    return out


class Bottleneck_Baseline(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super(Bottleneck_Baseline, self).__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        """One block on NCHW ``x`` (eval mode), unit by unit through ``hipt_conv2d`` in fp32; the network forward does not
        come through here (it is one library call)."""
        if self.training:
            raise RuntimeError("Bottleneck_Baseline: BatchNorm in train() mode needs batch statistics (not implemented); call .eval()")
        N.require_cuda(x, "Bottleneck_Baseline")
        xh = x.detach().float().permute(0, 2, 3, 1).contiguous()
        w1, b1 = pack_conv_bn(self.conv1, self.bn1)
        w2, b2 = pack_conv_bn(self.conv2, self.bn2)
        w3, b3 = pack_conv_bn(self.conv3, self.bn3)
        t = conv2d_nhwc(xh, w1, b1, 1, relu=True)
        t = conv2d_nhwc(t, w2, b2, 3, self.stride, 1, relu=True)
        r = xh
        if self.downsample is not None:
            wd, bd = pack_conv_bn(self.downsample[0], self.downsample[1])
            r = conv2d_nhwc(xh, wd, bd, 1, self.downsample[0].stride[0])
        return conv2d_nhwc(t, w3, b3, 1, resid=r, relu=True).permute(0, 3, 1, 2)


class _PackedNet:
    """Device-side image of one extractor for one compute dtype: BN-folded weights (``<entry>_pack_weights``) plus the ctypes
    structs that describe them.  Rebuilt when a parameter or running statistic changes."""

    def __init__(self, model, code: int, dev, fields: dict):
        keep = []
        layers = [getattr(model, name) for name in model._LAYERS]
        convs = [(model.conv1, model.bn1)]
        for layer in layers:
            for blk in layer:   # state-dict order: conv1.. of the block, then its downsample
                convs += [(getattr(blk, f"conv{i}"), getattr(blk, f"bn{i}")) for i in (1, 2, 3) if hasattr(blk, f"conv{i}")]
                if blk.downsample is not None:
                    convs.append((blk.downsample[0], blk.downsample[1]))
        self.convs = (N.ConvBN * len(convs))(*[_conv_bn_struct(c, b, keep) for c, b in convs])
        w = model._WEIGHTS(dtype=code, n_convs=len(convs), **fields)
        for i, layer in enumerate(layers):
            w.layers[i] = len(layer)
        w.convs = C.cast(self.convs, C.POINTER(N.ConvBN))
        self.w = w
        nbytes = getattr(N.lib(), model._ENTRY + "_packed_bytes")(C.byref(w))
        if not nbytes:
            raise ValueError(f"{type(model).__name__}: this layer configuration is outside the library's network "
                             f"({N.lib().hipt_last_error().decode(errors='replace')})")
        self.image = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        N.call(model._ENTRY + "_pack_weights", C.byref(w), N.ptr(self.image), N.stream_ptr(dev))
        self.keep = keep  # the fp32 sources stay alive until the packing kernels (enqueued above) have read them

    @property
    def ref(self):
        return C.byref(self.w)


class _ResNetHost(WeightImageCache, nn.Module):
    """What the extractors share: the modules that hold the parameters, the settings, the weight image and the one library call
    that runs stem, maxpool, the layers and the average pool.  A subclass states what differs."""
    _image_buffers = True  # the BN running statistics are folded into the image with the parameters
    _LAYERS = ()           # attribute names of the layers the network runs
    _WEIGHTS = None        # ctypes struct the library takes
    _ENTRY = ""            # entry-point family: <_ENTRY>_packed_bytes / _pack_weights / _workspace_bytes / _forward
    _SLOT = ""             # workspace slot name
    FEATURES = 0           # width of the pooled features

    def _build(self, block, layers):
        """stem, maxpool, one layer per name in ``_LAYERS`` (64, 128, ... planes, stride 2 from the second on), average pool"""
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for i, name in enumerate(self._LAYERS):
            setattr(self, name, self._make_layer(block, 64 << i, layers[i], stride=2 if i else 1))
        self.avgpool = nn.AdaptiveAvgPool2d(1)

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._init_host()
        self._norm = IMAGENET_MEAN + IMAGENET_STD

    def _make_layer(self, block, planes, blocks, stride=1):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(
                nn.Conv2d(self.inplanes, planes * block.expansion, kernel_size=1, stride=stride, bias=False),
                nn.BatchNorm2d(planes * block.expansion),
            )
        layers = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes))
        return nn.Sequential(*layers)

    # ---- settings ---------------------------------------------------------------------------------------------------
    def set_input_normalization(self, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """Per-channel ``Normalize(mean, std)`` applied on the device to uint8 input (after ``/ 255``); fp32 input is taken as
        already normalised.  A scalar applies to all three channels (``--use_transforms HIPT``: ``0.5, 0.5``)."""
        mean = tuple(float(v) for v in (mean if hasattr(mean, "__len__") else (mean,) * 3))
        std = tuple(float(v) for v in (std if hasattr(std, "__len__") else (std,) * 3))
        if len(mean) != 3 or len(std) != 3 or any(s == 0 for s in std):
            raise ValueError(f"set_input_normalization: need 3 means and 3 non-zero stds, got {mean}, {std}")
        self._norm = mean + std
        return self

    # ---- weights ------------------------------------------------------------------------------------------------------
    @property
    def weight_device(self):
        """Device the weights live on; survives DataParallel replication (``next(self.parameters())`` does not)."""
        return self.conv1.weight.device

    def _check_inference_only(self):
        name = type(self).__name__
        if self.training:
            raise RuntimeError(f"{name} HIP forward: BatchNorm in train() mode needs batch statistics (inference kernels "
                               "only); call .eval()")
        self._warn_no_grad_fn(f"HIP {name} forward returns tensors without grad_fn: no gradient flows into the extractor "
                              "weights (the reference uses it as a frozen feature extractor)")

    def _struct_fields(self) -> dict:
        """Fields of ``_WEIGHTS`` beyond dtype, layers and convs; they are part of the image's cache key."""
        return {}

    def _packed_for(self, dev) -> _PackedNet:
        self._check_inference_only()
        fields = self._struct_fields()
        return self._cached(dev, tuple(fields.values()), lambda code: _PackedNet(self, code, dev, fields))

    # ---- forward ------------------------------------------------------------------------------------------------------
    @staticmethod
    def _input_kind(x: torch.Tensor) -> int:
        if x.dtype == torch.uint8:
            return N.RESNET_IN_U8_HWC if (x.dim() == 4 and x.shape[-1] == 3 and x.shape[1] != 3) else N.RESNET_IN_U8
        return N.RESNET_IN_F32

    def _pooled(self, x):
        """``[B, FEATURES]`` fp32 of ``[B, 3, H, W]`` float (normalised) or uint8 (``[B, 3, H, W]`` / ``[B, H, W, 3]``): the
        network up to and including the average pool, one library call."""
        name = type(self).__name__
        N.require_cuda(x, name)
        kind = self._input_kind(x)
        if x.dim() != 4 or (x.shape[-1] if kind == N.RESNET_IN_U8_HWC else x.shape[1]) != 3:
            raise ValueError(f"{name}: expected [B,3,H,W] (or uint8 [B,H,W,3]) images, got {tuple(x.shape)}")
        dev = x.device
        N.same_device(name, self.weight_device, x)
        pk = self._packed_for(dev)
        x = x.detach().contiguous() if kind != N.RESNET_IN_F32 else x.detach().float().contiguous()
        B = x.shape[0]
        H, W = (x.shape[1], x.shape[2]) if kind == N.RESNET_IN_U8_HWC else (x.shape[2], x.shape[3])
        out = torch.empty((B, self.FEATURES), dtype=torch.float32, device=dev)
        need = getattr(N.lib(), self._ENTRY + "_workspace_bytes")(pk.ref, B, H, W)
        # one scratch per stream: two streams driving the model at once never share activations
        ws = Fn.workspace(dev, need, slot=(self._SLOT, torch.cuda.current_stream(dev).cuda_stream))
        norm = (C.c_float * 6)(*self._norm)
        N.call(self._ENTRY + "_forward", pk.ref, N.ptr(pk.image), N.ptr(x), kind, C.cast(norm, C.c_void_p), B, H, W, N.ptr(out),
               N.ptr(ws), ws.numel(), N.stream_ptr(dev))
        return out


class ResNet_Baseline(_ResNetHost):
    _LAYERS = ("layer1", "layer2", "layer3")   # layers[3] of the reference's call is not built there either
    _WEIGHTS, _ENTRY, _SLOT, FEATURES = N.ResnetWeights, "hipt_resnet", "resnet", 1024

    def __init__(self, block, layers):
        super(ResNet_Baseline, self).__init__()
        self._build(block, layers)
        self._init_weights()

    def forward(self, x):
        """``[B, 1024]`` fp32 features of ``[B, 3, H, W]`` float (normalised) or uint8 (``[B, 3, H, W]`` / ``[B, H, W, 3]``)."""
        return self._pooled(x)


def resnet18_baseline(pretrained=False, dataset='ImageNet'):
    """The reference builds torchvision's ResNet-18 here (models/resnet_custom.py:resnet18_baseline); that network is not
    part of this library."""
    raise NotImplementedError("resnet18_baseline: torchvision's ResNet-18 is not implemented by hipt_abmil_atec23_amd; "
                              "use resnet50_baseline (or --model_type resnet50 / HIPT_4K)")


def resnet50_baseline(pretrained=False, dataset='ImageNet'):
    """Constructs a Modified ResNet-50 model.
    Args:
        pretrained (bool): If True, loads the ImageNet (or 'Histo') checkpoint from the local torch hub cache
    """
    model = ResNet_Baseline(Bottleneck_Baseline, [3, 4, 6, 3])
    if pretrained:
        if dataset == 'ImageNet':
            model = load_pretrained_weights(model, 'resnet50')
        elif dataset == 'Histo':
            model = load_pretrained_weights(model, 'resnet50_histo')
    return model


def cached_checkpoint_path(name: str) -> str:
    """Where ``torch.utils.model_zoo.load_url(model_urls[name])`` keeps its download: ``<torch.hub.get_dir()>/checkpoints/<file>``."""
    return os.path.join(torch.hub.get_dir(), "checkpoints", os.path.basename(urlparse(model_urls[name]).path))


def load_pretrained_weights(model, name):
    """The reference downloads through ``model_zoo.load_url``; this reads the file that call would have cached and never
    touches the network.  Missing file: ``FileNotFoundError`` naming the path to put it at."""
    path = cached_checkpoint_path(name)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"pretrained '{name}' weights not found at {path}; this package never downloads: place the "
                                f"checkpoint of {model_urls[name]} there (or load a state dict with model.load_state_dict(sd, strict=False))")
    pretrained_dict = torch.load(path, map_location="cpu")
    model.load_state_dict(pretrained_dict, strict=False)
    return model
