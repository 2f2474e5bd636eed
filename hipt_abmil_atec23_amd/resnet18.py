"""HistoResNet-18 extractor: what the reference's ``models/resnet_custom.py:resnet18_baseline`` builds (torchvision's
``resnet18``), on top of the gfx950 library.

``ResNet18_Baseline`` carries torchvision's 122 state-dict keys (``conv1``, ``bn1``, ``layer{1..4}.{0,1}.{conv,bn}{1,2}``,
``layer{2,3,4}.0.downsample.{0,1}``, ``fc``, ``num_batches_tracked`` included), so a torchvision or Lightning checkpoint
loads as it does there.  The modules only HOLD parameters: ``forward`` runs stem, maxpool, layer1..layer4 and the average
pool as HIP kernels in one ``hipt_resnet_basic_forward`` call (eval-mode BatchNorm folded into the conv weights), then
applies ``fc`` as the module holds it: the empty ``nn.Sequential`` the reference's Histo route leaves there returns the
``[B, 512]`` features, an ``nn.Linear`` goes through ``hipt_linear``.  No CPU path, no train-mode path.

Input, normalisation and compute dtype are those of :mod:`.resnet_custom` (``[B, 3, H, W]`` float already normalised, or raw
uint8 planar / interleaved; ``set_input_normalization``; ``set_compute_dtype`` / ``HIPT_AMD_DTYPE``).  H and W: multiples of 32.

``resnet_custom.resnet18_baseline`` still raises ``NotImplementedError``; reference scripts reach this module through
``dropin.install(resnet18=True)``.
"""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.nn as nn

from . import _native as N
from . import functional as Fn
from ._host import WeightImageCache
from .resnet_custom import IMAGENET_MEAN, IMAGENET_STD, ResNet_Baseline, _conv_bn_struct, conv2d_nhwc, load_pretrained_weights, pack_conv_bn

__all__ = ['ResNet18_Baseline', 'BasicBlock_Baseline', 'resnet18_baseline', 'HISTO_CKPT_PATH', 'conv2d_nhwc_ex', 'conv_tile_rows']

# where the reference looks for the Histo checkpoint (models/resnet_custom.py:121), relative to the working directory
HISTO_CKPT_PATH = "../../mount_outputs/tenpercent_resnet18.ckpt"


def conv_tile_rows(m: int, cout: int) -> int:
    """Output-pixel tile height (64 or 128) the network's driver launches a conv of ``m`` output pixels and ``cout``
    channels with (``hipt_conv_tile_rows``)."""
    rows = N.lib().hipt_conv_tile_rows(int(m), int(cout))
    if not rows:
        raise ValueError(f"conv_tile_rows: bad conv shape m={m} cout={cout}")
    return rows


def conv2d_nhwc_ex(x: torch.Tensor, w_packed: torch.Tensor, bias: torch.Tensor, kernel_size: int, stride: int = 1, padding: int = 0,
                   resid: torch.Tensor = None, relu: bool = False, dtype: int = N.HIPT_F32, tile_rows: int = 0) -> torch.Tensor:
    """:func:`.resnet_custom.conv2d_nhwc` with the tile height chosen: 128, 64, or 0 for :func:`conv_tile_rows`.  Both heights
    give the same bits."""
    N.require_cuda(x, "conv2d_nhwc_ex")
    x = x.detach().to(Fn.torch_dtype(dtype)).contiguous()
    n, h, w, cin = x.shape
    cout = w_packed.shape[0]
    oh, ow = (h + 2 * padding - kernel_size) // stride + 1, (w + 2 * padding - kernel_size) // stride + 1
    out = torch.empty((n, oh, ow, cout), dtype=x.dtype, device=x.device)
    r = None if resid is None else resid.detach().to(x.dtype).contiguous()
    if r is not None and tuple(r.shape) != tuple(out.shape):
        raise ValueError(f"conv2d_nhwc_ex: residual {tuple(r.shape)} does not match the output {tuple(out.shape)}")
    N.call("hipt_conv2d_ex", N.ptr(x), n, h, w, cin, N.ptr(w_packed), N.ptr(bias), cout, kernel_size, kernel_size, stride, padding,
           N.ptr(r), int(relu), N.ptr(out), dtype, int(tile_rows), N.stream_ptr(x.device))
    return out


class BasicBlock_Baseline(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super(BasicBlock_Baseline, self).__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        """One block on NCHW ``x`` (eval mode), unit by unit through ``hipt_conv2d`` in fp32; the network forward does not
        come through here (it is one library call)."""
        if self.training:
            raise RuntimeError("BasicBlock_Baseline: BatchNorm in train() mode needs batch statistics (not implemented); call .eval()")
        N.require_cuda(x, "BasicBlock_Baseline")
        xh = x.detach().float().permute(0, 2, 3, 1).contiguous()
        w1, b1 = pack_conv_bn(self.conv1, self.bn1)
        w2, b2 = pack_conv_bn(self.conv2, self.bn2)
        t = conv2d_nhwc(xh, w1, b1, 3, self.stride, 1, relu=True)
        r = xh
        if self.downsample is not None:
            wd, bd = pack_conv_bn(self.downsample[0], self.downsample[1])
            r = conv2d_nhwc(xh, wd, bd, 1, self.downsample[0].stride[0])
        return conv2d_nhwc(t, w2, b2, 3, 1, 1, resid=r, relu=True).permute(0, 3, 1, 2)


class _PackedResnet18:
    """Device-side image of one ResNet18_Baseline for one compute dtype (``hipt_resnet_basic_pack_weights``) plus the ctypes
    structs that describe it.  Rebuilt when a parameter or running statistic changes."""

    def __init__(self, model, code: int, dev, tile_rows: int = 0):
        keep = []
        layers = (model.layer1, model.layer2, model.layer3, model.layer4)
        convs = [(model.conv1, model.bn1)]
        for layer in layers:
            for blk in layer:
                convs += [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2)]
                if blk.downsample is not None:
                    convs.append((blk.downsample[0], blk.downsample[1]))
        self.convs = (N.ConvBN * len(convs))(*[_conv_bn_struct(c, b, keep) for c, b in convs])
        w = N.ResnetBasicWeights()
        w.dtype = code
        for i, layer in enumerate(layers):
            w.layers[i] = len(layer)
        w.convs = C.cast(self.convs, C.POINTER(N.ConvBN))
        w.n_convs = len(convs)
        w.tile_rows = tile_rows
        self.w = w
        nbytes = N.lib().hipt_resnet_basic_packed_bytes(C.byref(w))
        if not nbytes:
            raise ValueError("ResNet18_Baseline: this layer configuration is outside the library's network "
                             f"({N.lib().hipt_last_error().decode(errors='replace')})")
        self.image = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        N.call("hipt_resnet_basic_pack_weights", C.byref(w), N.ptr(self.image), N.stream_ptr(dev))
        self.keep = keep  # the fp32 sources stay alive until the packing kernels (enqueued above) have read them

    @property
    def ref(self):
        return C.byref(self.w)


class ResNet18_Baseline(WeightImageCache, nn.Module):
    _image_buffers = True  # the BN running statistics are folded into the image with the parameters
    FEATURES = 512

    def __init__(self, layers=(2, 2, 2, 2), num_classes=1000):
        self.inplanes = 64
        super(ResNet18_Baseline, self).__init__()
        block = BasicBlock_Baseline
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(self.FEATURES * block.expansion, num_classes)

        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._init_host()
        self._norm = IMAGENET_MEAN + IMAGENET_STD
        self._tile_rows = 0

    _make_layer = ResNet_Baseline._make_layer
    set_input_normalization = ResNet_Baseline.set_input_normalization
    weight_device = ResNet_Baseline.weight_device
    _input_kind = staticmethod(ResNet_Baseline._input_kind)

    def set_tile_rows(self, rows: int = 0):
        """``0``: every conv's tile height comes from the library's rule (:func:`conv_tile_rows`); ``128``: 128-row tiles on every
        conv.  The features are the same bits either way; this is the switch of the rule's A/B (tools/resnet18_bench.py)."""
        if rows not in (0, 128):
            raise ValueError(f"set_tile_rows: 0 (the rule) or 128, got {rows!r}")
        self._tile_rows = int(rows)
        return self

    def _check_inference_only(self):
        if self.training:
            raise RuntimeError("ResNet18_Baseline HIP forward: BatchNorm in train() mode needs batch statistics (inference kernels "
                               "only); call .eval()")
        self._warn_no_grad_fn("HIP ResNet18_Baseline forward returns tensors without grad_fn: no gradient flows into the extractor "
                              "weights (the reference uses it as a frozen feature extractor)")

    def _packed_for(self, dev) -> _PackedResnet18:
        self._check_inference_only()
        rows = self._tile_rows
        return self._cached(dev, (rows,), lambda code: _PackedResnet18(self, code, dev, rows))

    def features(self, x):
        """``[B, 512]`` fp32: the network up to and including the average pool."""
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
        need = N.lib().hipt_resnet_basic_workspace_bytes(pk.ref, B, H, W)
        # one scratch per stream: two streams driving the model at once never share activations
        ws = Fn.workspace(dev, need, slot=("resnet18", torch.cuda.current_stream(dev).cuda_stream))
        norm = (C.c_float * 6)(*self._norm)
        N.call("hipt_resnet_basic_forward", pk.ref, N.ptr(pk.image), N.ptr(x), kind, C.cast(norm, C.c_void_p), B, H, W, N.ptr(out),
               N.ptr(ws), ws.numel(), N.stream_ptr(dev))
        return out

    def forward(self, x):
        """``fc(features(x))``: ``[B, 512]`` fp32 with the Histo route's empty ``nn.Sequential``, ``[B, out_features]`` fp32 with
        an ``nn.Linear`` (fp32 ``hipt_linear`` whatever the compute dtype: it is 0.03 % of the network's work)."""
        fc = self.fc
        if not ((isinstance(fc, nn.Sequential) and len(fc) == 0) or isinstance(fc, nn.Linear)):
            raise NotImplementedError(f"ResNet18_Baseline: fc is {type(fc).__name__}; only nn.Linear and the empty nn.Sequential of the "
                                      "reference's Histo route have a HIP path")
        h = self.features(x)
        if isinstance(fc, nn.Linear):
            h = Fn.linear(h, fc.weight.detach(), None if fc.bias is None else fc.bias.detach())
        return h


def resnet18_baseline(pretrained=False, dataset='ImageNet', ckpt_path=None):
    """ResNet18, as the reference builds it (models/resnet_custom.py:112-135).  ``dataset='ImageNet'`` with ``pretrained`` reads
    the torch hub cache file; ``dataset='Histo'`` with ``pretrained`` reads the Lightning checkpoint at ``ckpt_path`` (default: the
    reference's relative path), strips ``'model.'`` / ``'resnet.'`` from its keys, loads the keys the model has and replaces ``fc``
    by an empty ``nn.Sequential`` (output ``[B, 512]``).  In every other case ``fc`` stays (output ``[B, 1000]``), as in the
    reference.  Nothing is ever downloaded."""
    model = ResNet18_Baseline()
    if dataset == 'ImageNet' and pretrained:
        model = load_pretrained_weights(model, 'resnet18')
    if pretrained and dataset == "Histo":
        path = HISTO_CKPT_PATH if ckpt_path is None else ckpt_path
        if not os.path.isfile(path):
            raise FileNotFoundError(f"histo-pretrained ResNet18 checkpoint not found at {path} (tenpercent_resnet18.ckpt of "
                                    "https://github.com/ozanciga/self-supervised-histopathology; this package never downloads)")
        ckpt = torch.load(path, map_location='cpu')['state_dict']
        cleaned = {k.replace('model.', '').replace('resnet.', ''): v for k, v in ckpt.items()}
        own = model.state_dict()
        found = {k: v for k, v in cleaned.items() if k in own}
        print('Loading histo-pretrained ResNet18' if found else 'No weight could be loaded..')
        own.update(found)
        model.load_state_dict(own)
        model.fc = nn.Sequential()
    return model
