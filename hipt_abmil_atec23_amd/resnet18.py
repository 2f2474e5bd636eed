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

import os

import torch
import torch.nn as nn

from . import _native as N
from . import functional as Fn
from .resnet_custom import _conv2d, _ResNetHost, conv2d_nhwc, load_pretrained_weights, pack_conv_bn

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
    return _conv2d("conv2d_nhwc_ex", "hipt_conv2d_ex", x, w_packed, bias, kernel_size, stride, padding, resid, relu, dtype, int(tile_rows))


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


class ResNet18_Baseline(_ResNetHost):
    _LAYERS = ("layer1", "layer2", "layer3", "layer4")
    _WEIGHTS, _ENTRY, _SLOT, FEATURES = N.ResnetBasicWeights, "hipt_resnet_basic", "resnet18", 512

    def __init__(self, layers=(2, 2, 2, 2), num_classes=1000):
        super(ResNet18_Baseline, self).__init__()
        self._build(BasicBlock_Baseline, layers)
        self.fc = nn.Linear(self.FEATURES * BasicBlock_Baseline.expansion, num_classes)
        self._init_weights()
        self._tile_rows = 0

    def set_tile_rows(self, rows: int = 0):
        """``0``: every conv's tile height comes from the library's rule (:func:`conv_tile_rows`); ``128``: 128-row tiles on every
        conv.  The features are the same bits either way; this is the switch of the rule's A/B (tools/resnet18_bench.py)."""
        if rows not in (0, 128):
            raise ValueError(f"set_tile_rows: 0 (the rule) or 128, got {rows!r}")
        self._tile_rows = int(rows)
        return self

    def _struct_fields(self) -> dict:
        return {"tile_rows": self._tile_rows}

    def features(self, x):
        """``[B, 512]`` fp32: the network up to and including the average pool."""
        return self._pooled(x)

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
