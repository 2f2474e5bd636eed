"""Two independent statements of torchvision's ResNet-18 (what the reference's models/resnet_custom.py:resnet18_baseline
builds), written from its public definition, and the fixtures the ResNet-18 tests share:

  * ``TorchResNet18``: a stock ``torch.nn`` composition (Conv2d, BatchNorm2d in eval, ReLU, MaxPool2d, AdaptiveAvgPool2d,
    Linear) in fp32, carrying the 122 state-dict keys;
  * ``forward_fp64``: a functional restatement in float64 in the style of tests/resnet_ref.py, and its twin
    ``forward_bf16_emulated`` with the bf16 mode's rounding points.

tests/test_resnet18_host.py holds the two against each other on the CPU.  torchvision is not installed where these tests
were written, so NO stored output of the reference's own module exists and no golden file is committed for this network:
the references are these two restatements alone."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from hipt_abmil_atec23_amd import synth
from resnet_ref import conv_bn as _conv_bn  # noqa: F401  (eval-mode conv + BN in float64; the tests use it as R._conv_bn)
from resnet_ref import normalized  # noqa: F401  (ToTensor + Normalize of uint8 [B, 3, H, W] in fp32 ops)

LAYERS = (2, 2, 2, 2)
# (name, batch, H, W, pixel seed): 32 x 32 ends in a 1 x 1 map (the average pool sums one value)
CASES = (("64", 2, 64, 64, 201), ("96x64", 1, 96, 64, 202), ("32", 3, 32, 32, 203))


def key_list(layers=LAYERS):
    """torchvision resnet18's state-dict keys, in order, written out by rule."""
    bn = lambda p: [p + s for s in (".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked")]
    keys = ["conv1.weight"] + bn("bn1")
    for L, nb in enumerate(layers):
        for b in range(nb):
            p = f"layer{L + 1}.{b}."
            keys += [p + "conv1.weight"] + bn(p + "bn1") + [p + "conv2.weight"] + bn(p + "bn2")
            if L > 0 and b == 0:
                keys += [p + "downsample.0.weight"] + bn(p + "downsample.1")
    return keys + ["fc.weight", "fc.bias"]


def state_dict():
    """hash weights, running statistics and fc (synth.resnet18_param_specs)"""
    return synth.make_state_dict(synth.resnet18_param_specs())


def pixels(b, h, w, seed):
    return synth.hash_u8_np((b, 3, h, w), seed)


# ---- statement 1: stock torch.nn modules ---------------------------------------------------------------------------------
class _Block(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, stride, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(cout)
        self.conv2 = nn.Conv2d(cout, cout, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(cout)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride, bias=False), nn.BatchNorm2d(cout))

    def forward(self, x):
        identity = x if self.downsample is None else self.downsample(x)
        out = torch.relu(self.bn1(self.conv1(x)))
        return torch.relu(self.bn2(self.conv2(out)) + identity)


class TorchResNet18(nn.Module):
    def __init__(self, layers=LAYERS, num_classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        cin = 64
        for L, nb in enumerate(layers):
            cout = 64 << L
            blocks = [_Block(cin if b == 0 else cout, cout, 2 if (L > 0 and b == 0) else 1) for b in range(nb)]
            setattr(self, f"layer{L + 1}", nn.Sequential(*blocks))
            cin = cout
        self.fc = nn.Linear(cin, num_classes)

    def features(self, x):
        x = F.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        for L in range(1, 5):
            x = getattr(self, f"layer{L}")(x)
        return F.adaptive_avg_pool2d(x, 1).flatten(1)

    def forward(self, x):
        return self.fc(self.features(x))


# ---- statement 2: functional, float64 ------------------------------------------------------------------------------------
def forward_fp64(sd, x, layers=LAYERS) -> torch.Tensor:
    """[B, 512] float64 features (before fc) of x [B, 3, H, W]"""
    x = F.max_pool2d(F.relu(_conv_bn(x.double(), sd, "conv1", "bn1", 2, 3)), 3, 2, 1)
    for L, nb in enumerate(layers):
        for b in range(nb):
            p = f"layer{L + 1}.{b}."
            s = 2 if (L > 0 and b == 0) else 1
            t = F.relu(_conv_bn(x, sd, p + "conv1", p + "bn1", s, 1))
            r = _conv_bn(x, sd, p + "downsample.0", p + "downsample.1", s) if (p + "downsample.0.weight") in sd else x
            x = F.relu(_conv_bn(t, sd, p + "conv2", p + "bn2", 1, 1) + r)
    return x.mean(dim=(2, 3))


def forward_bf16_emulated(sd, x, layers=LAYERS) -> torch.Tensor:
    """The bf16 mode's rounding points with float64 arithmetic in between: the normalised input, every BN-folded weight (folded in
    float64, rounded to fp32 and then to bf16, as the packing kernel does) and each of the 20 stored activations (stem, 16 block
    convs, 3 downsample branches) rounded to bf16; biases (fp32) and the pools exact.  The library's bf16 forward differs from this
    only by fp32 accumulation order."""
    bf = lambda t: t.float().to(torch.bfloat16).double()

    def cbn(t, conv, bn, stride=1, pad=0, eps=1e-5):
        d = lambda k: sd[k].double()
        scale = d(bn + ".weight") / torch.sqrt(d(bn + ".running_var") + eps)
        w = bf(d(conv + ".weight") * scale[:, None, None, None])
        bias = (d(bn + ".bias") - d(bn + ".running_mean") * scale).float().double()
        return F.conv2d(t, w, stride=stride, padding=pad) + bias[None, :, None, None]

    x = bf(x.double())
    x = F.max_pool2d(bf(F.relu(cbn(x, "conv1", "bn1", 2, 3))), 3, 2, 1)
    for L, nb in enumerate(layers):
        for b in range(nb):
            p = f"layer{L + 1}.{b}."
            s = 2 if (L > 0 and b == 0) else 1
            t = bf(F.relu(cbn(x, p + "conv1", p + "bn1", s, 1)))
            r = bf(cbn(x, p + "downsample.0", p + "downsample.1", s)) if (p + "downsample.0.weight") in sd else x
            x = bf(F.relu(cbn(t, p + "conv2", p + "bn2", 1, 1) + r))
    return x.mean(dim=(2, 3))
