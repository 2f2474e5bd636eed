#!/usr/bin/env python3
"""Generate tests/golden/resnet50_baseline.npz and resnet50_baseline_keys.txt by running the REFERENCE's own
``models/resnet_custom.py:resnet50_baseline(pretrained=False)`` on the CPU in fp32.

Run ONLY in the build container (needs the read-only reference checkout):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_resnet.py [--ref /root/reference]

``torchvision`` is not installed here; resnet_custom.py imports it at module level but only resnet18_baseline uses it,
so an empty in-process module satisfies the import (as in make_golden.py).

Weights: ``synth.resnet_param_specs`` (integer hash).  The BatchNorm running statistics are calibrated once -- train-mode
passes with ``momentum=None`` (a cumulative average) over hash-generated images -- so that activations stay O(1) through
the 13 blocks; they are stored, since no spec can produce them.  Pixels: ``synth.hash_u8_np`` bytes through ToTensor +
Normalize(ImageNet) in fp32 torch ops (datasets/dataset_h5.py:21-37).  Stored: the running statistics, the features for
256 x 256 (2 images), 128 x 128 (2) and 224 x 160 (1, H x W) inputs (fp32 as the reference runs, plus the same module in
float64), and the model's state-dict key list.  No weights.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from hipt_abmil_atec23_amd import synth  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
# (name, batch, H, W, pixel seed) of the stored outputs
CASES = (("256", 2, 256, 256, 101), ("128", 2, 128, 128, 102), ("224x160", 1, 224, 160, 103))
CALIB = ((4, 256, 256, 201), (4, 256, 256, 202))


def normalized(u8: np.ndarray, mean=MEAN, std=STD) -> torch.Tensor:
    """ToTensor + Normalize on uint8 [B, 3, H, W] bytes, in the reference's fp32 ops."""
    x = torch.from_numpy(u8).float().div(255)
    return x.sub(torch.tensor(mean, dtype=torch.float32)[:, None, None]).div(torch.tensor(std, dtype=torch.float32)[:, None, None])


def import_reference(ref):
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    for n in ("torchvision", "torchvision.transforms", "torchvision.datasets", "torchvision.models"):
        if n not in sys.modules:
            sys.modules[n] = types.ModuleType(n)
    import models.resnet_custom as rc
    return rc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    rc = import_reference(args.ref)
    torch.manual_seed(0)
    model = rc.resnet50_baseline(pretrained=False)
    missing, unexpected = model.load_state_dict(synth.make_state_dict(synth.resnet_param_specs()), strict=False)
    assert not unexpected and all(k.endswith(("running_mean", "running_var", "num_batches_tracked")) for k in missing), missing
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.reset_running_stats()
        m.momentum = None
    model.train()
    with torch.no_grad():
        for b, h, w, seed in CALIB:
            model(normalized(synth.hash_u8_np((b, 3, h, w), seed)))
    model.eval()
    out = {}
    names = {m: n for n, m in model.named_modules()}
    for m in bns:
        out[names[m] + ".running_mean"] = m.running_mean.numpy().astype(np.float32)
        out[names[m] + ".running_var"] = m.running_var.numpy().astype(np.float32)
    with torch.no_grad():
        for name, b, h, w, seed in CASES:
            out["out_" + name] = model(normalized(synth.hash_u8_np((b, 3, h, w), seed))).numpy()
            print(name, out["out_" + name].shape, float(np.abs(out["out_" + name]).max()), float(out["out_" + name].std()))
        # the same module in float64: the fp32 outputs above carry ~2-4e-6 (rel-L2) of fp32 rounding accumulated over 43
        # convolutions; the fp64 twin pins the tests' own fp64 restatement to ~1e-15
        model.double()
        for name, b, h, w, seed in CASES:
            out["out64_" + name] = model(normalized(synth.hash_u8_np((b, 3, h, w), seed)).double()).numpy()
    np.savez_compressed(os.path.join(HERE, "resnet50_baseline.npz"), **out)
    with open(os.path.join(HERE, "resnet50_baseline_keys.txt"), "w") as f:
        for k, v in model.state_dict().items():
            f.write(f"{k} {'x'.join(str(d) for d in v.shape) if v.dim() else '-'}\n")
    print("wrote", os.path.join(HERE, "resnet50_baseline.npz"))


if __name__ == "__main__":
    main()
