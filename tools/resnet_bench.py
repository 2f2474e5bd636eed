#!/usr/bin/env python3
"""ResNet-50 baseline extractor (``--model_type resnet50``) throughput on one MI355X; prints ONE JSON line.

Legs (256 x 256 uint8 patches resident on the device unless said otherwise):
  * ``hip``: ``ResNet_Baseline.forward`` (one ``hipt_resnet_forward`` call) at batch 32 and 256, bf16 and fp32;
  * ``eager``: PyTorch-ROCm eager on the same network built from plain ``torch.nn`` modules (channels_last, same dtype,
    BatchNorm in eval mode, the uint8 -> ToTensor + Normalize step included), timed in rounds interleaved with ``hip``;
  * ``extract_slide``: ``feature_store.extract_slide`` over pinned HOST uint8 batches of 32 (bf16), end to end.
FLOP: counted here from the conv shapes (2 * M * N * K per conv, the pools ignored) -> achieved TFLOP/s and the fraction of the
dense MFMA peak of the dtype (MI355X spec: 2.5 PF bf16, 157.3 TF fp32).  Times: device events around ``--steps`` calls after
``--warmup``; the median of ``--rounds`` rounds.

    python tools/resnet_bench.py [--steps 20 --warmup 3 --rounds 5] [--profile]

``--profile``: a short run (bf16 + fp32, batch 256, two calls each) for ``rocprofv3 --kernel-trace --stats``."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hipt_abmil_atec23_amd import resnet_custom as rc, synth  # noqa: E402

DEV = "cuda:0"
PEAK = {"bf16": 2.5e15, "fp32": 157.3e12}
TDT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def flops_per_patch(h=256, w=256, layers=(3, 4, 6)) -> float:
    tot = 0.0
    hh, ww = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    tot += 2.0 * hh * ww * 64 * 147
    hh, ww = (hh + 1) // 2, (ww + 1) // 2
    inplanes = 64
    for L, nb in enumerate(layers):
        planes = 64 << L
        for b in range(nb):
            s = 2 if (L and b == 0) else 1
            tot += 2.0 * hh * ww * planes * inplanes          # conv1 1x1
            h2, w2 = (hh - 1) // s + 1, (ww - 1) // s + 1
            tot += 2.0 * h2 * w2 * planes * planes * 9         # conv2 3x3 / s
            tot += 2.0 * h2 * w2 * planes * 4 * planes         # conv3 1x1
            if b == 0 and (s != 1 or inplanes != planes * 4):
                tot += 2.0 * h2 * w2 * planes * 4 * inplanes   # downsample 1x1 / s
            hh, ww, inplanes = h2, w2, planes * 4
    return tot


def make_model():
    m = rc.resnet50_baseline()
    sd = synth.make_state_dict(synth.resnet_param_specs())
    g = os.path.join(ROOT, "tests", "golden", "resnet50_baseline.npz")
    if os.path.isfile(g):  # calibrated running statistics: O(1) activations, as with trained weights
        for k, v in np.load(g).items():
            if k.endswith(("running_mean", "running_var")):
                sd[k] = torch.from_numpy(v)
    m.load_state_dict(sd, strict=False)
    return m.eval().to(DEV)


class EagerResnet(nn.Module):
    """The same network in stock torch.nn, for the eager baseline (weights copied from the HIP model)."""

    def __init__(self, src, dtype):
        super().__init__()
        import copy
        self.net = copy.deepcopy(src).to(TDT[dtype]).to(memory_format=torch.channels_last).eval()
        self.mean = torch.tensor(rc.IMAGENET_MEAN, device=DEV).view(1, 3, 1, 1)
        self.std = torch.tensor(rc.IMAGENET_STD, device=DEV).view(1, 3, 1, 1)
        self.dtype = TDT[dtype]

    def forward(self, u8):
        n = self.net
        x = ((u8.float() / 255 - self.mean) / self.std).to(self.dtype).contiguous(memory_format=torch.channels_last)
        x = n.maxpool(F.relu(n.bn1(n.conv1(x))))
        for layer in (n.layer1, n.layer2, n.layer3):
            for blk in layer:
                r = x if blk.downsample is None else blk.downsample[1](blk.downsample[0](x))
                t = F.relu(blk.bn1(blk.conv1(x)))
                t = F.relu(blk.bn2(blk.conv2(t)))
                x = F.relu(blk.bn3(blk.conv3(t)) + r)
        return x.float().mean(dim=(2, 3))


def time_calls(fn, x, steps, warmup) -> float:
    """seconds per call (device events around `steps` calls)"""
    for _ in range(warmup):
        fn(x)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn(x)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / 1e3 / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--slide-patches", type=int, default=2048)
    ap.add_argument("--profile", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet_bench: no GPU visible (nothing is measured on the CPU)")
    torch.backends.cudnn.benchmark = True
    model = make_model()
    fpp = flops_per_patch()
    u8 = {b: torch.from_numpy(synth.hash_u8_np((b, 3, 256, 256), 7)).to(DEV) for b in (32, 256)}
    if a.profile:
        with torch.no_grad():
            for dt in ("bf16", "fp32"):
                model.set_compute_dtype(dt)
                for _ in range(2):
                    model(u8[256])
        torch.cuda.synchronize()
        print(json.dumps({"profile_run": "ok"}))
        return
    res = {"metric": "resnet50_baseline_patches_per_s", "patch": [256, 256], "input": "uint8 planar resident",
           "gflop_per_patch": round(fpp / 1e9, 3), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds,
           "gpu": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for dt in ("bf16", "fp32"):
            model.set_compute_dtype(dt)
            eager = EagerResnet(model, dt)
            # parity of the two legs on the timed inputs
            ref = eager(u8[32]).float()
            got = model(u8[32])
            rel = float((got - ref).norm() / ref.norm())
            res[f"rel_l2_vs_eager_{dt}"] = round(rel, 6)
            for b in (32, 256):
                th, te = [], []
                for _ in range(a.rounds):
                    th.append(time_calls(model, u8[b], a.steps, a.warmup))
                    te.append(time_calls(eager, u8[b], a.steps, a.warmup))
                sh, se = statistics.median(th), statistics.median(te)
                res[f"hip_{dt}_b{b}_patches_per_s"] = round(b / sh, 1)
                res[f"eager_{dt}_b{b}_patches_per_s"] = round(b / se, 1)
                res[f"hip_{dt}_b{b}_spread"] = round((max(th) - min(th)) / sh, 4)
                res[f"hip_{dt}_b{b}_tflops"] = round(fpp * b / sh / 1e12, 2)
                res[f"hip_{dt}_b{b}_frac_peak"] = round(fpp * b / sh / PEAK[dt], 4)
                res[f"hip_over_eager_{dt}_b{b}"] = round(se / sh, 3)
            del eager
            torch.cuda.empty_cache()
        # extract_slide: pinned host uint8 batches of 32, bf16
        from hipt_abmil_atec23_amd.feature_store import extract_slide
        model.set_compute_dtype("bf16")
        n = a.slide_patches
        host = torch.from_numpy(synth.hash_u8_np((n, 3, 256, 256), 11)).pin_memory()
        batches = [(host[i:i + 32], torch.zeros(min(32, n - i), 2, dtype=torch.int64)) for i in range(0, n, 32)]
        with tempfile.TemporaryDirectory() as d:
            extract_slide(model, batches[:4], d, "warm")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            extract_slide(model, batches, d, "slide")
            torch.cuda.synchronize()
            dt_s = time.perf_counter() - t0
        res["extract_slide_host_b32_bf16_patches_per_s"] = round(n / dt_s, 1)
        res["extract_slide_patches"] = n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
