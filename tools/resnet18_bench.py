#!/usr/bin/env python3
"""HistoResNet-18 extractor (``--model_type resnet18``) throughput on one MI355X; prints ONE JSON line and, with ``--out``,
writes it to a file.

Legs (256 x 256 uint8 patches resident on the device, batch 32 -- the reference's -- and 256, bf16 and fp32):
  * ``hip``: ``ResNet18_Baseline.forward`` with ``fc = nn.Sequential()`` (one ``hipt_resnet_basic_forward`` call);
  * ``eager``: PyTorch-ROCm eager on the same network built from stock ``torch.nn`` modules (channels_last, same dtype,
    BatchNorm in eval mode, the uint8 -> ToTensor + Normalize step included), timed in rounds interleaved with ``hip``;
  * the tile-rule A/B at each batch: the rule (64-row tiles where 128-row tiles leave CUs idle) against 128 rows forced on every
    conv (``ResNet18_Baseline.set_tile_rows(128)``), interleaved, ``--ab-rounds`` rounds; both give the same bits.
Times: device events around ``--steps`` calls after ``--warmup``; medians over rounds, spreads as (max - min) / median.

    python tools/resnet18_bench.py [--steps 20 --warmup 3 --rounds 5 --ab-rounds 3] [--out profiles/resnet18_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from hipt_abmil_atec23_amd import resnet18 as r18, resnet_custom as rc, synth  # noqa: E402

DEV = "cuda:0"
TDT = {"bf16": torch.bfloat16, "fp32": torch.float32}


def flops_per_patch(h=256, w=256) -> float:
    """2 * M * N * K per conv, from the conv table (the pools ignored)"""
    tot, s = 0.0, (h // 2, w // 2)
    for conv, _, cout, cin, k in synth.resnet18_conv_bn_names():
        if conv == "conv1":
            tot += 2.0 * s[0] * s[1] * cout * cin * k * k
            s = (s[0] // 2, s[1] // 2)
            continue
        if conv.endswith(".0.conv1") and not conv.startswith("layer1"):
            s = (s[0] // 2, s[1] // 2)
        tot += 2.0 * s[0] * s[1] * cout * cin * k * k
    return tot


def make_model():
    m = r18.resnet18_baseline()
    m.load_state_dict(synth.make_state_dict(synth.resnet18_param_specs()), strict=False)
    m.fc = nn.Sequential()
    return m.eval().to(DEV)


class EagerResnet18(nn.Module):
    """The same network in stock torch.nn (weights copied from the HIP model)."""

    def __init__(self, src, dtype):
        super().__init__()
        conv = lambda c: nn.Conv2d(c.in_channels, c.out_channels, c.kernel_size, c.stride, c.padding, bias=False)
        self.stem = nn.Sequential(conv(src.conv1), nn.BatchNorm2d(64))
        self.blocks = nn.ModuleList()
        for layer in (src.layer1, src.layer2, src.layer3, src.layer4):
            for blk in layer:
                mods = nn.ModuleDict({"c1": conv(blk.conv1), "b1": nn.BatchNorm2d(blk.conv1.out_channels),
                                      "c2": conv(blk.conv2), "b2": nn.BatchNorm2d(blk.conv2.out_channels)})
                if blk.downsample is not None:
                    mods["cd"], mods["bd"] = conv(blk.downsample[0]), nn.BatchNorm2d(blk.downsample[0].out_channels)
                self.blocks.append(mods)
        pairs = [(self.stem[0], self.stem[1], src.conv1, src.bn1)]
        for mods, blk in zip(self.blocks, [b for layer in (src.layer1, src.layer2, src.layer3, src.layer4) for b in layer]):
            pairs += [(mods["c1"], mods["b1"], blk.conv1, blk.bn1), (mods["c2"], mods["b2"], blk.conv2, blk.bn2)]
            if blk.downsample is not None:
                pairs.append((mods["cd"], mods["bd"], blk.downsample[0], blk.downsample[1]))
        for c, b, sc, sb in pairs:
            c.load_state_dict(sc.state_dict())
            b.load_state_dict(sb.state_dict())
        self.to(DEV).to(TDT[dtype]).to(memory_format=torch.channels_last).eval()
        self.mean = torch.tensor(rc.IMAGENET_MEAN, device=DEV).view(1, 3, 1, 1)
        self.std = torch.tensor(rc.IMAGENET_STD, device=DEV).view(1, 3, 1, 1)
        self.dtype = TDT[dtype]

    def forward(self, u8):
        x = ((u8.float() / 255 - self.mean) / self.std).to(self.dtype).contiguous(memory_format=torch.channels_last)
        x = F.max_pool2d(F.relu(self.stem(x)), 3, 2, 1)
        for m in self.blocks:
            r = m["bd"](m["cd"](x)) if "cd" in m else x
            t = F.relu(m["b1"](m["c1"](x)))
            x = F.relu(m["b2"](m["c2"](t)) + r)
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
    ap.add_argument("--ab-rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resnet18_bench: no GPU visible (nothing is measured on the CPU)")
    torch.backends.cudnn.benchmark = True
    model = make_model()
    fpp = flops_per_patch()
    u8 = {b: torch.from_numpy(synth.hash_u8_np((b, 3, 256, 256), 7)).to(DEV) for b in (32, 256)}
    res = {"metric": "resnet18_baseline_patches_per_s", "patch": [256, 256], "input": "uint8 planar resident",
           "gflop_per_patch": round(fpp / 1e9, 3), "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds, "ab_rounds": a.ab_rounds,
           "gpu": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        for dt in ("bf16", "fp32"):
            model.set_compute_dtype(dt)
            eager = EagerResnet18(model, dt)
            ref = eager(u8[32]).float()
            got = model(u8[32])
            res[f"rel_l2_vs_eager_{dt}"] = round(float((got - ref).norm() / ref.norm()), 6)
            model.set_tile_rows(128)
            res[f"rule_and_128_rows_same_bits_{dt}"] = bool(torch.equal(model(u8[32]), got))
            model.set_tile_rows(0)
            for b in (32, 256):
                th, te = [], []
                for _ in range(a.rounds):
                    th.append(time_calls(model, u8[b], a.steps, a.warmup))
                    te.append(time_calls(eager, u8[b], a.steps, a.warmup))
                sh, se = statistics.median(th), statistics.median(te)
                res[f"hip_{dt}_b{b}_patches_per_s"] = round(b / sh, 1)
                res[f"eager_{dt}_b{b}_patches_per_s"] = round(b / se, 1)
                res[f"hip_{dt}_b{b}_spread"] = round((max(th) - min(th)) / sh, 4)
                res[f"eager_{dt}_b{b}_spread"] = round((max(te) - min(te)) / se, 4)
                res[f"hip_{dt}_b{b}_tflops"] = round(fpp * b / sh / 1e12, 2)
                # the tile rule against 128 rows everywhere, interleaved
                tr, t128 = [], []
                for _ in range(a.ab_rounds):
                    model.set_tile_rows(0)
                    tr.append(time_calls(model, u8[b], a.steps, a.warmup))
                    model.set_tile_rows(128)
                    t128.append(time_calls(model, u8[b], a.steps, a.warmup))
                model.set_tile_rows(0)
                res[f"ab_{dt}_b{b}_rule_ms"] = [round(t * 1e3, 4) for t in tr]
                res[f"ab_{dt}_b{b}_rows128_ms"] = [round(t * 1e3, 4) for t in t128]
            del eager
            torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
