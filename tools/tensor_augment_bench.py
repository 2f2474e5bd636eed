"""Tensor-space augmentation on one MI355X: microseconds per call and effective GB/s of tensor_augment.augment_tensor on 256 resident
uint8 regions of 256 x 256 (bytes the algorithm needs over call time: 3 B read + 12 B written per pixel, the read twice for `all`, whose
contrast mean takes a pass of its own), per policy and layout, beside the same op sequence written with torch ops on the device (batched
over the regions; `all` grouped by the order of its colour ops) -- the only route there is without the kernel.  The two are timed
alternately, with device events around `--iters` calls each.  The records are drawn once, outside the timed window.  Prints one JSON line.

    python tools/tensor_augment_bench.py [--regions 256] [--size 256] [--iters 50] [--rounds 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from hipt_abmil_atec23_amd import tensor_augment as TA  # noqa: E402


def _gray(x):
    return (0.2989 * x[:, 0] + 0.587 * x[:, 1] + 0.114 * x[:, 2]).unsqueeze(1)


def _blend(a, b, ratio):
    return (ratio * a + (1.0 - ratio) * b).clamp(0, 1)


def _hue(x, hue):
    r, g, b = x.unbind(1)
    maxc, minc = x.max(1).values, x.min(1).values
    eqc = maxc == minc
    cr = maxc - minc
    ones = torch.ones_like(maxc)
    s = cr / torch.where(eqc, ones, maxc)
    div = torch.where(eqc, ones, cr)
    rc, gc, bc = (maxc - r) / div, (maxc - g) / div, (maxc - b) / div
    h = (maxc == r) * (bc - gc) + ((maxc == g) & (maxc != r)) * (2.0 + rc - bc) + ((maxc != g) & (maxc != r)) * (4.0 + gc - rc)
    h = (torch.fmod(h / 6.0 + 1.0, 1.0) + hue) % 1.0
    i = torch.floor(h * 6.0)
    f = h * 6.0 - i
    i = i.to(torch.int32) % 6
    v = maxc
    p, q, t = (v * (1.0 - s)).clamp(0, 1), (v * (1.0 - s * f)).clamp(0, 1), (v * (1.0 - s * (1.0 - f))).clamp(0, 1)
    pick = lambda opts: torch.stack(opts, 0).gather(0, i.long().unsqueeze(0))[0]   # noqa: E731
    return torch.stack((pick((v, q, p, p, t, v)), pick((t, v, v, q, p, p)), pick((p, p, t, v, v, q))), 1)


class TorchRoute:
    """the op sequence of tensor_augment on torch device ops; everything that depends on the records alone is prepared once"""

    def __init__(self, params, rows, cols, dev):
        n = len(params)
        self.hf = torch.tensor([p.hflip for p in params], device=dev).view(n, 1, 1, 1)
        self.vf = torch.tensor([p.vflip for p in params], device=dev).view(n, 1, 1, 1)
        theta = torch.tensor([p.theta for p in params], dtype=torch.float32, device=dev).view(n, 2, 3)
        base = torch.empty(1, rows, cols, 3, device=dev)
        base[..., 0].copy_(torch.linspace(-cols * 0.5 + 0.5, cols * 0.5 - 0.5, cols, device=dev))
        base[..., 1].copy_(torch.linspace(-rows * 0.5 + 0.5, rows * 0.5 - 0.5, rows, device=dev).unsqueeze(-1))
        base[..., 2].fill_(1)
        self.base = base.view(1, rows * cols, 3).expand(n, -1, -1)
        self.rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * cols, 0.5 * rows], device=dev)
        self.shape = (n, rows, cols, 2)
        groups = {}
        for i, p in enumerate(params):
            groups.setdefault(p.order, []).append(i)
        col = lambda name: torch.tensor([getattr(p, name) for p in params], dtype=torch.float32, device=dev).view(n, 1, 1, 1)   # noqa: E731
        self.b, self.c, self.s, self.h = col("brightness"), col("contrast"), col("saturation"), col("hue").view(n, 1, 1)
        self.groups = [(order, torch.tensor(idx, device=dev)) for order, idx in groups.items() if order]
        self.mean = torch.tensor(TA.IMAGENET_MEAN, device=dev).view(1, 3, 1, 1)
        self.std = torch.tensor(TA.IMAGENET_STD, device=dev).view(1, 3, 1, 1)

    def __call__(self, planar_u8):
        x = planar_u8.float().div(255)
        x = torch.where(self.hf, x.flip(-1), x)
        x = torch.where(self.vf, x.flip(-2), x)
        grid = self.base.bmm(self.rescaled).view(self.shape)
        x = torch.nn.functional.grid_sample(x, grid, mode="nearest", padding_mode="zeros", align_corners=False)
        for order, idx in self.groups:
            y = x[idx]
            for op in order:
                if op == TA.OP_BRIGHTNESS:
                    y = _blend(y, torch.zeros_like(y), self.b[idx])
                elif op == TA.OP_CONTRAST:
                    y = _blend(y, _gray(y).mean(dim=(1, 2, 3), keepdim=True), self.c[idx])
                elif op == TA.OP_SATURATION:
                    y = _blend(y, _gray(y), self.s[idx])
                else:
                    y = _hue(y, self.h[idx])
            x[idx] = y
        return (x - self.mean) / self.std


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / iters * 1e3   # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=256)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tensor_augment_bench: no HIP device (there is nothing to measure without one)")
    dev = torch.device("cuda:0")
    n, S = args.regions, args.size
    res = {"gpu": torch.cuda.get_device_name(0), "regions": n, "size": S, "iters": args.iters, "rounds": args.rounds}
    g = torch.Generator(device=dev).manual_seed(0)
    il = torch.randint(0, 256, (n, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    planar = il.permute(0, 3, 1, 2).contiguous()
    out = torch.empty((n, 3, S, S), dtype=torch.float32, device=dev)
    for policy in ("spatial", "all"):
        params = TA.draw_tensor_region_params(policy, 0, "bench", 1, 0, n, S, S)
        nbytes = n * S * S * (12 + 3 * (2 if policy == "all" else 1))
        route = TorchRoute(params, S, S, dev)
        calls = {"kernel_planar": lambda: TA.augment_tensor(planar, params, out=out),
                 "kernel_interleaved": lambda: TA.augment_tensor(il, params, out=out),
                 "torch_ops": lambda: route(planar)}
        diff = (calls["kernel_planar"]() - route(planar)).abs().max().item()
        res[f"{policy}_max_abs_kernel_minus_torch_ops"] = diff
        for fn in calls.values():   # warm-up of every shape of the timed window
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        best = {k: float("inf") for k in calls}
        for _ in range(args.rounds):   # alternating
            for k, fn in calls.items():
                best[k] = min(best[k], timed(fn, args.iters))
        for k, us in best.items():
            res[f"{policy}_{k}_us"] = round(us, 1)
            res[f"{policy}_{k}_GBps"] = round(nbytes / (us * 1e-6) / 1e9, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
