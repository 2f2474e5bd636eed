"""Region augmentation on one MI355X: effective GB/s of hipt_augment_regions on resident 4096 x 4096 uint8 regions (bytes read
plus written over kernel time, per policy and layout), and regions/s of feature_store.extract_slide_augmented (n_augs = 1)
against feature_store.extract_slide on the same loader batches.  Prints one JSON line.

    python tools/augment_bench.py [--regions 24] [--iters 10] [--slide-regions 48]
"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from hipt_abmil_atec23_amd import HIPT_4K, synth  # noqa: E402
from hipt_abmil_atec23_amd import augment as A  # noqa: E402
from hipt_abmil_atec23_amd.feature_store import extract_slide, extract_slide_augmented  # noqa: E402


def kernel_gbps(regions, params, iters):
    out = torch.empty_like(regions)
    for _ in range(2):
        A.augment_regions(regions, params, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        A.augment_regions(regions, params, out=out)
    t1.record()
    t1.synchronize()
    ms = t0.elapsed_time(t1) / iters
    return 2 * regions.numel() / (ms * 1e-3) / 1e9, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--regions", type=int, default=24)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--slide-regions", type=int, default=48)
    args = ap.parse_args()
    dev = "cuda:0"
    R, S = args.regions, 4096
    res = {"regions": R, "size": S}
    g = torch.Generator(device=dev).manual_seed(0)
    il = torch.randint(0, 256, (R, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    for policy in ("HIPT_augment", "HIPT_augment_colour", "HIPT_wang", "HIPT_blur", "HIPT"):
        params = A.draw_region_params(policy, 0, "bench", 1, 0, R, S, S)
        for name, x in (("interleaved", il), ("planar", il.permute(0, 3, 1, 2).contiguous())):
            gbps, ms = kernel_gbps(x, params, args.iters)
            res[f"{policy}_{name}_GBps"] = round(gbps, 1)
            res[f"{policy}_{name}_ms"] = round(ms, 3)
    del il
    torch.cuda.empty_cache()

    m = HIPT_4K(None, None, dev, dev)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(dev)
    m.set_compute_dtype("bf16")
    n = args.slide_regions
    base = torch.randint(0, 256, (4, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    batches = [(base[i % 4:i % 4 + 1], torch.tensor([[i, 0]])) for i in range(n)]  # batch-1 loader batches, resident
    with tempfile.TemporaryDirectory() as d:
        for warm in (True, False):
            torch.cuda.synchronize()
            t = time.perf_counter()
            extract_slide(m, batches[:8] if warm else batches, d, "plain")
            torch.cuda.synchronize()
            t_plain = time.perf_counter() - t
            t = time.perf_counter()
            extract_slide_augmented(m, batches[:8] if warm else batches, d, "aug", "HIPT_augment", 1)
            torch.cuda.synchronize()
            t_aug = time.perf_counter() - t
    res["extract_slide_regions_per_s"] = round(n / t_plain, 1)
    res["extract_slide_augmented_n1_regions_per_s"] = round(n / t_aug, 1)
    # the target: augmented >= 0.95 x (plain / 2) -- two forwards per region, augmentation <= 5 % of a forward
    res["augmented_vs_half_plain"] = round((n / t_aug) / (n / t_plain / 2), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
