"""Hierarchical heat-maps on the device: one resident 4096 x 4096 region, all 48 pictures.

Timed with device events around ``iters`` calls, median of ``rounds`` rounds, every shape warmed up first:
  compose      ``compose_heatmaps`` (two rank launches + the render launch) at scale 4 and at scale 1
  ranks        the two ``hipt_hier_ranks`` launches alone
  render       compose minus ranks: the render launch (plus the small permute in front of the ranks)
  whole call   ``hierarchical_heatmaps`` at scale 4 (four regions through ViT-256 / ViT-4K, Pillow's resize on the host --
               ``host_resize=True``; tools/resize_bench.py times the default, the device resize -- and the pictures), with a
               host clock around calls that end in a device synchronise
The render kernel's figure of merit is the bytes it must write (144 per pixel for 48 pictures) per second, against the HBM peak
(8.0 TB/s specified; MI355X_MICROARCH: 6.29 TB/s measured for a copy).  Attention maps are seeded random numbers: the kernels'
time does not depend on the values.  The pictures of the scale-4 case are compared with the numpy restatement when
``--check`` is given (tests/hier_heatmap_ref.py; takes seconds).

    python tools/hier_heatmap_bench.py --json profiles/hier_heatmap_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12       # bytes / s, specified
HBM_COPY = 6.29e12      # bytes / s, measured for a float4 copy (MI355X_MICROARCH)


def event_ms(fn, iters, rounds, warmup=2):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        per.append(a.elapsed_time(b) / iters)
    return statistics.median(per), per


def main():
    import torch

    from hipt_abmil_atec23_amd import HIPT_4K, synth
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hier_heatmap_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    g = args.side // 256
    n, nh = g * g, 6
    rng = np.random.default_rng(0)
    a256 = torch.from_numpy(rng.random((4, n, nh, 256), dtype=np.float32)).to(dev)
    a4k = torch.from_numpy(rng.random((4, nh, n), dtype=np.float32)).to(dev)
    results = []
    for scale in (4, 1):
        side = args.side // scale
        base = torch.from_numpy(rng.integers(0, 256, (side, side, 3), dtype=np.uint8)).to(dev)
        out = {k: torch.empty((m, side, side, 3), dtype=torch.uint8, device=dev) for k, m in (("4k", nh), ("256", nh), ("blend", nh * nh))}
        iters = args.iters if scale > 1 else max(1, args.iters // 4)

        def compose():
            HH.compose_heatmaps(a256, a4k, g, g, base, scale=scale, out=out)

        def ranks():
            HH.hier_ranks(a4k, 256 // scale)
            HH.hier_ranks(a256[:2].permute(0, 2, 1, 3).contiguous(), 16 // scale)
        c_ms, c_rounds = event_ms(compose, iters, args.rounds)
        r_ms, r_rounds = event_ms(ranks, iters, args.rounds)
        written = 48 * side * side * 3
        render_s = (c_ms - r_ms) / 1e3
        res = {"case": "compose_heatmaps", "region": args.side, "scale": scale, "pictures": 48, "picture_side": side, "iters": iters,
               "compose_ms": round(c_ms, 4), "compose_ms_rounds": [round(x, 4) for x in c_rounds],
               "ranks_ms": round(r_ms, 4), "ranks_ms_rounds": [round(x, 4) for x in r_rounds],
               "render_ms": round(c_ms - r_ms, 4), "bytes_written": written,
               "render_written_TB_per_s": round(written / render_s / 1e12, 3),
               "render_written_over_hbm_peak": round(written / render_s / HBM_PEAK, 3),
               "render_written_over_measured_copy": round(written / render_s / HBM_COPY, 3),
               "bound": "bytes written over the HBM peak (the tables are L2-sized; the float64 and blend arithmetic is not counted)"}
        if args.check and scale == 4:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import hier_heatmap_ref as HR
            import matplotlib
            t0 = time.perf_counter()
            want = HR.pictures(a256.cpu().numpy(), a4k.cpu().numpy(), g, g, base.cpu().numpy(), scale=scale,
                               cmap=matplotlib.colormaps["coolwarm"])
            res["host_restatement_s"] = round(time.perf_counter() - t0, 2)
            compose()
            res["equal"] = all(bool(np.array_equal(out[k].cpu().numpy(), want[k])) for k in out)
        results.append(res)
        print(json.dumps(res))
        del out, base
    # the whole call: ViTs included (synthetic weights: the time does not depend on them), bf16 as the benchmark runs them
    m = HIPT_4K(None, None, dev, dev)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(dev)
    m.set_compute_dtype("bf16")
    region = synth.hash_u8_np((args.side, args.side, 3), 9)
    from PIL import Image
    t0 = time.perf_counter()
    base = np.array(Image.fromarray(region).resize((args.side // 4, args.side // 4)))
    resize_s = time.perf_counter() - t0
    region_d = torch.from_numpy(region).to(dev)

    def whole(**kw):
        HH.hierarchical_heatmaps(m, region_d, scale=4, **kw)
        torch.cuda.synchronize()
    per = {"with_host_resize": [], "base_given": []}
    whole(host_resize=True), whole(base=base)
    for _ in range(args.rounds):
        for name, kw in (("with_host_resize", {"host_resize": True}), ("base_given", {"base": base})):
            t0 = time.perf_counter()
            whole(**kw)
            per[name].append(time.perf_counter() - t0)
    res = {"case": "hierarchical_heatmaps", "region": args.side, "scale": 4, "compute_dtype": "bf16", "clock": "host, each call ends in a synchronise",
           "call_ms": round(statistics.median(per["with_host_resize"]) * 1e3, 2),
           "call_ms_rounds": [round(x * 1e3, 2) for x in per["with_host_resize"]],
           "call_ms_base_given": round(statistics.median(per["base_given"]) * 1e3, 2),
           "call_ms_base_given_rounds": [round(x * 1e3, 2) for x in per["base_given"]],
           "pillow_resize_ms": round(resize_s * 1e3, 2)}
    results.append(res)
    print(json.dumps(res))
    doc = {"tool": "tools/hier_heatmap_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "protocol": "device events around `iters` calls per round, median of the rounds, two warm-up calls per shape; the whole call by a "
                       "host clock around calls that end in a synchronise",
           "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_measured_copy_bytes_per_s": HBM_COPY, "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
