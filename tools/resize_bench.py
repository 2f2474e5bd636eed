"""Pillow-exact resize on the device: the two hot shapes, each route, against Pillow on this box's host.

Timed with device events around ``iters`` calls, median of ``rounds`` rounds, every shape warmed up first:
  region    one resident 4096 x 4096 region -> 1024 x 1024 (the heat-maps' background), bicubic
  patches   256 resident patches 512 x 512 -> 256 x 256 (``custom_downsample=2``), bicubic
  identity  ``resize_u8`` to the same size: the kernel as a plain copy, what its loads and stores alone cost
Each for the fused route (one launch, no intermediate image in memory) and the general one (two launches, the intermediate image
through the workspace).  The figure of merit is (bytes read + bytes written) / time -- for the general route the bytes the fused
one moves, so that both are measured against the same necessary traffic -- against the 8.0 TB/s the project quotes for HBM.
Pillow's ``resize`` of the same arrays runs on the host in the same process (a host clock; the median of ``rounds`` calls).
Then the whole ``hierarchical_heatmaps`` call at scale 4 in three forms: the default (device resize), ``host_resize=True`` and
``base`` handed in; a host clock around calls that end in a device synchronise.  ``--check`` compares every device result with
Pillow's bytes.

    python tools/resize_bench.py --check --json profiles/resize_bench.json
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
    from PIL import Image

    from hipt_abmil_atec23_amd import HIPT_4K, synth
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    from hipt_abmil_atec23_amd import resize as RZ
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resize_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    results = []
    for case, n, side, out_side in (("region", 1, 4096, 1024), ("patches", 256, 512, 256), ("identity", 1, 4096, 4096)):
        host = rng.integers(0, 256, (n, side, side, 3), dtype=np.uint8)
        x = torch.from_numpy(host).to(dev)
        out = torch.empty((n, out_side, out_side, 3), dtype=torch.uint8, device=dev)
        moved = x.numel() + out.numel()
        res = {"case": case, "n": n, "in": [side, side], "out": [out_side, out_side], "filter": "bicubic", "iters": args.iters,
               "bytes_read_plus_written": moved}
        want = None
        if case != "identity":
            per = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                want = [np.array(Image.fromarray(a).resize((out_side, out_side))) for a in host]
                per.append(time.perf_counter() - t0)
            res["pillow_host_ms"] = round(statistics.median(per) * 1e3, 3)
            res["pillow_host_ms_rounds"] = [round(v * 1e3, 3) for v in per]
        for route in (("fused", "general") if case != "identity" else (None,)):
            ms, rounds = event_ms(lambda: RZ.resize_u8(x, (out_side, out_side), out=out, _route=route), args.iters, args.rounds)
            name = route or "copy"
            res[f"{name}_ms"] = round(ms, 4)
            res[f"{name}_ms_rounds"] = [round(v, 4) for v in rounds]
            res[f"{name}_TB_per_s"] = round(moved / (ms / 1e3) / 1e12, 3)
            res[f"{name}_over_hbm_peak"] = round(moved / (ms / 1e3) / HBM_PEAK, 4)
            res[f"{name}_over_measured_copy"] = round(moved / (ms / 1e3) / HBM_COPY, 4)
            if want is not None:
                res[f"pillow_over_{name}"] = round(res["pillow_host_ms"] / ms, 1)
            if args.check:
                out.zero_()
                RZ.resize_u8(x, (out_side, out_side), out=out, _route=route)
                ref = host if want is None else np.stack(want)
                res[f"{name}_equal"] = bool(np.array_equal(out.cpu().numpy(), ref))
        results.append(res)
        print(json.dumps(res))
        del x, out, host
    # the whole heat-map call: ViTs included (synthetic weights: the time does not depend on them), bf16 as the benchmark runs them
    m = HIPT_4K(None, None, dev, dev)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(dev)
    m.set_compute_dtype("bf16")
    region = synth.hash_u8_np((4096, 4096, 3), 9)
    base = np.array(Image.fromarray(region).resize((1024, 1024)))
    region_d = torch.from_numpy(region).to(dev)
    forms = (("default", {}), ("host_resize", {"host_resize": True}), ("base_given", {"base": base}))

    def whole(**kw):
        res = HH.hierarchical_heatmaps(m, region_d, scale=4, **kw)
        torch.cuda.synchronize()
        return res
    pictures = {name: whole(**kw) for name, kw in forms}   # (the warm-up)
    per = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, kw in forms:
            t0 = time.perf_counter()
            whole(**kw)
            per[name].append(time.perf_counter() - t0)
    res = {"case": "hierarchical_heatmaps", "region": 4096, "scale": 4, "compute_dtype": "bf16",
           "clock": "host, each call ends in a synchronise"}
    for name, _ in forms:
        res[f"call_ms_{name}"] = round(statistics.median(per[name]) * 1e3, 2)
        res[f"call_ms_{name}_rounds"] = [round(v * 1e3, 2) for v in per[name]]
    if args.check:
        res["equal"] = all(bool(torch.equal(pictures["default"][k], pictures[name][k])) for name in ("host_resize", "base_given")
                           for k in pictures["default"])
    results.append(res)
    print(json.dumps(res))
    doc = {"tool": "tools/resize_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "protocol": "device events around `iters` calls per round, median of the rounds, two warm-up calls per shape; Pillow and the "
                       "whole heat-map call by a host clock (the latter around calls that end in a synchronise)",
           "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_measured_copy_bytes_per_s": HBM_COPY, "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
