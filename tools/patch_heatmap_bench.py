"""Patch-level heat-maps on the device: P = 256 resident patches, six heads, with a threshold (both pictures).

Timed with device events around ``iters`` calls, median of ``rounds`` rounds, every shape warmed up first:
  compose      ``compose_patch_heatmaps`` (the rank launch + the render launch), pictures and the three-across mosaics
  ranks        the ``hipt_hier_ranks`` launch alone
  render       compose minus ranks: the render launch
  whole call   ``patch_heatmaps`` (the 2 P layers through ViT-256 in bf16, the ranks and the pictures), with a host clock around
               calls that end in a device synchronise
  host         the numpy restatement (tests/patch_heatmap_ref.py: upscale, scipy's rankdata, slices, matplotlib, the blend) for
               ``--host-patches`` patches on the same box, interleaved with the device rounds; it has no ViT in it
The render kernel's figure of merit is the bytes it must write (2 * nh * 196 608 per patch) per second, against the HBM peak
(8.0 TB/s specified; MI355X_MICROARCH: 6.29 TB/s measured for a copy).  Attention maps are seeded random numbers: the kernels'
time does not depend on the values.  The pictures of the host patches are compared with the restatement's.

    python tools/patch_heatmap_bench.py --json profiles/patch_heatmap_bench.json
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
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12       # bytes / s, specified
HBM_COPY = 6.29e12      # bytes / s, measured for a float4 copy (MI355X_MICROARCH)


def event_ms(fn, iters):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    import matplotlib
    import patch_heatmap_ref as PR
    import torch

    from hipt_abmil_atec23_amd import HIPT_4K, synth
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--patches", type=int, default=256)
    ap.add_argument("--host-patches", type=int, default=2)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("patch_heatmap_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    p, nh, thr = args.patches, 6, 0.5
    rng = np.random.default_rng(0)
    a256_h = rng.random((p, 2, nh, 256), dtype=np.float32)
    patches_h = rng.integers(0, 256, (p, 256, 256, 3), dtype=np.uint8)
    a256, patches = torch.from_numpy(a256_h).to(dev), torch.from_numpy(patches_h).to(dev)
    out = {k: torch.empty((p, nh, 256, 256, 3), dtype=torch.uint8, device=dev) for k in ("256", "256th")}
    out_m = {k: torch.empty((p, 512, 768, 3), dtype=torch.uint8, device=dev) for k in ("256", "256th")}

    m = HIPT_4K(None, None, dev, dev)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m = m.eval().to(dev)
    m.set_compute_dtype("bf16")

    def compose():
        PH.compose_patch_heatmaps(a256, patches, threshold=thr, out=out)

    def compose_mosaic():
        PH.compose_patch_heatmaps(a256, patches, threshold=thr, concat=True, cols=3, out=out_m)

    def ranks():
        HH.hier_ranks(a256, 16)

    def whole():
        t0 = time.perf_counter()
        PH.patch_heatmaps(m.model256, patches, threshold=thr)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def host():
        cmap = matplotlib.colormaps["coolwarm"]
        t0 = time.perf_counter()
        want = [PR.pictures(a256_h[i], patches_h[i], cmap=cmap, threshold=thr) for i in range(args.host_patches)]
        return (time.perf_counter() - t0) * 1e3 / args.host_patches, want

    for fn in (compose, compose_mosaic, ranks, whole):   # warm-up: every shape twice
        fn(), fn()
    torch.cuda.synchronize()
    per = {k: [] for k in ("compose", "mosaic", "ranks", "whole", "host")}
    want = None
    for _ in range(args.rounds):   # interleaved: every round measures every leg
        per["compose"].append(event_ms(compose, args.iters))
        per["mosaic"].append(event_ms(compose_mosaic, args.iters))
        per["ranks"].append(event_ms(ranks, args.iters))
        per["whole"].append(whole())
        ms, want = host()
        per["host"].append(ms)
    med = {k: statistics.median(v) for k, v in per.items()}
    compose()
    torch.cuda.synchronize()
    equal = all(bool(np.array_equal(out[k][i].cpu().numpy(), want[i][k])) for k in out for i in range(args.host_patches))
    written = 2 * nh * 256 * 256 * 3 * p
    render_s = (med["compose"] - med["ranks"]) / 1e3
    res = {"case": "compose_patch_heatmaps", "patches": p, "heads": nh, "threshold": thr, "iters": args.iters,
           "compose_ms": round(med["compose"], 4), "compose_ms_rounds": [round(x, 4) for x in per["compose"]],
           "compose_mosaic_ms": round(med["mosaic"], 4), "compose_mosaic_ms_rounds": [round(x, 4) for x in per["mosaic"]],
           "ranks_ms": round(med["ranks"], 4), "ranks_ms_rounds": [round(x, 4) for x in per["ranks"]],
           "render_ms": round(med["compose"] - med["ranks"], 4), "bytes_written": written,
           "render_written_TB_per_s": round(written / render_s / 1e12, 3),
           "render_written_over_hbm_peak": round(written / render_s / HBM_PEAK, 3),
           "render_written_over_measured_copy": round(written / render_s / HBM_COPY, 3),
           "bound": "bytes written over the HBM peak (the patches read are 1 / 12 of them; the ranks and the table are L2-sized; the "
                    "float64 and blend arithmetic is not counted)",
           "whole_call_ms": round(med["whole"], 2), "whole_call_ms_rounds": [round(x, 2) for x in per["whole"]],
           "whole_call_compute_dtype": "bf16", "whole_call_clock": "host, each call ends in a synchronise",
           "host_restatement_ms_per_patch": round(med["host"], 2), "host_restatement_ms_per_patch_rounds": [round(x, 2) for x in per["host"]],
           "host_patches": args.host_patches, "host_restatement_has_no_vit": True,
           "compose_ms_per_patch": round(med["compose"] / p, 5),
           "host_over_device_per_patch": round(med["host"] / (med["compose"] / p), 1), "equal": equal}
    print(json.dumps(res))
    doc = {"tool": "tools/patch_heatmap_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "protocol": "interleaved rounds; device events around `iters` calls per leg and round, median of the rounds, two warm-up calls "
                       "per shape; the whole call and the host restatement by a host clock",
           "hbm_peak_bytes_per_s": HBM_PEAK, "hbm_measured_copy_bytes_per_s": HBM_COPY, "results": [res]}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not equal:
        raise SystemExit("patch_heatmap_bench: the device pictures differ from the restatement's")


if __name__ == "__main__":
    main()
