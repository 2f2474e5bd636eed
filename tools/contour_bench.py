"""Contour tracing on the device: ``segment.trace_contours`` on one resident synthetic tissue-like 4096 x 4096 mask
-- seeded noise, smoothed and thresholded: blobs with holes and islands (tests/contour_ref.py: smooth_mask) -- against the least
the host route can cost: reading the mask back, and ``scipy.ndimage.label`` of it (both connectivities, which a host tracer needs
before it follows a single border).  ``trace_contours`` synchronises (its one read-back), so it is timed by a host clock around
``iters`` calls after a device synchronisation, median of ``rounds`` rounds, warmed up first; the read-back likewise.  No time is
promised: the figures are what was measured, and ``slower_than_host_floor`` says plainly when the device call loses.

    python tools/contour_bench.py --json profiles/contour_bench.json
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


def main():
    import torch
    from scipy import ndimage

    import contour_ref as CR
    from hipt_abmil_atec23_amd import segment as SG
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=24.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("contour_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    side = args.side
    host = CR.smooth_mask(side, side, seed=args.seed, sigma=args.sigma)
    x = torch.from_numpy(host).to(dev)

    def timed(f):
        f()
        f()
        per = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.iters):
                f()
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3 / args.iters)
        return round(statistics.median(per), 4), [round(v, 4) for v in per]

    points, offsets, hier = SG.trace_contours(x)
    lengths = np.diff(offsets.cpu().numpy())
    res = {"side": side, "sigma": args.sigma, "seed": args.seed, "iters": args.iters, "foreground_share": round(float((host != 0).mean()), 4),
           "contours": int(hier.shape[0]), "holes": int((hier[:, 3] >= 0).sum()), "points": int(points.shape[0]),
           "longest_border": int(lengths.max()) if len(lengths) else 0}
    res["trace_contours_ms"], res["trace_contours_ms_rounds"] = timed(lambda: SG.trace_contours(x))
    res["mask_readback_ms"], res["mask_readback_ms_rounds"] = timed(lambda: x.cpu())
    t0 = time.perf_counter()
    fg = host != 0
    _, n_fg = ndimage.label(fg, structure=np.ones((3, 3), dtype=int))
    _, n_bg = ndimage.label(~np.pad(fg, 1))
    res["scipy_label_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res["components_agree"] = bool(n_fg + n_bg - 1 == res["contours"] and n_bg - 1 == res["holes"])
    res["host_floor_ms"] = round(res["mask_readback_ms"] + res["scipy_label_ms"], 1)
    res["slower_than_host_floor"] = bool(res["trace_contours_ms"] > res["host_floor_ms"])
    res["slower_than_mask_readback"] = bool(res["trace_contours_ms"] > res["mask_readback_ms"])
    print(json.dumps(res), flush=True)
    doc = {"tool": "tools/contour_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "protocol": "host clock around `iters` calls between device synchronisations (the call itself synchronises: one read-back), "
                       "median of the rounds, two warm-up calls; scipy.ndimage.label (8-connected foreground, 4-connected padded "
                       "background) once by a host clock; host_floor = mask read-back + scipy label, the least a host tracer costs",
           "results": [res]}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
