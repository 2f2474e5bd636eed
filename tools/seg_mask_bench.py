"""The tissue mask from contours on the device: ``segment.seg_mask`` on the traced contours of the synthetic
tissue-like 4096 x 4096 mask of tools/contour_bench.py, drawn with holes on canvases at scale 1/32 (128 x 128) and 1/4 (1024 x
1024), against the sequential numpy restatement (tests/seg_mask_ref.py) on the same box, masks compared.  Two device figures:
the whole call with device tensors in (its read-back of the points for the draw order and the host's area sums included; host
clock, it synchronises), and the native launch alone with everything resident (device events around ``iters`` launches).  The
fraction of the HBM peak counts the bytes that must move once -- the points read, the mask written -- over the launch's time.
No time is promised: the figures are what was measured.

    python tools/seg_mask_bench.py --json profiles/seg_mask_bench.json
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
HBM_PEAK_GBS = 8000.0   # MI355X: 8 TB/s


def main():
    import torch

    import contour_ref as CR
    import seg_mask_ref as SM
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import segment as SG
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--sigma", type=float, default=24.0)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("seg_mask_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    side = args.side
    x = torch.from_numpy(CR.smooth_mask(side, side, seed=args.seed, sigma=args.sigma)).to(dev)
    traced = SG.trace_contours(x)
    pts, off, hier = (t.cpu().numpy() for t in traced)
    outer = np.flatnonzero(hier[:, 3] == -1)
    contours = [pts[off[k]:off[k + 1]].reshape(-1, 1, 2) for k in outer]
    holes = [[pts[off[j]:off[j + 1]].reshape(-1, 1, 2) for j in np.flatnonzero(hier[:, 3] == k)] for k in outer]
    results = []
    for down in (32, 4):
        size, scale = (side // down, side // down), [1.0 / down, 1.0 / down]
        res = {"side": side, "scale": f"1/{down}", "canvas": list(size), "contours": len(contours), "holes": int((hier[:, 3] >= 0).sum()),
               "points": int(pts.shape[0]), "use_holes": True, "iters": args.iters}
        got = SG.seg_mask(traced, None, size, scale, use_holes=True)
        t0 = time.perf_counter()
        want = SM.seg_mask_ref(contours, holes, size, scale, use_holes=True)
        res["numpy_restatement_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["masks_equal"] = bool(np.array_equal(got.cpu().numpy(), want))
        res["tissue_share"] = round(float(want.mean()), 4)
        per = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(3):
                SG.seg_mask(traced, None, size, scale, use_holes=True)
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) * 1e3 / 3)
        res["seg_mask_call_ms"], res["seg_mask_call_ms_rounds"] = round(statistics.median(per), 4), [round(v, 4) for v in per]
        seen = {}
        fill = SG._fill
        SG._fill = lambda *a: (seen.setdefault("args", a), fill(*a))    # the launch's resident operands, as seg_mask hands them over
        SG.seg_mask(traced, None, size, scale, use_holes=True)
        SG._fill = fill
        per = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.iters):
                fill(*seen["args"])
            stop.record()
            stop.synchronize()
            per.append(start.elapsed_time(stop) / args.iters)
        res["launch_ms"], res["launch_ms_rounds"] = round(statistics.median(per), 4), [round(v, 4) for v in per]
        moved = 8 * res["points"] + size[0] * size[1]
        res["bytes_that_must_move"] = moved
        res["hbm_peak_fraction"] = round(moved / (res["launch_ms"] * 1e-3) / (HBM_PEAK_GBS * 1e9), 6)
        bands = (size[1] + 3) // 4 * ((size[0] + N.FILL_MAX_COLS - 1) // N.FILL_MAX_COLS)
        res["workgroups"] = bands
        res["edge_visits"] = bands * res["points"]     # an upper bound: a workgroup skips a collection whose rows miss its band
        res["edge_visits_per_us"] = round(res["edge_visits"] / (res["launch_ms"] * 1e3), 1)
        res["bound_by"] = ("the edge walk: every workgroup (four canvas rows) visits every edge of every collection whose rows meet its band, "
                           "two vertex loads from L2 and four float64 products per visit; HBM traffic is negligible")
        res["speedup_over_numpy_restatement"] = round(res["numpy_restatement_ms"] / res["seg_mask_call_ms"], 1)
        print(json.dumps(res), flush=True)
        results.append(res)
    doc = {"tool": "tools/seg_mask_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "protocol": "seg_mask_call_ms: host clock around 3 whole calls (device tensors in, draw order computed: one read-back of the "
                       "points) between device synchronisations; launch_ms: device events around `iters` native launches with resident "
                       "operands; medians of the rounds after a warm-up call; the numpy restatement once by a host clock; "
                       "hbm_peak_fraction = (8 bytes per point + 1 byte per canvas pixel) / launch time / 8 TB/s",
           "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
