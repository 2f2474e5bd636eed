"""Tissue segmentation mask on the device: the whole ``tissue_mask`` call and each stage on one resident
4096 x 4096 x 4 image (a segmentation-level picture as ``read_region`` returns it), for two of the reference's presets:

  tcga        mthresh 7, close 4, fixed threshold
  betterseg   mthresh 5, close 100, Otsu
The image is the tests' fixture maker's (tests/segment_ref.py: make_image).  Timed with device events around ``iters`` calls, the
whole call and the stages interleaved within a round, median of ``rounds`` rounds, every function warmed up first.  Bytes moved are
what the launches read and write by design (the source once, one plane written by the median kernel, one plane read and one written
per closing pass), over the time, against the 8.0 TB/s the project quotes for HBM; a share far below one means the kernels are
bound by instruction issue (vector ALU and LDS), not by HBM.  The host figure is the same stages from numpy and scipy.ndimage
(median_filter, maximum_filter, minimum_filter -- the filters the host tests show equal to the restatement) in the same process,
one call by a host clock; its mask must equal the device's.

    python tools/segment_bench.py --json profiles/segment_bench.json
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
PRESETS = {"tcga": (7, 4, False), "betterseg": (5, 100, True)}


def host_mask(img, sthresh, mthresh, close, use_otsu):
    import segment_ref as SR
    from scipy import ndimage
    med = ndimage.median_filter(SR.saturation(img), size=mthresh, mode="nearest")
    t = SR.otsu(SR.histogram(med)) if use_otsu else sthresh
    m = SR.threshold(med, t, 255)
    if close:
        m = ndimage.maximum_filter(m, size=(close, close), mode="constant", cval=0)
        m = ndimage.minimum_filter(m, size=(close, close), mode="constant", cval=255)
    return m


def main():
    import torch

    import segment_ref as SR
    from hipt_abmil_atec23_amd import segment as SG
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_bench: no HIP device (nothing is measured without one)")
    dev = torch.device("cuda:0")
    side = args.side
    tile = SR.make_image(1024, 1024, 4, seed=5)
    host = np.ascontiguousarray(np.tile(tile, (side // 1024 + 1, side // 1024 + 1, 1))[:side, :side])
    x = torch.from_numpy(host).to(dev)
    n = side * side
    results = []
    for name, (m, c, o) in PRESETS.items():
        out = torch.empty((side, side), dtype=torch.uint8, device=dev)
        tmp = torch.empty_like(out)
        mask, med, sat, thr = SG.tissue_mask(x, 20, 255, m, c, o, return_parts=True)
        binary = SG.tissue_mask(x, 20, 255, m, 0, o)
        passes = 4 if c else 1
        fns = {"tissue_mask": lambda: SG.tissue_mask(x, 20, 255, m, c, o, out=out),
               "saturation": lambda: SG.saturation_u8(x, out=tmp),
               "median": lambda: SG.median_blur_u8(sat, m, out=tmp),
               "otsu": lambda: SG.otsu_threshold(med),
               "close": lambda: SG.morph_close_u8(binary, c, out=tmp)}
        moved = {"tissue_mask": 4 * n + n + passes * 2 * n, "saturation": 4 * n + n, "median": 2 * n, "otsu": n, "close": 4 * 2 * n}
        for f in fns.values():
            f()
            f()
        torch.cuda.synchronize()
        per = {k: [] for k in fns}
        for _ in range(args.rounds):
            for k, f in fns.items():   # interleaved: every round times all of them
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    f()
                b.record()
                b.synchronize()
                per[k].append(a.elapsed_time(b) / args.iters)
        res = {"preset": name, "side": side, "channels": 4, "mthresh": m, "close": c, "use_otsu": o, "iters": args.iters,
               "threshold": int(thr.cpu()[0]), "foreground_share": round(float((mask != 0).float().mean()), 4)}
        for k in fns:
            ms = statistics.median(per[k])
            res[f"{k}_ms"] = round(ms, 4)
            res[f"{k}_ms_rounds"] = [round(v, 4) for v in per[k]]
            res[f"{k}_bytes_moved"] = moved[k]
            share = moved[k] / (ms / 1e3) / HBM_PEAK
            res[f"{k}_over_hbm_peak"] = round(share, 4)
            res[f"{k}_bound"] = "HBM" if share > 0.5 else "instruction issue (vector ALU / LDS), not HBM"
        t0 = time.perf_counter()
        want = host_mask(host, 20, m, c, o)
        res["numpy_scipy_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        res["numpy_scipy_over_device"] = round(res["numpy_scipy_ms"] / res["tissue_mask_ms"], 1)
        res["mask_equals_host"] = bool(np.array_equal(out.cpu().numpy(), want))
        results.append(res)
        print(json.dumps(res), flush=True)
    doc = {"tool": "tools/segment_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds,
           "protocol": "device events around `iters` calls, the whole call and the stages interleaved within a round, median of the rounds, "
                       "two warm-up calls each; numpy / scipy.ndimage once by a host clock",
           "hbm_peak_bytes_per_s": HBM_PEAK, "results": results}
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
