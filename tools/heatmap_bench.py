"""Heat-map rasteriser: ``render_heatmap`` on the device against the numpy restatement (tests/heatmap_ref.py: the reference's
two Python loops) on the same box's CPU.

Two cases, both N = 100 000 patches of 256 x 256 level-0 pixels on a 317-wide grid at 50 % overlap (stride 128):
  ds32   drawn at a 32x downsample: patches of 8 x 8 canvas pixels at stride 4, canvas 1272 x 1268
  ds4    drawn at a 4x downsample: patches of 64 x 64 canvas pixels at stride 32, canvas 10176 x 10144
with a random uint8 canvas, a tissue mask with a hole and alpha = 0.4, everything the call reads and writes resident on the
device (tensors in, tensor out).

  device_ms     one ``render_heatmap`` call (its few elementwise torch launches, the memset and the six kernels), HIP events
                around ``--iters`` back-to-back calls after ``--warmup`` calls, median of ``--repeats`` such windows
  bytes         what the algorithm has to move: xy, value and paint flag per patch, canvas and mask in, image out
  gbytes_per_s  bytes / device_ms, and its share of the 8 TB/s HBM3E peak (an end-to-end figure of the whole call, not one
                kernel's)
  numpy_s       the restatement, one run, wall clock (``--no-ref`` skips it and the comparison)
  equal         the device image equals the restatement's, byte for byte

    python tools/heatmap_bench.py [--cases ds32,ds4] [--out profiles/heatmap_bench.json]
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

import heatmap_ref as R  # noqa: E402

HBM_PEAK = 8.0e12
N_PATCHES, GRID_W, PATCH, STRIDE = 100000, 317, 256, 128
CASES = {"ds32": 32, "ds4": 4}


def make_case(downsample, seed=0):
    rng = np.random.default_rng(seed)
    idx = np.arange(N_PATCHES)
    coords = np.stack([idx % GRID_W, idx // GRID_W], axis=1) * STRIDE
    coords = coords[rng.permutation(N_PATCHES)]
    scores = rng.uniform(0, 100, N_PATCHES)
    w, h = ((coords[:, k].max() + PATCH) // downsample for k in (0, 1))
    mask = np.ones((h, w), dtype=bool)
    mask[h // 3:h // 2, w // 3:w // 2] = False
    canvas = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    return scores, coords, (int(w), int(h)), mask, canvas


def run_case(name, downsample, args):
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords, (w, h), mask, canvas = make_case(downsample)
    scale = 1.0 / downsample
    dev = torch.device("cuda")
    t = [torch.from_numpy(a).to(dev) for a in (scores, coords, mask, canvas)]
    kw = dict(alpha=0.4, mask=t[2], canvas=t[3])
    for _ in range(args.warmup):
        out = H.render_heatmap(t[0], t[1], PATCH, scale, (w, h), **kw)
    torch.cuda.synchronize()
    windows = []
    for _ in range(args.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            out = H.render_heatmap(t[0], t[1], PATCH, scale, (w, h), **kw)
        e1.record()
        e1.synchronize()
        windows.append(e0.elapsed_time(e1) / args.iters)
    ms = statistics.median(windows)
    nbytes = N_PATCHES * (8 + 8 + 1) + w * h * (3 + 1 + 3)
    res = {"case": name, "downsample": downsample, "n_patches": N_PATCHES, "patch_px": int(np.ceil(PATCH * scale)), "canvas": [w, h],
           "device_ms": round(ms, 4), "device_ms_windows": [round(x, 4) for x in windows], "iters": args.iters, "bytes": nbytes,
           "gbytes_per_s": round(nbytes / ms / 1e6, 1), "share_of_hbm_peak": round(nbytes / (ms * 1e-3) / HBM_PEAK, 4)}
    if not args.no_ref:
        print(f"[{name}] numpy restatement on the CPU ...", flush=True)
        t0 = time.perf_counter()
        want = R.render(scores, coords, PATCH, scale, (w, h), canvas=canvas, mask=mask, alpha=0.4)
        res["numpy_s"] = round(time.perf_counter() - t0, 3)
        res["equal"] = bool(np.array_equal(out.cpu().numpy(), want))
        res["speedup"] = round(res["numpy_s"] * 1e3 / ms, 1)
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="ds32,ds4")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("heatmap_bench: no HIP device (there is no CPU path to time)")
    results = [run_case(name, CASES[name], args) for name in args.cases.split(",")]
    doc = {"tool": "tools/heatmap_bench.py", "device": torch.cuda.get_device_name(0), "hbm_peak_bytes_per_s": HBM_PEAK, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
