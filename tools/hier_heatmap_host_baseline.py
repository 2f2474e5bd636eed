"""The host route the device pictures replace: the numpy restatement of the reference's loops
(tests/hier_heatmap_ref.py: np.repeat, scipy's rankdata per patch and per map, slicing, matplotlib, the blend) for one
4096 x 4096 region at scale 4, all 48 pictures, run ONCE with a wall clock.  Opens no GPU; takes seconds to minutes.

    python tools/hier_heatmap_host_baseline.py --json hier_heatmap_host_baseline.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import matplotlib

    import hier_heatmap_ref as HR
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--scale", type=int, default=4)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    g, nh = args.side // 256, 6
    rng = np.random.default_rng(0)
    a256 = rng.random((4, g * g, nh, 256), dtype=np.float32)
    a4k = rng.random((4, nh, g * g), dtype=np.float32)
    side = args.side // args.scale
    base = rng.integers(0, 256, (side, side, 3), dtype=np.uint8)
    t0 = time.perf_counter()
    out = HR.pictures(a256, a4k, g, g, base, scale=args.scale, cmap=matplotlib.colormaps["coolwarm"])
    wall = time.perf_counter() - t0
    doc = {"tool": "tools/hier_heatmap_host_baseline.py", "region": args.side, "scale": args.scale,
           "pictures": int(sum(out[k].shape[0] for k in ("4k", "256", "blend"))), "runs": 1, "wall_s": round(wall, 2),
           "cpus": os.cpu_count()}
    print(json.dumps(doc))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
