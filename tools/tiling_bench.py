"""Patch coordinates of one synthetic slide: the single ``tiling.process_contours`` call against the numpy restatement of the tests
(tests/tiling_ref.py), on the same box.

The slide: a 100 000 x 100 000 level 0 with 100 tissue contours, one per cell of a 10 x 10 lattice, each the 8-connected pixel chain
(CHAIN_APPROX_NONE keeps every boundary pixel) of a seeded blob whose size is drawn log-uniformly, with 0 to 8 holes; 256-pixel patches
at step 256, ``four_pt``.  The device call is timed from the host (wall time around the call, which ends in the read-back of the
flags: launch, copy and the compaction into coordinates included) with the polygons resident (``pack_slide``); the kernel alone is
timed with device events around ``return_flags=True`` calls.  Device and numpy rounds are interleaved -- device, numpy, device, numpy
... -- and each figure is the median over the rounds with the spread beside it.  The two coordinate sets must be equal.  One JSON
document goes to profiles/tiling_bench.json (or the path given).  python tools/tiling_bench.py [out.json] [rounds=3] [reps=5]"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tiling_ref as TR  # noqa: E402

from hipt_abmil_atec23_amd import tiling as T  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "tiling_bench.json")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5

LEVEL0, CELL, GRID = 100_000, 10_000, 10
KW = dict(patch_size=256, step_size=256, contour_fn="four_pt")


def make_slide(seed=0):
    rng = np.random.default_rng(seed)
    conts, holes = [], []
    for k in range(GRID * GRID):
        cx, cy = (k % GRID) * CELL + CELL // 2, (k // GRID) * CELL + CELL // 2
        target = float(np.exp(rng.uniform(np.log(1e2), np.log(5e4))))   # boundary pixels asked for
        r = min(max(target / 7.0, 14.0), 0.46 * CELL)                   # a blob's chain has about 7 r of them
        conts.append(TR.pixel_chain(TR.blob(1000 + k, cx, cy, r, max(12, int(r / 4)))))
        hs = []
        for j in range(int(rng.integers(0, 9)) if r > 200 else 0):
            a, d = rng.uniform(0, 2 * np.pi), rng.uniform(0.1, 0.6) * r
            hs.append(TR.pixel_chain(TR.blob(5000 + 10 * k + j, cx + d * np.cos(a), cy + d * np.sin(a), rng.uniform(0.03, 0.12) * r, 24)))
        holes.append(hs)
    return conts, holes


def stats(v, unit="ms"):
    return {f"median_{unit}": round(statistics.median(v), 3), f"min_{unit}": round(min(v), 3), f"max_{unit}": round(max(v), 3)}


if not torch.cuda.is_available():
    raise SystemExit("tiling_bench: no HIP device (a timing taken elsewhere says nothing about one)")
conts, holes = make_slide()
dim0, ds = (LEVEL0, LEVEL0), (1.0, 1.0)
packed = T.pack_slide(conts, holes)
plan = T.plan_contours(packed, None, dim0, ds, **KW)
n_verts = [len(c) for c in conts]
result = {"device": torch.cuda.get_device_name(0), "level0": [LEVEL0, LEVEL0], "contours": len(conts), "holes": sum(len(h) for h in holes),
          "holes_per_contour": [min(len(h) for h in holes), max(len(h) for h in holes)],
          "contour_vertices": [min(n_verts), max(n_verts)], "vertices": packed.n_verts, "candidates": int(plan.flags.numel()),
          "workgroups": plan.n_units, "settings": KW, "rounds": rounds, "device_reps_per_round": reps,
          "timing": "host wall time per call, interleaved rounds, median (min ... max); kernel: device events around the launch"}

per, dev_coords = T.process_contours(packed, None, dim0, ds, **KW)   # warm-up: code object, allocator
torch.cuda.synchronize()
dev_ms, kern_ms, np_ms, np_coords = [], [], [], None
for _ in range(rounds):
    t0 = time.perf_counter()
    for _ in range(reps):
        per, dev_coords = T.process_contours(packed, None, dim0, ds, **KW)
    dev_ms.append((time.perf_counter() - t0) * 1e3 / reps)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        plan.run()
    e1.record()
    torch.cuda.synchronize()
    kern_ms.append(e0.elapsed_time(e1) / reps)
    t0 = time.perf_counter()
    np_coords = np.concatenate([TR.process_contour(c, h, dim0, ds, **KW) for c, h in zip(conts, holes)])
    np_ms.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"device_ms": round(dev_ms[-1], 3), "kernel_ms": round(kern_ms[-1], 3), "numpy_ms": round(np_ms[-1], 1)}), flush=True)

equal = bool(dev_coords.dtype == np_coords.dtype and dev_coords.shape == np_coords.shape and np.array_equal(dev_coords, np_coords))
assert equal, "device and numpy coordinates differ"
edge_tests = sum(g[4] * g[5] * len(c) * 4 for g, c in zip(plan.grids, conts))
result.update(coordinates=int(len(dev_coords)), coordinates_equal=equal, contour_edge_tests=int(edge_tests),
              process_contours=stats(dev_ms), kernel=stats(kern_ms), numpy_restatement=stats(np_ms),
              speedup_of_medians=round(statistics.median(np_ms) / statistics.median(dev_ms), 1))
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
print(json.dumps(result))
