"""CLAM_MB wide heads over 64 resident bags: ONE ``forward_bags`` call with ``bags_one_call`` and ``bags_wide`` set
(csrc/abmil_wide_mb.hip) against the loop of per-bag ``forward`` calls (per bag: the K branches through the per-bag kernels).

Bag sets: 50 ... 400 rows and 500 ... 4000 rows (the sets of tools/clam_wide_bags_bench.py).  Heads: [1024, 512, 256] (small, what
``CLAM_MB()`` is built with) and [1024, 256, 64] (tiny), bf16 and fp32, K = 2 classes.  The method is that tool's: both forms are timed
from the host (wall time around a synchronised batch of repetitions), in interleaved rounds on one box, and each figure is the median
over the rounds with the spread (min ... max) beside it.  One JSON document is written to profiles/clam_wide_mb_bags_bench.json (or the
path given).
python tools/clam_wide_mb_bags_bench.py [out.json] [rounds=9] [reps=5]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hipt_abmil_atec23_amd import CLAM_MB, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clam_wide_mb_bags_bench.json")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = "cuda:0"
B, K = 64, 2
# ragged row counts from the hash generator (no RNG state): the same on every box
draw = (synth.hash_uniform_torch((B,), 77).abs() * 1e6).long()
ROW_SETS = {"50..400": [50 + int(v) for v in draw % 351], "500..4000": [500 + int(v) for v in draw % 3501]}


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def stats(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


def model(size, dtype):
    m = CLAM_MB(size_arg=list(size), n_classes=K)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=K, multi=True), size[0]))
    m.relocate()
    return m.eval().set_compute_dtype(dtype)


result = {"device": torch.cuda.get_device_name(0), "bags": B, "branches": K, "row_sets": ROW_SETS, "rounds": rounds, "reps_per_round": reps,
          "timing": "host wall time per call, synchronised batches, interleaved rounds, median (min ... max)", "cases": []}
for set_name, rows in ROW_SETS.items():
    for size in ((1024, 512, 256), (1024, 256, 64)):
        for dtype in ("bf16", "fp32"):
            m = model(size, dtype)
            cat = synth.hash_uniform_torch((sum(rows), size[0]), 78, device=dev)
            if dtype == "bf16":
                cat = cat.bfloat16()
            bags = list(cat.split(rows, dim=0))
            m.bags_one_call = m.bags_wide = True
            with torch.no_grad():
                one = lambda: m.forward_bags(bags)           # torch.cat + one native call
                loop = lambda: [m(b) for b in bags]          # 64 forward calls
                for _ in range(2):
                    one(), loop()
                assert m.bags_route == "bags"
                t_one, t_loop = [], []
                for _ in range(rounds):
                    t_one.append(timed(one, reps))
                    t_loop.append(timed(loop, reps))
            flops = 2.0 * sum(rows) * size[1] * (size[0] + 2 * size[2])
            case = {"rows": set_name, "total_rows": sum(rows), "size": list(size), "dtype": dtype, "branches": K, "route": m.bags_route,
                    "forward_bags": stats(t_one), "per_bag_loop": stats(t_loop), "gemm_flops": flops}
            case["speedup_of_medians"] = round(case["per_bag_loop"]["median_us"] / case["forward_bags"]["median_us"], 2)
            case["one_call_faster"] = case["forward_bags"]["median_us"] < case["per_bag_loop"]["median_us"]
            case["separated"] = case["forward_bags"]["max_us"] < case["per_bag_loop"]["min_us"]   # slowest one call < fastest loop
            case["gemm_TFLOPs_at_median"] = round(flops / case["forward_bags"]["median_us"] / 1e6, 2)
            result["cases"].append(case)
            print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
