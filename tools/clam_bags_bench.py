"""CLAM_SB over 64 resident bags of 50 ... 400 rows: ONE ``forward_bags`` call against the loop of per-bag ``forward`` calls.

Four cases (x 384 and x 192 features, [S0, 128, 64]; bf16 and fp32).  Both forms are timed from the host (wall time around a
synchronised batch of repetitions: the loop's cost IS its launches and host work), in interleaved rounds on one box -- bags, loop,
bags, loop ... -- and each figure is the median over the rounds, with the spread (min ... max) beside it.  One JSON document is
written to profiles/clam_bags_bench.json (or the path given).  python tools/clam_bags_bench.py [out.json] [rounds=15] [reps=20]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hipt_abmil_atec23_amd import CLAM_SB, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clam_bags_bench.json")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = "cuda:0"
B = 64
# ragged row counts in 50 ... 400 from the hash generator (no RNG state): the same on every box
rows = [50 + int(v) for v in (synth.hash_uniform_torch((B,), 77).abs() * 1e6).long() % 351]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def stats(v):
    return {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)}


result = {"device": torch.cuda.get_device_name(0), "bags": B, "rows": rows, "total_rows": sum(rows), "rounds": rounds, "reps_per_round": reps,
          "timing": "host wall time per call, synchronised batches, interleaved rounds, median (min ... max)", "cases": []}
for s0 in (384, 192):
    size = (s0, 128, 64)
    for dtype in ("bf16", "fp32"):
        m = CLAM_SB(size_arg=list(size))
        m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size), s0))
        m.relocate()
        m = m.eval().set_compute_dtype(dtype)
        cat = synth.hash_uniform_torch((sum(rows), s0), 78, device=dev)
        if dtype == "bf16":
            cat = cat.bfloat16()
        bags = list(cat.split(rows, dim=0))
        with torch.no_grad():
            one = lambda: m.forward_bags(bags)           # torch.cat + one native call
            loop = lambda: [m(b) for b in bags]          # 64 native calls
            for _ in range(3):
                one(), loop()
            assert m.bags_route in ("bags", "per_bag")
            t_one, t_loop = [], []
            for _ in range(rounds):
                t_one.append(timed(one))
                t_loop.append(timed(loop))
        case = {"size": list(size), "dtype": dtype, "route": m.bags_route, "forward_bags": stats(t_one), "per_bag_loop": stats(t_loop)}
        case["speedup_of_medians"] = round(case["per_bag_loop"]["median_us"] / case["forward_bags"]["median_us"], 2)
        case["separated"] = case["forward_bags"]["max_us"] < case["per_bag_loop"]["min_us"]   # beyond the run-to-run spread of the two
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
