"""CLAM_SB narrow heads over 64 resident bags: ONE ``forward_bags`` call with ``bags_narrow`` set (csrc/abmil_narrow.hip) against the loop
of per-bag ``forward`` calls (the generic path: six launches per bag).

Bag sets: 15 ... 75 rows (the region counts of the reference's HIPT-ABMIL slides) and 50 ... 400 rows (the set of
tools/clam_bags_bench.py).  Heads: [192, 16, 8] (hipt_smaller) and [1024, 32, 8], bf16 and fp32.  The method is that tool's: both forms
are timed from the host (wall time around a synchronised batch of repetitions), in interleaved rounds on one box, and each figure is
the median over the rounds with the spread (min ... max) beside it.  Last, without a bar: one 100 000-row x 192 bag through B = 1, with
the bytes the call must move (the bag once, A_raw once) over its time.  One JSON document is written to
profiles/clam_narrow_bags_bench.json (or the path given).  python tools/clam_narrow_bags_bench.py [out.json] [rounds=15] [reps=20]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hipt_abmil_atec23_amd import CLAM_SB, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clam_narrow_bags_bench.json")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = "cuda:0"
B = 64
# ragged row counts from the hash generator (no RNG state): the same on every box
draw = (synth.hash_uniform_torch((B,), 77).abs() * 1e6).long()
ROW_SETS = {"15..75": [15 + int(v) for v in draw % 61], "50..400": [50 + int(v) for v in draw % 351]}


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
    m = CLAM_SB(size_arg=list(size))
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size), size[0]))
    m.relocate()
    return m.eval().set_compute_dtype(dtype)


result = {"device": torch.cuda.get_device_name(0), "bags": B, "row_sets": ROW_SETS, "rounds": rounds, "reps_per_round": reps,
          "timing": "host wall time per call, synchronised batches, interleaved rounds, median (min ... max)", "cases": []}
for set_name, rows in ROW_SETS.items():
    for size in ((192, 16, 8), (1024, 32, 8)):
        for dtype in ("bf16", "fp32"):
            m = model(size, dtype)
            cat = synth.hash_uniform_torch((sum(rows), size[0]), 78, device=dev)
            if dtype == "bf16":
                cat = cat.bfloat16()
            bags = list(cat.split(rows, dim=0))
            m.bags_narrow = True
            with torch.no_grad():
                one = lambda: m.forward_bags(bags)           # torch.cat + one native call
                loop = lambda: [m(b) for b in bags]          # 64 native calls, six launches each
                for _ in range(3):
                    one(), loop()
                assert m.bags_route == "bags"
                t_one, t_loop = [], []
                for _ in range(rounds):
                    t_one.append(timed(one, reps))
                    t_loop.append(timed(loop, reps))
            case = {"rows": set_name, "total_rows": sum(rows), "size": list(size), "dtype": dtype, "route": m.bags_route,
                    "forward_bags": stats(t_one), "per_bag_loop": stats(t_loop)}
            case["speedup_of_medians"] = round(case["per_bag_loop"]["median_us"] / case["forward_bags"]["median_us"], 2)
            case["separated"] = case["forward_bags"]["max_us"] < case["per_bag_loop"]["min_us"]   # slowest one call < fastest loop
            result["cases"].append(case)
            print(json.dumps(case), flush=True)

# one long bag through B = 1: the bag is read once, A_raw written once (weights and partials are noise beside them)
result["long_bag"] = []
n_long = 100_000
for dtype in ("bf16", "fp32"):
    m = model((192, 16, 8), dtype)
    m.bags_narrow = True
    x = synth.hash_uniform_torch((n_long, 192), 79, device=dev)
    if dtype == "bf16":
        x = x.bfloat16()
    with torch.no_grad():
        one = lambda: m.forward_bags((x, [0, n_long]))
        for _ in range(3):
            one()
        assert m.bags_route == "bags"
        t = [timed(one, reps) for _ in range(rounds)]
    nbytes = n_long * 192 * x.element_size() + n_long * 4
    s = stats(t)
    case = {"rows": n_long, "size": [192, 16, 8], "dtype": dtype, "forward_bags": s, "bytes_moved": nbytes,
            "GBps_at_median": round(nbytes / s["median_us"] / 1e3, 1),
            "note": "host wall time of the whole call (offset check and upload, three launches); HBM peak fraction = GBps / the box's peak"}
    result["long_bag"].append(case)
    print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
