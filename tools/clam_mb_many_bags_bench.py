"""CLAM_MB with five classes over 64 resident bags: ONE ``forward_bags`` call with ``bags_one_call`` and ``bags_many`` set
(csrc/abmil_bags_mb8.hip) against the loop of per-bag ``forward`` calls (per bag: the K branches through the per-bag kernels, the
route these models take without the switches).

Workloads: 15 ... 75 rows x 192 at ``hipt_big`` [192, 128, 64] and 50 ... 400 rows x 1024 at ``tiny128`` [1024, 128, 32], bf16 and
fp32, K = 5 classes (the reference's ovarian_5class).  The method is that of tools/clam_wide_mb_bags_bench.py: both forms are timed from
the host (wall time around a synchronised batch of repetitions), in interleaved rounds on one box, and each figure is the median over
the rounds with the spread (min ... max) beside it.  ``input_GBps_at_median`` is the bags' bytes (read once) over the one call's median
host time: an achieved rate for the whole call, launches and the concatenation included, not a kernel time.  One JSON document is written
to profiles/clam_mb_many_bags_bench.json (or the path given).
python tools/clam_mb_many_bags_bench.py [out.json] [rounds=9] [reps=5]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hipt_abmil_atec23_amd import CLAM_MB, synth  # noqa: E402
from hipt_abmil_atec23_amd.model_clam import SIZE_DICT  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "clam_mb_many_bags_bench.json")
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 9
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dev = "cuda:0"
B, K = 64, 5
HBM_PEAK_GBPS = 8000.0   # MI355X datasheet
# ragged row counts from the hash generator (no RNG state): the same on every box
draw = (synth.hash_uniform_torch((B,), 77).abs() * 1e6).long()
WORKLOADS = (("hipt_big", "15..75", [15 + int(v) for v in draw % 61]), ("tiny128", "50..400", [50 + int(v) for v in draw % 351]))


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


result = {"device": torch.cuda.get_device_name(0), "bags": B, "branches": K, "row_sets": {w[0]: w[2] for w in WORKLOADS}, "rounds": rounds,
          "reps_per_round": reps, "timing": "host wall time per call, synchronised batches, interleaved rounds, median (min ... max)",
          "hbm_peak_GBps": HBM_PEAK_GBPS, "cases": []}
for name, set_name, rows in WORKLOADS:
    size = tuple(SIZE_DICT[name])
    for dtype in ("bf16", "fp32"):
        m = model(size, dtype)
        cat = synth.hash_uniform_torch((sum(rows), size[0]), 78, device=dev)
        if dtype == "bf16":
            cat = cat.bfloat16()
        bags = list(cat.split(rows, dim=0))
        with torch.no_grad():
            loop = lambda: [m(b) for b in bags]          # 64 forward calls, K branches each

            def one():                                   # torch.cat + one native call
                m.bags_one_call = m.bags_many = True
                try:
                    return m.forward_bags(bags)
                finally:
                    del m.bags_one_call, m.bags_many
            for _ in range(2):
                one(), loop()
            assert m.bags_route == "bags"
            t_one, t_loop = [], []
            for _ in range(rounds):
                t_one.append(timed(one, reps))
                t_loop.append(timed(loop, reps))
        flops = 2.0 * sum(rows) * size[1] * (size[0] + 2 * size[2])
        nbytes = sum(rows) * size[0] * cat.element_size()
        case = {"head": name, "rows": set_name, "total_rows": sum(rows), "size": list(size), "dtype": dtype, "branches": K, "route": m.bags_route,
                "forward_bags": stats(t_one), "per_bag_loop": stats(t_loop), "gemm_flops": flops, "input_bytes": nbytes}
        case["speedup_of_medians"] = round(case["per_bag_loop"]["median_us"] / case["forward_bags"]["median_us"], 2)
        case["one_call_faster"] = case["forward_bags"]["median_us"] < case["per_bag_loop"]["median_us"]
        case["separated"] = case["forward_bags"]["max_us"] < case["per_bag_loop"]["min_us"]   # slowest one call < fastest loop
        case["gemm_TFLOPs_at_median"] = round(flops / case["forward_bags"]["median_us"] / 1e6, 3)
        case["input_GBps_at_median"] = round(nbytes / case["forward_bags"]["median_us"] / 1e3, 2)
        case["fraction_of_hbm_peak"] = round(case["input_GBps_at_median"] / HBM_PEAK_GBPS, 5)
        result["cases"].append(case)
        print(json.dumps(case), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(result, f, indent=1)
    f.write("\n")
