"""Times MIL_fc / MIL_fc_mc (csrc/mil.hip) against the same module's PyTorch-op sequence on the same device and writes
profiles/mil_bench.json.

  one bag    a resident 100 000 x 1024 bag, fp32 and bf16, MIL_fc and MIL_fc_mc (C = 3): ``forward`` (native) vs ``_torch_forward``
  many bags  64 bags of 500 .. 4000 rows: ``forward_bags`` (one native call) vs the loop of ``forward`` calls vs the loop of ``_torch_forward``

The legs alternate inside every round (interleaved: drift hits all alike); per leg the median over the rounds of the host wall time of
one synchronised call and of the HIP-event time around it.  Bounds quoted beside the times: 2 N S0 S1 flop = 105 GFLOP per 100 000-row
bag on the matrix pipe, and the bag's bytes (205 MB in bf16, 410 MB in fp32) at 5.7 TB/s.  The PyTorch legs run in the module's own
dtype (fp32 weights; the bag as given).

    python tools/mil_bench.py [--rounds 7] [--rows 100000] [--out profiles/mil_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from hipt_abmil_atec23_amd import MIL_fc, MIL_fc_mc, synth  # noqa: E402

PEAK_BF16_TFLOPS, PEAK_F32_TFLOPS, HBM_TBS = 2500.0, 157.3, 5.7   # MI355X data sheet: dense bf16 MFMA, fp32 matrix, HBM3E


def timed(fn, dev):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize(dev)
    return (time.perf_counter() - t0) * 1e3, a.elapsed_time(b)


def interleaved(legs, rounds, dev):
    for fn in legs.values():   # warm-up: weight images, workspaces, kernel setup
        fn()
    got = {k: [] for k in legs}
    for _ in range(rounds):
        for k, fn in legs.items():
            got[k].append(timed(fn, dev))
    return {k: {"wall_ms_median": statistics.median(w for w, _ in v), "event_ms_median": statistics.median(e for _, e in v),
                "event_ms_min": min(e for _, e in v), "rounds": len(v)} for k, v in got.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--rows", type=int, default=100000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mil_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S0, S1 = 1024, 512
    result = {"device": torch.cuda.get_device_name(dev), "rows": args.rows, "sizes": [S0, S1], "rounds": args.rounds, "one_bag": {}, "many_bags": {}}
    bag32 = synth.hash_uniform_torch((args.rows, S0), 11, device=dev)
    sizes = [500 + (3500 * ((i * 37) % 64)) // 63 for i in range(64)]
    bags32 = [synth.hash_uniform_torch((n, S0), 100 + i, device=dev) for i, n in enumerate(sizes)]
    flop = 2.0 * args.rows * S0 * S1
    with torch.no_grad():
        for name, make in (("MIL_fc", lambda: MIL_fc()), ("MIL_fc_mc_3", lambda: MIL_fc_mc(n_classes=3))):
            for dtype in ("bf16", "fp32"):
                m = make().to(dev).eval().set_compute_dtype(dtype)
                td = torch.bfloat16 if dtype == "bf16" else torch.float32
                bag, bags = bag32.to(td), [b.to(td) for b in bags32]
                r = interleaved({"native": lambda: m(bag), "torch_ops": lambda: m._torch_forward(bag32, False)}, args.rounds, dev)
                t = r["native"]["event_ms_median"] * 1e-3
                peak = PEAK_BF16_TFLOPS if dtype == "bf16" else PEAK_F32_TFLOPS
                r["bounds"] = {"gflop": flop / 1e9, "tflops_reached": flop / t / 1e12, "fraction_of_matrix_peak": flop / t / 1e12 / peak,
                               "hbm_mb": bag.numel() * bag.element_size() / 1e6, "hbm_bound_us": bag.numel() * bag.element_size() / (HBM_TBS * 1e12) * 1e6,
                               "fraction_of_hbm_bound": bag.numel() * bag.element_size() / (HBM_TBS * 1e12) / t}
                result["one_bag"][f"{name}_{dtype}"] = r
                result["many_bags"][f"{name}_{dtype}"] = dict(interleaved(
                    {"forward_bags": lambda: m.forward_bags(bags), "loop_forward": lambda: [m(b) for b in bags],
                     "loop_torch_ops": lambda: [m._torch_forward(b, False) for b in bags32]}, args.rounds, dev), rows_total=sum(sizes), bags=len(sizes))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: {c: {l: round(v["event_ms_median"], 4) for l, v in legs.items() if isinstance(v, dict) and "event_ms_median" in v}
                          for c, legs in result[k].items()} for k in ("one_bag", "many_bags")}))


if __name__ == "__main__":
    main()
