"""Single-bag CLAM inference, host wall time per ``forward`` (the host work around the launches included): ``CLAM_SB`` [384, 128, 64]
bf16 on a 2 000-row and a 100 000-row bag, ``CLAM_MB`` [192, 128, 64] K = 3 bf16 on 100 000 rows in one pass and branch by branch.
The method is tools/clam_narrow_bags_bench.py's: wall time around a synchronised batch of repetitions, the cases interleaved in rounds on
one box, each figure the median over the rounds with the spread (min ... max) beside it.  To compare two commits, run the tool from a
checkout of each, alternating, more than once each: a commit's own run-to-run spread is the yardstick.
python tools/clam_forward_bench.py [out.json] [rounds=15] [reps=20]"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, synth  # noqa: E402

out_path = sys.argv[1] if len(sys.argv) > 1 else None
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
dev = "cuda:0"


def timed(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def model(cls, size, **kw):
    m = cls(size_arg=list(size), **kw)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=kw.get("n_classes", 2), multi=cls is CLAM_MB), size[0]))
    m.relocate()
    return m.eval().set_compute_dtype("bf16")


sb, mb = model(CLAM_SB, (384, 128, 64)), model(CLAM_MB, (192, 128, 64), n_classes=3)
by_branch = model(CLAM_MB, (192, 128, 64), n_classes=3)
by_branch.one_pass = False
bag = lambda n, s0, seed: synth.hash_uniform_torch((n, s0), seed, device=dev).bfloat16()
h2k, h100k, m100k = bag(2000, 384, 91), bag(100_000, 384, 92), bag(100_000, 192, 93)
cases = {"CLAM_SB [384,128,64] bf16, 2000 rows": lambda: sb(h2k), "CLAM_SB [384,128,64] bf16, 100000 rows": lambda: sb(h100k),
         "CLAM_MB [192,128,64] K=3 bf16, 100000 rows, one pass": lambda: mb(m100k),
         "CLAM_MB [192,128,64] K=3 bf16, 100000 rows, branch by branch": lambda: by_branch(m100k)}
times = {name: [] for name in cases}
with torch.no_grad():
    for fn in cases.values():
        for _ in range(3):
            fn()
    for _ in range(rounds):
        for name, fn in cases.items():
            times[name].append(timed(fn, reps))
result = {"device": torch.cuda.get_device_name(0), "rounds": rounds, "reps_per_round": reps,
          "timing": "host wall time per forward, synchronised batches, interleaved rounds, median (min ... max)",
          "cases": {name: {"median_us": round(statistics.median(v), 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1)} for name, v in times.items()}}
print(json.dumps(result), flush=True)
if out_path:
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
