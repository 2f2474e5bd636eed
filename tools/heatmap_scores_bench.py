"""Heat-map scores on the device (csrc/percentile.hip) against what they replace, on one MI355X with every input
resident on the device.  Routes that are compared run in the same process in interleaved rounds; every figure is the median of the
rounds, each round a host clock around ``iters`` calls that end in a device synchronise (the replaced routes contain host work, so
device events alone would not see them).

  (a) score2percentile   ``score2percentile(q, ref)`` at nq = nref of 10 000, 100 000 and 1 000 000, float64 tensors in, tensor out,
                         against the reference's loop (vis_utils/heatmap_utils.py:75-77: one ``scipy.stats.percentileofscore(ref, s)``
                         per score) on this box's CPU.  The loop is TIMED ON ``--loop-scores`` SCORES AND EXTRAPOLATED to nq
                         (``scipy_loop_s_extrapolated``); where scipy does not import, the field is absent.  ``pairs_per_s`` is
                         nq * nref / device time.
  (a') to_percentiles    the rank kernel on a device tensor against the route it replaces (``.cpu()``, numpy ``argsort`` ranks,
                         copy back) at the same three sizes: the brute force is O(n^2), the sort O(n log n), so this is where a
                         crossover would show.
  (b) render_heatmap     ``render_heatmap(..., convert_to_percentiles=True)`` on device tensors at N = 100 000 (the ds32 case of
                         tools/heatmap_bench.py), against the same call with the ranks taken over the host round trip as before.
  equal                  the device result equals the replaced route's, bit for bit (for (a): on the scores the loop was timed on)

    python tools/heatmap_scores_bench.py [--sizes 10000,100000,1000000] [--out profiles/heatmap_scores_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))


def timed(fn, iters):
    """Seconds per call: host clock around ``iters`` calls, device idle before and after."""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters, out


def rounds_of(routes, iters, rounds, warmup=1):
    """{name: (median seconds per call, [per round], last result)} with the routes taking turns inside every round."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    per = {k: [] for k in routes}
    last = {}
    for _ in range(rounds):
        for k, fn in routes.items():
            s, last[k] = timed(fn, iters)
            per[k].append(s)
    return {k: (statistics.median(v), v, last[k]) for k, v in per.items()}


def ms(s):
    return round(s * 1e3, 4)


def host_ranks_round_trip(s):
    """The replaced route of ``_device_inputs``: the scores leave the device, numpy ranks them, the ranks come back."""
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    return torch.from_numpy(H.to_percentiles(s.cpu().numpy())).to(s.device)


def bench_scores(n, args):
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(n)
    ref = rng.standard_normal(n).astype(np.float32).astype(np.float64)   # attention scores are float32
    q = np.concatenate([ref[rng.permutation(n)[:n // 2]], rng.standard_normal(n - n // 2)])   # half of them tie with the reference
    dev = torch.device("cuda")
    q_t, ref_t = torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev)
    iters = max(1, min(200, int(2e10 / (float(n) * n))))   # (about 2e10 pairs per round)
    got = rounds_of({"device": lambda: H.score2percentile(q_t, ref_t)}, iters, args.rounds)["device"]
    res = {"case": "score2percentile", "nq": n, "nref": n, "iters": iters, "device_ms": ms(got[0]), "device_ms_rounds": [ms(x) for x in got[1]],
           "pairs_per_s": float(f"{float(n) * n / got[0]:.4g}")}
    try:
        from scipy.stats import percentileofscore
    except ImportError:
        percentileofscore = None
    if percentileofscore is not None:
        k = min(args.loop_scores, n)
        t0 = time.perf_counter()
        loop = np.array([percentileofscore(ref, s) for s in q[:k]])
        dt = time.perf_counter() - t0
        res.update(scipy_loop_scores_timed=k, scipy_loop_s_timed=round(dt, 4), scipy_loop_s_extrapolated=round(dt / k * n, 2),
                   equal=bool(np.array_equal(got[2][:k].cpu().numpy().view(np.int64), loop.view(np.int64))),
                   speedup_extrapolated=round(dt / k * n / got[0], 1))
    print(json.dumps(res), flush=True)

    both = rounds_of({"device": lambda: H.to_percentiles(q_t), "host_round_trip": lambda: host_ranks_round_trip(q_t)}, iters, args.rounds)
    res2 = {"case": "to_percentiles", "n": n, "iters": iters, "device_ms": ms(both["device"][0]),
            "device_ms_rounds": [ms(x) for x in both["device"][1]], "host_round_trip_ms": ms(both["host_round_trip"][0]),
            "host_round_trip_ms_rounds": [ms(x) for x in both["host_round_trip"][1]],
            "equal": bool(torch.equal(both["device"][2].view(torch.int64), both["host_round_trip"][2].view(torch.int64))),
            "device_over_host": round(both["device"][0] / both["host_round_trip"][0], 3)}
    print(json.dumps(res2), flush=True)
    return [res, res2]


def bench_render(args):
    import torch
    import heatmap_bench as B
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords, (w, h), mask, canvas = B.make_case(32)
    scores = np.round(scores, 2)   # ties, as real attention scores rounded by float32 have
    dev = torch.device("cuda")
    s_t, c_t, m_t, cv_t = (torch.from_numpy(a).to(dev) for a in (scores, coords, mask, canvas))
    kw = dict(alpha=0.4, mask=m_t, canvas=cv_t)
    args_ = (c_t, B.PATCH, 1.0 / 32, (w, h))
    routes = {"device": lambda: H.render_heatmap(s_t, *args_, convert_to_percentiles=True, **kw),
              "host_round_trip": lambda: H.render_heatmap(host_ranks_round_trip(s_t), *args_, **kw)}
    got = rounds_of(routes, args.render_iters, args.rounds, warmup=2)
    res = {"case": "render_heatmap", "n_patches": B.N_PATCHES, "canvas": [w, h], "convert_to_percentiles": True, "iters": args.render_iters,
           "device_ms": ms(got["device"][0]), "device_ms_rounds": [ms(x) for x in got["device"][1]],
           "host_round_trip_ms": ms(got["host_round_trip"][0]), "host_round_trip_ms_rounds": [ms(x) for x in got["host_round_trip"][1]],
           "equal": bool(torch.equal(got["device"][2], got["host_round_trip"][2])),
           "speedup": round(got["host_round_trip"][0] / got["device"][0], 2)}
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--render-iters", type=int, default=10)
    ap.add_argument("--loop-scores", type=int, default=1000)
    ap.add_argument("--no-render", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("heatmap_scores_bench: no HIP device (there is no CPU path to time)")
    results = []
    for n in (int(v) for v in args.sizes.split(",") if v):
        results += bench_scores(n, args)
    if not args.no_render:
        results.append(bench_render(args))
    doc = {"tool": "tools/heatmap_scores_bench.py", "device": torch.cuda.get_device_name(0), "rounds": args.rounds, "results": results}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
