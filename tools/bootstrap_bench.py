"""Bootstrapped evaluation metrics at the reference's default B = 100 000: where the time of one
``bootstrap_metrics`` call goes, and what the reference's loop costs on the same box.

Per case (n = 285 and n = 714 binary, n = 150 with three classes) one JSON line with
  draw_s      the host draws alone: ``np.random.randint(0, n, size=(chunk, n))`` into the pinned int32 buffer, all chunks
  copy_s      the pinned -> device copies alone (HIP events)
  kernel_s    ``hipt_bootstrap_metrics`` alone on resident indices, all chunks (HIP events)
  call_s      wall time of the whole call (draws, copies, kernels overlapped; read-back; min of ``--repeats``)
  sklearn_ms_per_replicate  the reference's loop body (bootstrapping.py:79-87: the same four scikit-learn calls on the same
              Python lists) timed over ``--sklearn-replicates`` replicates, and its extrapolation to B
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bootstrap_ref as R  # noqa: E402
from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import bootstrap as Bt  # noqa: E402

DEV = "cuda:0"


def fixture(n, K):
    rng = np.random.RandomState(n)
    y = (np.arange(n) % K).astype(np.int64)
    if K == 2:
        p1 = np.round(np.clip(0.5 + 0.12 * (2 * y - 1) + 0.22 * rng.randn(n), 0, 1), 2)
        return y, (p1 > 0.5).astype(np.int64), p1
    z = rng.randn(n, K) + 1.2 * np.eye(K)[y]
    p = np.exp(z) / np.exp(z).sum(axis=1, keepdims=True)
    return y, p.argmax(axis=1).astype(np.int64), p


def sklearn_loop(Y, Y_hat, probs, K, reps):
    """The reference's loop body on its own data structures (lists; a DataFrame for the multi-class probabilities)."""
    import warnings

    import pandas as pd
    from sklearn.metrics import accuracy_score, balanced_accuracy_score, f1_score, roc_auc_score
    all_Ys, all_Yhats = list(Y), list(Y_hat)
    all_p1s = list(probs) if K == 2 else None
    all_probs = None if K == 2 else pd.DataFrame(probs)
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(reps):
            idxs = np.random.choice(range(len(all_Ys)), len(all_Ys))
            if K == 2:
                f1_score([all_Ys[i] for i in idxs], [all_Yhats[i] for i in idxs])
                roc_auc_score([all_Ys[i] for i in idxs], [all_p1s[i] for i in idxs])
            else:
                f1_score([all_Ys[i] for i in idxs], [all_Yhats[i] for i in idxs], average="macro")
                roc_auc_score([all_Ys[i] for i in idxs], [all_probs.iloc[i, :] for i in idxs], multi_class="ovr")
            accuracy_score([all_Ys[i] for i in idxs], [all_Yhats[i] for i in idxs])
            balanced_accuracy_score([all_Ys[i] for i in idxs], [all_Yhats[i] for i in idxs])
    return (time.perf_counter() - t0) / reps


def parts(Y, Y_hat, probs, B, chunk):
    y32, yh32, order, tie, K = Bt.prepare_scores(Y, Y_hat, probs)
    n = len(y32)
    const = [torch.from_numpy(a).to(DEV) for a in (y32, yh32, order, tie)]
    stage = torch.empty((chunk, n), dtype=torch.int32, pin_memory=True)
    stage_np = stage.numpy()
    dbuf = torch.empty((chunk, n), dtype=torch.int32, device=DEV)
    out = torch.empty((B, 4), dtype=torch.float64, device=DEV)
    flags = torch.zeros(1, dtype=torch.int32, device=DEV)
    sizes = [min(chunk, B - b) for b in range(0, B, chunk)]
    np.random.seed(0)
    t0 = time.perf_counter()
    for m in sizes:
        np.copyto(stage_np[:m], np.random.randint(0, n, size=(m, n)), casting="unsafe")
    draw = time.perf_counter() - t0
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    st = N.stream_ptr(DEV)
    dbuf.copy_(stage, non_blocking=True)   # warm
    N.call("hipt_bootstrap_metrics", *(N.ptr(c) for c in const), n, K, N.ptr(dbuf), sizes[0], N.ptr(out), N.ptr(flags), st)
    torch.cuda.synchronize()
    e[0].record()
    for m in sizes:
        dbuf[:m].copy_(stage[:m], non_blocking=True)
    e[1].record()
    torch.cuda.synchronize()
    e[2].record()
    b0 = 0
    for m in sizes:
        N.call("hipt_bootstrap_metrics", *(N.ptr(c) for c in const), n, K, N.ptr(dbuf), m, out.data_ptr() + b0 * 32, N.ptr(flags), st)
        b0 += m
    e[3].record()
    torch.cuda.synchronize()
    return draw, e[0].elapsed_time(e[1]) / 1e3, e[2].elapsed_time(e[3]) / 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bootstraps", type=int, default=100000)
    ap.add_argument("--chunk", type=int, default=Bt.DEFAULT_CHUNK)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sklearn-replicates", type=int, default=20)
    args = ap.parse_args()
    B = args.bootstraps
    for n, K in ((285, 2), (714, 2), (150, 3)):
        Y, Y_hat, probs = fixture(n, K)
        draw, copy, kern = parts(Y, Y_hat, probs, B, min(args.chunk, B))
        calls = []
        for _ in range(args.repeats):
            np.random.seed(1)
            t0 = time.perf_counter()
            res = Bt.bootstrap_metrics(Y, Y_hat, probs, B, chunk=args.chunk, device=DEV)
            calls.append(time.perf_counter() - t0)
        chk = R.replicate_metrics(Y, Y_hat, probs, (np.random.seed(1), np.random.randint(0, n, size=(1, n)))[1][0], K)
        assert abs(chk[0] - res.auc[0]) <= 1e-15 and chk[2] == res.accuracy[0]
        sk = sklearn_loop(Y, Y_hat, probs, K, args.sklearn_replicates) if args.sklearn_replicates > 0 else float("nan")
        print(json.dumps({"n": n, "K": K, "B": B, "chunk": args.chunk, "draw_s": round(draw, 4), "copy_s": round(copy, 4),
                          "kernel_s": round(kern, 4), "call_s": round(min(calls), 4), "call_s_all": [round(c, 4) for c in calls],
                          "auc_mean": float(np.mean(res.auc)), "sklearn_ms_per_replicate": round(sk * 1e3, 3),
                          "sklearn_s_for_B": round(sk * B, 1), "speedup": round(sk * B / min(calls), 1)}), flush=True)


if __name__ == "__main__":
    main()
