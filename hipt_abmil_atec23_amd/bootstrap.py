"""Bootstrapped evaluation metrics (the reference's ``bootstrapping.py``) on the HIP library.

The reference resamples the n pooled fold predictions ``--bootstraps`` times (``np.random.choice(range(n), n)``,
bootstrapping.py:79) and calls four scikit-learn metrics on Python lists per replicate (:80-87).  Here a replicate is a row of
drawn indices and one workgroup of ``hipt_bootstrap_metrics`` (csrc/bootstrap.hip) turns it into the same four numbers from
integer counts: AUC, F1 (macro F1 for more than two classes), accuracy, balanced accuracy.

Host work, by design: the scores are sorted once per call (the device sees only their order and their tie groups, so equal
float64 scores tie exactly as in ``roc_curve``), and the draws come from the global ``np.random`` state, a chunk at a time, so a
seed set by the caller reproduces the reference's replicates.  While the device works on one chunk the host draws the next into
pinned memory; the only synchronisation of a call is the read-back of its results.  The eight summary numbers are
``np.mean`` / ``np.std`` of the per-replicate arrays on the host, as in the reference (:95-102).

    python -m hipt_abmil_atec23_amd.bootstrap --model_names m1,m2 --bootstraps 100000 --run_repeats 10 --folds 10

takes the reference's flags and writes the same ``metric_results/<name>.csv``.
"""
from __future__ import annotations

import argparse
import os
from dataclasses import dataclass

import numpy as np

from . import _native as N

MAX_N, MAX_CLASSES, MAX_REPLICATES = N.BOOTSTRAP_MAX_N, N.BOOTSTRAP_MAX_CLASSES, N.BOOTSTRAP_MAX_REPLICATES
DEFAULT_CHUNK = 4096   # replicates per launch and per pinned staging buffer


@dataclass
class BootstrapResult:
    """Per-replicate float64 arrays of length B, in the order the replicates were drawn."""
    auc: np.ndarray
    f1: np.ndarray
    accuracy: np.ndarray
    balanced_accuracy: np.ndarray

    def summary(self):
        """The reference's eight numbers in its order (bootstrapping.py:95-102): the means of AUC, F1, accuracy and balanced
        accuracy, then their population standard deviations."""
        cols = (self.auc, self.f1, self.accuracy, self.balanced_accuracy)
        return tuple(np.mean(c) for c in cols) + tuple(np.std(c) for c in cols)


def prepare_scores(Y, Y_hat, probs):
    """``(Y int32 [n], Y_hat int32 [n], order int32 [C, n], tie int32 [C, n], K)`` as ``hipt_bootstrap_metrics`` reads them.

    ``probs`` is ``p_1 [n]`` for two classes (C = 1: class 1 is scored) and ``[n, K]`` for K > 2 (C = K, one-vs-rest).
    ``order[c]`` sorts the samples ascending by class c's score (stable); ``tie[c][p] = lo | hi << 16`` is the range of
    positions holding the same float64 score as position p."""
    Y = np.asarray(Y)
    Y_hat = np.asarray(Y_hat)
    probs = np.asarray(probs, dtype=np.float64)
    if Y.ndim != 1 or Y_hat.shape != Y.shape or len(Y) < 1:
        raise ValueError(f"bootstrap_metrics: Y and Y_hat must be equal-length vectors, got {Y.shape} and {Y_hat.shape}")
    n = len(Y)
    if probs.ndim == 1:
        K, cols = 2, probs[None, :]
    elif probs.ndim == 2 and probs.shape[1] == 2:
        K, cols = 2, probs[:, 1][None, :]
    elif probs.ndim == 2 and probs.shape[1] > 2:
        K, cols = probs.shape[1], probs.T
    else:
        raise ValueError(f"bootstrap_metrics: probs must be p_1 [n] (or [n, 2]) for two classes or [n, K] for K > 2, got {probs.shape}")
    if cols.shape[1] != n:
        raise ValueError(f"bootstrap_metrics: {cols.shape[1]} score rows for {n} labels")
    if n > MAX_N or K > MAX_CLASSES:
        raise ValueError(f"bootstrap_metrics: n={n} / K={K} beyond the kernel's limits {MAX_N} / {MAX_CLASSES}")
    if not np.isfinite(cols).all():
        raise ValueError("bootstrap_metrics: probs contains NaN or infinity")
    for name, v in (("Y", Y), ("Y_hat", Y_hat)):
        if not np.issubdtype(v.dtype, np.integer) and not np.array_equal(v, np.floor(v)):
            raise ValueError(f"bootstrap_metrics: {name} must hold integer class ids")
        if v.min() < 0 or v.max() >= K:
            raise ValueError(f"bootstrap_metrics: {name} must hold class ids in 0..{K - 1}")
    order = np.empty((len(cols), n), dtype=np.int32)
    tie = np.empty((len(cols), n), dtype=np.int32)
    pos = np.arange(n)
    for c, s in enumerate(cols):
        o = np.argsort(s, kind="stable")
        first = np.ones(n, dtype=bool)
        first[1:] = s[o][1:] != s[o][:-1]
        starts = pos[first]
        g = np.cumsum(first) - 1
        lo = starts[g]
        hi = np.append(starts[1:], n)[g]
        order[c] = o
        tie[c] = lo | (hi << 16)
    return Y.astype(np.int32), Y_hat.astype(np.int32), order, tie, K


def _finish(out, flags):
    """The result object from the device's ``[B, 4]`` array and flag word; raises where the reference would have."""
    if flags & N.BOOTSTRAP_BAD_INPUT:
        raise RuntimeError("bootstrap_metrics: the kernel met an index or label outside its range (internal error)")
    bad = np.flatnonzero(np.isnan(out[:, 0]))
    if len(bad) or flags & N.BOOTSTRAP_DEGENERATE:
        which = int(bad[0]) if len(bad) else -1
        raise ValueError(f"Only one class present in y_true. ROC AUC score is not defined in that case. "
                         f"(bootstrap replicate {which} is the first of {len(bad)} without both a positive and a negative member "
                         f"of every scored class; the reference stops with sklearn's error there)")
    return BootstrapResult(*(np.ascontiguousarray(out[:, j]) for j in range(4)))


def bootstrap_metrics(Y, Y_hat, probs, n_bootstraps=None, *, idxs=None, chunk=DEFAULT_CHUNK, device=None) -> BootstrapResult:
    """AUC, F1, accuracy and balanced accuracy of ``n_bootstraps`` resamples of the pooled predictions ``(Y, Y_hat, probs)``.

    ``idxs=None``: replicate b is ``np.random.choice(range(n), n)`` of the global ``np.random`` state, exactly the b-th draw of
    the reference's loop (drawn as ``np.random.randint(0, n, size=(chunk, n))``, which consumes the same stream).
    ``idxs [B, n]``: run these replicates instead.  The result does not depend on ``chunk``.  Raises ``ValueError`` (after the
    call has completed) if a replicate lacks a positive or a negative member of a scored class, naming the first one."""
    import torch

    y32, yh32, order, tie, K = prepare_scores(Y, Y_hat, probs)
    n = len(y32)
    if idxs is not None:
        idxs = np.asarray(idxs)
        if idxs.ndim != 2 or idxs.shape[1] != n or not np.issubdtype(idxs.dtype, np.integer):
            raise ValueError(f"bootstrap_metrics: idxs must be integer [B, {n}], got {idxs.dtype} {idxs.shape}")
        if n_bootstraps is not None and int(n_bootstraps) != idxs.shape[0]:
            raise ValueError(f"bootstrap_metrics: n_bootstraps={n_bootstraps} but idxs has {idxs.shape[0]} rows")
        if idxs.size and (idxs.min() < 0 or idxs.max() >= n):
            raise IndexError(f"bootstrap_metrics: idxs outside 0..{n - 1}")
        B = idxs.shape[0]
    else:
        B = int(n_bootstraps) if n_bootstraps is not None else 0
    if B < 1:
        raise ValueError("bootstrap_metrics: at least one replicate is needed")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("bootstrap_metrics: chunk must be >= 1")
    chunk = min(chunk, B, MAX_REPLICATES)

    dev = torch.device("cuda" if device is None else device)
    if dev.type != "cuda":
        raise RuntimeError(f"bootstrap_metrics: device {dev}; hipt_abmil_atec23_amd runs only on a HIP device (there is deliberately no CPU path)")
    if not torch.cuda.is_available():
        raise RuntimeError("bootstrap_metrics: no HIP device; hipt_abmil_atec23_amd runs only on a HIP device (there is deliberately no CPU path)")
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        st = N.stream_ptr(dev)
        const = [torch.from_numpy(a).to(dev) for a in (y32, yh32, order, tie)]
        res = torch.empty(B * 4 + 1, dtype=torch.float64, device=dev)   # [B, 4] results + the flag word in the last 8 bytes
        res[-1:].zero_()
        flags_ptr = res.data_ptr() + B * 4 * 8
        copy_stream = torch.cuda.Stream(device=dev, priority=-1)
        stage = [torch.empty((chunk, n), dtype=torch.int32, pin_memory=True) for _ in range(2)]
        stage_np = [s.numpy() for s in stage]
        dbuf = [torch.empty((chunk, n), dtype=torch.int32, device=dev) for _ in range(2)]
        copy_stream.wait_stream(cur)   # the blocks come from this stream's pool: work enqueued here may just have freed them
        staged, free = [None, None], [None, None]
        for i, b0 in enumerate(range(0, B, chunk)):
            s, m = i & 1, min(chunk, B - b0)
            if staged[s] is not None:
                staged[s].synchronize()   # the copy out of this pinned buffer, two chunks ago (long complete)
            if idxs is None:
                np.copyto(stage_np[s][:m], np.random.randint(0, n, size=(m, n)), casting="unsafe")
            else:
                np.copyto(stage_np[s][:m], idxs[b0:b0 + m], casting="unsafe")
            if free[s] is not None:
                copy_stream.wait_event(free[s])   # the kernel that read this device buffer two chunks ago
            with torch.cuda.stream(copy_stream):
                dbuf[s][:m].copy_(stage[s][:m], non_blocking=True)
            staged[s] = torch.cuda.Event()
            staged[s].record(copy_stream)
            cur.wait_event(staged[s])
            N.call("hipt_bootstrap_metrics", N.ptr(const[0]), N.ptr(const[1]), N.ptr(const[2]), N.ptr(const[3]), n, K,
                   N.ptr(dbuf[s]), m, res.data_ptr() + b0 * 32, flags_ptr, st)
            free[s] = torch.cuda.Event()
            free[s].record(cur)
        host = res.cpu().numpy()   # the call's one synchronisation; everything enqueued above, copies included, precedes it
    flags = int(host[-1:].view(np.int32)[0])
    return _finish(host[:-1].reshape(B, 4), flags)


# ------------------------------------------------------------------------------------------------------------------------------
# the reference script's files
# ------------------------------------------------------------------------------------------------------------------------------
def read_eval_run(model_name, run_no, *, run_repeats, folds, num_classes, eval_root="eval_results"):
    """``(Y, Y_hat, probs, losses)`` of one run repeat, pooled over its folds as bootstrapping.py:36-57 pools them:
    ``EVAL_<name>_run<r>/fold_<k>.csv`` when there are several repeats, else ``EVAL_<name>/fold_<k>.csv``; ``p_1`` for two
    classes, the last K columns otherwise; the losses always from ``EVAL_<name>/summary.csv``."""
    import pandas as pd

    full = os.path.join(eval_root, "EVAL_" + model_name)
    losses = list(pd.read_csv(os.path.join(full, "summary.csv"))["loss"])
    ys, yhs, ps = [], [], []
    for fold_no in range(folds):
        d = f"{full}_run{run_no}" if run_repeats > 1 else full
        df = pd.read_csv(os.path.join(d, f"fold_{fold_no}.csv"))
        ys.append(df["Y"].to_numpy())
        yhs.append(df["Y_hat"].to_numpy())
        ps.append(df["p_1"].to_numpy(dtype=np.float64) if num_classes == 2 else df.iloc[:, -num_classes:].to_numpy(dtype=np.float64))
    return np.concatenate(ys), np.concatenate(yhs), np.concatenate(ps, axis=0), losses


def metric_frame(summaries):
    """The frame the reference writes (bootstrapping.py:112) from one ``summary()`` per run repeat: eight rows (AUC, accuracy,
    balanced accuracy, F1 means, then their sds in that order), one cell each holding the list over the repeats."""
    import pandas as pd

    cols = [[s[j] for s in summaries] for j in range(8)]
    auc_m, f1_m, acc_m, bacc_m, auc_s, f1_s, acc_s, bacc_s = cols
    return pd.DataFrame([[auc_m], [acc_m], [bacc_m], [f1_m], [auc_s], [acc_s], [bacc_s], [f1_s]])


def confusion_matrix(Y, Y_hat, K):
    c = np.zeros((K, K), dtype=np.int64)
    np.add.at(c, (np.asarray(Y, dtype=np.int64), np.asarray(Y_hat, dtype=np.int64)), 1)
    return c


def bootstrap_eval_dir(model_name, *, bootstraps=100000, run_repeats=10, folds=10, num_classes=2, eval_root="eval_results",
                       out_dir="metric_results", chunk=DEFAULT_CHUNK, device=None):
    """One model of the reference's loop (bootstrapping.py:24-113): per run repeat the pooled folds, the confusion matrix and
    the mean loss printed, ``bootstraps`` replicates on the device, the running lists of means and sds printed; then
    ``<out_dir>/<model_name>.csv``.  Returns the frame that was written.  Multi-class runs over several folds work (the
    reference's ``DataFrame.append`` no longer exists; the folds' probabilities are concatenated row-wise, as it intended)."""
    summaries = []
    for run_no in range(run_repeats):
        Y, Y_hat, probs, losses = read_eval_run(model_name, run_no, run_repeats=run_repeats, folds=folds, num_classes=num_classes,
                                                eval_root=eval_root)
        if num_classes > 2 and probs.shape[1] != num_classes:
            raise ValueError(f"{model_name}: fold CSVs have {probs.shape[1]} trailing columns, --num_classes is {num_classes}")
        print("run: ", run_no)
        print("confusion matrix (predicted x axis, true y axis): \n")
        print(confusion_matrix(Y, Y_hat, num_classes), "\n")
        print("average ce loss: ", np.mean(losses), "(not bootstrapped)")
        summaries.append(bootstrap_metrics(Y, Y_hat, probs, bootstraps, chunk=chunk, device=device).summary())
        col = lambda j: [s[j] for s in summaries]   # noqa: E731
        print("AUC mean: ", col(0), " AUC std: ", col(4))
        print("F1 mean: " if num_classes == 2 else "Macro F1 mean: ", col(1), " F1 std: ", col(5))
        print("accuracy mean: ", col(2), " accuracy std: ", col(6))
        print("balanced accuracy mean: ", col(3), " balanced accuracy std: ", col(7))
    df = metric_frame(summaries)
    os.makedirs(out_dir, exist_ok=True)
    df.to_csv(os.path.join(out_dir, model_name + ".csv"), index=False)
    return df


def make_parser():
    p = argparse.ArgumentParser(prog="python -m hipt_abmil_atec23_amd.bootstrap", description="Model names input split by commas")
    p.add_argument("--model_names", type=str, default=None, help="models to evaluate")
    p.add_argument("--bootstraps", type=int, default=100000, help="Number of bootstraps to calculate")
    p.add_argument("--run_repeats", type=int, default=10, help="Number of model repeats")
    p.add_argument("--folds", type=int, default=10, help="Number of cross-validation folds")
    p.add_argument("--data_csv", type=str, default="set_all_714.csv", help="accepted and unused, as in the reference")
    p.add_argument("--num_classes", type=int, default=2)
    p.add_argument("--plot_roc_curves", action="store_true", default=False, help="not supported: plotting is out of scope")
    p.add_argument("--roc_plot_dir", type=str, default="../mount_outputs/roc_plots/", help="accepted and unused")
    p.add_argument("--eval_root", type=str, default="eval_results", help="where the EVAL_<name> directories lie")
    p.add_argument("--out_dir", type=str, default="metric_results", help="where <name>.csv is written")
    return p


def main(argv=None):
    p = make_parser()
    args = p.parse_args(argv)
    if args.plot_roc_curves:
        p.error("--plot_roc_curves is not supported: ROC plotting is out of this package's scope (DESIGN.md 8); "
                "run the reference's bootstrapping.py with --bootstraps 1 for the plot")
    if not args.model_names:
        p.error("--model_names is required")
    for name in args.model_names.split(","):
        bootstrap_eval_dir(name, bootstraps=args.bootstraps, run_repeats=args.run_repeats, folds=args.folds,
                           num_classes=args.num_classes, eval_root=args.eval_root, out_dir=args.out_dir)


if __name__ == "__main__":
    main()
