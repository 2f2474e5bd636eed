#!/usr/bin/env python3
"""Generate tests/golden/bootstrap_binary.npz, bootstrap_3class.npz and the fold CSVs under tests/golden/bootstrap_eval/
by running the REFERENCE's own ``bootstrapping.py`` (scikit-learn metrics) in place.

Run ONLY where the read-only reference checkout exists:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_bootstrap.py [--ref /root/reference]

Inputs are this project's own synthetic predictions (tests/bootstrap_ref.py):
  binary   5 folds x 57 rows, ``p_1`` rounded to two decimals (many ties), seed 123, B = 300
  3-class  1 fold x 150 rows of softmax probabilities, seed 5, B = 60 (the reference's multi-class branch runs with one fold
           only: its ``DataFrame.append`` is gone from current pandas)
They are written as ``eval_results/EVAL_<name>/fold_<k>.csv`` + ``summary.csv`` in the layout the reference's eval.py leaves.
The script is executed with ``runpy.run_path`` in a temporary working directory after ``np.random.seed``; its per-replicate
lists and the eight summary lists are taken from the globals it leaves.  Stored per case: the pooled ``Y``, ``Y_hat``, ``probs``,
the seed and B, the drawn indices (int16; what ``np.random.randint(0, n, size=(B, n))`` gives after the same seed, which is
the stream of B successive ``np.random.choice(range(n), n)`` calls -- checked here through the recorded results), the
per-replicate values ``[B, 4]`` (AUC, F1, accuracy, balanced accuracy), the summaries and the CSV the script wrote.
"""
import argparse
import importlib
import os
import runpy
import shutil
import sys
import tempfile
import types

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bootstrap_ref as R  # noqa: E402

CASES = {"binary": dict(seed=123, B=300, K=2, folds=5), "3class": dict(seed=5, B=60, K=3, folds=1)}
LOSSES = {"binary": [0.61, 0.58, 0.66, 0.6, 0.63], "3class": [0.83]}


def fold_frames(name):
    if name == "binary":
        frames = []
        for f, (y, yh, p1) in enumerate(R.synthetic_binary()):
            frames.append(pd.DataFrame({"slide_id": [f"slide_{f}_{i}" for i in range(len(y))], "Y": y, "Y_hat": yh,
                                        "p_0": np.round(1.0 - p1, 2), "p_1": p1}))
        return frames
    y, yh, p = R.synthetic_multiclass()
    d = {"slide_id": [f"slide_0_{i}" for i in range(len(y))], "Y": y, "Y_hat": yh}
    d.update({f"p_{c}": p[:, c] for c in range(p.shape[1])})
    return [pd.DataFrame(d)]


def write_eval_dir(root, name):
    d = os.path.join(root, "eval_results", f"EVAL_{name}")
    os.makedirs(d, exist_ok=True)
    frames = fold_frames(name)
    for f, df in enumerate(frames):
        df.to_csv(os.path.join(d, f"fold_{f}.csv"), index=False)
    pd.DataFrame({"folds": list(range(len(frames))), "loss": LOSSES[name]}).to_csv(os.path.join(d, "summary.csv"), index=False)
    return d


def run_reference(ref, work, name, cfg):
    for n in ("matplotlib", "matplotlib.pyplot"):
        try:
            importlib.import_module(n)
        except ImportError:
            sys.modules[n] = types.ModuleType(n)
    os.makedirs(os.path.join(work, "metric_results"), exist_ok=True)
    argv, cwd = sys.argv, os.getcwd()
    sys.argv = ["bootstrapping.py", "--model_names", name, "--bootstraps", str(cfg["B"]), "--run_repeats", "1",
                "--folds", str(cfg["folds"]), "--num_classes", str(cfg["K"])]
    os.chdir(work)
    try:
        np.random.seed(cfg["seed"])
        g = runpy.run_path(os.path.join(ref, "bootstrapping.py"), run_name="__main__")
    finally:
        sys.argv = argv
        os.chdir(cwd)
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    args = ap.parse_args()
    sys.dont_write_bytecode = True
    eval_root = os.path.join(HERE, "bootstrap_eval")
    if os.path.isdir(eval_root):
        shutil.rmtree(eval_root)
    for name, cfg in CASES.items():
        write_eval_dir(eval_root, name)
        with tempfile.TemporaryDirectory() as work:
            shutil.copytree(os.path.join(eval_root, "eval_results"), os.path.join(work, "eval_results"))
            g = run_reference(args.ref, work, name, cfg)
            written = pd.read_csv(os.path.join(work, "metric_results", f"{name}.csv"))
        Y = np.asarray(g["all_Ys"], dtype=np.int64)
        Y_hat = np.asarray(g["all_Yhats"], dtype=np.int64)
        probs = np.asarray(g["all_p1s"], dtype=np.float64) if cfg["K"] == 2 else np.asarray(g["all_probs"], dtype=np.float64)
        n = len(Y)
        per = np.stack([np.asarray(g[k], dtype=np.float64) for k in ("AUC_scores", "f1s", "accuracies", "balanced_accuracies")], axis=1)
        assert per.shape == (cfg["B"], 4) and np.isfinite(per).all()
        summ = np.array([g[k][0] for k in ("all_auc_means", "all_f1_means", "all_accuracy_means", "all_balanced_accuracy_means",
                                            "all_auc_sds", "all_f1_sds", "all_accuracy_sds", "all_balanced_accuracy_sds")], dtype=np.float64)
        np.random.seed(cfg["seed"])
        idxs = np.random.randint(0, n, size=(cfg["B"], n))
        mine = R.bootstrap_metrics_ref(Y, Y_hat, probs, idxs, cfg["K"])
        d = np.abs(mine - per).max(axis=0)
        print(f"{name}: n={n} B={cfg['B']}  max|restatement - reference| auc {d[0]:.3g} f1 {d[1]:.3g} acc {d[2]:.3g} bacc {d[3]:.3g}; "
              f"accuracy bit-equal in {(mine[:, 2] == per[:, 2]).sum()} / {cfg['B']}")
        assert d.max() < 1e-12, "the seeded randint stream is not what the reference drew"
        np.savez_compressed(os.path.join(HERE, f"bootstrap_{name}.npz"), Y=Y.astype(np.int16), Y_hat=Y_hat.astype(np.int16), probs=probs,
                            seed=np.int64(cfg["seed"]), B=np.int64(cfg["B"]), K=np.int64(cfg["K"]), folds=np.int64(cfg["folds"]),
                            idxs=idxs.astype(np.int16), per_replicate=per, summary=summ, mean_loss=np.float64(np.mean(g["all_losses"])),
                            confusion=np.asarray(g["confusion_matrix"](g["all_Ys"], g["all_Yhats"]), dtype=np.int64),
                            written_csv=np.array(written.to_csv(index=False)))
    print("wrote", eval_root)


if __name__ == "__main__":
    main()
