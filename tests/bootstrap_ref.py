"""numpy restatement of the bootstrapped evaluation metrics (the reference's bootstrapping.py:78-102), written from the
metrics' definitions as ratios of integer counts; independent of the package's host preparation and of the HIP kernel.

A replicate is a multiset of the n pooled predictions, given as n drawn indices.  With cnt = bincount(indices):
  confusion[y, y_hat] = sum of cnt over the samples with those labels
  accuracy            = trace / n
  f1_c                = 2 tp / (2 tp + fp + fn)            (0 where the denominator is 0)
  recall_c            = tp / (tp + fn)                      (balanced accuracy: the mean over the classes that occur)
  auc_c               = (2 #{pos > neg} + #{pos = neg}) / (2 P N), pairs counted with multiplicity; two scores tie when their
                        float64 values are equal
K = 2: AUC and F1 of class 1 (scores ``p_1``).  K > 2: their means over the classes, one-vs-rest on column c of ``probs``.
A class without a positive or without a negative member in the replicate has no AUC: NaN.
"""
import numpy as np


def synthetic_binary(seed=2023, folds=5, rows=57):
    """The binary fixture of make_golden_bootstrap.py: ``(Y, Y_hat, p_1)`` per fold; p_1 has two decimals, so many scores tie."""
    rng = np.random.RandomState(seed)
    out = []
    for _ in range(folds):
        y = (rng.rand(rows) < 0.5).astype(np.int64)
        p1 = np.round(np.clip(0.5 + 0.12 * (2 * y - 1) + 0.22 * rng.randn(rows), 0.0, 1.0), 2)
        out.append((y, (p1 > 0.5).astype(np.int64), p1))
    return out


def synthetic_multiclass(seed=2024, rows=150, k=3):
    """The 3-class fixture: ``(Y, Y_hat, probs [rows, k])``, softmax rows."""
    rng = np.random.RandomState(seed)
    y = rng.randint(0, k, size=rows).astype(np.int64)
    z = rng.randn(rows, k) + 1.2 * np.eye(k)[y]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return y, p.argmax(axis=1).astype(np.int64), p


def limit_case(n, k, seed=7, levels=37):
    """Random labels and heavily tied scores (``levels`` distinct values per class) at a given size."""
    rng = np.random.RandomState(seed)
    y = rng.randint(0, k, size=n).astype(np.int64)
    y[:k] = np.arange(k)
    yh = np.where(rng.rand(n) < 0.6, y, rng.randint(0, k, size=n)).astype(np.int64)
    probs = rng.randint(0, levels, size=(n, k)).astype(np.float64) / levels
    return y, yh, (probs[:, 1] if k == 2 else probs)


def _auc_counts(cnt, pos_mask, score):
    """(numerator, P, N) of one class: numerator = 2 #{pos > neg} + #{pos = neg} over the multiset."""
    vals, g = np.unique(score, return_inverse=True)
    pos = np.zeros(len(vals), dtype=np.int64)
    neg = np.zeros(len(vals), dtype=np.int64)
    np.add.at(pos, g, np.where(pos_mask, cnt, 0))
    np.add.at(neg, g, np.where(pos_mask, 0, cnt))
    below = np.cumsum(neg) - neg
    return int(np.sum(2 * pos * below + pos * neg)), int(pos.sum()), int(neg.sum())


def replicate_metrics(Y, Y_hat, probs, idx, K):
    """``(auc, f1, accuracy, balanced_accuracy)`` of one replicate as Python floats."""
    Y = np.asarray(Y, dtype=np.int64)
    Y_hat = np.asarray(Y_hat, dtype=np.int64)
    probs = np.asarray(probs, dtype=np.float64)
    n = len(Y)
    cnt = np.bincount(np.asarray(idx, dtype=np.int64), minlength=n).astype(np.int64)
    conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(conf, (Y, Y_hat), cnt)
    tp = np.diag(conf)
    rows, cols = conf.sum(axis=1), conf.sum(axis=0)
    accuracy = float(tp.sum()) / float(n)
    recalls = [float(tp[c]) / float(rows[c]) for c in range(K) if rows[c] > 0]
    bal = 0.0
    for r in recalls:
        bal += r
    bal = bal / len(recalls)
    scored = [1] if K == 2 else list(range(K))
    f1 = 0.0
    auc = 0.0
    degenerate = False
    for c in scored:
        den = int(rows[c] + cols[c])
        f1 += float(2 * tp[c]) / float(den) if den > 0 else 0.0
        num, P, Nn = _auc_counts(cnt, Y == c, probs if K == 2 else probs[:, c])
        if P == 0 or Nn == 0:
            degenerate = True
        else:
            auc += float(num) / float(2 * P * Nn)
    return (float("nan") if degenerate else auc / len(scored)), f1 / len(scored), accuracy, bal


def bootstrap_metrics_ref(Y, Y_hat, probs, idxs, K):
    """float64 ``[B, 4]`` for ``idxs [B, n]``."""
    return np.array([replicate_metrics(Y, Y_hat, probs, row, K) for row in np.asarray(idxs)], dtype=np.float64).reshape(-1, 4)


def pairwise_auc(Y, score, idx, cls=1):
    """Brute force over all (positive, negative) pairs of the drawn multiset: wins + ties / 2 over P N."""
    y = np.asarray(Y)[idx] == cls
    s = np.asarray(score, dtype=np.float64)[idx]
    pos, neg = s[y], s[~y]
    wins = int((pos[:, None] > neg[None, :]).sum())
    ties = int((pos[:, None] == neg[None, :]).sum())
    return float(2 * wins + ties) / float(2 * len(pos) * len(neg))


def summary(per_replicate):
    """The reference's eight numbers (bootstrapping.py:95-102) from ``[B, 4]``: four means, four population sds."""
    a = np.asarray(per_replicate, dtype=np.float64)
    return np.array([np.mean(a[:, j]) for j in range(4)] + [np.std(a[:, j]) for j in range(4)])
