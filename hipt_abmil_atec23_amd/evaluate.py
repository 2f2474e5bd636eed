"""The numeric part of the reference's ``summary()`` (utils/eval_utils.py:115-179) and of ``validate_clam``
(utils/core_utils.py:506-597) over a whole split, with the model called on many slides at once (``CLAM_SB.forward_bags``) instead of
once per slide.

``evaluate_split`` returns what ``summary()`` accumulates: the probabilities, labels and predictions of every slide, the mean
error, the mean loss and the per-class correct / count pairs of ``Accuracy_Logger`` (utils/core_utils.py:17-49).  The AUC stays with
the caller: its inputs are exactly ``all_labels`` and ``all_probs`` (``bootstrap`` computes it on the device).  Every figure is a
function of the per-slide logits alone and those do not depend on how the split is cut into calls, so neither do the results.
"""
from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

DEFAULT_MAX_ROWS = 1 << 16


@dataclass
class SplitResult:
    all_probs: np.ndarray        # [n, C] float64 (summary(): np.zeros((len(loader), n_classes)))
    all_labels: np.ndarray       # [n] float64
    all_preds: np.ndarray        # [n] float64
    error: float                 # mean of calculate_error(Y_hat, label) (utils/utils.py:202-205)
    loss: float                  # mean of loss_fn(logits_b, label_b).item()
    acc: List[dict] = field(default_factory=list)   # Accuracy_Logger.data: [{"count", "correct"}] per class

    def class_accuracy(self, c: int):
        """``Accuracy_Logger.get_summary(c)``: (accuracy or None, correct, count)."""
        d = self.acc[c]
        return (float(d["correct"]) / d["count"] if d["count"] else None), d["correct"], d["count"]


def chunk_bags(rows: Sequence[int], max_rows_per_call: int) -> List[range]:
    """Consecutive runs of bags whose row counts add up to at most ``max_rows_per_call`` (a larger bag is a run of its own)."""
    if max_rows_per_call < 1:
        raise ValueError(f"max_rows_per_call must be positive, got {max_rows_per_call}")
    runs, start, acc = [], 0, 0
    for i, n in enumerate(rows):
        if i > start and acc + n > max_rows_per_call:
            runs.append(range(start, i))
            start, acc = i, 0
        acc += n
    if len(rows) > start:
        runs.append(range(start, len(rows)))
    return runs


def _split(bags_or_loader, labels):
    """(list of [N_b, S0] tensors, list of int labels) from a sequence of bags plus labels, or from a loader of (bag, label) pairs."""
    if labels is None:
        pairs = list(bags_or_loader)
        bags, labels = [p[0] for p in pairs], [p[1] for p in pairs]
    else:
        bags = list(bags_or_loader)
    labels = [int(l.reshape(-1)[0]) if isinstance(l, torch.Tensor) else int(l) for l in (labels.tolist() if isinstance(labels, (torch.Tensor, np.ndarray)) else labels)]
    if len(bags) != len(labels):
        raise ValueError(f"{len(bags)} bags but {len(labels)} labels")
    if not bags:
        raise ValueError("evaluate_split: empty split")
    return [b.reshape(-1, b.shape[-1]) for b in bags], labels


@contextlib.contextmanager
def _switches(model, values: dict):
    """``model.<name> = value`` for every pair of ``values`` whose switch the model's CLASS has, for the length of a ``with`` block;
    afterwards the instance is exactly as it was (its own value put back, or none: the attribute deleted, back to the class's), also
    after an exception."""
    values = {k: bool(v) for k, v in values.items() if hasattr(type(model), k)}
    absent = object()
    before = {k: model.__dict__.get(k, absent) for k in values}
    for k, v in values.items():
        setattr(model, k, v)
    try:
        yield
    finally:
        for k, v in before.items():
            if v is absent:
                delattr(model, k)
            else:
                setattr(model, k, v)


def _split_switches(narrow_one_call, wide_one_call, many_one_call) -> dict:
    """The model switches both split functions set: ``bags_narrow`` as asked; ``bags_wide`` and ``bags_many`` only where asked for --
    otherwise the model's own value stays in force --, ``many_one_call`` together with ``bags_one_call``."""
    s = {"bags_narrow": narrow_one_call}
    if wide_one_call:
        s["bags_wide"] = True
    if many_one_call:
        s.update(bags_one_call=True, bags_many=True)
    return s


def _prepare(model, bags_or_loader, labels, n_classes, loss_fn):
    """What both split functions start from: ``(bags, labels, loss_fn, device, (logits [n, C], probs [n, C], preds [n]))`` -- the
    checked split, the model's device (the bags' for a model without parameters) and the host buffers the runs are copied into."""
    bags, labels = _split(bags_or_loader, labels)
    n = len(bags)
    if any(l < 0 or l >= n_classes for l in labels):
        raise ValueError(f"labels must lie in [0, {n_classes})")
    params = list(model.parameters()) if hasattr(model, "parameters") else []
    dev = params[0].device if params else bags[0].device
    out = (torch.empty((n, n_classes), dtype=torch.float32), torch.empty((n, n_classes), dtype=torch.float32),
           torch.empty((n,), dtype=torch.int64))
    return bags, labels, F.cross_entropy if loss_fn is None else loss_fn, dev, out


def _copy_back(run, out, logits, probs, preds):
    """The one trip to the host of a run: its ``(logits, Y_prob, Y_hat, ...)`` into rows ``run`` of the split's buffers."""
    sl = slice(run.start, run.stop)
    logits[sl], probs[sl], preds[sl] = out[0].float().cpu(), out[1].float().cpu(), out[2].reshape(-1).cpu()


def _mean_loss(loss_fn, logits, labels):
    lab = torch.tensor(labels, dtype=torch.int64)
    return sum(float(loss_fn(logits[i:i + 1], lab[i:i + 1])) for i in range(len(labels))) / len(labels)


def _tally(preds, labels, n_classes):
    """``(acc, error)``: ``Accuracy_Logger.data`` per bag class and the mean of ``calculate_error``."""
    acc = [{"count": 0, "correct": 0} for _ in range(n_classes)]
    for p, l in zip(preds.tolist(), labels):
        acc[l]["count"] += 1
        acc[l]["correct"] += int(p == l)
    return acc, sum(d["count"] - d["correct"] for d in acc) / len(labels)


def evaluate_split(model, bags_or_loader, labels=None, n_classes: int = 2, loss_fn: Optional[Callable] = None,
                   max_rows_per_call: int = DEFAULT_MAX_ROWS, narrow_one_call: bool = True, wide_one_call: bool = False,
                   many_one_call: bool = False) -> SplitResult:
    """Evaluate ``model`` on every bag of a split.  ``bags_or_loader``: a sequence of ``[N_b, S0]`` tensors with ``labels``, or an
    iterable of ``(bag, label)`` pairs (a batch-size-1 loader) with ``labels=None``.  The bags go to the model's device and through
    ``model.forward_bags`` in runs of at most ``max_rows_per_call`` rows (a model without ``forward_bags`` is called bag by bag);
    the logits come back to the host once per run.  ``loss_fn(logits [1, C], label [1])`` defaults to cross-entropy.

    A ``CLAM_SB`` model runs with ``bags_narrow = narrow_one_call`` for the duration of the call: for the narrow heads
    (``hipt_smaller``, ``hipt_smallest``, ...: ``hipt_clam_narrow_bags_supported``) the numbers then come from the one-call kernel
    ``hipt_clam_sb_forward_bags_narrow``.  They equal those of the loop over ``forward`` (``narrow_one_call=False``) within the
    fp32 bar (1e-4); they are not bit-equal to it.  ``wide_one_call=True`` likewise sets ``bags_wide`` for the duration of the call:
    the wide heads (``tiny``, ``small``, ``big``, ``small_resnet18``: ``hipt_clam_wide_bags_supported``) then go through
    ``hipt_clam_sb_forward_bags_wide``.  ``False`` (the default) leaves the model's own ``bags_wide`` in force -- which is how a caller of
    ``dropin.install(evaluation=True)`` / ``(validation=True)`` opts in: ``model.bags_wide = True``.  A ``CLAM_MB`` at the wide widths
    needs ``bags_one_call`` as well to take ``hipt_clam_mb_forward_bags_wide``; this function sets only ``bags_wide``, so the model's own
    ``bags_one_call`` (default False: the loop) governs here.  ``many_one_call=True`` sets ``bags_one_call`` AND ``bags_many`` for the
    duration of the call: a ``CLAM_MB`` with 5 to 8 classes at the widths of ``hipt_clam_mb_forward_bags``
    (``hipt_clam_mb_many_bags_supported``) then goes through ``hipt_clam_mb_forward_bags_many``; its numbers equal the loop's within
    the fp32 bar in fp32, not bit for bit.  ``False`` (the default) leaves the model's own ``bags_many`` in force."""
    bags, labels, loss_fn, dev, (logits, probs, preds) = _prepare(model, bags_or_loader, labels, n_classes, loss_fn)
    fb = getattr(model, "forward_bags", None)
    with torch.no_grad(), _switches(model, _split_switches(narrow_one_call, wide_one_call, many_one_call)):
        for run in chunk_bags([b.shape[0] for b in bags], max_rows_per_call):
            part = [bags[i].to(dev) for i in run]
            if fb is not None:
                out = fb(part)
            else:
                outs = [model(b) for b in part]
                out = [torch.cat([o[k] for o in outs], dim=0) for k in range(3)]
            _copy_back(run, out, logits, probs, preds)
        loss = _mean_loss(loss_fn, logits, labels)
    acc, error = _tally(preds, labels, n_classes)
    return SplitResult(all_probs=probs.numpy().astype(np.float64), all_labels=np.asarray(labels, dtype=np.float64),
                       all_preds=preds.numpy().astype(np.float64), error=error, loss=loss, acc=acc)


@dataclass
class ValidationResult:
    """What ``validate_clam`` (utils/core_utils.py:506-597) accumulates over a split."""
    prob: np.ndarray             # [n, C] float64
    labels: np.ndarray           # [n] float64
    val_loss: float              # mean of loss_fn(logits_b, label_b).item()
    val_error: float             # mean of calculate_error(Y_hat, label)
    acc: List[dict] = field(default_factory=list)    # acc_logger.data: per bag class
    val_inst_loss: float = 0.0   # mean over the bags of instance_loss.item()
    inst_count: int = 0
    inst: List[dict] = field(default_factory=list)   # inst_logger.data, by the counting rule of Accuracy_Logger.log_batch


def validate_split(model, bags_or_loader, labels=None, n_classes: int = 2, loss_fn: Optional[Callable] = None,
                   max_rows_per_call: int = DEFAULT_MAX_ROWS, mb_one_call: bool = True, narrow_one_call: bool = True,
                   wide_one_call: bool = False, many_one_call: bool = False) -> ValidationResult:
    """The numbers of ``validate_clam`` for ``model`` on a split, with ``model.forward_bags(..., label=, instance_eval=True)`` called on
    runs of at most ``max_rows_per_call`` rows (``chunk_bags``) instead of ``model(bag, label=, instance_eval=True)`` once per slide.
    Arguments as :func:`evaluate_split`.  A ``CLAM_MB`` model runs with ``bags_one_call = mb_one_call`` for the duration of the call,
    a ``CLAM_SB`` with ``bags_narrow = narrow_one_call``: for the narrow heads (``hipt_smaller``, ``hipt_smallest``, ...) the numbers
    then come from the one-call kernel; they equal the loop's (``narrow_one_call=False``) within the fp32 bar (1e-4), not bit for bit.
    ``wide_one_call`` as in :func:`evaluate_split` (the wide heads; the default keeps the model's own ``bags_wide``).  A ``CLAM_MB`` at
    the wide widths with 2 to 4 classes takes ``hipt_clam_mb_forward_bags_wide`` when both hold: ``mb_one_call`` (set here, default True)
    and ``bags_wide`` (``wide_one_call=True`` or the model's own); its numbers equal the loop's within the fp32 bar in fp32, not bit for bit.
    ``many_one_call`` as in :func:`evaluate_split`: ``True`` sets ``bags_one_call`` and ``bags_many`` for the call, whatever ``mb_one_call``
    says, and a ``CLAM_MB`` with 5 to 8 classes at the widths of ``hipt_clam_mb_forward_bags`` takes ``hipt_clam_mb_forward_bags_many``;
    the default keeps the model's own ``bags_many`` (default False: the loop).
    The AUC stays with the caller (``labels`` and ``prob`` are its inputs).  The model is put in eval mode, as ``validate_clam`` does."""
    bags, labels, loss_fn, dev, (logits, probs, preds) = _prepare(model, bags_or_loader, labels, n_classes, loss_fn)
    n = len(bags)
    inst_loss = torch.empty((n,), dtype=torch.float32)
    inst = [{"count": 0, "correct": 0} for _ in range(n_classes)]
    model.eval()
    # (bags_one_call = mb_one_call first: many_one_call overrides it)
    with torch.no_grad(), _switches(model, {"bags_one_call": mb_one_call, **_split_switches(narrow_one_call, wide_one_call, many_one_call)}):
        for run in chunk_bags([b.shape[0] for b in bags], max_rows_per_call):
            out = model.forward_bags([bags[i].to(dev) for i in run], label=[labels[i] for i in run], instance_eval=True)
            _copy_back(run, out, logits, probs, preds)
            res = out[4]
            inst_loss[run.start:run.stop] = res["instance_loss"].float().cpu()
            for p, t in zip(res["inst_preds"], res["inst_labels"]):     # Accuracy_Logger.log_batch, one slide at a time
                p, t = np.asarray(p).astype(int), np.asarray(t).astype(int)
                for c in np.unique(t):
                    mask = t == c
                    inst[c]["count"] += int(mask.sum())
                    inst[c]["correct"] += int((p[mask] == t[mask]).sum())
        loss = _mean_loss(loss_fn, logits, labels)
    acc, error = _tally(preds, labels, n_classes)
    return ValidationResult(prob=probs.numpy().astype(np.float64), labels=np.asarray(labels, dtype=np.float64), val_loss=loss,
                            val_error=error, acc=acc, val_inst_loss=sum(float(v) for v in inst_loss) / n, inst_count=n, inst=inst)


def validate_clam_like(ref_module, max_rows_per_call: int = DEFAULT_MAX_ROWS) -> Callable:
    """A function with the signature and the four results of ``ref_module.validate_clam`` (``utils.core_utils``) whose numbers come
    from :func:`validate_split`: the writer scalars and the early-stopping call (checkpoint name, early_stopping file) included;
    one line is printed per call.  The AUC and the logger
    objects are made with that module's own imports (sklearn, ``Accuracy_Logger``)."""
    m = ref_module

    def validate_clam(cur, epoch, model, loader, n_classes, early_stopping=None, writer=None, loss_fn=None, results_dir=None):
        import os
        r = validate_split(model, loader, None, n_classes, loss_fn, max_rows_per_call)
        acc_logger, inst_logger = m.Accuracy_Logger(n_classes=n_classes), m.Accuracy_Logger(n_classes=n_classes)
        acc_logger.data = [dict(d) for d in r.acc]
        inst_logger.data = [dict(d) for d in r.inst]
        if n_classes == 2:
            auc = m.roc_auc_score(r.labels, r.prob[:, 1])
        else:
            onehot = m.label_binarize(r.labels, classes=list(range(n_classes)))
            per = []
            for c in range(n_classes):
                if c in r.labels:
                    fpr, tpr, _ = m.roc_curve(onehot[:, c], r.prob[:, c])
                    per.append(m.calc_auc(fpr, tpr))
                else:
                    per.append(float("nan"))
            auc = np.nanmean(np.array(per))
        scalars = {"val/loss": r.val_loss, "val/auc": auc, "val/error": r.val_error, "val/inst_loss": r.val_inst_loss}
        for c in range(n_classes):
            a = acc_logger.get_summary(c)[0]
            if a is not None:
                scalars[f"val/class_{c}_acc"] = a
        print(f"validation {epoch}: loss {r.val_loss:.4f} error {r.val_error:.4f} auc {auc:.4f} instance loss {r.val_inst_loss:.4f}; "
              "bags " + " ".join(f"{d['correct']}/{d['count']}" for d in r.acc) + "; instances " +
              " ".join(f"{d['correct']}/{d['count']}" for d in r.inst[:2]))
        if writer:
            for name, v in scalars.items():
                writer.add_scalar(name, v, epoch)
        if early_stopping:
            assert results_dir
            early_stopping(epoch, r.val_loss, model, ckpt_name=os.path.join(results_dir, "s_{}_checkpoint.pt".format(cur)))
            if early_stopping.early_stop:
                with open(os.path.join(results_dir, "early_stopping{}.txt".format(cur)), "w") as f:
                    f.write("Finished at epoch {}".format(epoch))
                print("Early stopping")
                return True, r.val_error, r.val_loss, auc
        return False, r.val_error, r.val_loss, auc

    validate_clam.__hipt_amd__ = True
    return validate_clam


def summary_like(ref_module, max_rows_per_call: int = DEFAULT_MAX_ROWS) -> Callable:
    """A function with the signature and the five results of ``ref_module.summary`` (``utils.eval_utils``) whose numbers come from
    ``evaluate_split``.  The AUC, the data frame and the logger object are made with that module's own imports (sklearn, pandas,
    ``Accuracy_Logger``), from the arrays ``evaluate_split`` returns."""
    m = ref_module

    def summary(model, loader, args, loss_fn=None):
        model.eval()
        C = args.n_classes
        r = evaluate_split(model, loader, None, C, loss_fn, max_rows_per_call)
        logger = m.Accuracy_Logger(n_classes=C)
        logger.data = [dict(d) for d in r.acc]
        if len(np.unique(r.all_labels)) == 1:
            score = -1
        elif C == 2:
            score = m.roc_auc_score(r.all_labels, r.all_probs[:, 1])
        else:
            onehot = m.label_binarize(r.all_labels, classes=list(range(C)))
            if args.micro_average:
                fpr, tpr, _ = m.roc_curve(onehot.ravel(), r.all_probs.ravel())
                score = m.auc(fpr, tpr)
            else:
                per = []
                for c in range(C):
                    if c in r.all_labels:
                        fpr, tpr, _ = m.roc_curve(onehot[:, c], r.all_probs[:, c])
                        per.append(m.auc(fpr, tpr))
                    else:
                        per.append(float("nan"))
                score = np.nanmean(np.array(per))
        table = {"slide_id": loader.dataset.slide_data["slide_id"], "Y": r.all_labels, "Y_hat": r.all_preds}
        table.update({f"p_{c}": r.all_probs[:, c] for c in range(C)})
        return r.error, score, m.pd.DataFrame(table), logger, r.loss

    summary.__hipt_amd__ = True
    return summary
