"""``CLAM_MB.forward`` in eval mode (models/model_clam.py:226-264) restated in numpy, in the dtype of its inputs (the tests hand it
float64), with the instance branch (:116-145, :234-245).  Built from the oracle's own pieces (``linear``, ``attn_net_gated``, ``softmax``,
``topk_desc``) and pinned against the reference module's outputs in tests/test_clam_validate_host.py."""
import numpy as np

from oracle.hipt_oracle import _gate_index, attn_net_gated, linear, softmax, topk_desc


def cross_entropy(lg, tgt):
    """nn.CrossEntropyLoss (mean) of logits [n, 2] against int targets [n]."""
    ls = lg - lg.max(axis=1, keepdims=True)
    lse = np.log(np.exp(ls).sum(axis=1))
    return float(np.mean(lse - ls[np.arange(len(tgt)), tgt]))


def instance_branch(A, h1, p, label, k_sample, subtyping, multi):
    """The loop of :156-178 / :234-245 over the instance classifiers: classes ascending; class c reads branch c (``multi``) or branch 0.
    Returns dict(instance_loss, inst_ids [per evaluated class], inst_preds, inst_labels)."""
    n_classes = sum(1 for k in p if k.startswith("instance_classifiers.") and k.endswith(".weight"))
    total, ids, preds, labels = 0.0, [], [], []
    for c in range(n_classes):
        a = A[c if multi else 0]
        if int(label) == c:
            tp, tn = topk_desc(a, k_sample), topk_desc(-a, k_sample)
            sel, tgt = np.concatenate([tp, tn]), np.concatenate([np.ones(k_sample, np.int64), np.zeros(k_sample, np.int64)])
        elif subtyping:
            sel, tgt = topk_desc(a, k_sample), np.zeros(k_sample, np.int64)
        else:
            continue
        lg = linear(h1[sel], p[f"instance_classifiers.{c}.weight"], p[f"instance_classifiers.{c}.bias"])
        total += cross_entropy(lg, tgt)
        ids.append(sel)
        preds.append(np.argmax(lg, axis=1))     # torch.topk(logits, 1): the first maximum
        labels.append(tgt)
    if subtyping:
        total /= n_classes
    return dict(instance_loss=total, inst_ids=ids, inst_preds=np.concatenate(preds), inst_labels=np.concatenate(labels))


def clam_mb_forward(h, p, k_sample=8, label=None, instance_eval=False, subtyping=False):
    """dict(logits [1, K], Y_prob [1, K], Y_hat [1, 1] int64, A_raw [K, N], M [K, S1]) and, with ``instance_eval``, the results of
    :func:`instance_branch`."""
    g = _gate_index(p)
    h1 = np.maximum(linear(h, p["attention_net.0.weight"], p["attention_net.0.bias"]), 0)
    A, _ = attn_net_gated(h1, p, f"attention_net.{g}.")
    A_raw = A.T                                   # [K, N]
    A = softmax(A_raw, axis=1)
    res = instance_branch(A, h1, p, label, k_sample, subtyping, True) if instance_eval else {}
    M = A @ h1                                    # [K, S1]
    K = A_raw.shape[0]
    logits = np.stack([linear(M[c:c + 1], p[f"classifiers.{c}.weight"], p[f"classifiers.{c}.bias"])[0, 0] for c in range(K)]).reshape(1, K)
    res.update(logits=logits, Y_prob=softmax(logits, axis=1), Y_hat=topk_desc(logits[0], 1).reshape(1, 1).astype(np.int64), A_raw=A_raw, M=M)
    return res
