"""The fp64 reference of the wide-head multi-bag CLAM_MB forward (csrc/abmil_wide_mb.hip; tests/test_gpu_clam_wide_mb.py):
``clam_mb_ref.clam_mb_forward`` with the rounding model of tests/clam_wide_ref.py applied per branch.  In bf16 mode the bag, W1, Wa and
Wb are bf16 values (``clam_bags_util.params64(..., rounded=True)`` and a bf16-rounded bag); h1 = ReLU(X W1^T + b1) is rounded to bf16
ONLY as the operand of the gate's two linear layers; the gate, the K scores, the K softmaxes and the K poolings M[k] = softmax(A[k]) h1
use unrounded h1.  ``round_h1=False`` (fp32 mode) rounds nothing: the function is then ``clam_mb_forward`` itself.  CPU only, fp64."""
import functools

import numpy as np

import clam_bags_util as U
from clam_wide_ref import bags_host, bf16_round
from oracle import hipt_oracle as O


def forward(h: np.ndarray, p: dict, round_h1: bool = True) -> dict:
    """``h``: the bag in fp64 (bf16-rounded where ``round_h1``); ``p``: ``clam_bags_util.params64(size, K, True, rounded=round_h1)``.
    The keys of ``clam_mb_ref.clam_mb_forward`` without the instance branch: logits [1, K], Y_prob [1, K], Y_hat [1, 1], A_raw [K, N],
    M [K, S1]."""
    g = O._gate_index(p)
    h1 = np.maximum(O.linear(h, p["attention_net.0.weight"], p["attention_net.0.bias"]), 0)
    A, _ = O.attn_net_gated(bf16_round(h1) if round_h1 else h1, p, f"attention_net.{g}.")   # the gate GEMM's operand is the only rounded copy
    A_raw = A.T                                   # [K, N]
    M = O.softmax(A_raw, axis=1) @ h1             # [K, S1], on unrounded h1
    K = A_raw.shape[0]
    logits = np.stack([O.linear(M[c:c + 1], p[f"classifiers.{c}.weight"], p[f"classifiers.{c}.bias"])[0, 0] for c in range(K)]).reshape(1, K)
    return {"logits": logits, "Y_prob": O.softmax(logits, axis=1), "Y_hat": O.topk_desc(logits[0], 1).reshape(1, 1).astype(np.int64),
            "A_raw": A_raw, "M": M}


def logit_gap(r: dict) -> float:
    """distance between the two largest logits of a bag's reference"""
    return float(np.diff(np.sort(r["logits"].reshape(-1))[-2:])[0])


@functools.lru_cache(maxsize=None)
def reference(size, seed, rows, n_classes=2, rounded=False, host=False):
    """Every bag alone through :func:`forward`.  ``rounded``: the bf16 model; ``host``: the bags are made on the CPU (bit-equal to the
    device's)."""
    bags = bags_host(size[0], seed, rows) if host else U.bags_of(size[0], seed, rows)
    p = U.params64(size, n_classes, True, rounded)
    return [forward((b.bfloat16() if rounded else b).double().cpu().numpy(), p, rounded) for b in bags]
