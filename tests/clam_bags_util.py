"""What the GPU tests of the multi-bag CLAM forward share (tests/test_gpu_clam_bags.py, test_gpu_clam_narrow.py,
test_gpu_clam_validate.py): models and bags made from ``synth``, the per-bag references and the comparison helpers.  A plain
module; each test file binds its own defaults (its ``ROWS``, its model class)."""
import functools

import numpy as np
import torch

import clam_mb_ref as R
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, synth
from oracle import hipt_oracle as O

DEV = "cuda:0"
TOL = 1e-4           # the project's fp32 bar (tests/test_gpu_parity.py)
OUTS = ("A_raw", "M", "logits", "Y_prob")
FENCE, FILL = 4096, 0xA5


def md(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a.astype(np.float64).reshape(-1) - np.asarray(b, dtype=np.float64).reshape(-1)).max())


def bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def make(size, dtype="fp32", cls=CLAM_SB, n_classes=2, subtyping=False, one_call=False):
    m = cls(size_arg=list(size), n_classes=n_classes, subtyping=subtyping)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=n_classes, multi=cls is CLAM_MB), size[0]), strict=True)
    m.relocate()
    if one_call:
        m.bags_one_call = True   # (an instance attribute; CLAM_SB ignores it)
    return m.eval().set_compute_dtype(dtype)


@functools.lru_cache(maxsize=None)
def params64(size, n_classes=2, multi=False, rounded=False):
    out = {}
    for k, v in synth.make_params_np(synth.clam_param_specs(size, n_classes=n_classes, multi=multi), size[0]).items():
        if rounded and k.endswith("weight") and ("attention_net.0." in k or "attention_a" in k or "attention_b" in k):
            v = torch.from_numpy(np.ascontiguousarray(v)).bfloat16().float().numpy()   # what the kernels read in bf16 mode
        out[k] = v.astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def bags_of(s0, seed, rows):
    cat = synth.hash_uniform_torch((sum(rows), s0), seed, device=DEV)
    return tuple(cat.split(list(rows), dim=0))


@functools.lru_cache(maxsize=None)
def reference(size, seed, rows, rounded=False, n_classes=2, multi=False):
    """Every bag ALONE (fp64 where ``rounded``: on the bf16-rounded bag and weights) through the oracle, or, ``multi``, through the
    fp64 restatement of CLAM_MB (tests/clam_mb_ref.py)."""
    bags = bags_of(size[0], seed, rows)
    if multi:
        p = params64(size, n_classes, True, rounded)
        return [R.clam_mb_forward((b.bfloat16() if rounded else b).double().cpu().numpy(), p) for b in bags]
    p = params64(size, rounded=True) if rounded else synth.make_params_np(synth.clam_param_specs(size), size[0])
    return [O.clam_sb_forward((b.bfloat16().double() if rounded else b).cpu().numpy(), p) for b in bags]


def per_bag(out, b, multi=False):
    """Bag ``b`` of a call's outputs, in the shapes of its reference: M ``[1, S1]``, or ``[K, S1]`` for the ``multi`` form"""
    return {"A_raw": out["A_raw"][b], "M": out["M"][b] if multi else out["M"][b:b + 1], "logits": out["logits"][b:b + 1],
            "Y_prob": out["Y_prob"][b:b + 1], "Y_hat": out["Y_hat"][b:b + 1]}


def errors(out, refs, multi=False):
    """worst |error| per output over the bags, and the bags whose Y_hat differs"""
    worst, wrong = {k: 0.0 for k in OUTS}, []
    for b, r in enumerate(refs):
        got = per_bag(out, b, multi)
        for k in OUTS:
            assert tuple(got[k].shape) == r[k].shape, (k, got[k].shape, r[k].shape)
            worst[k] = max(worst[k], md(got[k], r[k]))
        if int(got["Y_hat"].reshape(-1)[0]) != int(np.asarray(r["Y_hat"]).reshape(-1)[0]):
            wrong.append(b)
    return worst, wrong


def assert_same_bits(a, b, what):
    for k in (*OUTS, "Y_hat"):
        assert a[k].shape == b[k].shape and bits(a[k]) == bits(b[k]), f"{what}: {k} differs"
