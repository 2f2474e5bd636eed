"""fp64 ground truth of the CLAM training step (csrc/clam_train.hip; models/model_clam.py:147-191, 226-264; utils/core_utils.py:300-348)
and a hand-written fp64 backward that carries wrong-kernel variants.  tests/test_clam_train_ref.py holds the two to each other on the
CPU, measures the fp32 noise floor the bars are made of and checks that every variant clears them; tests/test_gpu_clam_train_units.py
runs the kernels against `truth` under those bars.

  truth(inp)            oracle.torch_cpu.clam_forward_train in float64 and autograd of

                            total = bag_weight CE(logits) + (1 - bag_weight) instance_loss + <cA, A_raw> + <cM, features>

                        (cA [K, N], cM [K, S1]: fixed hash-generated coefficients, None = the plain loss; without the instance branch
                        total = CE + the two products, as the training loop has it).  `autograd_step(inp, torch.float32)` is the same
                        in fp32: the noise floor.
  restated(inp, variant) the backward written out with the kernels' own formulas, float64, no autograd.  With variant=None it equals
                        `truth` to 1e-10; each variant is one plausible slip at a named line of clam_train.hip (VARIANTS).
  Case / inputs(case)   the shapes and options of the GPU cases (CASES) and their inputs: the standard `synth` weights or the EDGE
                        family (saturated gates, half of h1 exactly zero, A_raw over +-40: a peaky softmax).

Line numbers are those of csrc/clam_train.hip."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from hipt_abmil_atec23_amd import synth
from oracle import torch_cpu as TO

EPS32 = float(np.finfo(np.float32).eps)
BAG_WEIGHT = 0.7
DROP_P = 0.25
POOL_SPLIT_N, POOL_ROWS, TR = 4096, 512, 16  # :222, :31
EDGE_GATE_SCALE = 20.0   # Wa, Wb, ba, bb: pre-activations of std ~10, beyond +-30 at 3 sigma
EDGE_A_SPAN = 40.0       # max |A_raw - bc| after wc is rescaled
RELU_MARGIN = 4e-6       # ~40 x the fp32 round-off of a ReLU pre-activation (eps sqrt(S0) rms(x w) ~ 1e-7)

VARIANTS = OrderedDict([
    ("no_dA_ext", "the gradient arriving on A_raw is never added (:466)"),
    ("no_dM_ext", "the gradient arriving on `features` is never added (:427)"),
    ("dotM_wrap", "branches k >= 4 read dotM[k - 4] (:434)"),
    ("cls_wrap", "classes c >= 4 take the logit / M row of class c - 4 (:352, :621)"),
    ("sel_once", "a row selected twice gets its instance gradient once (:519)"),
    ("sel_unmasked", "the scattered instance rows bypass m1 [h1 > 0] (:524)"),
    ("gate_mask_fwd_only", "ma / mb missing from du / dv (:497-498)"),
    ("tail_tile", "the rows of the last partial 16-row tile missing from db1 / dwc / dbc"),
    ("split_tail", "the last row split's rows missing from dW1 / dWa / dWb (:569-570)"),
    ("pool_tail", "the last 512-row block missing from the long-bag pooling sums (:262)"),
])

# name, widths, rows, multi (CLAM_MB), classes (= branches of CLAM_MB), k_sample, subtyping, instance_eval, family, dropout, ext (cA / cM)
Case = namedtuple("Case", "name size n multi C k sub inst family drop ext")
BIG, TINY, SMALL, ODD, DEF = (192, 128, 64), (192, 8, 4), (32, 16, 8), (100, 132, 20), (1024, 512, 256)
# ODD: S0 = 100 is no multiple of 64 (a partial N-tile of the weight GEMMs), S1 = 132 is one 128-column pass of dot_rows + 4 and no power
# of two (CW = 256, RG = 1 in the pooling), S2 = 20 = 16 + 4 (a second trip of the :474 loop with four column groups live)
CASES = [
    Case("big_n1_sb", BIG, 1, False, 2, 1, False, True, "std", False, True),           # one row: p = 1, selected as top AND bottom
    Case("big_n15_sb", BIG, 15, False, 2, 8, False, True, "std", False, True),         # N < 2k: a row selected twice
    Case("big_n16_mb3", BIG, 16, True, 3, 8, True, True, "std", False, True),          # one full tile; branches share rows
    Case("big_n17_sb_drop", BIG, 17, False, 2, 8, False, True, "std", True, True),     # a one-row tail tile, masks
    Case("big_n100_sb_c5", BIG, 100, False, 5, 8, True, True, "std", False, True),     # 5 classes on one branch (:352 wraps)
    Case("big_n100_sb_plain", BIG, 100, False, 2, 8, False, True, "std", False, False),  # the plain loss (bc's gradient is zero)
    Case("big_n100_mb5", BIG, 100, True, 5, 8, True, True, "std", False, True),        # 5 branches (:434 wraps)
    Case("big_n100_mb8", BIG, 100, True, 8, 8, False, True, "std", False, True),       # KMAX branches, no subtyping
    Case("big_n100_sb_noinst", BIG, 100, False, 2, 8, False, False, "std", False, True),
    Case("tiny_n100_sb", TINY, 100, False, 2, 4, True, True, "std", False, True),
    Case("tiny_n17_mb3", TINY, 17, True, 3, 4, False, True, "std", False, True),
    Case("small_n37_mb5", SMALL, 37, True, 5, 4, True, True, "std", False, True),
    Case("small_n16_sb_c5", SMALL, 16, False, 5, 8, False, True, "std", False, True),
    Case("odd_n37_mb5_drop", ODD, 37, True, 5, 8, True, True, "std", True, True),
    Case("odd_n100_sb_drop", ODD, 100, False, 2, 8, False, True, "std", True, True),
    Case("odd_n17_mb8_noinst", ODD, 17, True, 8, 8, False, False, "std", False, True),
    Case("def_n33_sb", DEF, 33, False, 2, 8, False, True, "std", False, True),         # CLAM's own widths
    Case("big_n4096_sb", BIG, 4096, False, 2, 8, False, True, "std", False, True),     # the last single-workgroup size
    Case("big_n4097_mb3_drop", BIG, 4097, True, 3, 8, True, True, "std", True, True),  # both splits with a one-row tail, masks
    Case("big_n4097_sb", BIG, 4097, False, 2, 8, False, True, "std", False, True),
    Case("big_n8200_mb5", BIG, 8200, True, 5, 8, False, True, "std", False, True),     # three row splits, K > 1
    Case("odd_n4097_sb_c5", ODD, 4097, False, 5, 8, True, True, "std", False, True),
    Case("edge_big_n100_sb", BIG, 100, False, 2, 8, False, True, "edge", False, True),
    Case("edge_big_n4097_mb3", BIG, 4097, True, 3, 8, True, True, "edge", False, True),
    Case("edge_odd_n37_mb5", ODD, 37, True, 5, 8, True, True, "edge", False, True),
]
BY_NAME = {c.name: c for c in CASES}
# the case(s) each variant is designed for: there it must land >= 3 x beyond a bar on some tensor
VARIANT_CASES = {
    "no_dA_ext": ("big_n100_mb5", "big_n4097_sb"),
    "no_dM_ext": ("big_n100_mb5", "big_n4097_sb"),
    "dotM_wrap": ("big_n100_mb5", "big_n100_mb8", "big_n8200_mb5"),
    "cls_wrap": ("big_n100_sb_c5", "big_n100_mb8", "odd_n4097_sb_c5"),
    "sel_once": ("big_n1_sb", "big_n15_sb", "big_n16_mb3"),
    "sel_unmasked": ("big_n15_sb", "big_n17_sb_drop"),
    "gate_mask_fwd_only": ("big_n17_sb_drop", "odd_n37_mb5_drop", "big_n4097_mb3_drop"),
    "tail_tile": ("big_n17_sb_drop", "tiny_n17_mb3", "big_n4097_sb"),
    "split_tail": ("big_n4097_mb3_drop", "big_n8200_mb5"),
    "pool_tail": ("big_n4097_sb", "edge_big_n4097_mb3"),
}
SELECTED_TWICE = ("big_n1_sb", "big_n15_sb", "big_n16_mb3")

# tensors a comparison reports, by KIND (CLAM_MB's per-class classifiers and the instance classifiers share one bar per kind)
OUT_KINDS = ("logits", "A_raw", "M", "loss")
GRAD_KINDS = ("W1", "b1", "Wa", "ba", "Wb", "bb", "wc", "bc", "wcls", "bcls", "winst", "binst", "bag")
KINDS = OUT_KINDS + GRAD_KINDS


def group_of(case):
    """the bars' groups: the edge family, long bags (N > 4096: split pooling and weight reduction, fp32 atomics), short bags"""
    return "edge" if case.family == "edge" else ("long" if case.n > POOL_SPLIT_N else "short")


def kind_of(name):
    if name in OUT_KINDS or name == "bag":
        return name
    w = name.endswith("weight")
    if name.startswith("instance_classifiers"):
        return "winst" if w else "binst"
    if name.startswith("classifiers"):
        return "wcls" if w else "bcls"
    if name.startswith("attention_net.0."):
        return "W1" if w else "b1"
    for tag, kw, kb in (("attention_a", "Wa", "ba"), ("attention_b", "Wb", "bb"), ("attention_c", "wc", "bc")):
        if tag in name:
            return kw if w else kb
    raise KeyError(name)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
class Inputs:
    """case, p (name -> fp32 numpy, the module's state dict), bag [N, S0] fp32, masks (m1, ma, mb) fp32 or None, cA / cM fp32 or None, label"""

    def __init__(self, case, p, bag, masks, cA, cM, label):
        self.case, self.p, self.bag, self.masks, self.cA, self.cM, self.label = case, p, bag, masks, cA, cM, label
        self.bag_weight = BAG_WEIGHT if case.inst else 1.0

    @property
    def K(self):
        return self.case.C if self.case.multi else 1

    @property
    def pre(self):
        return f"attention_net.{3 if self.case.drop else 2}."

    def with_masks(self, masks):
        return Inputs(self.case, self.p, self.bag, masks, self.cA, self.cM, self.label)


def _seed(case):
    # (the one-row bag: its row is the positive AND the negative instance, d lg = (2 softmax(lg) - 1) / 2 -- seed 1000 draws an
    #  instance classifier with softmax(lg) = 0.5 +- 1e-3: a true gradient that is a 1000-fold cancellation, not a kernel's affair)
    return {"big_n1_sb": 1777}.get(case.name, 1000 + CASES.index(case) if case in CASES else 999)


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _fwd64(p, x, pre, masks=None):
    """(z1, h1, u, v, A_raw [K, N]) in float64 torch"""
    d = lambda a: torch.as_tensor(np.asarray(a)).double()
    z1 = x @ d(p["attention_net.0.weight"]).T + d(p["attention_net.0.bias"])
    h1 = torch.relu(z1)
    if masks is not None:
        h1 = h1 * masks[0].double()
    u = h1 @ d(p[pre + "attention_a.0.weight"]).T + d(p[pre + "attention_a.0.bias"])
    v = h1 @ d(p[pre + "attention_b.0.weight"]).T + d(p[pre + "attention_b.0.bias"])
    a, b = torch.tanh(u), torch.sigmoid(v)
    if masks is not None:
        a, b = a * masks[1].double(), b * masks[2].double()
    A = ((a * b) @ d(p[pre + "attention_c.weight"]).T + d(p[pre + "attention_c.bias"])).T
    return z1, h1, u, v, A


def hash_masks(case, seed):
    """scaled dropout masks (0 or 1 / (1 - p)) from the hash: what the CPU tests use where the module draws from torch's generator"""
    n, (_, s1, s2) = case.n, case.size
    mk = lambda cols, s: (synth.hash_uniform_torch((n, cols), s) >= 2.0 * DROP_P - 1.0).float() / (1.0 - DROP_P)
    return mk(s1, seed + 1), mk(s2, seed + 2), mk(s2, seed + 3)


def inputs(case, masks="hash"):
    """The inputs of a case.  masks: "hash" (hash_masks, dropout cases only), None, or a tuple of three tensors."""
    seed = _seed(case)
    s0 = case.size[0]
    K = case.C if case.multi else 1
    bag = synth.hash_uniform_torch((case.n, s0), seed)
    p = synth.make_params_np(synth.clam_param_specs(case.size, n_classes=case.C, multi=case.multi, dropout=case.drop), 190 + seed % 7)
    pre = f"attention_net.{3 if case.drop else 2}."
    if case.family == "edge":
        for nm in ("attention_a.0.weight", "attention_a.0.bias", "attention_b.0.weight", "attention_b.0.bias"):
            p[pre + nm] = p[pre + nm] * np.float32(EDGE_GATE_SCALE)
        z1 = _fwd64(p, bag.double(), pre)[0]
        # half of h1 exactly zero: b1 shifted by the median (the midpoint of the two middle values: no pre-activation AT zero)
        p["attention_net.0.bias"] = (p["attention_net.0.bias"].astype(np.float64) - float(np.median(z1.numpy()))).astype(np.float32)
        A = _fwd64(p, bag.double(), pre)[4]
        span = float((A - torch.as_tensor(p[pre + "attention_c.bias"]).double()[:, None]).abs().max())
        p[pre + "attention_c.weight"] = p[pre + "attention_c.weight"] * np.float32(EDGE_A_SPAN / span)
    # no ReLU pre-activation within RELU_MARGIN of zero: a unit that fp32 and fp64 put on different sides of the ReLU has two
    # different, equally valid gradients (one dz element in or out: ~1 / sqrt(N S1) of dW1, far beyond any round-off bar).  Columns
    # that hold such a unit get their bias moved by 3 margins until they hold none.
    b1 = p["attention_net.0.bias"]
    for _ in range(8):
        close = (_fwd64(p, bag.double(), pre)[0].abs() < RELU_MARGIN).any(dim=0).numpy()
        if not close.any():
            break
        b1[close] += np.float32(3 * RELU_MARGIN)
    if case.n > POOL_SPLIT_N and not case.drop:
        # long bags: branch 0's most attended row sits LAST, in the one-row tail of the split pooling (what pool_tail drops)
        top = int(_fwd64(p, bag.double(), pre)[4][0].argmax())
        idx = torch.arange(case.n)
        idx[top], idx[-1] = case.n - 1, top
        bag = bag[idx].contiguous()
    if masks == "hash":
        masks = hash_masks(case, seed) if case.drop else None
    cA = cM = None
    if case.ext:
        # scales that keep the external terms beside the loss's own: dA of the pooling is ~0.2 / N, dM of the classifier ~0.05
        cA = synth.hash_uniform_torch((K, case.n), seed + 11, scale=0.5 / case.n)
        cM = synth.hash_uniform_torch((K, case.size[1]), seed + 12, scale=0.05)
    return Inputs(case, p, bag, masks, cA, cM, label=case.C - 1)


# ---- ground truth: the oracle's forward, autograd ----------------------------------------------------------------------------------------
def autograd_step(inp, dtype=torch.float64):
    """-> (outputs, grads, aux): outputs logits / A_raw / M / loss (+ instance_loss, inst_preds), grads of every parameter by its
    state-dict name and "bag", aux["dA"] = d total / d A_raw [K, N].  All float64 numpy (computed in `dtype`)."""
    c = inp.case
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in inp.p.items()}
    h = inp.bag.to(dtype).clone().requires_grad_(True)
    masks = None if inp.masks is None else [m.to(dtype) for m in inp.masks]
    logits, _, _, a_raw, res = TO.clam_forward_train(h, p, c.C, c.multi, c.k, inp.label, c.inst, c.sub, masks)
    a_raw.retain_grad()
    total = F.cross_entropy(logits, torch.tensor([inp.label]))
    if c.inst:
        total = inp.bag_weight * total + (1 - inp.bag_weight) * res["instance_loss"]
    if inp.cA is not None:
        total = total + (inp.cA.to(dtype) * a_raw).sum() + (inp.cM.to(dtype) * res["features"]).sum()
    total.backward()
    n64 = lambda t: t.detach().double().numpy()
    out = dict(logits=n64(logits), A_raw=n64(a_raw), M=n64(res["features"]), loss=n64(total).reshape(1))
    if c.inst:
        out["instance_loss"], out["inst_preds"] = float(res["instance_loss"].detach()), res["inst_preds"].numpy()
    grads = {k: (n64(v.grad) if v.grad is not None else np.zeros(tuple(v.shape))) for k, v in p.items()}
    grads["bag"] = n64(h.grad)
    return out, grads, dict(dA=n64(a_raw.grad))


def truth(inp):
    return autograd_step(inp, torch.float64)


def evaluated_classes(case, label):
    """classes whose instance classifier the step uses (:156-178): the label's, all with subtyping, none without the branch"""
    if not case.inst:
        return ()
    return tuple(range(case.C)) if case.sub else (label,)


def zero_truth(inp, name):
    """is the TRUE gradient of this tensor zero?  attention_c.bias under the plain loss (softmax shift invariance); the
    instance classifiers of classes the step does not evaluate"""
    if name.startswith("instance_classifiers."):
        return int(name.split(".")[1]) not in evaluated_classes(inp.case, inp.label)
    return name.endswith("attention_c.bias") and inp.cA is None


def abs_bar(aux):
    """the absolute bar of a zero-gradient tensor: 64 eps_fp32 sum_n |dA[k, n]| (the largest branch)"""
    return 64.0 * EPS32 * float(np.abs(aux["dA"]).sum(axis=1).max())


def errors(got_out, got_grads, ref_out, ref_grads, inp):
    """per-tensor errors {name: (kind, value, absolute?)}: rel-L2 against the reference, max |x| where the true gradient is zero"""
    e = OrderedDict()
    for k in OUT_KINDS:
        e[k] = (k, _rel(np.asarray(got_out[k], np.float64).reshape(-1), ref_out[k].reshape(-1)), False)
    for k, r in ref_grads.items():
        g = np.asarray(got_grads[k], np.float64)
        assert g.shape == r.shape, (k, g.shape, r.shape)
        if zero_truth(inp, k):
            e[k] = (kind_of(k), float(np.abs(g).max()), True)
        else:
            e[k] = (kind_of(k), _rel(g.reshape(-1), r.reshape(-1)), False)
    return e


def worst_ratio(errs, bars, aux):
    """(max over tensors of error / bar, the tensor)"""
    worst, at = 0.0, None
    for name, (kind, v, absolute) in errs.items():
        r = v / (abs_bar(aux) if absolute else bars[kind])
        if r > worst:
            worst, at = r, name
    return worst, at


# ---- the conditions a case's inputs must meet ---------------------------------------------------------------------------------------------
def topk_sets(inp, A):
    """[(branch, sign, ids, gap)] of every top-k the step takes: gap = k-th minus (k+1)-th score (inf where k = N)"""
    c = inp.case
    sets = []
    for cl in evaluated_classes(c, inp.label):
        b = cl if c.multi else 0
        for sign in ((1, -1) if cl == inp.label else (1,)):
            v, ids = torch.sort(sign * A[b], descending=True, stable=True)
            gap = float(v[c.k - 1] - v[c.k]) if c.k < c.n else float("inf")
            sets.append((b, sign, ids[:c.k].clone(), gap))
    return sets


def conditions(inp):
    """what the input-condition assertions read, from the fp64 forward"""
    z1, h1, u, v, A = _fwd64(inp.p, inp.bag.double(), inp.pre, inp.masks)
    sets = topk_sets(inp, A)
    rows = torch.cat([s[2] for s in sets]) if sets else torch.zeros(0, dtype=torch.int64)
    gate = torch.cat([u.reshape(-1), v.reshape(-1)]).abs()
    return dict(min_abs_z1=float(z1.abs().min()), min_gap=min([s[3] for s in sets], default=float("inf")), selected_twice=int(rows.numel() - rows.unique().numel()),
                h1_zero=float((h1 == 0).double().mean()), gate_beyond_15=float((gate > 15).double().mean()), gate_max=float(gate.max()),
                p_max=float(torch.softmax(A, dim=1).max()), A_span=float(A.abs().max()))


# ---- the backward by hand, with the kernels' formulas ------------------------------------------------------------------------------------
def restated(inp, variant=None):
    """-> (outputs, grads) as autograd_step's, float64, no autograd; `variant`: one of VARIANTS"""
    assert variant is None or variant in VARIANTS, variant
    c, p, pre, K, C = inp.case, inp.p, inp.pre, inp.K, inp.case.C
    N, (S0, S1, S2) = c.n, c.size
    d = lambda a: torch.as_tensor(np.asarray(a)).double()
    x = inp.bag.double()
    W1, Wa, Wb = d(p["attention_net.0.weight"]), d(p[pre + "attention_a.0.weight"]), d(p[pre + "attention_b.0.weight"])
    wc = d(p[pre + "attention_c.weight"])
    one = torch.ones((), dtype=torch.float64)
    m1, ma, mb = (one, one, one) if inp.masks is None else [m.double() for m in inp.masks]
    if c.multi:
        wcls = torch.cat([d(p[f"classifiers.{k}.weight"]) for k in range(C)])
        bcls = torch.cat([d(p[f"classifiers.{k}.bias"]) for k in range(C)])
    else:
        wcls, bcls = d(p["classifiers.weight"]), d(p["classifiers.bias"])
    # ---- forward (F1, F2)
    z1, h1, u, v, A = _fwd64(p, x, pre, inp.masks)
    t, s = torch.tanh(u), torch.sigmoid(v)
    ad, bd = t * ma, s * mb
    g = ad * bd
    e = torch.exp(A - A.max(dim=1, keepdim=True)[0])
    pooled = torch.ones(N, dtype=torch.bool)
    if variant == "pool_tail" and N > POOL_SPLIT_N:
        pooled[((N - 1) // POOL_ROWS) * POOL_ROWS:] = False
    se = (e * pooled).sum(dim=1, keepdim=True)
    prob = e / se                               # what the backward recomputes from stats (:464)
    M = ((e * pooled) / se) @ h1                # [K, S1]
    logits = (wcls * (M if c.multi else M[0:1])).sum(dim=1) + bcls
    if variant == "cls_wrap":
        logits = torch.cat([logits[:4], logits[:C - 4]]) if C > 4 else logits
    # ---- the instance branch: slots [K][2][k] of ids, the gradient arriving on the gathered rows
    dsel = torch.zeros((K, 2, c.k if c.inst else 0, S1), dtype=torch.float64)
    ids = torch.zeros((K, 2, c.k if c.inst else 0), dtype=torch.int64)
    grads, inst_loss, preds = {}, 0.0, []
    for k in range(K if c.inst else 0):
        ids[k, 0] = torch.sort(A[k], descending=True, stable=True)[1][:c.k]
        ids[k, 1] = torch.sort(-A[k], descending=True, stable=True)[1][:c.k]
    for cl in range(C):
        wi, bi = d(p[f"instance_classifiers.{cl}.weight"]), d(p[f"instance_classifiers.{cl}.bias"])
        grads[f"instance_classifiers.{cl}.weight"], grads[f"instance_classifiers.{cl}.bias"] = torch.zeros_like(wi), torch.zeros_like(bi)
        if cl not in evaluated_classes(c, inp.label):
            continue
        b = cl if c.multi else 0
        both = cl == inp.label
        rows = torch.cat([ids[b, 0], ids[b, 1]]) if both else ids[b, 0]
        tg = torch.cat([torch.ones(c.k), torch.zeros(c.k)]).long() if both else torch.zeros(c.k).long()
        lg = h1[rows] @ wi.T + bi
        w_inst = (1 - inp.bag_weight) / (C if c.sub else 1)
        inst_loss = inst_loss + F.cross_entropy(lg, tg) / (C if c.sub else 1)
        preds.append(lg.argmax(dim=1))
        dlg = w_inst * (torch.softmax(lg, dim=1) - F.one_hot(tg, 2).double()) / rows.numel()
        grads[f"instance_classifiers.{cl}.weight"] = dlg.T @ h1[rows]
        grads[f"instance_classifiers.{cl}.bias"] = dlg.sum(dim=0)
        drows = dlg @ wi
        dsel[b, 0] += drows[:c.k]
        if both:
            dsel[b, 1] += drows[c.k:]
    ce = F.cross_entropy(logits.view(1, -1), torch.tensor([inp.label]))
    total = inp.bag_weight * ce + (1 - inp.bag_weight) * inst_loss if c.inst else ce
    if inp.cA is not None:
        total = total + (inp.cA.double() * A).sum() + (inp.cM.double() * M).sum()
    # ---- B1
    dlogits = inp.bag_weight * (torch.softmax(logits, dim=0) - F.one_hot(torch.tensor(inp.label), C).double())
    dM = dlogits[:, None] * wcls if c.multi else (dlogits[None, :] @ wcls)      # [K, S1]
    if inp.cM is not None and variant != "no_dM_ext":
        dM = dM + inp.cM.double()
    dotM = (dM * M).sum(dim=1)
    if variant == "dotM_wrap" and K > 4:
        dotM = torch.cat([dotM[:4], dotM[:K - 4]])
    dA = prob * (dM @ h1.T - dotM[:, None])                                        # [K, N]
    if inp.cA is not None and variant != "no_dA_ext":
        dA = dA + inp.cA.double()
    dg = dA.T @ wc                                                                 # [N, S2]
    fa, fb = (one, one) if variant == "gate_mask_fwd_only" else (ma, mb)
    du = dg * bd * fa * (1 - t * t)
    dv = dg * ad * fb * s * (1 - s)
    dh1 = prob.T @ dM + du @ Wa + dv @ Wb
    scat = torch.zeros_like(dh1)
    flat_ids, flat_d = ids.reshape(-1), dsel.reshape(-1, S1)
    seen = set()
    for eidx in range(flat_ids.numel()):
        r = int(flat_ids[eidx])
        if variant == "sel_once" and r in seen:
            continue
        seen.add(r)
        scat[r] += flat_d[eidx]
    live = m1 * (h1 > 0).double()
    dz = dh1 * live + scat if variant == "sel_unmasked" else (dh1 + scat) * live
    # ---- B2
    full = torch.ones(N, dtype=torch.float64)
    tile = full.clone()
    if variant == "tail_tile" and N % TR:
        tile[(N // TR) * TR:] = 0
    split = full.clone()
    if variant == "split_tail" and N > 4096:
        nsplit = min((N + 4095) // 4096, 64)
        per = (N + nsplit - 1) // nsplit
        split[(nsplit - 1) * per:] = 0
    grads["attention_net.0.weight"] = (dz * split[:, None]).T @ x
    grads["attention_net.0.bias"] = (dz * tile[:, None]).sum(dim=0)
    grads[pre + "attention_a.0.weight"] = (du * split[:, None]).T @ h1
    grads[pre + "attention_a.0.bias"] = du.sum(dim=0)
    grads[pre + "attention_b.0.weight"] = (dv * split[:, None]).T @ h1
    grads[pre + "attention_b.0.bias"] = dv.sum(dim=0)
    grads[pre + "attention_c.weight"] = (dA * tile) @ g
    grads[pre + "attention_c.bias"] = (dA * tile).sum(dim=1)
    if c.multi:
        for cl in range(C):
            row = cl - 4 if (variant == "cls_wrap" and cl >= 4) else cl
            grads[f"classifiers.{cl}.weight"] = (dlogits[cl] * M[row]).view(1, S1)
            grads[f"classifiers.{cl}.bias"] = dlogits[cl].view(1)
    else:
        grads["classifiers.weight"] = dlogits[:, None] * M[0][None, :]
        grads["classifiers.bias"] = dlogits
    grads["bag"] = dz @ W1
    n64 = lambda a: a.detach().double().numpy()
    out = dict(logits=n64(logits).reshape(1, -1), A_raw=n64(A), M=n64(M), loss=n64(total).reshape(1))
    if c.inst:
        out["instance_loss"], out["inst_preds"] = float(inst_loss), torch.cat(preds).numpy()
    return out, {k: n64(v) for k, v in grads.items()}
