"""CLAM / ABMIL aggregator host mirror (reference: ``models/model_clam.py``).

``CLAM_SB`` and ``Attn_Net_Gated`` keep the reference's constructor arguments, attributes and
state-dict keys (``attention_net.0.*``, ``attention_net.{2|3}.attention_{a,b}.0.*``,
``...attention_c.*``, ``classifiers.*``, ``instance_classifiers.{c}.*``), so checkpoints written by
``utils/core_utils.py`` load with ``strict=True`` after the key cleaning of
``utils/eval_utils.py:51-57``.  Inference forwards (no autograd) run as ONE fused HIP pass over
the bag (csrc/abmil.hip).

Training: a forward that must be differentiated (``main.py`` trains this module,
``utils/core_utils.py:300-348, 373-426``) or that has active dropout runs the TRAINING kernels
(csrc/clam_train.hip) behind a ``torch.autograd.Function``: two launches forward (rows; softmax pooling + classifier +
on-device top-k of the instance branch), two backward (rows; weight gradients), fp32, for ``CLAM_SB`` and the K-branch
``CLAM_MB`` alike.  Only the pieces the caller supplies as Python callables stay PyTorch ops: the instance classifiers'
``Linear(S1, 2)`` on the 2k gathered rows and ``instance_loss_fn`` (``SmoothTop1SVM`` in the reference's scripts).
Outside the HIP path, by design: the ungated ``Attn_Net`` variant (``gate=False``; SURVEY.md allows the fallback) and
bags that live on the CPU -- training or not -- which run the module's PyTorch-op sequence on the CPU: the reference picks
the CPU itself where no GPU is visible (``relocate``, models/model_clam.py:102-106; SURVEY.md 8b "CPU tensors -> CPU
restatement"), so ``main.py`` / ``eval.py`` still run there.  That is a property of where the CALLER put the tensors, never a
fallback: a bag on a HIP device always takes the kernels, and a missing library raises (``NativeLibraryError``).  The ViTs
have no CPU path at all.
"""
from __future__ import annotations

import ctypes as C_

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from . import functional as Fn
from ._host import WeightImageCache

SIZE_DICT = {"tinier3": [1024, 32, 8], "256": [256, 64, 16], "tinier_resnet18": [512, 64, 16],
             "tinier2_resnet18": [512, 32, 8], "tiny_resnet18": [512, 128, 32], "small_resnet18": [512, 256, 64],
             "tinier": [1024, 64, 16], "tiny128": [1024, 128, 32], "tiny": [1024, 256, 64], "small": [1024, 512, 256],
             "big": [1024, 512, 384], "hipt_big": [192, 128, 64], "hipt_medium": [192, 64, 32],
             "hipt_small": [192, 32, 16], "hipt_smaller": [192, 16, 8], "hipt_smallest": [192, 8, 4],
             # added for 384-d ViT-256 [CLS] bags (BASELINE configs 1 and 4; SURVEY.md §8d "384 sizing")
             "hipt_384": [384, 128, 64]}


def initialize_weights(module):
    """xavier-normal Linear weights, zero bias (utils/utils.py:217-225)."""
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_normal_(m.weight)
            m.bias.data.zero_()
        elif isinstance(m, nn.BatchNorm1d):
            nn.init.constant_(m.weight, 1)
            nn.init.constant_(m.bias, 0)


def _needs_autograd(module, *tensors) -> bool:
    if not torch.is_grad_enabled():
        return False
    return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in module.parameters())


def _all_on_cpu(module, x) -> bool:
    """The caller keeps module AND input on the CPU (what the reference's relocate() does where no GPU is visible)."""
    return not x.is_cuda and not any(p.is_cuda for p in module.parameters())


def _tree_sum(x):
    """Sum over the last dimension by halving it with elementwise additions: every output is the same sequence of roundings whatever
    the other dimensions hold."""
    while x.shape[-1] > 1:
        n = x.shape[-1]
        half = (n + 1) // 2
        lo, hi = x[..., :n // 2] + x[..., half:], x[..., n // 2:half]
        x = torch.cat([lo, hi], dim=-1) if n % 2 else lo
    return x[..., 0]


def _cast_shared(code, fc1, gated):
    """[Wa; Wb] and W1 in the compute dtype with their fp32 biases: what the K branches of ``CLAM_MB`` share (``fc1`` None: the head alone)."""
    wa, wb = gated.attention_a[0], gated.attention_b[0]
    keep = dict(wab=Fn.as_compute(torch.cat([wa.weight, wb.weight], dim=0), code), bab=Fn.f32c(torch.cat([wa.bias, wb.bias], dim=0)))
    if fc1 is not None:
        keep.update(w1=Fn.as_compute(fc1.weight, code), b1=Fn.f32c(fc1.bias))
    return keep


def _clam_weights(code, device, fc1, gated, wc, bc, wcls=None, bcls=None, n_classes=0, n_att=0, shared=None, bound=None, image=True):
    """One ``hipt_clam_weights`` (include/hipt_abmil.h) and the dict of tensors that keep its pointers alive.  ``fc1`` /
    ``gated``: the ``Linear(S0, S1)`` and the ``Attn_Net_Gated`` (``fc1`` None: the head alone, ``s0 = 0``, nothing pooled);
    ``wc`` / ``bc`` / ``wcls`` / ``bcls``: this struct's rows of ``attention_c`` and its bag classifier; ``shared``: an
    already-cast :func:`_cast_shared`; ``bound``: ``sum |wc|`` where the caller has read it back already."""
    keep = dict(_cast_shared(code, fc1, gated) if shared is None else shared, wc=Fn.f32c(wc), bc=Fn.f32c(bc))
    if wcls is not None:
        keep.update(wcls=Fn.f32c(wcls), bcls=Fn.f32c(bcls))
    w = N.ClamWeights()
    w.dtype, w.s0, w.s1, w.s2 = code, fc1.in_features if fc1 is not None else 0, gated.attention_a[0].in_features, gated.attention_a[0].out_features
    w.n_classes, w.n_att = n_classes, n_att
    for name, t in keep.items():
        setattr(w, name, t.data_ptr())
    if fc1 is None:
        return w, keep
    # |A_raw - bc| <= sum |wc_j| (tanh * sigmoid lies in (-1, 1)): lets the streaming kernel exponentiate against a fixed
    # shift instead of a running maximum (include/hipt_abmil.h, hipt_clam_weights.logit_bound); one tiny reduction per
    # set of weights, read back here once
    # (0 means "unknown" in the ABI: an all-zero attention_c -- a zero-initialised head -- has the bound 0 and still takes the
    #  streaming kernel through the smallest positive bound.  The read-back synchronises once per set of weights; pack outside
    #  a graph capture.)
    w.logit_bound = max(float(keep["wc"].abs().sum().item() if bound is None else bound), 1e-30)
    # the streaming kernel's LDS image of these weights (bf16 [384|192,128,64]): packed once here, copied straight by
    # LDS-DMA at every launch
    nb = N.lib().hipt_clam_stream_packed_bytes(C_.byref(w)) if image else 0
    if nb:
        keep["stream_pk"] = torch.empty(nb, dtype=torch.uint8, device=device)
        N.call("hipt_clam_stream_pack", C_.byref(w), N.ptr(keep["stream_pk"]), N.stream_ptr(device))
        w.stream_pk = keep["stream_pk"].data_ptr()
    return w, keep


class Attn_Net(nn.Module):
    """Ungated attention head (model_clam.py:15-31); plain PyTorch module (not on the HIP path)."""

    def __init__(self, L=1024, D=256, dropout=0.25, n_classes=1):
        super().__init__()
        layers = [nn.Linear(L, D), nn.Tanh()]
        if dropout > 0:
            layers.append(nn.Dropout(dropout))
        layers.append(nn.Linear(D, n_classes))
        self.module = nn.Sequential(*layers)

    def forward(self, x):
        return self.module(x), x


class Attn_Net_Gated(WeightImageCache, nn.Module):
    """Gated attention head (model_clam.py:41-64): A = (tanh(x Wa^T) * sigmoid(x Wb^T)) Wc^T."""

    def __init__(self, L=1024, D=256, dropout=0.0, n_classes=1):
        super().__init__()
        a = [nn.Linear(L, D), nn.Tanh()]
        b = [nn.Linear(L, D), nn.Sigmoid()]
        if dropout > 0:
            a.append(nn.Dropout(dropout))
            b.append(nn.Dropout(dropout))
        self.attention_a = nn.Sequential(*a)
        self.attention_b = nn.Sequential(*b)
        self.attention_c = nn.Linear(D, n_classes)
        self._init_host()

    def _torch_forward(self, x):
        return self.attention_c(self.attention_a(x).mul(self.attention_b(x))), x

    def _pack(self, device):
        c = self.attention_c
        return self._cached(device, (), lambda code: _clam_weights(code, device, None, self, c.weight.reshape(-1), c.bias))[0]

    def forward(self, x):
        dropout_on = self.training and any(isinstance(m, nn.Dropout) and m.p > 0 for m in self.modules())
        if self.attention_c.out_features != 1 or dropout_on or _needs_autograd(self, x) or _all_on_cpu(self, x):
            return self._torch_forward(x)  # training / multi-branch (CLAM_MB) / a CPU tensor: PyTorch ops on the same device
        N.require_cuda(x, "Attn_Net_Gated")
        w = self._pack(x.device)
        if x.dim() < 1 or x.shape[-1] != w.s1:
            raise RuntimeError(f"Attn_Net_Gated: input {tuple(x.shape)} does not end in the L = {w.s1} features the module was built for")
        xin = Fn.as_compute(x, w.dtype).reshape(-1, w.s1)  # nn.Linear semantics: any leading dims
        n = xin.shape[0]
        A = torch.empty((n, 1), dtype=torch.float32, device=x.device)
        if n:
            need = n * 2 * w.s2 * 4 + 4096
            st = N.stream_ptr(x.device)
            ws = Fn.workspace(x.device, need, ("gated", st.value))
            N.call("hipt_attn_net_gated", C_.byref(w), N.ptr(xin), n, N.ptr(A), N.ptr(ws), ws.numel(), st)
        return A.reshape(*x.shape[:-1], 1), x


def _train_supported(sizes, k_att, n_classes, need_dbag=False) -> bool:
    """Do the training kernels take this shape (widths, branches, classes AND the LDS their row tiles need)?  Asked of the
    library itself (hipt_clam_train_shape_supported), so the answer cannot drift from the kernels' own checks."""
    if not (all(v > 0 and v % 4 == 0 for v in sizes) and 1 <= k_att <= 8 and 1 <= n_classes <= 8):
        return False
    return bool(N.lib().hipt_clam_train_shape_supported(int(sizes[0]), int(sizes[1]), int(sizes[2]), int(k_att), int(n_classes), int(need_dbag)))


class _ClamTrainFn(torch.autograd.Function):
    """Differentiable CLAM forward on the training kernels (include/hipt_abmil.h: hipt_clam_train_forward / _backward).

    forward(cfg, bag, m1, ma, mb, w1, b1, wa, ba, wb, bb, wc, bc, *cls) -> (logits [1,C], A_raw [K,N], M [K,S1],
    h1_sel [K,2,k,S1], topk_ids [K,2,k] int64, Y_hat [1,1] int64); ``cls`` = (weight [C,S1], bias [C]) for CLAM_SB or the
    2C tensors of CLAM_MB's per-class ``Linear(S1, 1)`` (w_0, b_0, w_1, b_1, ...)."""

    @staticmethod
    def forward(ctx, cfg, bag, m1, ma, mb, w1, b1, wa, ba, wb, bb, wc, bc, *cls):
        dev = bag.device
        K, C, multi, k_sel = cfg["K"], cfg["C"], cfg["multi"], cfg["k_sample"]
        f = lambda t: None if t is None else t.detach().float().contiguous()
        x = f(bag)
        n, S0 = x.shape
        S1, S2 = w1.shape[0], wa.shape[0]
        if multi:
            wcls = torch.cat([f(cls[2 * c]).reshape(1, S1) for c in range(C)], dim=0)
            bcls = torch.cat([f(cls[2 * c + 1]).reshape(1) for c in range(C)], dim=0)
        else:
            wcls, bcls = f(cls[0]), f(cls[1])
        keep = [x, f(m1), f(ma), f(mb), f(w1), f(b1), f(wa), f(ba), f(wb), f(bb), f(wc).reshape(K, S2), f(bc), wcls, bcls]
        N.same_device("CLAM training forward", dev, *keep)
        w = N.ClamTrainWeights()
        w.s0, w.s1, w.s2, w.n_att, w.n_classes, w.multi_branch = S0, S1, S2, K, C, int(multi)
        for name, t in zip(("w1", "b1", "wa", "ba", "wb", "bb", "wc", "bc", "wcls", "bcls"), keep[4:]):
            setattr(w, name, t.data_ptr())
        e = lambda *shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
        h1, t, s, A_raw, stats, M = e(n, S1), e(n, S2), e(n, S2), e(K, n), e(K, 2), e(K, S1)
        logits, y_prob, y_hat = e(1, C), e(1, C), e(1, 1, dt=torch.int64)
        ids = e(K, 2, k_sel, dt=torch.int64) if k_sel > 0 else None
        h1_sel = e(K, 2, k_sel, S1) if k_sel > 0 else None
        st = N.stream_ptr(dev)
        N.call("hipt_clam_train_forward", C_.byref(w), N.ptr(x), n, N.ptr(keep[1]), N.ptr(keep[2]), N.ptr(keep[3]), N.ptr(h1), N.ptr(t),
               N.ptr(s), N.ptr(A_raw), N.ptr(stats), N.ptr(M), N.ptr(logits), N.ptr(y_prob), N.ptr(y_hat), k_sel, N.ptr(ids), N.ptr(h1_sel), st)
        ctx.cfg = cfg
        ctx.w = w          # (the pointers stay valid: every tensor they name is in ctx.keep)
        ctx.keep = keep
        # `f` returns the parameter's own storage when it is already fp32 and contiguous: an in-place update between forward
        # and backward (optimizer.step) would silently change what the backward reads -- autograd's saved-tensor version
        # check raises there, and so does this
        srcs = [bag, m1, ma, mb, w1, b1, wa, ba, wb, bb, wc, bc, *cls]
        ctx.versions = [(t, t._version) for t in srcs if t is not None]
        ctx.saved = (h1, t, s, A_raw, stats, M, ids)
        ctx.set_materialize_grads(False)
        if ids is None:
            ids, h1_sel = torch.empty((K, 2, 0), dtype=torch.int64, device=dev), torch.empty((K, 2, 0, S1), device=dev)
        ctx.mark_non_differentiable(ids, y_hat)
        return logits, A_raw, M, h1_sel, ids, y_hat

    @staticmethod
    def backward(ctx, dlogits, dA_raw, dM, dh1_sel, _ids, _yhat):
        cfg, w, keep = ctx.cfg, ctx.w, ctx.keep
        for t, v in ctx.versions:
            if t._version != v:
                raise RuntimeError("one of the variables needed for gradient computation has been modified by an inplace operation "
                                   f"(CLAM training step: a {tuple(t.shape)} tensor is at version {t._version}, expected {v})")
        x, m1, ma, mb = keep[:4]
        h1, t, s, A_raw, stats, M, ids = ctx.saved
        dev = x.device
        n, S0 = x.shape
        S1, S2, K, C = w.s1, w.s2, w.n_att, w.n_classes
        z = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        g = N.ClamTrainGrads()
        out = dict(dw1=z(S1, S0), db1=z(S1), dwa=z(S2, S1), dba=z(S2), dwb=z(S2, S1), dbb=z(S2), dwc=z(K, S2), dbc=z(K), dwcls=z(C, S1), dbcls=z(C))
        if ctx.needs_input_grad[1]:
            out["dbag"] = z(n, S0)
        for name, tns in out.items():
            setattr(g, name, tns.data_ptr())
        c = lambda tns: None if tns is None else tns.detach().float().contiguous()
        dl = c(dlogits) if dlogits is not None else torch.zeros((1, C), device=dev)
        dA, dMx, dsel = c(dA_raw), c(dM), c(dh1_sel)
        n_sel = 0
        sel_ids = None
        if dsel is not None and ids is not None and dsel.numel():
            sel_ids, n_sel = ids.reshape(-1), ids.numel()
        st = N.stream_ptr(dev)
        need = N.lib().hipt_clam_train_workspace_bytes(C_.byref(w), n)
        ws = Fn.workspace(dev, need, ("clam_train", st.value))
        N.call("hipt_clam_train_backward", C_.byref(w), N.ptr(x), n, N.ptr(m1), N.ptr(ma), N.ptr(mb), N.ptr(h1), N.ptr(t), N.ptr(s), N.ptr(A_raw),
               N.ptr(stats), N.ptr(M), N.ptr(dl), N.ptr(dA), N.ptr(dMx), N.ptr(sel_ids), N.ptr(dsel if n_sel else None), n_sel, C_.byref(g),
               N.ptr(ws), ws.numel(), st)
        if cfg["multi"]:
            gcls = []
            for cl in range(C):
                gcls += [out["dwcls"][cl:cl + 1], out["dbcls"][cl:cl + 1]]
        else:
            gcls = [out["dwcls"], out["dbcls"]]
        wc_shape = cfg["wc_shape"]
        return (None, out.get("dbag"), None, None, None, out["dw1"], out["db1"], out["dwa"], out["dba"], out["dwb"], out["dbb"],
                out["dwc"].reshape(wc_shape), out["dbc"], *gcls)


class CLAM_SB(WeightImageCache, nn.Module):
    """Single-branch CLAM / ABMIL (model_clam.py:77-191).

    ``size_arg`` is a key of the reference's size table (plus ``'hipt_384'``) or an explicit
    ``[S0, S1, S2]`` list."""

    _multi = False
    bags_wide = False    # forward_bags takes hipt_clam_sb_forward_bags_wide (all bags in one call) for the wide heads (tiny, small, big, small_resnet18); False: the loop over forward.  CLAM_MB: together with bags_one_call, hipt_clam_mb_forward_bags_wide
    bags_narrow = False  # forward_bags takes hipt_clam_sb_forward_bags_narrow (all bags in one call) for the narrow heads the multi-bag kernel does not have; False: the loop over forward

    def __init__(self, gate=True, size_arg="small", dropout=0.0, k_sample=8, n_classes=2,
                 instance_loss_fn=nn.CrossEntropyLoss(), subtyping=False):
        super().__init__()
        self.size_dict = dict(SIZE_DICT)
        size = list(size_arg) if isinstance(size_arg, (list, tuple)) else self.size_dict[size_arg]
        self._build(gate, size, dropout, k_sample, n_classes, instance_loss_fn, subtyping, att_branches=1,
                    classifiers=lambda: nn.Linear(size[1], n_classes))
        initialize_weights(self)

    def _build(self, gate, size, dropout, k_sample, n_classes, instance_loss_fn, subtyping, att_branches, classifiers):
        fc = [nn.Linear(size[0], size[1]), nn.ReLU()]
        if dropout > 0:
            fc.append(nn.Dropout(dropout))
        head = Attn_Net_Gated if gate else Attn_Net
        fc.append(head(L=size[1], D=size[2], dropout=dropout, n_classes=att_branches))
        self.attention_net = nn.Sequential(*fc)
        self.classifiers = classifiers()  # (registration order = the reference's: attention_net, classifiers, instance_classifiers)
        self.instance_classifiers = nn.ModuleList([nn.Linear(size[1], 2) for _ in range(n_classes)])
        self.k_sample = k_sample
        self.instance_loss_fn = instance_loss_fn
        self.n_classes = n_classes
        self.subtyping = subtyping
        self._gate = gate
        self._dropout = dropout
        self._sizes = tuple(size)
        self._bags_route = None
        self._init_host()

    def relocate(self):
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.attention_net = self.attention_net.to(device)
        self.classifiers = self.classifiers.to(device)
        self.instance_classifiers = self.instance_classifiers.to(device)

    @staticmethod
    def create_positive_targets(length, device):
        return torch.full((length,), 1, device=device).long()

    @staticmethod
    def create_negative_targets(length, device):
        return torch.full((length,), 0, device=device).long()

    # ---- instance-level branches (model_clam.py:116-145) ------------------------------------------
    # rows_p / rows_n: the h1 rows of the k highest / k lowest attention scores of the branch
    def _inst_eval_rows(self, rows_p, rows_n, classifier):
        device = rows_p.device
        targets = torch.cat([self.create_positive_targets(self.k_sample, device),
                             self.create_negative_targets(self.k_sample, device)], dim=0)
        logits = classifier(torch.cat([rows_p, rows_n], dim=0))
        preds = torch.topk(logits, 1, dim=1)[1].squeeze(1)
        return self.instance_loss_fn(logits, targets), preds, targets

    def _inst_eval_out_rows(self, rows_p, classifier):
        targets = self.create_negative_targets(self.k_sample, rows_p.device)
        logits = classifier(rows_p)
        preds = torch.topk(logits, 1, dim=1)[1].squeeze(1)
        return self.instance_loss_fn(logits, targets), preds, targets

    def inst_eval(self, A, h, classifier):
        """Reference signature (model_clam.py:116-132): top-k of A by PyTorch ops on whatever device A lives on."""
        if A.dim() == 1:
            A = A.view(1, -1)
        top_p_ids = torch.topk(A, self.k_sample)[1][-1]
        top_n_ids = torch.topk(-A, self.k_sample, dim=1)[1][-1]
        return self._inst_eval_rows(torch.index_select(h, 0, top_p_ids), torch.index_select(h, 0, top_n_ids), classifier)

    def inst_eval_out(self, A, h, classifier):
        if A.dim() == 1:
            A = A.view(1, -1)
        top_p_ids = torch.topk(A, self.k_sample)[1][-1]
        return self._inst_eval_out_rows(torch.index_select(h, 0, top_p_ids), classifier)

    def _instance_branch(self, rows_of, label):
        """The instance loop of forward (:156-178 / :234-245).  rows_of(branch) -> (rows_p [k,S1], rows_n [k,S1])."""
        total, all_preds, all_targets = 0.0, [], []
        inst_labels = F.one_hot(label, num_classes=self.n_classes).squeeze()
        for i, classifier in enumerate(self.instance_classifiers):
            rows_p, rows_n = rows_of(i if self._multi else 0)
            if inst_labels[i].item() == 1:
                loss, preds, targets = self._inst_eval_rows(rows_p, rows_n, classifier)
            elif self.subtyping:
                loss, preds, targets = self._inst_eval_out_rows(rows_p, classifier)
            else:
                continue
            all_preds.extend(preds.cpu().numpy())
            all_targets.extend(targets.cpu().numpy())
            total += loss
        if self.subtyping:
            total /= len(self.instance_classifiers)
        return {'instance_loss': total, 'inst_labels': np.array(all_targets), 'inst_preds': np.array(all_preds)}

    def _bag_logits(self, M):
        return self.classifiers(M)  # :181

    # ---- the reference op sequence as PyTorch ops (ungated head; CPU tensors in training) ----------
    def _torch_forward(self, h, label, instance_eval, return_features, attention_only):
        A, h = self.attention_net(h)
        A = torch.transpose(A, 1, 0)
        if attention_only:
            return A
        A_raw = A
        A = F.softmax(A, dim=1)
        results = {}
        if instance_eval:
            def rows_of(b):
                a = A[b].view(1, -1)
                return (torch.index_select(h, 0, torch.topk(a, self.k_sample)[1][-1]),
                        torch.index_select(h, 0, torch.topk(-a, self.k_sample, dim=1)[1][-1]))
            results = self._instance_branch(rows_of, label)
        M = torch.mm(A, h)
        logits = self._bag_logits(M)
        Y_hat = torch.topk(logits, 1, dim=1)[1]
        Y_prob = F.softmax(logits, dim=1)
        if return_features:
            results.update({'features': M})
        return logits, Y_prob, Y_hat, A_raw, results

    # ---- HIP training path ----------------------------------------------------------------------------
    def _cls_tensors(self):
        return [self.classifiers.weight, self.classifiers.bias]

    def _check_bag(self, h):
        if h.dim() != 2 or h.shape[0] == 0 or h.shape[1] != self._sizes[0]:
            raise ValueError(f"expected a non-empty [N, {self._sizes[0]}] bag, got {tuple(h.shape)}")

    def _train_forward(self, h, label, instance_eval, return_features, attention_only):
        N.same_device(type(self).__name__, h.device, *self.parameters())
        self._check_bag(h)
        fc1, gated = self.attention_net[0], self.attention_net[-1]
        wa, wb, wc = gated.attention_a[0], gated.attention_b[0], gated.attention_c
        n, (S0, S1, S2), K = h.shape[0], self._sizes, wc.out_features
        m1 = ma = mb = None
        if self.training and self._dropout > 0:  # the masks nn.Dropout would draw, in the reference's order (:86, :48-52)
            ones = lambda c: torch.ones((n, c), dtype=torch.float32, device=h.device)
            m1, ma, mb = (F.dropout(ones(S1), self._dropout, True), F.dropout(ones(S2), self._dropout, True),
                          F.dropout(ones(S2), self._dropout, True))
        k_sel = self.k_sample if (instance_eval and not attention_only) else 0
        cfg = dict(K=K, C=self.n_classes, multi=self._multi, k_sample=k_sel, wc_shape=tuple(wc.weight.shape))
        logits, A_raw, M, h1_sel, _ids, Y_hat = _ClamTrainFn.apply(
            cfg, h, m1, ma, mb, fc1.weight, fc1.bias, wa.weight, wa.bias, wb.weight, wb.bias, wc.weight, wc.bias, *self._cls_tensors())
        if attention_only:
            return A_raw
        results = self._instance_branch(lambda b: (h1_sel[b, 0], h1_sel[b, 1]), label) if instance_eval else {}
        Y_prob = F.softmax(logits, dim=1)
        if return_features:
            results.update({'features': M})
        return logits, Y_prob, Y_hat, A_raw, results

    def _use_train_kernels(self, h, dropout_on) -> bool:
        if not self._gate or not h.is_cuda or not (dropout_on or _needs_autograd(self, h)):
            return False  # (asked first: an inference forward does not pay for the library's answer below)
        K = self.attention_net[-1].attention_c.out_features
        return _train_supported(self._sizes, K, self.n_classes, need_dbag=torch.is_grad_enabled() and h.requires_grad)

    # ---- HIP inference path ---------------------------------------------------------------------------
    def _pack(self, device):
        def build(code):
            fc1, gated = self.attention_net[0], self.attention_net[-1]
            c = gated.attention_c
            return _clam_weights(code, device, fc1, gated, c.weight.reshape(-1), c.bias, self.classifiers.weight, self.classifiers.bias,
                                 n_classes=self.classifiers.out_features)
        return self._cached(device, (), build)[0]

    def _route(self, h) -> str:
        """Which path ``forward`` takes on ``h``.  ``'train'``: the training kernels.  ``'torch'``: whatever those do not take (ungated head,
        CPU tensors, > 8 classes, widths beyond their LDS) keeps the PyTorch-op sequence as soon as dropout is active or a gradient is
        needed -- the inference kernels have neither -- and so does a bag the caller keeps on the CPU (the reference's relocate() chooses
        the CPU where there is no GPU, models/model_clam.py:102-106): PyTorch ops on the CPU.  ``'infer'``: the rest; a bag on a HIP device
        never comes to ``'torch'`` this way (a CPU bag handed to a module on a HIP device is a caller's mistake and raises in ``_infer``)."""
        dropout_on = self.training and self._dropout > 0
        if self._use_train_kernels(h, dropout_on):
            return 'train'
        if not self._gate or dropout_on or _needs_autograd(self, h) or _all_on_cpu(self, h):
            return 'torch'
        return 'infer'

    def forward(self, h, label=None, instance_eval=False, return_features=False, attention_only=False):
        route = self._route(h)
        run = self._infer if route == 'infer' else self._train_forward if route == 'train' else self._torch_forward
        return run(h, label, instance_eval, return_features, attention_only)

    def _infer_plan(self, device, n, attention_only):
        """``(weights, form, views, w_gather, out)`` of ``_infer`` on ``n`` rows: what ``functional.clam_forward`` is called with (lists: one call
        per pair), the weights to gather h1 rows with, and the outputs the calls fill between them (None: what the one call returns)."""
        w = self._pack(device)
        return w, "sb", None, w, None

    def _infer(self, h, label, instance_eval, return_features, attention_only):
        """model_clam.py:147-191 / :226-264 without autograd, for both classes: A [K, N] -> softmax over N per branch -> M [K, S1] ->
        logits, K = 1 for ``CLAM_SB``."""
        N.require_cuda(h, type(self).__name__)
        self._check_bag(h)
        dev, n = h.device, h.shape[0]
        w, form, views, wg, out = self._infer_plan(dev, n, attention_only)
        bag = h if h.dtype == Fn.torch_dtype(wg.dtype) and h.is_contiguous() else Fn.as_compute(h, wg.dtype)   # (only its address is used)
        got = Fn.clam_forward(w, bag, attention_only, views, form=form)
        A_raw, M, logits, Y_prob, Y_hat = got if out is None else out
        if attention_only:
            return A_raw
        if Y_hat is None:  # the K-branch calls leave these to the host (:251-252, on K numbers); CLAM_SB keeps the kernel's own
            Y_hat = torch.topk(logits, 1, dim=1)[1]
            Y_prob = F.softmax(logits, dim=1)
        results = {}
        if instance_eval:
            # inst_eval in eval mode (validate_clam, core_utils.py:506-560): top-k / bottom-k ids per branch on the device (softmax is monotone:
            # the ids of A_raw are those of softmax(A_raw)), then the library recomputes only the 2 K k selected rows of h1, not h1 [N, S1]
            K, k, st = A_raw.shape[0], self.k_sample, N.stream_ptr(dev)
            if k > n:
                raise RuntimeError(f"selected index k out of range: k_sample={k} > {n} rows (torch.topk, model_clam.py:120)")
            ids = torch.empty((K, 2, k), dtype=torch.int64, device=dev)
            N.call("hipt_topk_rows", N.ptr(A_raw), K, n, k, N.ptr(ids), st)
            rows = torch.empty((K, 2, k, wg.s1), dtype=torch.float32, device=dev)
            N.call("hipt_clam_gather_h1", C_.byref(wg), N.ptr(bag), N.ptr(ids), 2 * K * k, N.ptr(rows), st)
            results = self._instance_branch(lambda b: (rows[b, 0], rows[b, 1]), label)   # (b = 0 for CLAM_SB's one branch)
        if return_features:
            results.update({'features': M})
        return logits, Y_prob, Y_hat, A_raw, results

    # ---- many bags in one call ------------------------------------------------------------------------
    @property
    def bags_route(self):
        """Which route the last ``forward_bags`` took: ``'bags'`` (one ``hipt_clam_sb_forward_bags`` call), ``'per_bag'`` (the loop
        over ``forward``) or None before the first call."""
        return self._bags_route

    def _bags_input(self, bags):
        """``(cat [rows, S0], offsets)`` from a sequence of ``[N_b, S0]`` tensors or from a pair ``(cat, offsets)``; offsets checked on the host."""
        S0 = self._sizes[0]
        pair = (isinstance(bags, (tuple, list)) and len(bags) == 2 and isinstance(bags[0], torch.Tensor) and
                (isinstance(bags[1], Fn.BagOffsets) or not isinstance(bags[1], torch.Tensor) or bags[1].dim() == 1))
        if pair:
            cat, off = bags
            if cat.dim() != 2 or cat.shape[1] != S0:
                raise ValueError(f"expected concatenated bags [rows, {S0}], got {tuple(cat.shape)}")
            if isinstance(off, Fn.BagOffsets):
                if off.host[-1] != cat.shape[0]:
                    raise ValueError(f"bag offsets end at {off.host[-1]} but the concatenated bags have {cat.shape[0]} rows")
                return cat, off
            if isinstance(off, torch.Tensor) and off.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("forward_bags: device offsets cannot be checked inside a graph capture; make a functional.BagOffsets before it")
            return cat, (Fn.BagOffsets(off, cat.shape[0], cat.device) if cat.is_cuda else Fn.check_offsets(off, cat.shape[0]))
        bags = list(bags)
        if not bags:
            raise ValueError("forward_bags: no bags")
        for b, t in enumerate(bags):
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] == 0 or t.shape[1] != S0:
                raise ValueError(f"bag {b}: expected a non-empty [N, {S0}] tensor, got {tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        host, acc = [0], 0
        for t in bags:
            acc += t.shape[0]
            host.append(acc)
        cat = torch.cat(bags, dim=0)  # ONE concatenation, on the bags' device
        return cat, (Fn.BagOffsets(host, acc, cat.device) if cat.is_cuda else tuple(host))

    def _bags_form(self, device):
        """``(weight image, form)`` of the one ``functional.clam_forward_bags`` call that serves ``forward_bags`` on ``device``, or
        None: the loop over ``forward``.  The rows of ``functional._BAGS_FORMS`` of this model's kind, in order: the first whose switches
        are all set and whose predicate holds.  The weight image is packed when the first row gets as far as its predicate."""
        if not self._gate or device.type != "cuda":
            return None
        w = None
        for f in Fn.BAGS_FORMS_OF["CLAM_MB" if self._multi else "CLAM_SB"]:
            if all(getattr(self, s) for s in f.switches):
                if w is None:
                    w, lib = self._pack_stacked(device) if self._multi else self._pack(device), N.lib()
                if getattr(lib, f.supported)(C_.byref(w)):
                    return w, f.name
        return None

    def forward_bags(self, bags, attention_only=False, return_features=False, label=None, instance_eval=False):
        """``forward`` over B bags at once, inference only (no autograd; dropout inactive as in ``eval()``).

        ``bags``: a sequence of ``[N_b, S0]`` tensors, or ``(cat [sum N_b, S0], offsets)`` with the B+1 row offsets as a list, a
        tensor or a ``functional.BagOffsets``.  Returns ``logits [B, C]``, ``Y_prob [B, C]``, ``Y_hat [B, 1]``, ``A_raw`` as a
        list of ``[1, N_b]`` views of one buffer and ``{'features': M [B, S1]}`` when asked (``attention_only``: the list alone).
        The rule: the first form of this model's kind in ``functional._BAGS_FORMS`` whose switches are all set on the model and whose
        ``*_supported`` predicate holds is taken, as ONE native call whose per-bag results do not depend on the other bags; otherwise
        -- also for the ungated head and CPU tensors -- it loops over ``forward`` and returns the same structure.  ``bags_route`` tells which.

            kind     form     switches (default False)      heads
            CLAM_SB  sb       -                             S1 in {128, 64}, fp32 also 32; S2 in {64, 32, 16}
            CLAM_SB  narrow   bags_narrow                   hipt_smaller [192, 16, 8], hipt_smallest [192, 8, 4], (32, 8), (32, 16)
            CLAM_SB  wide     bags_wide                     tiny, small, big, small_resnet18
            CLAM_MB  mb       bags_one_call                 the widths of sb, 2 to 4 classes
            CLAM_MB  mb_many  bags_one_call, bags_many      the widths of sb, 5 to 8 classes
            CLAM_MB  mb_wide  bags_one_call, bags_wide      the widths of wide, 2 to 4 classes (``CLAM_MB()`` is built with ``small``)

        A width both kernels have keeps the first.  With a switch of its form off a model keeps the loop, with the bits of ``forward``;
        the numbers of a one-call form equal the loop's within the fp32 bar (1e-4), not bit for bit.  The ``CLAM_MB`` forms return
        ``A_raw`` as a list of ``[K, N_b]`` views and features ``[B, K, S1]``.

        ``instance_eval=True`` with ``label`` (B class ids: a list, a numpy array or a tensor) adds what ``forward(h, label=,
        instance_eval=True)`` returns per bag (validate_clam, utils/core_utils.py:506-560): ``instance_loss`` (a ``[B]`` tensor),
        ``inst_preds`` and ``inst_labels`` (lists of B numpy arrays, in the order of ``_instance_branch``: classes ascending).  On
        the ``'bags'`` route that is one segmented top-k, one gather of the selected h1 rows of the concatenated bags, the instance
        classifiers over all selected rows and ONE read-back for the call (a ``label`` tensor on the device together with an
        ``instance_loss_fn`` other than the default ``nn.CrossEntropyLoss`` costs a second one: hand the labels over on the host)."""
        cat, off = self._bags_input(bags)
        if self.training and _needs_autograd(self, cat):
            raise RuntimeError("forward_bags is inference only: in training mode, with gradients asked for, call forward(h) bag by bag")
        host = off.host if isinstance(off, Fn.BagOffsets) else off
        inst = instance_eval and not attention_only
        if inst:
            lab = self._bag_labels(label, len(host) - 1)
            for b in range(len(host) - 1):  # before anything is launched, as torch.topk in forward
                if self.k_sample > host[b + 1] - host[b]:
                    raise RuntimeError(f"selected index k out of range: k_sample={self.k_sample} > {host[b + 1] - host[b]} rows (torch.topk, model_clam.py:120)")
        with torch.no_grad():
            route = self._bags_form(cat.device)
            if route is None:
                return self._forward_bags_loop(cat, host, attention_only, return_features, lab if inst else None)
            w, form = route
            self._bags_route = "bags"
            x = Fn.as_compute(cat, w.dtype)
            A_raw, M, logits, Y_prob, Y_hat = Fn.clam_forward_bags(w, x, off, attention_only, form=form)
            A2 = A_raw if form in Fn.BAGS_FORMS_K else A_raw.view(1, -1)   # [K, rows] / [1, rows]
            views = [A2[:, host[b]:host[b + 1]] for b in range(len(off))]
            if attention_only:
                return views
            results = self._instance_bags(w, x, off, A_raw, lab) if inst else {}
            if return_features:
                results['features'] = M
            return logits, Y_prob, Y_hat.view(-1, 1), views, results

    def _bag_labels(self, label, B):
        """``label`` of ``forward_bags`` as (list of B ints or None, int64 [B] tensor or None): the host form where the caller has it there."""
        if label is None:
            raise ValueError("forward_bags(instance_eval=True) needs the B class ids in `label`")
        if isinstance(label, torch.Tensor) and label.is_cuda:
            lab = label.detach().reshape(-1).long()
            if lab.numel() != B:
                raise ValueError(f"{B} bags but {lab.numel()} labels")
            return None, lab
        flat = (label.detach().reshape(-1).tolist() if isinstance(label, torch.Tensor) else
                np.asarray(label).reshape(-1).tolist() if isinstance(label, np.ndarray) else
                [int(l.reshape(-1)[0]) if isinstance(l, (torch.Tensor, np.ndarray)) else int(l) for l in label])
        flat = [int(l) for l in flat]
        if len(flat) != B:
            raise ValueError(f"{B} bags but {len(flat)} labels")
        if any(l < 0 or l >= self.n_classes for l in flat):
            raise ValueError(f"labels must lie in [0, {self.n_classes})")
        return flat, None

    def _default_instance_loss(self) -> bool:
        f = self.instance_loss_fn
        return (type(f) is nn.CrossEntropyLoss and f.weight is None and f.reduction == "mean" and f.ignore_index == -100 and
                getattr(f, "label_smoothing", 0.0) == 0.0)

    def _instance_bags(self, w, x, off, A_raw, lab):
        """The instance branch (:156-178 / :234-245) of every bag of a ``'bags'``-route call.  Softmax is monotone, so the top-k ids of
        A_raw are those of softmax(A_raw); classifier c reads the rows selected by branch c (``CLAM_MB``) or by the one branch."""
        lab_host, lab_dev = lab
        dev, B, k, C, S1 = x.device, len(off), self.k_sample, self.n_classes, self._sizes[1]
        Ka = w.n_att if self._multi else 1
        _, gids = Fn.topk_segments(A_raw, off, k)
        rows = torch.empty((B, Ka, 2 * k, S1), dtype=torch.float32, device=dev)
        N.call("hipt_clam_gather_h1", C_.byref(w), N.ptr(x), N.ptr(gids), B * Ka * 2 * k, N.ptr(rows), N.stream_ptr(dev))
        # classifier c on the 2k rows of its branch, for every bag: [B, C, 2k, 2]; inst_eval_out reads the first k of them.  Products and
        # pairwise sums are elementwise kernels, so a bag's numbers do not depend on the other bags of the call (a GEMM's blocking may)
        Wi = torch.stack([cl.weight for cl in self.instance_classifiers]).float()            # [C, 2, S1]
        bi = torch.stack([cl.bias for cl in self.instance_classifiers]).float()              # [C, 2]
        sel = rows if self._multi else rows.expand(B, C, 2 * k, S1)
        L = _tree_sum(sel.unsqueeze(3) * Wi.view(1, C, 1, 2, S1)) + bi.view(1, C, 1, 2)
        preds = torch.topk(L, 1, dim=-1)[1].squeeze(-1)                       # [B, C, 2k]
        t_in = torch.cat([self.create_positive_targets(k, dev), self.create_negative_targets(k, dev)], dim=0)
        t_out = self.create_negative_targets(k, dev)
        if lab_dev is None:
            lab_dev = torch.tensor(lab_host, dtype=torch.int64, device=dev)
        elif not self._default_instance_loss():
            lab_host = lab_dev.tolist()
        total = torch.zeros((B,), dtype=torch.float32, device=dev)
        if self._default_instance_loss():
            # cross-entropy of two logits per row, written out: -log softmax = logsumexp - the target's logit
            l0, l1 = L[..., 0], L[..., 1]
            mx = torch.maximum(l0, l1)
            lse = mx + torch.log(torch.exp(l0 - mx) + torch.exp(l1 - mx))
            ce_in = _tree_sum(torch.cat([(lse - l1)[..., :k], (lse - l0)[..., k:]], dim=-1)) / (2 * k)    # [B, C]: targets 1 x k, 0 x k
            ce_out = _tree_sum((lse - l0)[..., :k]) / k                                                   # targets 0 x k
            for c in range(C):   # classes ascending, as _instance_branch accumulates
                mine = lab_dev == c
                total = total + torch.where(mine, ce_in[:, c], ce_out[:, c] if self.subtyping else torch.zeros_like(total))
        else:
            per = []
            for b in range(B):
                acc = 0.0
                for c in range(C):
                    if lab_host[b] == c:
                        acc = acc + self.instance_loss_fn(L[b, c], t_in)
                    elif self.subtyping:
                        acc = acc + self.instance_loss_fn(L[b, c, :k], t_out)
                per.append(acc if isinstance(acc, torch.Tensor) else torch.zeros((), device=dev))
            total = torch.stack([p.reshape(()).float() for p in per])
        if self.subtyping:
            total = total / C
        back = torch.cat([preds.reshape(-1), lab_dev]).cpu().numpy()         # THE read-back of the call
        p_host, lab_np = back[:B * C * 2 * k].reshape(B, C, 2 * k), back[B * C * 2 * k:]
        if lab_host is None and (lab_np.min() < 0 or lab_np.max() >= C):
            raise ValueError(f"labels must lie in [0, {C})")
        t_in_np = np.concatenate([np.ones(k, dtype=np.int64), np.zeros(k, dtype=np.int64)])
        inst_preds, inst_labels = [], []
        for b in range(B):
            ps, ts = [], []
            for c in range(C):
                if int(lab_np[b]) == c:
                    ps.append(p_host[b, c])
                    ts.append(t_in_np)
                elif self.subtyping:
                    ps.append(p_host[b, c, :k])
                    ts.append(t_in_np[k:])
            inst_preds.append(np.concatenate(ps))
            inst_labels.append(np.concatenate(ts))
        return {'instance_loss': total, 'inst_labels': inst_labels, 'inst_preds': inst_preds}

    def _forward_bags_loop(self, cat, host, attention_only, return_features, lab=None):
        self._bags_route = "per_bag"
        was_training = self.training
        self.train(False)
        try:
            if lab is None:
                outs = [self.forward(cat[host[b]:host[b + 1]], attention_only=attention_only, return_features=return_features)
                        for b in range(len(host) - 1)]
            else:
                labels = lab[0] if lab[0] is not None else lab[1].tolist()
                outs = [self.forward(cat[host[b]:host[b + 1]], label=torch.tensor([labels[b]], dtype=torch.int64, device=cat.device),
                                     instance_eval=True, return_features=return_features) for b in range(len(host) - 1)]
        finally:
            self.train(was_training)
        if attention_only:
            return outs
        results = {'features': (torch.stack if self._multi else torch.cat)([o[4]['features'] for o in outs], dim=0)} if return_features else {}
        if lab is not None:
            results['instance_loss'] = torch.stack([torch.as_tensor(o[4]['instance_loss'], dtype=torch.float32, device=cat.device).reshape(())
                                                    for o in outs])
            results['inst_preds'] = [o[4]['inst_preds'] for o in outs]
            results['inst_labels'] = [o[4]['inst_labels'] for o in outs]
        return (torch.cat([o[0] for o in outs], dim=0), torch.cat([o[1] for o in outs], dim=0), torch.cat([o[2] for o in outs], dim=0),
                [o[3] for o in outs], results)


class CLAM_MB(CLAM_SB):
    """Multi-branch CLAM (model_clam.py:193-264): one attention branch and one ``Linear(S1, 1)`` bag classifier per class.

    Inference (eval mode, no gradient asked for) runs the SAME streaming kernels as ``CLAM_SB`` -- MFMA projections, one pass
    over the bag per branch (``hipt_clam_sb_forward`` with the branch's ``attention_c`` row and its one-row classifier: the K
    branches share W1 and [Wa; Wb], only ``wc [K, S2]``, ``bc [K]`` and the pooled sums differ), in both compute dtypes; a
    forward that must be differentiable (or has active dropout) runs the K-branch fp32 training kernels of csrc/clam_train.hip;
    ``gate=False`` and CPU tensors take the PyTorch-op sequence."""

    _multi = True
    one_pass = True  # inference takes the "mb" form of functional.clam_forward (one pass over the bag for all branches) where the library has it; False: branch by branch
    bags_one_call = False  # forward_bags takes hipt_clam_mb_forward_bags (all bags, all branches in one call) where the library has it; False: the loop over forward
    bags_many = False      # together with bags_one_call: forward_bags takes hipt_clam_mb_forward_bags_many for 5 to 8 classes at the widths of hipt_clam_mb_forward_bags; False: the loop over forward

    def __init__(self, gate=True, size_arg="small", dropout=0.0, k_sample=8, n_classes=2,
                 instance_loss_fn=nn.CrossEntropyLoss(), subtyping=False):
        nn.Module.__init__(self)
        self.size_dict = dict(SIZE_DICT)
        size = list(size_arg) if isinstance(size_arg, (list, tuple)) else self.size_dict[size_arg]
        self._build(gate, size, dropout, k_sample, n_classes, instance_loss_fn, subtyping, att_branches=n_classes,
                    classifiers=lambda: nn.ModuleList([nn.Linear(size[1], 1) for _ in range(n_classes)]))
        initialize_weights(self)

    def _cls_tensors(self):
        out = []
        for c in self.classifiers:
            out += [c.weight, c.bias]
        return out

    def _pack_branches(self, device, stacked=False):
        """``(ws, mb)``: one ``hipt_clam_weights`` per attention branch for the inference kernels -- shared W1 / [Wa; Wb] tensors, the
        branch's row of ``attention_c`` and its ``Linear(S1, 1)`` as a one-class bag classifier -- and the stacked struct of the one-pass
        kernel, or None where the library does not take the configuration (cached like ``_pack``)."""
        def build(code):
            fc1, gated, K = self.attention_net[0], self.attention_net[-1], self.n_classes
            shared = _cast_shared(code, fc1, gated)
            wc_all, bc_all = Fn.f32c(gated.attention_c.weight), Fn.f32c(gated.attention_c.bias)
            bounds = wc_all.abs().sum(dim=1).tolist()  # per branch: |A_raw[k] - bc[k]| <= sum_j |wc[k][j]| (one read-back per set of weights)
            made = [_clam_weights(code, device, fc1, gated, wc_all[k], bc_all[k:k + 1], self.classifiers[k].weight, self.classifiers[k].bias,
                                  n_classes=1, shared=shared, bound=bounds[k]) for k in range(K)]
            # all K branches in ONE pass over the bag (hipt_clam_mb_forward, round 6) where the streaming kernel takes the configuration:
            # the same shared tensors, wc / bc / the K one-row classifiers stacked, the image packed with its K rows of wc
            wm, keep = _clam_weights(code, device, fc1, gated, wc_all, bc_all, torch.cat([c.weight for c in self.classifiers], dim=0),
                                     torch.cat([c.bias for c in self.classifiers], dim=0), n_classes=K, n_att=K, shared=shared,
                                     bound=max(bounds), image=2 <= K <= 4)
            mb = wm if wm.stream_pk and N.lib().hipt_clam_mb_supported(C_.byref(wm)) else None
            return [w for w, _ in made], mb, (made, wm, keep)
        full = self._cached(device, ("mb",), build)
        return full[2][1] if stacked else full[:2]

    def _pack_stacked(self, device):
        """The stacked K-branch struct of ``_pack_branches`` (``wm``: wc [K, S2], bc [K], the K one-row classifiers [K, S1]) whatever the
        one-pass streaming kernel says about it: what ``hipt_clam_mb_forward_bags`` takes.  The same cache entry."""
        return self._pack_branches(device, stacked=True)

    def _infer_plan(self, device, n, attention_only):
        """ONE pass over the bag for all branches (gate once per row, K logits, h1 left in bf16 for the pooling kernel: two launches
        instead of K) where ``one_pass`` is set and the library takes the stacked image; else branch by branch through the
        ``CLAM_SB`` kernels, each call into its rows of the shared outputs (logits[0, c] = classifiers[c](M[c]), :248-250)."""
        ws, mb = self._pack_branches(device)
        if self.one_pass and mb is not None:
            return mb, "mb", None, ws[0], None
        K, e = self.n_classes, lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=device)
        A_raw = e((K, n))
        if attention_only:
            return ws, "sb", [(A_raw[k], None, None, None, None) for k in range(K)], ws[0], (A_raw, None, None, None, None)
        M, logits, junk_p, junk_y = e((K, self._sizes[1])), e((1, K)), e((K,)), e((K,), torch.int64)   # (junk: the one-class softmax / argmax of a branch, 1 and 0)
        views = [(A_raw[k], M[k], logits[0, k:k + 1], junk_p[k:k + 1], junk_y[k:k + 1]) for k in range(K)]
        return ws, "sb", views, ws[0], (A_raw, M, logits, None, None)

    def _bag_logits(self, M):  # :248-250
        logits = torch.empty(1, self.n_classes).float().to(M.device)
        for c in range(self.n_classes):
            logits[0, c] = self.classifiers[c](M[c])
        return logits
