"""Max-pooling MIL baselines (reference: ``models/model_mil.py``; ``main.py --model_type mil``).

``MIL_fc`` (two classes) and ``MIL_fc_mc`` (three to eight) keep the reference's constructor arguments, attributes, asserts,
``relocate()``, ``initialize_weights`` and state-dict keys (``classifier.0.*`` plus ``classifier.2.*`` without dropout or
``classifier.3.*`` with it; ``fc.0.*`` and ``classifiers.{c}.*``), so its checkpoints load with ``strict=True``.

Both forwards are ``h1 = ReLU(h W1^T + b1)``, ``logits = h1 W2^T + b2``, ``y_probs = softmax(logits)`` per row and then ONE selected row:
``MIL_fc`` takes the row with the largest ``y_probs[:, 1]``, ``MIL_fc_mc`` the first maximum of ``y_probs`` flattened to ``[N * C]``.
Equal keys: the lowest row wins, then the lowest class -- ``argmax`` does that already; ``torch.topk`` leaves the order of equal
values open, so for ``MIL_fc`` this is the project's rule.  On a HIP device all of it is one native call (csrc/mil.hip,
``hipt_mil_forward_bags``) for one bag or for many.

Where the reference cannot run its own code the intended behaviour is followed: ``MIL_fc.forward(return_features=True)`` indexes
``self.classifier.module`` (there only under ``DataParallel``) -- here the features are the selected row of h1, as for ``MIL_fc_mc``; and
``top_k != 1`` fails at ``.view(1,)`` -- here the constructor raises ``ValueError``.
"""
from __future__ import annotations

import ctypes as C_

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _native as N
from . import functional as Fn
from ._host import WeightImageCache
from .model_clam import CLAM_SB, _all_on_cpu, _needs_autograd, initialize_weights

SIZE_DICT = {"small": [1024, 512]}
MAX_CLASSES = 8


def _size(size_arg):
    """``[S0, S1]`` of a key of the reference's table or of an explicit pair inside the kernel's envelope."""
    if isinstance(size_arg, str):
        if size_arg not in SIZE_DICT:
            raise ValueError(f"size_arg {size_arg!r}: not one of {sorted(SIZE_DICT)} nor an [S0, S1] pair")
        return list(SIZE_DICT[size_arg])
    size = [int(v) for v in size_arg] if isinstance(size_arg, (list, tuple)) else None
    if size is None or len(size) != 2 or size[1] not in (256, 512) or size[0] <= 0 or size[0] % 32:
        raise ValueError(f"size_arg {size_arg!r}: expected 'small' or [S0, S1] with S1 in (256, 512) and S0 a positive multiple of 32 (bf16: of 64)")
    return size


def mil_forward_bags(w, cat: torch.Tensor, offsets: Fn.BagOffsets, features: bool = True, out=None, ws=None):
    """``hipt_mil_forward_bags`` (include/hipt_abmil.h) on ``cat [rows, S0]``, contiguous and in the dtype of the weight image ``w`` (an
    ``_native.MilWeights``).  Returns ``(y_probs [rows, C], top_idx [B], top_logits [B, C], top_prob [B, C], y_hat [B], top_features
    [B, S1] or None)``.  ``out`` / ``ws``: buffers to write into instead of fresh ones (tests: guard rows, graph capture)."""
    N.require_cuda(cat, "mil_forward_bags")
    dev, B, rows = cat.device, len(offsets), cat.shape[0]
    if cat.dim() != 2 or not cat.is_contiguous() or cat.dtype != Fn.torch_dtype(w.dtype) or cat.shape[1] != w.s0:
        raise ValueError(f"expected contiguous [rows, {w.s0}] bags in {Fn.torch_dtype(w.dtype)}, got {tuple(cat.shape)} {cat.dtype}")
    if offsets.host[-1] != rows:
        raise ValueError(f"bag offsets end at {offsets.host[-1]} but the concatenated bags have {rows} rows")
    N.same_device("mil_forward_bags", dev, offsets.dev)
    if not N.lib().hipt_mil_bags_supported(C_.byref(w)):
        raise RuntimeError(f"mil_forward_bags: [{w.s0}, {w.s1}] with {w.n_classes} classes is outside the kernel's envelope "
                           "(S1 in (256, 512), S0 a multiple of 32 in fp32 / 64 in bf16, 2 to 8 classes)")
    st = N.stream_ptr(dev)
    if ws is None:
        ws = Fn.workspace(dev, N.lib().hipt_mil_bags_workspace_bytes(C_.byref(w), B, rows), ("mil_bags", st.value))
    if out is None:
        e = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=dev)
        C = w.n_classes
        out = (e((rows, C)), e((B,), torch.int64), e((B, C)), e((B, C)), e((B,), torch.int64), e((B, w.s1)) if features else None)
    y_probs, idx, logits, prob, y_hat, feats = out
    N.call("hipt_mil_forward_bags", C_.byref(w), N.ptr(cat), N.ptr(offsets.dev), B, rows, N.ptr(y_probs), N.ptr(idx), N.ptr(logits),
           N.ptr(prob), N.ptr(y_hat), N.ptr(feats), N.ptr(ws), ws.numel(), st)
    return out


class _MaxPoolMIL(WeightImageCache, nn.Module):
    """What ``MIL_fc`` and ``MIL_fc_mc`` share: routing, the weight image, the native call and ``forward_bags``."""

    _multi = False

    def _setup(self, size, dropout, n_classes, top_k):
        if top_k != 1:
            raise ValueError(f"top_k = {top_k}: only top_k = 1 is defined (the reference's forward fails at .view(1,) for any other value)")
        self.size_dict = dict(SIZE_DICT)
        self.top_k = top_k
        self._sizes = tuple(size)
        self._dropout = bool(dropout)
        self._n_out = n_classes
        self._bags_route = None
        self._init_host()

    # ---- the module's pieces -------------------------------------------------------------------------
    def _fc1(self) -> nn.Linear:
        raise NotImplementedError

    def _hidden(self, h):
        """h1 through the module's own first stage (Linear, ReLU and, where built in, Dropout)."""
        raise NotImplementedError

    def _logits(self, h1):
        raise NotImplementedError

    def _w2(self):
        """``(weight [C, S1], bias [C])`` of the classifier stage."""
        raise NotImplementedError

    def _finish(self, logits, y_probs, h1, return_features):
        raise NotImplementedError

    # ---- routing ---------------------------------------------------------------------------------------
    def route(self, h) -> str:
        """Which path ``forward`` takes on ``h``.  ``'torch'``: the module's PyTorch-op sequence -- dropout active in train mode, or
        module and bag both on the CPU (where the reference's ``relocate()`` leaves them without a GPU).  ``'train'``: a forward that must
        be differentiable with dropout inactive -- the native call selects, PyTorch ops recompute the selected row.  ``'infer'``: the
        rest, the native call alone.  A bag on a HIP device never comes to ``'torch'`` for lack of the library: that raises
        ``NativeLibraryError``."""
        if (self.training and self._dropout) or _all_on_cpu(self, h):
            return 'torch'
        return 'train' if _needs_autograd(self, h) else 'infer'

    def _check_bag(self, h):
        if h.dim() != 2 or h.shape[0] == 0 or h.shape[1] != self._sizes[0]:
            raise ValueError(f"expected a non-empty [N, {self._sizes[0]}] bag, got {tuple(h.shape)}")

    def _pack(self, device):
        def build(code):
            fc1 = self._fc1()
            w2, b2 = self._w2()
            keep = dict(w1=Fn.as_compute(fc1.weight, code), b1=Fn.f32c(fc1.bias), w2=Fn.f32c(w2), b2=Fn.f32c(b2))
            w = N.MilWeights()
            w.dtype, w.s0, w.s1, w.n_classes, w.multi_class = code, fc1.in_features, fc1.out_features, self._n_out, int(self._multi)
            for name, t in keep.items():
                setattr(w, name, t.data_ptr())
            return w, keep
        return self._cached(device, (), build)[0]

    def _native(self, cat, off, features):
        w = self._pack(cat.device)
        return mil_forward_bags(w, Fn.as_compute(cat, w.dtype), off, features)

    # ---- forward ---------------------------------------------------------------------------------------
    def _torch_forward(self, h, return_features):
        h1 = self._hidden(h)
        logits = self._logits(h1)
        y_probs = F.softmax(logits, dim=1)
        return self._finish(logits, y_probs, h1, return_features)

    def _shape_out(self, top_instance, Y_prob, y_hat, y_probs, feats, return_features):
        Y_hat = y_hat.view(1) if self._multi else y_hat.view(1, 1)
        return top_instance, Y_prob, Y_hat, y_probs, ({'features': feats} if return_features else {})

    def forward(self, h, return_features=False):
        """``(top_instance [1, C], Y_prob [1, C], Y_hat, y_probs [N, C], results_dict)`` as the reference returns them (``Y_hat`` int64,
        ``[1, 1]`` for ``MIL_fc`` and ``[1]`` for ``MIL_fc_mc``); ``results_dict['features']`` is the selected row of h1 ``[1, S1]``.

        On the ``'train'`` route ``top_instance`` (and ``Y_prob``, the features) carry the reference's gradient: there, too, only the
        selected row feeds ``top_instance``.  ``y_probs`` comes back DETACHED on that route -- the reference's training and validation
        loops discard it; a gradient through ``y_probs`` is outside this package."""
        route = self.route(h)
        if route == 'torch':
            return self._torch_forward(h, return_features)
        N.require_cuda(h, type(self).__name__)
        self._check_bag(h)
        off = Fn.BagOffsets((0, h.shape[0]), h.shape[0], h.device)
        if route == 'infer':
            y_probs, _idx, logits, prob, y_hat, feats = self._native(h, off, return_features)
            return self._shape_out(logits, prob, y_hat, y_probs, feats, return_features)
        with torch.no_grad():
            y_probs, idx, _l, _p, y_hat, _f = self._native(h, off, False)
        h1 = self._hidden(torch.index_select(h, 0, idx))    # dropout is inactive on this route: ReLU(row W1^T + b1)
        top_instance = self._logits(h1)
        if not self._multi:
            y_hat = torch.topk(top_instance, 1, dim=1)[1]
        return self._shape_out(top_instance, F.softmax(top_instance, dim=1), y_hat, y_probs, h1, return_features)

    # ---- many bags in one call ---------------------------------------------------------------------------
    @property
    def bags_route(self):
        """Which route the last ``forward_bags`` took: ``'bags'`` (one ``hipt_mil_forward_bags`` call), ``'per_bag'`` (the loop over
        ``forward``: CPU tensors) or None before the first call."""
        return self._bags_route

    _bags_input = CLAM_SB._bags_input

    def forward_bags(self, bags, return_features=False):
        """``forward`` over B bags at once, inference only.  ``bags``: a sequence of ``[N_b, S0]`` tensors or ``(cat, offsets)`` as
        ``CLAM_SB.forward_bags`` takes them.  Returns ``top_instance [B, C]``, ``Y_prob [B, C]``, ``Y_hat [B, 1]``, ``y_probs`` as a list of
        ``[N_b, C]`` views of one buffer and ``{'features': [B, S1]}`` when asked: row ``b`` of each is what ``forward`` returns for bag
        ``b``, bit for bit, whatever the other bags of the call are."""
        cat, off = self._bags_input(bags)
        if self.training and _needs_autograd(self, cat):
            raise RuntimeError("forward_bags is inference only: in training mode, with gradients asked for, call forward(h) bag by bag")
        host = off.host if isinstance(off, Fn.BagOffsets) else off
        with torch.no_grad():
            if not cat.is_cuda:
                self._bags_route = "per_bag"
                was = self.training
                self.train(False)
                try:
                    outs = [self.forward(cat[host[b]:host[b + 1]], return_features) for b in range(len(host) - 1)]
                finally:
                    self.train(was)
                res = {'features': torch.cat([o[4]['features'] for o in outs], dim=0)} if return_features else {}
                return (torch.cat([o[0] for o in outs], dim=0), torch.cat([o[1] for o in outs], dim=0),
                        torch.cat([o[2].view(1, 1) for o in outs], dim=0), [o[3] for o in outs], res)
            self._bags_route = "bags"
            y_probs, _idx, logits, prob, y_hat, feats = self._native(cat, off, return_features)
            views = [y_probs[host[b]:host[b + 1]] for b in range(len(host) - 1)]
            return logits, prob, y_hat.view(-1, 1), views, ({'features': feats} if return_features else {})


class MIL_fc(_MaxPoolMIL):
    """Two-class max-pooling MIL (model_mil.py:7-43): the instance with the largest probability of class 1 speaks for the bag."""

    def __init__(self, gate=True, size_arg="small", dropout=False, n_classes=2, top_k=1):
        super().__init__()
        assert n_classes == 2
        size = _size(size_arg)
        fc = [nn.Linear(size[0], size[1]), nn.ReLU()]
        if dropout:
            fc.append(nn.Dropout(0.25))
        fc.append(nn.Linear(size[1], n_classes))
        self.classifier = nn.Sequential(*fc)
        initialize_weights(self)
        self._setup(size, dropout, n_classes, top_k)

    def relocate(self):
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.classifier.to(device)

    def _fc1(self):
        return self.classifier[0]

    def _hidden(self, h):
        return self.classifier[:-1](h)

    def _logits(self, h1):
        return self.classifier[-1](h1)

    def _w2(self):
        return self.classifier[-1].weight, self.classifier[-1].bias

    def _finish(self, logits, y_probs, h1, return_features):
        # the first of the largest values (torch.topk's order among equal values is not defined)
        idx = torch.argmax(y_probs[:, 1], dim=0).view(1,)
        top_instance = torch.index_select(logits, dim=0, index=idx)
        Y_hat = torch.topk(top_instance, 1, dim=1)[1]
        Y_prob = F.softmax(top_instance, dim=1)
        results = {'features': torch.index_select(h1, dim=0, index=idx)} if return_features else {}
        return top_instance, Y_prob, Y_hat, y_probs, results


class MIL_fc_mc(_MaxPoolMIL):
    """Multi-class max-pooling MIL (model_mil.py:46-93): one ``Linear(S1, 1)`` per class; the largest of all N * C probabilities
    names the instance and the class."""

    _multi = True

    def __init__(self, gate=True, size_arg="small", dropout=False, n_classes=2, top_k=1):
        super().__init__()
        assert n_classes > 2
        if n_classes > MAX_CLASSES:
            raise ValueError(f"n_classes = {n_classes}: the kernel takes 3 to {MAX_CLASSES} classes")
        size = _size(size_arg)
        fc = [nn.Linear(size[0], size[1]), nn.ReLU()]
        if dropout:
            fc.append(nn.Dropout(0.25))
        self.fc = nn.Sequential(*fc)
        self.classifiers = nn.ModuleList([nn.Linear(size[1], 1) for _ in range(n_classes)])
        initialize_weights(self)
        self.n_classes = n_classes
        self._setup(size, dropout, n_classes, top_k)

    def relocate(self):
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.fc = self.fc.to(device)
        self.classifiers = self.classifiers.to(device)

    def _fc1(self):
        return self.fc[0]

    def _hidden(self, h):
        return self.fc(h)

    def _logits(self, h1):
        return torch.cat([c(h1) for c in self.classifiers], dim=1)

    def _w2(self):
        return torch.cat([c.weight for c in self.classifiers], dim=0), torch.cat([c.bias for c in self.classifiers], dim=0)

    def _finish(self, logits, y_probs, h1, return_features):
        m = y_probs.reshape(1, -1).argmax(1)
        row, cls = m // self.n_classes, m % self.n_classes
        results = {'features': torch.index_select(h1, dim=0, index=row)} if return_features else {}
        return logits[row], y_probs[row], cls, y_probs, results
