"""The one host path of single-bag CLAM inference (``CLAM_SB._infer`` over ``functional.clam_forward``) on its three routes: ``CLAM_SB``
(one ``hipt_clam_sb_forward``), ``CLAM_MB`` in one pass (one ``hipt_clam_mb_forward``) and ``CLAM_MB`` branch by branch (K
``hipt_clam_sb_forward`` into rows of shared outputs), each with and without ``attention_only`` and ``instance_eval``.

Two kinds of assertion.  The native calls a forward issues -- symbol, scalar arguments, which pointers are NULL, the workspace slot --
against literal lists, written down from the code this path replaced.  And bits: every output equals what the same entry points give
when the test calls them itself with the module's packed weights, a second forward on the same stream repeats them (the workspace's
ticket block is left at zero), and the instance branch equals ``_instance_branch`` on rows the test gathers itself.

Widths: [192, 128, 64] in bf16 (the streaming kernel) and fp32 (the fused kernel), [1024, 512, 256] fp32 (the generic GEMM route, as
``test_clam_generic_then_streaming_model_share_one_workspace``).  Rows 1, ``k_sample`` = 8 and 257 (two 128-row tiles and one row)."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from hipt_abmil_atec23_amd import _native as N, functional as Fn, synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
K_SAMPLE = 8
WIDTHS = [("bf16", (192, 128, 64)), ("fp32", (192, 128, 64)), ("fp32", (1024, 512, 256))]
# (class, branches, one_pass)
MODELS = [("sb", 1, True), ("mb", 2, True), ("mb", 4, True), ("mb", 2, False), ("mb", 4, False)]
FORWARDS = ("hipt_clam_sb_forward", "hipt_clam_mb_forward")
P, Z = True, False   # a pointer argument is given / NULL

_modules = {}


def module(kind, K, dtype, size):
    key = (kind, K, dtype, size)
    if key not in _modules:
        from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB
        multi = kind == "mb"
        m = (CLAM_MB if multi else CLAM_SB)(size_arg=list(size), k_sample=K_SAMPLE, n_classes=K if multi else 2, subtyping=True)
        m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=K if multi else 2, multi=multi), 40 + K), strict=True)
        _modules[key] = m.eval().to(DEV).set_compute_dtype(dtype)
    return _modules[key]


class Recorder:
    """``_native.call`` that notes every call and forwards it to the real one"""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __call__(self, name, *args):
        self.calls.append((name, args))
        return self.real(name, *args)

    def summary(self, slot):
        """[(symbol, scalar arguments, which pointer arguments are given)]; the workspace of a forward call is checked against the slot's
        buffer here and its byte count left out of the scalars"""
        out = []
        for name, args in self.calls:
            scalars = tuple(a for a in args if isinstance(a, int))
            ptrs = [a for a in args if not isinstance(a, (int, N.StreamArg))]
            given = tuple(a is not None and not (isinstance(a, C.c_void_p) and not a.value) for a in ptrs)
            if name in FORWARDS:
                ws = Fn._workspaces[("cuda", 0, (slot, N.stream_ptr(torch.device(DEV)).value))]
                assert ptrs[-1].value == ws.data_ptr() and scalars[-1] == ws.numel(), (name, slot)
                scalars = scalars[:-1]
            out.append((name, scalars, given))
        return out


def expected_calls(route, K, n, attention_only, instance_eval):
    """The calls of one forward, as the code before the single path issued them (model_clam.py of the parent commit: CLAM_SB.forward,
    CLAM_MB._multi_infer, _multi_finish)."""
    a = int(attention_only)
    if route == "mb":      # (w, bag, n, attention_only, A_raw, M, logits, ws, bytes, stream)
        calls = [("hipt_clam_mb_forward", (n, a), (P, P, P, Z, Z, P) if a else (P, P, P, P, P, P))]
    else:                  # (w, bag, n, attention_only, A_raw, M, logits, Y_prob, Y_hat, ws, bytes, stream), once per branch
        calls = [("hipt_clam_sb_forward", (n, a), (P, P, P, Z, Z, Z, Z, P) if a else (P, P, P, P, P, P, P, P))] * K
    if instance_eval and not attention_only:
        calls += [("hipt_topk_rows", (K, n, K_SAMPLE), (P, P)),                       # (A_raw, K, n, k, ids, stream)
                  ("hipt_clam_gather_h1", (2 * K * K_SAMPLE,), (P, P, P, P))]         # (w, bag, ids, rows, out, stream)
    return calls


def direct(route, ws_branches, w_one, bag):
    """(A_raw [K, n], M [K, S1], logits [1, C or K], Y_prob, Y_hat) from the entry points themselves, on a workspace of the test's own"""
    dev, n = bag.device, bag.shape[0]
    st = N.stream_ptr(dev)
    e = lambda *shape, dt=torch.float32: torch.full(shape, -7, dtype=dt, device=dev)
    if route == "mb":
        w = w_one
        K = w.n_att
        A, M, lg = e(K, n), e(K, w.s1), e(1, K)
        ws = torch.zeros(N.lib().hipt_clam_mb_workspace_bytes(C.byref(w), n), dtype=torch.uint8, device=dev)
        N.call("hipt_clam_mb_forward", C.byref(w), N.ptr(bag), n, 0, N.ptr(A), N.ptr(M), N.ptr(lg), N.ptr(ws), ws.numel(), st)
        return A, M, lg, F.softmax(lg, dim=1), torch.topk(lg, 1, dim=1)[1]
    K = len(ws_branches)
    w0 = ws_branches[0]
    A, M, lg, yp, yh = e(K, n), e(K, w0.s1), e(K, w0.n_classes), e(K, w0.n_classes), e(K, 1, dt=torch.int64)
    ws = torch.zeros(N.lib().hipt_clam_workspace_bytes(C.byref(w0), n), dtype=torch.uint8, device=dev)
    for k, w in enumerate(ws_branches):
        N.call("hipt_clam_sb_forward", C.byref(w), N.ptr(bag), n, 0, N.ptr(A[k]), N.ptr(M[k]), N.ptr(lg[k]), N.ptr(yp[k]), N.ptr(yh[k]),
               N.ptr(ws), ws.numel(), st)
    if route == "sb":
        return A, M, lg, yp, yh
    lg = lg.reshape(1, K)       # (one-class branches: logits [K, 1] -> [1, K]; Y_prob / Y_hat over the K of them by torch, :251-252)
    return A, M, lg, F.softmax(lg, dim=1), torch.topk(lg, 1, dim=1)[1]


def gathered_rows(w, bag, A_raw, k):
    """h1 rows of the k highest / k lowest scores per branch, [K, 2, k, S1], by the test's own calls"""
    K, n = A_raw.shape
    st = N.stream_ptr(bag.device)
    ids = torch.empty((K, 2, k), dtype=torch.int64, device=bag.device)
    N.call("hipt_topk_rows", N.ptr(A_raw.contiguous()), K, n, k, N.ptr(ids), st)
    rows = torch.empty((K, 2, k, w.s1), dtype=torch.float32, device=bag.device)
    N.call("hipt_clam_gather_h1", C.byref(w), N.ptr(bag), N.ptr(ids), 2 * K * k, N.ptr(rows), st)
    return rows


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)


@pytest.mark.parametrize("n", [1, K_SAMPLE, 257])
@pytest.mark.parametrize("dtype,size", WIDTHS, ids=[f"{d}-{s[0]}x{s[1]}x{s[2]}" for d, s in WIDTHS])
@pytest.mark.parametrize("kind,K,one_pass", MODELS, ids=[f"{k}{b}{'' if o else '-by-branch'}" for k, b, o in MODELS])
def test_forward_issues_the_calls_and_returns_the_bits_of_direct_calls(monkeypatch, kind, K, one_pass, dtype, size, n):
    dev = torch.device(DEV)
    m = module(kind, K, dtype, size)
    monkeypatch.setattr(m, "one_pass", one_pass, raising=False)
    h = synth.hash_uniform_torch((n, size[0]), 300 + n, device=DEV)
    label = torch.tensor([1], device=DEV)
    with torch.no_grad():
        m(h, attention_only=True)   # (packs the weight images, outside the recording)
    if kind == "sb":
        w_one, branches = m._pack(dev), [m._pack(dev)]
        assert bool(w_one.stream_pk) == (dtype == "bf16")      # bf16 [192, 128, 64]: the streaming kernel's image exists
        route, slot = "sb", "clam"
    else:
        branches, w_one = m._pack_branches(dev)
        assert (w_one is not None) == (dtype == "bf16")        # the one-pass kernel is the streaming one: bf16 only
        route = "mb" if one_pass and w_one is not None else "branches"
        slot = "clam_mb" if route == "mb" else "clam"
    bag = Fn.as_compute(h, branches[0].dtype)
    A, M, lg, yp, yh = direct(route, branches, w_one, bag)
    real = N.call
    for attention_only in (False, True):
        for instance_eval in (False, True):
            rec = Recorder(real)
            monkeypatch.setattr(N, "call", rec)
            kw = dict(label=label, instance_eval=instance_eval, return_features=True, attention_only=attention_only)
            fails = instance_eval and not attention_only and n < K_SAMPLE
            with torch.no_grad():
                if fails:
                    with pytest.raises(RuntimeError, match=f"selected index k out of range: k_sample={K_SAMPLE} > {n} rows"):
                        m(h, **kw)
                else:
                    out, again = m(h, **kw), m(h, **kw)
            monkeypatch.setattr(N, "call", real)
            torch.cuda.synchronize()
            want = expected_calls(route, K if kind == "mb" else 1, n, attention_only, instance_eval and not fails)
            assert rec.summary(slot) == (want if fails else want + want), (attention_only, instance_eval)
            ticket = Fn._workspaces.get(("cuda", 0, ("clam", N.stream_ptr(dev).value)))    # (none yet where only the one-pass call has run)
            assert ticket is None or int(ticket[:256].sum()) == 0
            if fails:
                continue
            if attention_only:
                assert same(out, A) and same(again, A)
                continue
            for got in (out, again):
                logits, Y_prob, Y_hat, A_raw, res = got
                assert same(A_raw, A) and same(logits, lg) and same(res["features"], M) and same(Y_prob, yp) and same(Y_hat, yh)
            if instance_eval:
                rows = gathered_rows(branches[0], bag, A, K_SAMPLE)
                ref = m._instance_branch(lambda b: (rows[b, 0], rows[b, 1]), label)
                for got in (out, again):
                    res = got[4]
                    assert sorted(res) == ["features", "inst_labels", "inst_preds", "instance_loss"]
                    assert same(res["instance_loss"], ref["instance_loss"])
                    assert (res["inst_preds"] == ref["inst_preds"]).all() and (res["inst_labels"] == ref["inst_labels"]).all()
                    assert len(res["inst_preds"]) == len(ref["inst_preds"]) == K_SAMPLE * (2 + (len(m.instance_classifiers) - 1))
            else:
                assert sorted(out[4]) == ["features"]


def test_clam_forward_writes_into_given_outputs_and_forward_checks_the_bag():
    """``functional.clam_forward`` with ``out=`` and ``ws=``: the given buffers are the ones returned and written, with the bits of a
    call that allocates its own.  The bag is checked once, in ``forward``: a wrong shape or device is refused, by both classes with one
    message, before anything is launched."""
    dev = torch.device(DEV)
    m = module("sb", 1, "bf16", (192, 128, 64))
    w = m._pack(dev)
    bag = synth.hash_uniform_torch((257, 192), 557, device=DEV).bfloat16()
    fresh = Fn.clam_forward(w, bag)
    out = (torch.empty(1, 257, device=DEV), torch.empty(1, 128, device=DEV), torch.empty(1, 2, device=DEV), torch.empty(1, 2, device=DEV),
           torch.empty(1, 1, dtype=torch.int64, device=DEV))
    ws = torch.zeros(N.lib().hipt_clam_workspace_bytes(C.byref(w), 257), dtype=torch.uint8, device=DEV)
    got = Fn.clam_forward(w, bag, out=out, ws=ws)
    torch.cuda.synchronize()
    assert all(a is b for a, b in zip(got, out)) and all(same(a, b) for a, b in zip(got, fresh))
    before = N.calls
    with torch.no_grad():
        for mod in (m, module("mb", 2, "bf16", (192, 128, 64))):
            for bad in (bag[:, :128], bag[:0], bag[0], bag.reshape(1, 257, 192)):
                with pytest.raises(ValueError, match=r"expected a non-empty \[N, 192\] bag"):
                    mod(bad)
            with pytest.raises(RuntimeError, match="HIP device"):
                mod(bag.cpu())
    assert N.calls == before
