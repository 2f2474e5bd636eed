"""What the GPU tests of the multi-bag CLAM forward share: ``FORMS``, the test-side registry of the six forms of
``functional._BAGS_FORMS`` (tests/test_gpu_clam_forms.py runs the battery every form shares over it; the per-form files keep what is
their own), models and bags made from ``synth``, the per-bag references, the runners and the comparison helpers.  A plain module."""
import collections
import contextlib
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import clam_mb_ref as R
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N, synth
from hipt_abmil_atec23_amd import functional as Fn
from oracle import hipt_oracle as O

DEV = "cuda:0"
TOL = 1e-4           # the project's fp32 bar (tests/test_gpu_parity.py)
OUTS = ("A_raw", "M", "logits", "Y_prob")
FENCE, FILL = 4096, 0xA5

FAKE = 1 << 20       # a non-null, 4 KiB-aligned address that no call dereferences before its checks (the host tests' pointers)
E_BADARG, E_UNSUPPORTED = -1, -4


def W(s0, s1, s2, K=1, dtype=N.HIPT_F32, n_classes=None):
    """the fields of a ``ClamWeights`` for the host tests: K = 1 is CLAM_SB with two classes, K > 1 a CLAM_MB with K classes"""
    return dict(dtype=dtype, s0=s0, s1=s1, s2=s2, n_att=K, n_classes=(2 if K == 1 else K) if n_classes is None else n_classes)


# The test-side registry, under the names and in the order of functional._BAGS_FORMS.  GPU side: model class, the switches to set, the
# functional wrapper (the entry point is "hipt_" + its name), its workspace and supported symbols, K-branch outputs, the row counts of a
# call (bags of 1 and 2 rows, ends before, on and after a block of the kernel and a 128-row unit), the (size, K) cases of the invariance
# test, the workgroup cap of its small-grid run (HIPT_BAGS_MAX_WG).  Host side: weights the form takes, weights it does not take, the
# (size, classes) of a CPU model.
Form = collections.namedtuple("Form", "cls switches call ws_bytes supported multi rows invariance grid_cap takes takes_not cpu")
BF16 = N.HIPT_BF16
FORMS = {
    "sb": Form(CLAM_SB, (), Fn.clam_sb_forward_bags, "hipt_clam_bags_workspace_bytes", "hipt_clam_bags_supported", False,
               (1, 127, 128, 129, 300, 2, 1000), [((384, 128, 64), 2)], 3,
               W(384, 128, 64), [W(1024, 512, 256), W(192, 32, 16, dtype=BF16)], ([64, 128, 64], 2)),
    "narrow": Form(CLAM_SB, ("bags_narrow",), Fn.clam_sb_forward_bags_narrow, "hipt_clam_narrow_bags_workspace_bytes",
                   "hipt_clam_narrow_bags_supported", False, (1, 2, 31, 33, 127, 128, 129, 300, 1100),
                   [((192, 16, 8), 2), ((192, 8, 4), 2), ((1024, 32, 8), 2)], 3,
                   W(192, 16, 8), [W(384, 128, 64), W(1024, 512, 256), W(192, 64, 32), W(200, 16, 8), W(96, 16, 8, dtype=BF16)], ([192, 16, 8], 2)),
    "wide": Form(CLAM_SB, ("bags_wide",), Fn.clam_sb_forward_bags_wide, "hipt_clam_wide_bags_workspace_bytes", "hipt_clam_wide_bags_supported",
                 False, (1, 2, 31, 33, 63, 65, 127, 128, 129, 300, 1100), [((128, 256, 64), 2), ((128, 512, 256), 2), ((1024, 512, 384), 2)], 3,
                 W(1024, 512, 256), [W(384, 128, 64), W(192, 16, 8), W(100, 512, 256), W(96, 256, 64, dtype=BF16)], ([64, 256, 64], 2)),
    "mb": Form(CLAM_MB, ("bags_one_call",), Fn.clam_mb_forward_bags, "hipt_clam_mb_bags_workspace_bytes", "hipt_clam_mb_bags_supported", True,
               (1, 127, 128, 129, 300, 2, 1100), [((384, 128, 64), 2)], 3,
               W(384, 128, 64, 2), [W(384, 128, 64, 2, n_classes=3), W(384, 128, 64, 5), W(1024, 512, 256, 2)], ([64, 128, 64], 2)),
    "mb_many": Form(CLAM_MB, ("bags_one_call", "bags_many"), Fn.clam_mb_forward_bags_many, "hipt_clam_mb_many_bags_workspace_bytes",
                    "hipt_clam_mb_many_bags_supported", True, (1, 2, 15, 17, 127, 128, 129, 300), [((64, 128, 64), 5), ((128, 64, 16), 7)], 1,
                    W(384, 128, 64, 5), [W(384, 128, 64, 4), W(384, 128, 64, 9), W(1024, 512, 256, 5)], ([64, 128, 64], 5)),
    "mb_wide": Form(CLAM_MB, ("bags_one_call", "bags_wide"), Fn.clam_mb_forward_bags_wide, "hipt_clam_mb_wide_bags_workspace_bytes",
                    "hipt_clam_mb_wide_bags_supported", True, (1, 2, 31, 33, 63, 65, 127, 128, 129, 300),
                    [((128, 256, 64), 4), ((128, 512, 256), 3), ((1024, 512, 384), 2)], 3,
                    W(1024, 512, 256, 2), [W(384, 128, 64, 2), W(1024, 512, 256, 5), W(96, 256, 64, 2, dtype=BF16)], ([64, 256, 64], 2)),
}


def entry_of(form):
    return "hipt_" + FORMS[form].call.__name__


def md(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return float(np.abs(a.astype(np.float64).reshape(-1) - np.asarray(b, dtype=np.float64).reshape(-1)).max())


def bits(t):
    return t.detach().contiguous().cpu().numpy().tobytes()


@functools.lru_cache(maxsize=None)
def make(size, dtype="fp32", cls=CLAM_SB, n_classes=2, subtyping=False):
    m = cls(size_arg=list(size), n_classes=n_classes, subtyping=subtyping)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=n_classes, multi=cls is CLAM_MB), size[0]), strict=True)
    m.relocate()
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


# ---- the scaffolding of the per-form files and of tests/test_gpu_clam_forms.py ------------------------------------------------------
def model(form, size, dtype="fp32", K=2, subtyping=False):
    """the cached model of ``form``'s class, its switches at their defaults"""
    return make(tuple(size), dtype, FORMS[form].cls, K, subtyping)


def pack(form, m):
    """the weight image the form's call takes"""
    return m._pack_stacked(torch.device(DEV)) if FORMS[form].multi else m._pack(torch.device(DEV))


@contextlib.contextmanager
def switched(m, switches):
    """``switches`` (a form's name, or a tuple of switch names) set on a cached model for a ``with`` block, then deleted"""
    names = FORMS[switches].switches if isinstance(switches, str) else tuple(switches)
    for s in names:
        setattr(m, s, True)
    try:
        yield m
    finally:
        for s in names:
            delattr(m, s)


def as_out(ret):
    logits, y_prob, y_hat, a_raw, res = ret
    return {"A_raw": a_raw, "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat, "res": res}


def run_form(m, form, bags, **kw):
    """forward_bags on a sequence of bags or on ``(cat, BagOffsets)`` with the form's switches set, on the one-call route"""
    with switched(m, form):
        pair = len(bags) == 2 and isinstance(bags[1], Fn.BagOffsets)
        ret = m.forward_bags(bags if pair else list(bags), return_features=True, **kw)
        assert m.bags_route == "bags"
    torch.cuda.synchronize()
    return as_out(ret)


def run_loop(m, bags):
    with torch.no_grad():   # (with gradients enabled forward() takes the fp32 training kernels)
        outs = [m(b, return_features=True) for b in bags]
    torch.cuda.synchronize()
    return {"A_raw": [o[3] for o in outs], "M": (torch.stack if m._multi else torch.cat)([o[4]["features"] for o in outs]),
            "logits": torch.cat([o[0] for o in outs]), "Y_prob": torch.cat([o[1] for o in outs]), "Y_hat": torch.cat([o[2] for o in outs])}


def offsets_of(rows):
    return Fn.BagOffsets(np.cumsum([0, *rows]), sum(rows), torch.device(DEV))


def direct(form, w, bags, rows, **kw):
    """the form's ``functional`` wrapper on the concatenated bags: ``(its five outputs, cat, offsets)``"""
    cat = Fn.as_compute(torch.cat(list(bags), dim=0), w.dtype)
    off = offsets_of(rows)
    return FORMS[form].call(w, cat, off, **kw), cat, off


def a_bits(views):
    """the [K, rows] score matrix of a call (K = 1: [1, rows]), from its per-bag views"""
    return bits(torch.cat(list(views), dim=1))


def fenced_buffers():
    """``(buf, fences_hold)``: ``buf(nbytes, dtype)`` is a 256-byte aligned buffer of FILL bytes between two guard regions of FENCE
    bytes; ``fences_hold()`` asserts that every guard region made so far still holds FILL."""
    fenced = []

    def buf(nbytes, dt=torch.uint8):
        raw = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        fenced.append((raw, nbytes))
        return raw[FENCE:FENCE + nbytes].view(dt)

    def fences_hold():
        for raw, n in fenced:
            assert bool((raw[:FENCE] == FILL).all()) and bool((raw[FENCE + n:] == FILL).all()), "a write outside a buffer"
    return buf, fences_hold


def fenced_out(form, buf, w, B, rows):
    """the five outputs of the form's call on B bags of ``rows`` rows in all, each exactly its size between guard regions"""
    K = w.n_att
    a, m, l = ((K, rows), (B, K, w.s1), (B, K)) if FORMS[form].multi else ((rows,), (B, w.s1), (B, w.n_classes))
    f = lambda shape: buf(4 * math.prod(shape), torch.float32).view(shape)   # noqa: E731
    return f(a), f(m), f(l), f(l), buf(B * 8, torch.int64)


# ---- the checks every form shares, stated once: a form's own file runs them on its cases, tests/test_gpu_clam_forms.py on the rest ----
def setup(form, size, K, dtype, rows=None, seed=9):
    rows = tuple(FORMS[form].rows if rows is None else rows)
    return model(form, size, dtype, K), bags_of(size[0], seed, rows), rows


def check_neighbours(form, size, K, dtype, monkeypatch):
    """A bag does not see its neighbours: against the bag alone, the reversed order, the order shifted by one, and the small grid"""
    m, bags, _ = setup(form, size, K, dtype)
    multi, B = FORMS[form].multi, len(bags)
    full = run_form(m, form, bags)
    rev = run_form(m, form, bags[::-1])
    mid = run_form(m, form, [bags[(b + 1) % B] for b in range(B)])      # every bag one place earlier: the first goes last
    monkeypatch.setenv("HIPT_BAGS_MAX_WG", str(FORMS[form].grid_cap))   # all work units over 3 workgroups (mb_many: one) instead of one each
    few = run_form(m, form, bags)
    monkeypatch.delenv("HIPT_BAGS_MAX_WG")
    for b in range(B):
        assert_same_bits(per_bag(full, b, multi), per_bag(run_form(m, form, [bags[b]]), 0, multi), f"bag {b} alone")
        assert_same_bits(per_bag(full, b, multi), per_bag(rev, B - 1 - b, multi), f"bag {b} reversed order")
        assert_same_bits(per_bag(full, b, multi), per_bag(mid, (b - 1) % B, multi), f"bag {b} shifted")
        assert_same_bits(per_bag(full, b, multi), per_bag(few, b, multi), f"bag {b} small grid")


def check_attention_only(form, size, K, dtype):
    """``attention_only`` writes A_raw alone: the views of ``forward_bags`` and the form's wrapper, into fenced outputs with a fenced
    workspace of exactly workspace_bytes; a short or misaligned workspace is refused in this mode too"""
    m, bags, rows = setup(form, size, K, dtype)
    full = run_form(m, form, bags)
    with switched(m, form):
        views = m.forward_bags(list(bags), attention_only=True)
        assert m.bags_route == "bags"
    Ka = K if FORMS[form].multi else 1
    assert [tuple(v.shape) for v in views] == [(Ka, n) for n in rows] and [bits(v) for v in views] == [bits(a) for a in full["A_raw"]]
    w = pack(form, m)
    need = getattr(N.lib(), FORMS[form].ws_bytes)(C.byref(w), len(rows), sum(rows))
    assert need > 0 and need % 256 == 0
    buf, fences_hold = fenced_buffers()
    out, ws = fenced_out(form, buf, w, len(rows), sum(rows)), buf(need)
    direct(form, w, bags, rows, attention_only=True, out=out, ws=ws)
    torch.cuda.synchronize()
    fences_hold()
    assert bits(out[0]) == a_bits(full["A_raw"])
    assert all(bool((t.contiguous().view(torch.uint8) == FILL).all()) for t in out[1:]), "attention_only wrote a pooled output"
    for bad in (ws[:need - 256], ws[16:]):
        with pytest.raises(RuntimeError, match="code -?[0-9]+"):
            direct(form, w, bags, rows, attention_only=True, out=out, ws=bad)
    fences_hold()


def check_fences(form, size, K, dtype, rows=None):
    """Outputs and a workspace of exactly workspace_bytes stay inside fenced buffers and hold the bits of ``forward_bags``; a second
    call on the used workspace gives the same bits; a short or misaligned workspace is refused before anything is written"""
    m, bags, rows = setup(form, size, K, dtype, rows)
    w = pack(form, m)
    need = getattr(N.lib(), FORMS[form].ws_bytes)(C.byref(w), len(rows), sum(rows))
    assert need > 0 and need % 256 == 0
    buf, fences_hold = fenced_buffers()
    out, ws = fenced_out(form, buf, w, len(rows), sum(rows)), buf(need)
    full = run_form(m, form, bags)
    for call in ("first", "second, on the used workspace"):
        for t in out:
            t.view(torch.uint8).fill_(FILL)
        direct(form, w, bags, rows, out=out, ws=ws)
        torch.cuda.synchronize()
        fences_hold()
        assert bits(out[0]) == a_bits(full["A_raw"]) and bits(out[1]) == bits(full["M"]) and bits(out[2]) == bits(full["logits"]), call
        assert bits(out[3]) == bits(full["Y_prob"]) and bits(out[4]) == bits(full["Y_hat"]), call
    for bad in (ws[:need - 256], ws[16:]):
        with pytest.raises(RuntimeError, match="code -?[0-9]+"):
            direct(form, w, bags, rows, out=out, ws=bad)
    fences_hold()


# ---- the host side (no GPU; every pointer is FAKE): the calls and the checks the forms share ----------------------------------------
ARGUMENT_CASES = [
    ("null weights", dict(w=None, nbytes=1 << 20)), ("null bags", dict(bags=None)), ("null offsets", dict(offsets=None)),
    ("null A_raw", dict(A_raw=None)), ("null M", dict(M=None)), ("null logits", dict(logits=None)), ("null Y_prob", dict(Y_prob=None)),
    ("null Y_hat", dict(Y_hat=None)), ("null workspace", dict(ws=None)), ("misaligned bags", dict(bags=FAKE + 8)),
    ("no bag", dict(B=0, nbytes=1 << 20)), ("negative B", dict(B=-3, nbytes=1 << 20)), ("fewer rows than bags", dict(B=7, rows=6, nbytes=1 << 20)),
    ("short workspace", dict(nbytes="short")), ("misaligned workspace", dict(ws=FAKE + 16)),
]


def fake_weights(dtype, s0, s1, s2, n_classes, n_att):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_classes, n_att=n_att)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def call_entry(form, w, bags=FAKE, offsets=FAKE, B=7, rows=1000, attention_only=0, A_raw=FAKE, M=FAKE, logits=FAKE, Y_prob=FAKE, Y_hat=FAKE,
               ws=FAKE, nbytes=None):
    """the form's C entry point on fake pointers: ``(return code, hipt_last_error)``"""
    lib = N.lib()
    if nbytes is None:
        nbytes = getattr(lib, FORMS[form].ws_bytes)(C.byref(w), B, rows)
    rc = getattr(lib, entry_of(form))(C.byref(w) if w is not None else None, bags, offsets, B, rows, attention_only, A_raw, M, logits, Y_prob,
                                      Y_hat, ws, nbytes, None)
    return rc, lib.hipt_last_error().decode()


def check_argument_error(form, case, kw):
    """a case of ARGUMENT_CASES comes back as HIPT_E_BADARG under the entry point's own name, before any device work"""
    kw = dict(kw)
    w = kw.pop("w", fake_weights(**FORMS[form].takes))
    if kw.get("nbytes") == "short":
        need = getattr(N.lib(), FORMS[form].ws_bytes)(C.byref(w), 7, 1000)
        assert need > 0
        kw["nbytes"] = need - 1
    rc, msg = call_entry(form, w, **kw)
    assert rc == E_BADARG, case
    assert msg.startswith(entry_of(form)[len("hipt_"):] + ": "), msg
    if "workspace" in case and "null" not in case:
        assert "workspace" in msg, msg


def check_attention_only_needs_no_pooled_outputs(form):
    """M .. Y_hat may be NULL -- the call gets past its checks (a short workspace is then what stops it)"""
    rc, msg = call_entry(form, fake_weights(**FORMS[form].takes), attention_only=1, M=None, logits=None, Y_prob=None, Y_hat=None, nbytes=256)
    assert rc == E_BADARG and "workspace" in msg, msg


def check_outside(form, outside=None):
    """every configuration of ``outside`` (default: the registry's) is unsupported, refused under the entry point's name, and sizes to zero"""
    f, lib = FORMS[form], N.lib()
    for takes_not in f.takes_not if outside is None else outside:
        w = fake_weights(**takes_not)
        rc, msg = call_entry(form, w, nbytes=1 << 24)
        assert rc == E_UNSUPPORTED and msg.startswith(entry_of(form)[len("hipt_"):] + ": "), (takes_not, msg)
        assert getattr(lib, f.supported)(C.byref(w)) == 0 and getattr(lib, f.ws_bytes)(C.byref(w), 7, 1000) == 0, takes_not
    assert getattr(lib, f.supported)(None) == 0 and getattr(lib, f.ws_bytes)(None, 7, 1000) == 0


def check_workspace_grows(form, takes=None):
    """the workspace of a configuration the form takes grows with B and the rows, in multiples of 256 bytes, and is 0 for no bags"""
    f, lib = FORMS[form], N.lib()
    takes = f.takes if takes is None else takes
    w = fake_weights(**takes)
    assert getattr(lib, f.supported)(C.byref(w)) == 1
    size = lambda B, rows: getattr(lib, f.ws_bytes)(C.byref(w), B, rows)   # noqa: E731
    base = size(7, 1000)
    assert base > 0 and base % 256 == 0
    assert size(64, 1000) > base and size(7, 100_000) > base and size(1, 1) > 0
    for B, rows in ((1, 1), (1, 129), (64, 14_400), (3, 100_000)):
        assert size(B, rows) % 256 == 0
        units = (rows + 127) // 128 + B      # upper bound of sum ceil(N_b / 128): what the host can know without reading the offsets
        assert size(B, rows) >= units * (16 + 4 * takes["n_att"] * (2 + takes["s1"])) + 4 * (B + 1)
    assert size(0, 10) == 0 and size(5, 4) == 0 and size(-1, 10) == 0


def cpu_model(form, **kw):
    torch.manual_seed(0)
    size, K = FORMS[form].cpu
    return FORMS[form].cls(size_arg=list(size), n_classes=K, **kw).eval()


def check_split_switch(form, keyword, flag, preset):
    """``narrow_one_call`` sets ``bags_narrow`` to what it says (default True); ``wide_one_call=True`` sets ``bags_wide``, ``False`` (the
    default) leaves the model's own value in force.  In every case the instance is afterwards as it was, also after an exception."""
    from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split
    switch = FORMS[form].switches[0]
    m = cpu_model(form, k_sample=2)
    if preset is not None:
        setattr(m, switch, preset)
    inside = (flag, flag) if switch == "bags_narrow" else (flag or bool(preset), True)      # (this switch, bags_narrow) inside the call
    seen = []
    inner = m.forward_bags

    def spy(*a, **kw):
        seen.append((getattr(m, switch), m.bags_narrow))
        return inner(*a, **kw)

    def boom(*a, **kw):
        seen.append((getattr(m, switch), m.bags_narrow))
        raise KeyError("inside forward_bags")

    def as_before():
        other = "bags_narrow" in m.__dict__ if switch != "bags_narrow" else False
        return m.__dict__.get(switch, None) is preset and getattr(m, switch) is bool(preset) and not other

    m.forward_bags = spy
    bags = [torch.randn(n, m._sizes[0]) for n in (4, 5, 3)]
    labels = [0, 1, 1]
    evaluate_split(m, bags, labels, 2, **{keyword: flag})
    validate_split(m, bags, labels, 2, **{keyword: flag})
    assert seen == [inside, inside] and as_before()
    m.forward_bags = boom
    for fn in (evaluate_split, validate_split):
        with pytest.raises(KeyError):
            fn(m, bags, labels, 2, **{keyword: flag})
        assert as_before()
    assert seen[2:] == [inside, inside]
