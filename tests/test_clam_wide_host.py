"""Host tests (no GPU) of the multi-bag CLAM_SB call for the wide heads (csrc/abmil_wide.hip): the three entry points exist in the
library, the header and the binding; the envelope table answers yes for exactly (S1, S2) in {(256, 64), (512, 256), (512, 384)} with
S0 a multiple of the K-slab, in both dtypes, and leaves ``hipt_clam_bags_supported`` as it was; the workspace size is 0 outside the
envelope; every argument error comes back as HIPT_E_BADARG with the entry point's prefix before anything is dereferenced or launched
(all pointers here are fake addresses); ``CLAM_SB.bags_wide`` is off by default, does nothing on the CPU, and ``evaluate_split`` /
``validate_split`` set it for their own duration only."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from hipt_abmil_atec23_amd import CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks
E_BADARG, E_UNSUPPORTED = -1, -4
NAMES = ("hipt_clam_wide_bags_supported", "hipt_clam_wide_bags_workspace_bytes", "hipt_clam_sb_forward_bags_wide")
PREFIX = "clam_sb_forward_bags_wide: "
F32, BF16 = N.HIPT_F32, N.HIPT_BF16
PAIRS = ((256, 64), (512, 256), (512, 384))
WIDE = [(dt, s0, s1, s2) for dt in (F32, BF16) for s0 in (128, 512, 1024) for s1, s2 in PAIRS] + [(F32, 96, 256, 64), (F32, 32, 512, 256)]


def weights(dtype=F32, s0=1024, s1=512, s2=256, n_classes=2):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_classes, n_att=1)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def forward(lib, w, bags=FAKE, offsets=FAKE, B=7, rows=1000, attention_only=0, A_raw=FAKE, M=FAKE, logits=FAKE, Y_prob=FAKE, Y_hat=FAKE,
            ws=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = lib.hipt_clam_wide_bags_workspace_bytes(C.byref(w), B, rows)
    return lib.hipt_clam_sb_forward_bags_wide(C.byref(w) if w is not None else None, bags, offsets, B, rows, attention_only, A_raw, M,
                                              logits, Y_prob, Y_hat, ws, nbytes, None)


def test_symbols_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    declared = set(re.findall(r"\b(hipt_[a-z0-9_]+)\s*\(", hdr))
    lib = N.lib()
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert N.SIGNATURES["hipt_clam_sb_forward_bags_wide"] == N.SIGNATURES["hipt_clam_sb_forward_bags"]
    assert N.SIGNATURES["hipt_clam_wide_bags_workspace_bytes"] == N.SIGNATURES["hipt_clam_bags_workspace_bytes"]
    assert "wide" in Fn._BAGS_FORMS and Fn._BAGS_FORMS["wide"][:2] == NAMES[:0:-1]
    assert callable(Fn.clam_sb_forward_bags_wide)


def test_supported_is_the_wide_table():
    lib = N.lib()
    sup = lambda *a: lib.hipt_clam_wide_bags_supported(C.byref(weights(*a)))
    assert [sup(*a) for a in WIDE] == [1] * len(WIDE)
    no = [(F32, 384, 128, 64), (BF16, 384, 128, 64), (F32, 192, 16, 8), (BF16, 192, 16, 8),   # the other two forms' heads
          (F32, 100, 512, 256), (BF16, 100, 512, 256),                                       # S0 = 100
          (BF16, 96, 256, 64),                                                               # a multiple of 32, not of 64, in bf16
          (F32, 1024, 512, 128), (F32, 1024, 256, 128), (F32, 1024, 512, 64), (F32, 1024, 1024, 256), (F32, 1024, 256, 256),
          (2, 1024, 512, 256)]                                                               # no such dtype
    assert [sup(*a) for a in no] == [0] * len(no)
    # exactly the three pairs: every other (S1, S2) of the grid is refused
    for dt in (F32, BF16):
        for s1 in (32, 64, 128, 256, 384, 512, 768, 1024):
            for s2 in (16, 32, 64, 128, 256, 384, 512):
                assert sup(dt, 1024, s1, s2) == int((s1, s2) in PAIRS), (dt, s1, s2)
    assert lib.hipt_clam_wide_bags_supported(None) == 0


def test_the_other_forms_answer_as_before():
    lib = N.lib()
    for a in WIDE:
        w = weights(*a)
        assert lib.hipt_clam_bags_supported(C.byref(w)) == 0 and lib.hipt_clam_narrow_bags_supported(C.byref(w)) == 0, a
        assert lib.hipt_clam_bags_workspace_bytes(C.byref(w), 7, 1000) == 0, a
    w = weights(F32, 1024, 512, 256)      # CLAM_SB() with no arguments: `small`
    rc = lib.hipt_clam_sb_forward_bags(C.byref(w), FAKE, FAKE, 7, 1000, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 24, None)
    assert rc == E_UNSUPPORTED


@pytest.mark.parametrize("a", [(F32, 1024, 512, 256), (BF16, 1024, 512, 384), (BF16, 512, 256, 64)])
def test_workspace_grows_with_bags_and_rows(a):
    lib = N.lib()
    w = weights(*a)
    s1 = a[2]
    size = lambda B, rows: lib.hipt_clam_wide_bags_workspace_bytes(C.byref(w), B, rows)
    base = size(7, 1000)
    assert base > 0 and base % 256 == 0
    assert size(64, 1000) > base and size(7, 100_000) > base and size(1, 1) > 0
    for B, rows in ((1, 1), (1, 129), (64, 14_400), (3, 100_000)):
        units = (rows + 127) // 128 + B
        assert size(B, rows) % 256 == 0 and size(B, rows) >= units * (16 + 4 * (2 + s1)) + 4 * (B + 1)
    assert size(0, 10) == 0 and size(5, 4) == 0 and size(-1, 10) == 0


def test_workspace_is_zero_outside_the_envelope():
    lib = N.lib()
    for a in ((F32, 384, 128, 64), (F32, 192, 16, 8), (F32, 100, 512, 256), (BF16, 96, 256, 64)):
        assert lib.hipt_clam_wide_bags_workspace_bytes(C.byref(weights(*a)), 7, 1000) == 0, a
    assert lib.hipt_clam_wide_bags_workspace_bytes(None, 7, 1000) == 0


@pytest.mark.parametrize("case,kw", [
    ("null weights", dict(w=None, nbytes=1 << 20)), ("null bags", dict(bags=None)), ("null offsets", dict(offsets=None)),
    ("null A_raw", dict(A_raw=None)), ("null M", dict(M=None)), ("null logits", dict(logits=None)), ("null Y_prob", dict(Y_prob=None)),
    ("null Y_hat", dict(Y_hat=None)), ("null workspace", dict(ws=None)), ("misaligned bags", dict(bags=FAKE + 8)),
    ("no bag", dict(B=0, nbytes=1 << 20)), ("negative B", dict(B=-3, nbytes=1 << 20)), ("fewer rows than bags", dict(B=7, rows=6, nbytes=1 << 20)),
    ("short workspace", dict(nbytes="short")), ("misaligned workspace", dict(ws=FAKE + 16)),
])
def test_argument_errors_come_back_before_any_device_work(case, kw):
    lib = N.lib()
    kw = dict(kw)
    w = kw.pop("w", weights())
    if kw.get("nbytes") == "short":
        kw["nbytes"] = lib.hipt_clam_wide_bags_workspace_bytes(C.byref(w), 7, 1000) - 1
    assert forward(lib, w, **kw) == E_BADARG, case
    assert lib.hipt_last_error().decode().startswith(PREFIX), (case, lib.hipt_last_error().decode())


def test_attention_only_needs_no_pooled_outputs_and_other_widths_are_unsupported():
    lib = N.lib()
    assert forward(lib, weights(), attention_only=1, M=None, logits=None, Y_prob=None, Y_hat=None, nbytes=256) == E_BADARG
    assert "workspace" in lib.hipt_last_error().decode()
    for a in ((F32, 384, 128, 64), (F32, 192, 16, 8), (BF16, 100, 512, 256)):
        assert forward(lib, weights(*a), nbytes=1 << 24) == E_UNSUPPORTED, a
        msg = lib.hipt_last_error().decode()
        assert msg.startswith(PREFIX) and "(256,64)" in msg and "(512,256)" in msg and "(512,384)" in msg, msg


# ---- the Python switch --------------------------------------------------------------------------------------------------------
def wide_cpu_model(**kw):
    torch.manual_seed(0)
    return CLAM_SB(size_arg=[64, 256, 64], **kw).eval()


def test_bags_wide_is_off_by_default_and_a_cpu_model_ignores_it():
    assert CLAM_SB.bags_wide is False
    m = wide_cpu_model()
    assert "bags_wide" not in m.__dict__
    bags = [torch.randn(n, 64) for n in (1, 5, 3)]
    want = m.forward_bags(bags)
    assert m.bags_route == "per_bag"
    m.bags_wide = True
    before = N.calls
    got = m.forward_bags(bags)
    assert m.bags_route == "per_bag" and N.calls == before
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("preset", [None, True, False])
@pytest.mark.parametrize("flag", [True, False])
def test_split_functions_set_the_switch_for_their_duration_only(preset, flag):
    """``wide_one_call=True`` sets ``bags_wide`` inside the call; ``False`` (the default) leaves the model's own value in force.  In
    every case the instance is afterwards as it was, also after an exception."""
    m = wide_cpu_model(k_sample=2)
    if preset is not None:
        m.bags_wide = preset
    inside = flag or bool(preset)
    seen = []
    inner = m.forward_bags

    def spy(*a, **kw):
        seen.append((m.bags_wide, m.bags_narrow))
        return inner(*a, **kw)

    m.forward_bags = spy
    bags = [torch.randn(n, 64) for n in (4, 5, 3)]
    labels = [0, 1, 1]
    evaluate_split(m, bags, labels, 2, wide_one_call=flag)
    validate_split(m, bags, labels, 2, wide_one_call=flag)
    assert seen == [(inside, True), (inside, True)]
    assert m.__dict__.get("bags_wide", None) is preset and m.bags_wide is bool(preset) and "bags_narrow" not in m.__dict__

    def boom(*a, **kw):
        seen.append((m.bags_wide, m.bags_narrow))
        raise KeyError("inside forward_bags")

    m.forward_bags = boom
    for fn in (evaluate_split, validate_split):
        with pytest.raises(KeyError):
            fn(m, bags, labels, 2, wide_one_call=flag)
        assert m.__dict__.get("bags_wide", None) is preset and m.bags_wide is bool(preset) and "bags_narrow" not in m.__dict__
    assert seen[2:] == [(inside, True), (inside, True)]


def test_the_keyword_defaults_to_the_loop():
    import inspect
    for fn in (evaluate_split, validate_split):
        assert inspect.signature(fn).parameters["wide_one_call"].default is False
