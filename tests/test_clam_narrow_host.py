"""Host tests (no GPU) of the multi-bag CLAM_SB call for the narrow heads (csrc/abmil_narrow.hip): the three entry points exist in the
library, the header and the binding; the envelope table answers yes and no where it should and leaves ``hipt_clam_bags_supported``
as it was; the workspace size follows B and the row count; every argument error comes back before anything is dereferenced or
launched (all pointers here are fake addresses); ``CLAM_SB.bags_narrow`` is off by default, does nothing on the CPU, and
``evaluate_split`` / ``validate_split`` set it for their own duration only."""
import ctypes as C
import os
import re

import pytest
import torch

from conftest import ROOT
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks
E_BADARG, E_UNSUPPORTED = -1, -4
NAMES = ("hipt_clam_narrow_bags_supported", "hipt_clam_narrow_bags_workspace_bytes", "hipt_clam_sb_forward_bags_narrow")
F32, BF16 = N.HIPT_F32, N.HIPT_BF16
NARROW = [(dt, s0, s1, s2) for dt in (F32, BF16) for s0, s1, s2 in ((192, 8, 4), (192, 16, 8), (512, 32, 8), (1024, 32, 8), (192, 32, 16))]


def weights(dtype=F32, s0=192, s1=16, s2=8, n_classes=2):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_classes, n_att=1)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def forward(lib, w, bags=FAKE, offsets=FAKE, B=7, rows=1000, attention_only=0, A_raw=FAKE, M=FAKE, logits=FAKE, Y_prob=FAKE, Y_hat=FAKE,
            ws=FAKE, nbytes=None):
    if nbytes is None:
        nbytes = lib.hipt_clam_narrow_bags_workspace_bytes(C.byref(w), B, rows)
    return lib.hipt_clam_sb_forward_bags_narrow(C.byref(w) if w is not None else None, bags, offsets, B, rows, attention_only, A_raw, M,
                                                logits, Y_prob, Y_hat, ws, nbytes, None)


def test_symbols_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    declared = set(re.findall(r"\b(hipt_[a-z0-9_]+)\s*\(", hdr))
    lib = N.lib()
    for name in NAMES:
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
    assert N.SIGNATURES["hipt_clam_sb_forward_bags_narrow"] == N.SIGNATURES["hipt_clam_sb_forward_bags"]
    assert N.SIGNATURES["hipt_clam_narrow_bags_workspace_bytes"] == N.SIGNATURES["hipt_clam_bags_workspace_bytes"]
    # additions only: the version stays where other tests of this suite pin it
    assert lib.hipt_abi_version() == N.ABI_VERSION == 6 and re.search(r"#define HIPT_ABI_VERSION 6\b", hdr)


def test_supported_is_the_narrow_table():
    lib = N.lib()
    sup = lambda *a: lib.hipt_clam_narrow_bags_supported(C.byref(weights(*a)))
    assert [sup(*a) for a in NARROW] == [1] * len(NARROW)
    no = [(F32, 200, 16, 8),        # S0 not a multiple of 32
          (BF16, 96, 16, 8),        # S0 not a multiple of 64 in bf16
          (F32, 1024, 512, 256), (F32, 192, 64, 32), (BF16, 192, 64, 32), (F32, 384, 128, 64),   # the wide heads
          (F32, 192, 16, 4), (F32, 192, 8, 8), (BF16, 192, 16, 16), (F32, 192, 4, 2), (F32, 192, 24, 8),
          (2, 192, 16, 8)]          # no such dtype
    assert [sup(*a) for a in no] == [0] * len(no)
    assert lib.hipt_clam_narrow_bags_supported(None) == 0


def test_the_wide_call_answers_as_before():
    """The multi-bag call of the wide heads keeps its envelope: what tests/test_clam_bags_host.py pins, and every narrow width but
    fp32 (32, 16), which both tables hold."""
    lib = N.lib()
    for a in NARROW:
        both = a[0] == F32 and a[2:] == (32, 16)
        w = weights(*a)
        assert lib.hipt_clam_bags_supported(C.byref(w)) == int(both), a
        assert (lib.hipt_clam_bags_workspace_bytes(C.byref(w), 7, 1000) > 0) == both, a
    w = weights(F32, 192, 8, 4)
    rc = lib.hipt_clam_sb_forward_bags(C.byref(w), FAKE, FAKE, 7, 1000, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 24, None)
    assert rc == E_UNSUPPORTED
    w = weights(BF16, 192, 32, 16)
    rc = lib.hipt_clam_sb_forward_bags(C.byref(w), FAKE, FAKE, 7, 1000, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 24, None)
    assert rc == E_UNSUPPORTED


@pytest.mark.parametrize("a", NARROW)
def test_workspace_grows_with_bags_and_rows(a):
    lib = N.lib()
    w = weights(*a)
    s1 = a[2]
    size = lambda B, rows: lib.hipt_clam_narrow_bags_workspace_bytes(C.byref(w), B, rows)
    base = size(7, 1000)
    assert base > 0 and base % 256 == 0
    assert size(64, 1000) > base and size(7, 100_000) > base and size(1, 1) > 0
    for B, rows in ((1, 1), (1, 129), (64, 14_400), (3, 100_000)):
        assert size(B, rows) % 256 == 0
        units = (rows + 127) // 128 + B      # upper bound of sum ceil(N_b / 128): what the host can know without reading the offsets
        assert size(B, rows) >= units * (16 + 4 * (2 + s1)) + 4 * (B + 1)
    assert size(0, 10) == 0 and size(5, 4) == 0 and size(-1, 10) == 0


def test_workspace_is_zero_outside_the_envelope():
    lib = N.lib()
    for a in ((F32, 1024, 512, 256), (F32, 192, 64, 32), (F32, 200, 16, 8), (BF16, 96, 16, 8)):
        assert lib.hipt_clam_narrow_bags_workspace_bytes(C.byref(weights(*a)), 7, 1000) == 0, a
    assert lib.hipt_clam_narrow_bags_workspace_bytes(None, 7, 1000) == 0


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
        kw["nbytes"] = lib.hipt_clam_narrow_bags_workspace_bytes(C.byref(w), 7, 1000) - 1
    assert forward(lib, w, **kw) == E_BADARG, case
    assert lib.hipt_last_error().decode() != ""


def test_attention_only_needs_no_pooled_outputs_and_other_widths_are_unsupported():
    lib = N.lib()
    # attention_only: M .. Y_hat may be NULL -- the call gets past its checks (a short workspace is then what stops it)
    assert forward(lib, weights(), attention_only=1, M=None, logits=None, Y_prob=None, Y_hat=None, nbytes=256) == E_BADARG
    assert "workspace" in lib.hipt_last_error().decode()
    for a in ((F32, 1024, 512, 256), (F32, 192, 64, 32), (BF16, 384, 128, 64), (F32, 200, 16, 8)):
        assert forward(lib, weights(*a), nbytes=1 << 24) == E_UNSUPPORTED, a
        msg = lib.hipt_last_error().decode()
        assert "(8,4)" in msg and "(16,8)" in msg and "(32,8)" in msg and "(32,16)" in msg, msg   # the message names the widths


# ---- the Python switch --------------------------------------------------------------------------------------------------------
def narrow_cpu_model(cls=CLAM_SB, **kw):
    torch.manual_seed(0)
    return cls(size_arg="hipt_smaller", **kw).eval()


def test_bags_narrow_is_off_by_default_and_a_cpu_model_still_loops():
    assert CLAM_SB.bags_narrow is False
    m = narrow_cpu_model()
    assert "bags_narrow" not in m.__dict__
    bags = [torch.randn(n, 192) for n in (1, 5, 3)]
    want = m.forward_bags(bags)
    assert m.bags_route == "per_bag"
    m.bags_narrow = True
    before = N.calls
    got = m.forward_bags(bags)
    assert m.bags_route == "per_bag" and N.calls == before
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.parametrize("preset", [None, True, False])
@pytest.mark.parametrize("flag", [True, False])
def test_split_functions_set_the_switch_for_their_duration_only(preset, flag):
    m = narrow_cpu_model(k_sample=2)
    if preset is not None:
        m.bags_narrow = preset
    seen = []
    inner = m.forward_bags

    def spy(*a, **kw):
        seen.append(m.bags_narrow)
        return inner(*a, **kw)

    m.forward_bags = spy
    bags = [torch.randn(n, 192) for n in (4, 5, 3)]
    labels = [0, 1, 1]
    evaluate_split(m, bags, labels, 2, narrow_one_call=flag)
    validate_split(m, bags, labels, 2, narrow_one_call=flag)
    assert seen == [flag, flag]
    assert m.__dict__.get("bags_narrow", None) is preset and m.bags_narrow is bool(preset)
    # ... also after an exception inside the call
    def boom(*a, **kw):
        seen.append(m.bags_narrow)
        raise KeyError("inside forward_bags")

    m.forward_bags = boom
    for fn in (evaluate_split, validate_split):
        with pytest.raises(KeyError):
            fn(m, bags, labels, 2, narrow_one_call=flag)
        assert m.__dict__.get("bags_narrow", None) is preset and m.bags_narrow is bool(preset)
    assert seen[2:] == [flag, flag]


def test_validate_split_still_restores_bags_one_call():
    torch.manual_seed(0)
    m = CLAM_MB(size_arg="hipt_smaller", k_sample=2).eval()
    validate_split(m, [torch.randn(4, 192), torch.randn(3, 192)], [0, 1], 2)
    assert "bags_one_call" not in m.__dict__ and "bags_narrow" not in m.__dict__


@pytest.mark.parametrize("preset", [None, True, False])
def test_validate_split_restores_bags_one_call_after_an_exception(preset):
    torch.manual_seed(0)
    m = CLAM_MB(size_arg="hipt_smaller", k_sample=2).eval()
    if preset is not None:
        m.bags_one_call = preset
    seen = []

    def boom(*a, **kw):
        seen.append((m.bags_one_call, m.bags_narrow))
        raise KeyError("inside forward_bags")

    m.forward_bags = boom
    with pytest.raises(KeyError):
        validate_split(m, [torch.randn(4, 192), torch.randn(3, 192)], [0, 1], 2, mb_one_call=False, narrow_one_call=True)
    assert seen == [(False, True)]
    assert m.__dict__.get("bags_one_call", None) is preset and "bags_narrow" not in m.__dict__
