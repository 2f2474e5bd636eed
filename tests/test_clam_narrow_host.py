"""Host tests (no GPU) of the multi-bag CLAM_SB call for the narrow heads (csrc/abmil_narrow.hip): the envelope table answers yes and no
where it should and leaves ``hipt_clam_bags_supported`` as it was, and a refusal names the widths (all pointers here are fake
addresses).  What the form shares with the other five (symbols, argument errors, workspace sizes, the switch) is stated in
tests/clam_bags_util.py and run here on this form's cases."""
import ctypes as C
import pytest

from hipt_abmil_atec23_amd import _native as N
from clam_bags_util import (ARGUMENT_CASES, W, check_argument_error, check_attention_only_needs_no_pooled_outputs, check_outside,
                                       check_split_switch, check_workspace_grows)

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks
E_UNSUPPORTED = -4
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


def test_attention_only_needs_no_pooled_outputs_and_other_widths_are_unsupported():
    check_attention_only_needs_no_pooled_outputs("narrow")
    lib = N.lib()
    for a in ((F32, 1024, 512, 256), (F32, 192, 64, 32), (BF16, 384, 128, 64), (F32, 200, 16, 8)):
        assert forward(lib, weights(*a), nbytes=1 << 24) == E_UNSUPPORTED, a
        msg = lib.hipt_last_error().decode()
        assert "(8,4)" in msg and "(16,8)" in msg and "(32,8)" in msg and "(32,16)" in msg, msg   # the message names the widths


# ---- the checks every form shares (tests/clam_bags_util.py), on this form's cases ----
@pytest.mark.parametrize("a", NARROW)
def test_workspace_grows_with_bags_and_rows(a):
    check_workspace_grows("narrow", W(*a[1:], dtype=a[0]))


def test_workspace_is_zero_outside_the_envelope():
    check_outside("narrow", [W(1024, 512, 256), W(192, 64, 32), W(200, 16, 8), W(96, 16, 8, dtype=BF16)])


@pytest.mark.parametrize("case,kw", ARGUMENT_CASES)
def test_argument_errors_come_back_before_any_device_work(case, kw):
    check_argument_error("narrow", case, kw)


@pytest.mark.parametrize("preset", [None, True, False])
@pytest.mark.parametrize("flag", [True, False])
def test_split_functions_set_the_switch_for_their_duration_only(preset, flag):
    check_split_switch("narrow", "narrow_one_call", flag, preset)
