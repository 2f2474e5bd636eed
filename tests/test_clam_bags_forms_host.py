"""Host tests (no GPU) of the argument checks that the three forms of the multi-bag CLAM call share (csrc/capi.hip:
``clam_bags_forward``): the wide heads, the narrow heads and the K branches of CLAM_MB.  Every error comes back before anything is
dereferenced or launched (all pointers here are fake addresses), as ``HIPT_E_BADARG`` with a message that starts with the entry
point's own name; a configuration outside the form's envelope is ``HIPT_E_UNSUPPORTED`` and needs a workspace of zero bytes."""
import ctypes as C

import pytest

from hipt_abmil_atec23_amd import _native as N

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks
E_BADARG, E_UNSUPPORTED = -1, -4
# form -> (entry point, its workspace size, weights it takes, weights it does not take)
FORMS = {
    "sb": ("hipt_clam_sb_forward_bags", "hipt_clam_bags_workspace_bytes", dict(s0=384, s1=128, s2=64), dict(s0=1024, s1=512, s2=256)),
    "narrow": ("hipt_clam_sb_forward_bags_narrow", "hipt_clam_narrow_bags_workspace_bytes", dict(s0=192, s1=16, s2=8), dict(s0=384, s1=128, s2=64)),
    "mb": ("hipt_clam_mb_forward_bags", "hipt_clam_mb_bags_workspace_bytes", dict(s0=384, s1=128, s2=64, n_classes=2, n_att=2),
           dict(s0=384, s1=128, s2=64, n_classes=3, n_att=2)),
}
CASES = [
    ("null weights", dict(w=None, nbytes=1 << 20)), ("null bags", dict(bags=None)), ("null offsets", dict(offsets=None)),
    ("null A_raw", dict(A_raw=None)), ("null M", dict(M=None)), ("null logits", dict(logits=None)), ("null Y_prob", dict(Y_prob=None)),
    ("null Y_hat", dict(Y_hat=None)), ("null workspace", dict(ws=None)), ("misaligned bags", dict(bags=FAKE + 8)),
    ("no bag", dict(B=0, nbytes=1 << 20)), ("negative B", dict(B=-3, nbytes=1 << 20)), ("fewer rows than bags", dict(B=7, rows=6, nbytes=1 << 20)),
    ("short workspace", dict(nbytes="short")), ("misaligned workspace", dict(ws=FAKE + 16)),
]


def weights(s0, s1, s2, n_classes=2, n_att=1, dtype=N.HIPT_F32):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_classes, n_att=n_att)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def forward(form, w, bags=FAKE, offsets=FAKE, B=7, rows=1000, attention_only=0, A_raw=FAKE, M=FAKE, logits=FAKE, Y_prob=FAKE, Y_hat=FAKE,
            ws=FAKE, nbytes=None):
    lib, (entry, ws_bytes) = N.lib(), FORMS[form][:2]
    if nbytes is None:
        nbytes = getattr(lib, ws_bytes)(C.byref(w), B, rows)
    rc = getattr(lib, entry)(C.byref(w) if w is not None else None, bags, offsets, B, rows, attention_only, A_raw, M, logits, Y_prob, Y_hat,
                             ws, nbytes, None)
    return rc, lib.hipt_last_error().decode()


@pytest.mark.parametrize("case,kw", CASES)
@pytest.mark.parametrize("form", list(FORMS))
def test_argument_errors_come_back_before_any_device_work(form, case, kw):
    entry, ws_bytes, takes, _ = FORMS[form]
    kw = dict(kw)
    w = kw.pop("w", weights(**takes))
    if kw.get("nbytes") == "short":
        need = getattr(N.lib(), ws_bytes)(C.byref(w), 7, 1000)
        assert need > 0
        kw["nbytes"] = need - 1
    rc, msg = forward(form, w, **kw)
    assert rc == E_BADARG, case
    assert msg.startswith(entry[len("hipt_"):] + ": "), msg
    if "workspace" in case and "null" not in case:
        assert "workspace" in msg, msg


@pytest.mark.parametrize("form", list(FORMS))
def test_a_configuration_outside_the_form_is_unsupported_and_sizes_to_zero(form):
    entry, ws_bytes, takes, takes_not = FORMS[form]
    rc, msg = forward(form, weights(**takes_not), nbytes=1 << 24)
    assert rc == E_UNSUPPORTED and msg.startswith(entry[len("hipt_"):] + ": "), msg
    lib = N.lib()
    assert getattr(lib, ws_bytes)(C.byref(weights(**takes_not)), 7, 1000) == 0
    assert getattr(lib, ws_bytes)(C.byref(weights(**takes)), 7, 1000) > 0 and getattr(lib, ws_bytes)(None, 7, 1000) == 0
