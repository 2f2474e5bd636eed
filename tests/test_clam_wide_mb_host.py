"""Host tests (no GPU) of the multi-bag CLAM_MB call for the wide heads (csrc/abmil_wide_mb.hip): ``hipt_clam_mb_wide_bags_supported``
answers yes for exactly (S1, S2) in {(256, 64), (512, 256), (512, 384)} x {fp32, bf16} x K in {2, 3, 4} with K classes and S0 a multiple
of the K-slab; the workspace is the sum of the three carves; a refusal names the widths and the K range; and the forms that existed
before answer as they did.  All pointers here are fake addresses.  What the form shares with the other five (symbols, argument errors,
the switches, the routing) is in tests/test_clam_bags_forms_host.py."""
import ctypes as C
import pytest

from hipt_abmil_atec23_amd import _native as N

FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its checks
E_BADARG, E_UNSUPPORTED = -1, -4
PREFIX = "clam_mb_forward_bags_wide: "
F32, BF16 = N.HIPT_F32, N.HIPT_BF16
PAIRS = ((256, 64), (512, 256), (512, 384))


def weights(dtype=F32, s0=1024, s1=512, s2=256, n_att=2, n_classes=None):
    w = N.ClamWeights(dtype=dtype, s0=s0, s1=s1, s2=s2, n_classes=n_att if n_classes is None else n_classes, n_att=n_att)
    for name in ("w1", "b1", "wab", "bab", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


def forward(lib, w, B=7, rows=1000, nbytes=None, attention_only=0):
    if nbytes is None:
        nbytes = lib.hipt_clam_mb_wide_bags_workspace_bytes(C.byref(w), B, rows)
    return lib.hipt_clam_mb_forward_bags_wide(C.byref(w), FAKE, FAKE, B, rows, attention_only, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, nbytes, None)


def test_supported_is_the_wide_table_times_two_to_four_branches():
    lib = N.lib()
    sup = lambda *a, **kw: lib.hipt_clam_mb_wide_bags_supported(C.byref(weights(*a, **kw)))
    for dt in (F32, BF16):
        for s1 in (32, 64, 128, 256, 384, 512, 768, 1024):
            for s2 in (16, 32, 64, 128, 256, 384, 512):
                for K in (1, 2, 3, 4, 5):
                    assert sup(dt, 1024, s1, s2, K) == int((s1, s2) in PAIRS and 2 <= K <= 4), (dt, s1, s2, K)
    for s1, s2 in PAIRS:
        assert sup(F32, 96, s1, s2) == 1 and sup(BF16, 96, s1, s2) == 0      # a multiple of 32, not of 64
        assert sup(BF16, 128, s1, s2) == 1 and sup(F32, 100, s1, s2) == 0
        for K, C_ in ((2, 3), (3, 2), (4, 1), (2, 1)):
            assert sup(F32, 1024, s1, s2, K, n_classes=C_) == 0, (K, C_)          # n_att != n_classes
    assert sup(F32, 384, 128, 64) == 0 and sup(BF16, 384, 128, 64) == 0      # the mid-width form's head
    assert sup(2, 1024, 512, 256) == 0                                       # no such dtype
    assert lib.hipt_clam_mb_wide_bags_supported(None) == 0


@pytest.mark.parametrize("dt,s1,s2,K", [(F32, 512, 256, 2), (BF16, 512, 384, 4), (BF16, 256, 64, 3)])
def test_workspace_is_the_sum_of_its_three_carves(dt, s1, s2, K):
    """unit table [units x 16 B] | tile_start [B + 1 ints] | partials [units x K x (2 + S1) floats], each rounded up to 256 bytes;
    units = ceil(rows / 128) + B."""
    lib = N.lib()
    w = weights(dt, 1024, s1, s2, K)
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    for B, rows in ((1, 1), (1, 129), (7, 1000), (64, 14_400), (3, 100_000)):
        units = (rows + 127) // 128 + B
        want = al(units * 16) + al(4 * (B + 1)) + al(4 * units * K * (2 + s1))
        assert lib.hipt_clam_mb_wide_bags_workspace_bytes(C.byref(w), B, rows) == want, (B, rows)
    size = lambda B, rows: lib.hipt_clam_mb_wide_bags_workspace_bytes(C.byref(w), B, rows)
    assert size(0, 10) == 0 and size(5, 4) == 0 and size(-1, 10) == 0
    assert lib.hipt_clam_mb_wide_bags_workspace_bytes(None, 7, 1000) == 0
    for bad in (weights(dt, 1024, s1, s2, 5), weights(dt, 1024, s1, s2, 1), weights(dt, 1024, 128, 64, K), weights(dt, 1024, s1, s2, K, n_classes=K + 1)):
        assert lib.hipt_clam_mb_wide_bags_workspace_bytes(C.byref(bad), 7, 1000) == 0


def test_a_refusal_names_the_widths_and_the_branch_range():
    lib = N.lib()
    for w in (weights(F32, 384, 128, 64), weights(F32, 1024, 512, 256, 5), weights(F32, 1024, 512, 256, 1), weights(BF16, 96, 256, 64),
              weights(F32, 1024, 512, 256, 2, n_classes=3)):
        assert forward(lib, w, nbytes=1 << 24) == E_UNSUPPORTED
        msg = lib.hipt_last_error().decode()
        assert msg.startswith(PREFIX) and "(256,64)" in msg and "(512,256)" in msg and "(512,384)" in msg, msg
        assert "2 <= branches <= 4" in msg and f"[{w.s0},{w.s1},{w.s2}]" in msg, msg
    w = weights()
    short = lib.hipt_clam_mb_wide_bags_workspace_bytes(C.byref(w), 7, 1000) - 1
    assert forward(lib, w, nbytes=short) == E_BADARG and lib.hipt_last_error().decode().startswith(PREFIX)
    assert forward(lib, w, B=0, nbytes=1 << 20) == E_BADARG and lib.hipt_last_error().decode().startswith(PREFIX)


def test_the_other_forms_answer_as_before():
    lib = N.lib()
    for dt in (F32, BF16):
        for s1, s2 in PAIRS:
            for K in (1, 2, 4, 5):
                w = weights(dt, 1024, s1, s2, K)
                assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 0 and lib.hipt_clam_mb_bags_workspace_bytes(C.byref(w), 7, 1000) == 0
                assert lib.hipt_clam_wide_bags_supported(C.byref(w)) == 1       # the one-branch wide form does not read n_att
        for K in (2, 3, 4):
            w = weights(dt, 384, 128, 64, K)
            assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 1 and lib.hipt_clam_wide_bags_supported(C.byref(w)) == 0
        assert lib.hipt_clam_mb_bags_supported(C.byref(weights(dt, 384, 128, 64, 5))) == 0
    w = weights(F32, 1024, 512, 256, 2)      # CLAM_MB() with no arguments: `small`
    rc = lib.hipt_clam_mb_forward_bags(C.byref(w), FAKE, FAKE, 7, 1000, 0, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, 1 << 24, None)
    assert rc == E_UNSUPPORTED and lib.hipt_last_error().decode().startswith("clam_mb_forward_bags: ")
