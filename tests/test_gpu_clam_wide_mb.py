"""GPU tests (-m gpu) of the ragged multi-bag CLAM_MB forward for the wide heads (csrc/abmil_wide_mb.hip,
``hipt_clam_mb_forward_bags_wide``; ``CLAM_MB`` with ``bags_one_call`` and ``bags_wide`` both set).

Weights and bags are made as in tests/test_gpu_clam_wide.py.  The row counts of a call are ``ROWS`` (879 rows, 12 work units): bags of
one and two rows, bags one row short of and one row past the kernel's sub-tiles (32 rows in fp32, 64 in bf16), bags that end before, on
and after a 128-row unit, and a bag of 300 rows = 3 units.  ``CASES``: K = 2 and K = 4 on every shape, K = 3 on (128, 512, 256).

The bars.  Reference: tests/clam_wide_mb_ref.py (fp64; in bf16 mode the bag, W1, Wa, Wb rounded to bf16 and h1 rounded to bf16 for the
gate only).  Per dtype and output, the worst |error| over CASES of the loop of ``forward`` calls on the same bags -- the route these
models took before this kernel -- was measured on one MI355X (MEASURED[dtype][output][1]; [0] is this kernel's figure in the same run);
the bar is twice the loop's figure, the factor covering the different fold order (sub-tile online softmax against the loop's), and in
fp32 never above the project's 1e-4.  SEED was chosen on the host from the fp64 reference alone: of seeds 21..32 the one whose smallest
gap between a bag's two largest reference logits, over CASES, both rounding modes and all bags, is largest (7.4e-2); the host test
tests/test_clam_wide_mb_ref.py holds that gap against 4x the logits bars.  Each test prints its figures before it asserts.

What this form shares with the others is stated once in tests/clam_bags_util.py; graph capture, the two input forms and either
switch off run from tests/test_gpu_clam_forms.py."""
import ctypes as C
import functools

import pytest
import torch

import clam_bags_util as U
import clam_wide_mb_ref as WM
from clam_bags_util import DEV, OUTS, TOL, errors, md, run_loop
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd.evaluate import validate_split

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 31, 33, 63, 65, 127, 128, 129, 300)
assert ROWS == U.FORMS["mb_wide"].rows
CASES = [((128, 256, 64), 2), ((128, 256, 64), 4), ((128, 512, 256), 2), ((128, 512, 256), 3), ((128, 512, 256), 4),
         ((1024, 512, 384), 2), ((1024, 512, 384), 4)]
SEED = 27
# worst |error| per output over CASES against tests/clam_wide_mb_ref.py, measured: (this kernel, the loop of forward calls)
MEASURED = {
    "fp32": {"A_raw": (2.862e-6, 2.977e-6), "M": (2.125e-6, 2.125e-6), "logits": (6.973e-7, 6.675e-7), "Y_prob": (2.014e-7, 1.229e-7)},
    "bf16": {"A_raw": (7.810e-4, 7.811e-4), "M": (1.338e-5, 1.338e-5), "logits": (2.150e-6, 2.082e-6), "Y_prob": (6.494e-7, 6.494e-7)},
}
BARS = {dt: {k: (min(2.0 * v[1], TOL) if dt == "fp32" else 2.0 * v[1]) for k, v in d.items()} for dt, d in MEASURED.items()}


make = functools.partial(U.model, "mb_wide")


def bags_of(s0, seed=SEED, rows=ROWS):
    return U.bags_of(s0, seed, rows)


def run_wide(m, bags, **kw):
    return U.run_form(m, "mb_wide", bags, **kw)


# ---------------------------------------------------------------- 1. parity against the fp64 reference, and the route
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", CASES)
def test_parity_per_bag(size, K, dtype):
    m = make(size, dtype, K)
    w = m._pack_stacked(torch.device(DEV))
    lib = N.lib()
    assert lib.hipt_clam_mb_bags_supported(C.byref(w)) == 0 and lib.hipt_clam_mb_wide_bags_supported(C.byref(w)) == 1
    bags = bags_of(size[0])
    refs = WM.reference(size, SEED, ROWS, K, dtype == "bf16")
    loop, _ = errors(run_loop(m, bags), refs, True)
    before = N.calls
    out = run_wide(m, bags)
    assert N.calls == before + 1, "one native call for the whole set"
    assert out["logits"].shape == (len(ROWS), K) and out["Y_prob"].shape == (len(ROWS), K)
    assert out["Y_hat"].shape == (len(ROWS), 1) and out["Y_hat"].dtype == torch.int64
    assert out["M"].shape == (len(ROWS), K, size[1])
    assert [tuple(a.shape) for a in out["A_raw"]] == [(K, n) for n in ROWS]
    worst, wrong = errors(out, refs, True)
    print(f"wide mb forward_bags {dtype} {size} K={K}: " + ", ".join(f"{k} {worst[k]:.3e} (per-bag loop {loop[k]:.3e})" for k in OUTS))
    gaps = [WM.logit_gap(r) for r in refs]
    print(f"  smallest reference logit gap {min(gaps):.3e}")
    bars = BARS[dtype]
    if dtype == "fp32":
        assert max(bars.values()) <= TOL
    for k in OUTS:
        assert worst[k] <= bars[k], (k, worst[k], bars[k])
    assert min(gaps) > 4.0 * bars["logits"], (min(gaps), bars["logits"])   # every bag's class is decided beyond the logit bar
    assert wrong == []                                                     # no bag left out


# ---------------------------------------------------------------- the checks every form shares (clam_bags_util), on this form's cases
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", U.FORMS["mb_wide"].invariance)
def test_a_bag_does_not_see_its_neighbours(size, K, dtype, monkeypatch):
    U.check_neighbours("mb_wide", size, K, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("size,K", [((128, 256, 64), 2), ((128, 512, 256), 4)])
def test_attention_only_writes_a_raw_alone_and_nothing_leaves_its_buffer(size, K, dtype):
    U.check_attention_only("mb_wide", size, K, dtype)
    U.check_fences("mb_wide", size, K, dtype)


# ---------------------------------------------------------------- 2. validation of a split
def test_validate_split_in_one_call_agrees_with_the_loop():
    size, K = (128, 512, 256), 2
    m = make(size, "fp32", K)
    assert m.k_sample == 8
    rows = (20, 45, 64, 65, 100, 127, 128, 129, 200, 256, 257, 300)
    bags = bags_of(128, 23, rows)
    labels = [b % 2 for b in range(len(rows))]
    v1 = validate_split(m, bags, labels, K, wide_one_call=True)
    assert m.bags_route == "bags" and "bags_wide" not in m.__dict__ and "bags_one_call" not in m.__dict__
    v0 = validate_split(m, bags, labels, K, wide_one_call=True, mb_one_call=False)
    assert m.bags_route == "per_bag"
    print(f"validate_split wide mb: prob {md(v1.prob, v0.prob):.3e}, loss {abs(v1.val_loss - v0.val_loss):.3e}, "
          f"instance loss {abs(v1.val_inst_loss - v0.val_inst_loss):.3e} (bar {TOL:.1e})")
    assert md(v1.prob, v0.prob) <= TOL and abs(v1.val_loss - v0.val_loss) <= TOL and abs(v1.val_inst_loss - v0.val_inst_loss) <= TOL
    assert v1.val_error == v0.val_error
    assert v1.acc == v0.acc and v1.inst == v0.inst and v1.inst_count == v0.inst_count
    assert v1.labels.tobytes() == v0.labels.tobytes()
