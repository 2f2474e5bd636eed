"""GPU tests (-m gpu) that every form of the multi-bag CLAM forward shares, run over ``clam_bags_util.FORMS``: a list of bags and
``(cat, BagOffsets)`` agree; one call is captured on a single stream and replayed; with a switch of the form off, ``forward_bags`` keeps
the loop and its bits.  The other shared checks -- a bag does not see its neighbours, ``attention_only`` writes ``A_raw`` alone, fenced
buffers and a stateless workspace -- are stated once in ``clam_bags_util`` (``check_neighbours``, ``check_attention_only``,
``check_fences``) and run from each form's own file, on that form's cases.  What belongs to one form alone (parity against its reference
and its bars, golden bags, the instance branch, the split functions) is in that form's file.

A form runs a check at the cases listed below -- at the least its first invariance case, on its own ``ROWS``, in both dtypes.  Bags are
made from seed 9 unless a test says otherwise."""
import pytest
import torch

import clam_bags_util as U
from clam_bags_util import FORMS, assert_same_bits, bits, per_bag, setup

pytestmark = pytest.mark.gpu
DTYPES = ("fp32", "bf16")
LOOP_ROWS = (1, 129, 300)


def first(form):
    return FORMS[form].invariance[0]


def params(cases):
    """(form, size, K, dtype[, rows]) tuples as pytest parameters with readable ids"""
    return [pytest.param(*c, id="-".join([c[0], "x".join(map(str, c[1])), f"K{c[2]}", c[3]] + ([f"{len(c[4])}bags"] if len(c) > 4 else []))) for c in cases]


def over(table, dtypes=DTYPES):
    return [(form, size, K, dt) for form, cases in table.items() for size, K in cases for dt in dtypes]


PAIR = over({form: [first(form)] for form in FORMS if form != "mb_wide"} | {"mb_wide": [first("mb_wide"), ((128, 512, 256), 3)]})
GRAPH = over({"sb": [((384, 128, 64), 2)], "narrow": [((192, 16, 8), 2)], "wide": [((128, 512, 256), 2)], "mb": [((384, 128, 64), 2)],
              "mb_wide": [((128, 512, 256), 2)], "mb_many": [((64, 128, 64), 5)]})
# switches off: on LOOP_ROWS, and wide and mb on the form's ROWS as well; "sb" has no switch
DEFAULTS = [c + (LOOP_ROWS,) for c in over({"narrow": [((192, 16, 8), 2)], "mb_wide": [((128, 512, 256), 2)], "mb_many": [((64, 128, 64), 5)]})]
DEFAULTS += [("wide", (128, 256, 64), 2, "fp32", LOOP_ROWS)] + [c + (FORMS[c[0]].rows,) for c in over({"wide": [first("wide")], "mb": [first("mb")]})]


# ---------------------------------------------------------------- 1. the two input forms
@pytest.mark.parametrize("form,size,K,dtype", params(PAIR))
def test_list_and_concatenated_inputs_agree(form, size, K, dtype):
    m, bags, rows = setup(form, size, K, dtype)
    full = U.run_form(m, form, bags)
    pair = U.run_form(m, form, (torch.cat(list(bags), dim=0), U.offsets_of(rows)))
    for b in range(len(bags)):
        assert_same_bits(per_bag(full, b, FORMS[form].multi), per_bag(pair, b, FORMS[form].multi), f"bag {b}")


# ---------------------------------------------------------------- 2. graph capture
@pytest.mark.parametrize("form,size,K,dtype", params(GRAPH))
def test_one_call_is_captured_and_replayed(form, size, K, dtype):
    """The call is three launches on the capturing stream and nothing else (no copy, no synchronisation, no second stream), so the
    captured graph is a chain; replays on new contents of the same shape equal an eager call bit for bit."""
    m, bags, rows = setup(form, size, K, dtype)
    static = torch.cat(bags, dim=0).clone()
    off = U.offsets_of(rows)                          # checked and uploaded BEFORE the capture
    with U.switched(m, form):
        call = lambda: m.forward_bags((static, off), return_features=True)   # noqa: E731
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call()                                    # weight image, workspace and per-device kernel setup exist before the capture
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                     # one capture on a single stream
            logits, y_prob, y_hat, a_raw, res = call()
        assert m.bags_route == "bags"
    for seed in (31, 32):                             # two replays, each on new bags
        static.copy_(torch.cat(U.bags_of(size[0], seed, rows), dim=0))
        g.replay()
        torch.cuda.synchronize()
        got = {"A_raw": torch.cat(a_raw, dim=1), "M": res["features"], "logits": logits, "Y_prob": y_prob, "Y_hat": y_hat}
        eager = U.run_form(m, form, U.bags_of(size[0], seed, rows))
        eager["A_raw"] = torch.cat(eager["A_raw"], dim=1)
        assert_same_bits(got, eager, f"replay on seed {seed}")


# ---------------------------------------------------------------- 3. the switches
@pytest.mark.parametrize("form,size,K,dtype,rows", params(DEFAULTS))
def test_a_switch_off_keeps_the_loop_and_its_bits(form, size, K, dtype, rows):
    """The form's switches at their defaults, and each single switch of a two-switch form set alone"""
    f = FORMS[form]
    m, bags, _ = setup(form, size, K, dtype, rows, seed=13)
    assert all(getattr(f.cls, s) is False for s in f.switches) and not any(s in m.__dict__ for s in f.switches)
    want = U.run_loop(m, bags)
    for flags in [()] + ([(s,) for s in f.switches] if len(f.switches) > 1 else []):
        with U.switched(m, flags):
            got = U.as_out(m.forward_bags(list(bags), return_features=True))
            assert m.bags_route == "per_bag", flags
        assert not any(s in m.__dict__ for s in f.switches), flags
        assert U.a_bits(got["A_raw"]) == U.a_bits(want["A_raw"]), flags
        for k in ("M", "logits", "Y_prob", "Y_hat"):
            assert got[k].shape == want[k].shape and bits(got[k]) == bits(want[k]), (flags, k)
