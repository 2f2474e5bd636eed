"""Host tests (no GPU) of what the six forms of the multi-bag CLAM call share (``functional._BAGS_FORMS``; csrc/capi.hip:
``clam_bags_forward``): the three symbols of a form are exported, declared, let out by the export map and bound; every argument error
comes back before anything is dereferenced or launched (all pointers here are fake addresses), as ``HIPT_E_BADARG`` with a message that
starts with the entry point's own name; a configuration outside the form's envelope is ``HIPT_E_UNSUPPORTED`` and needs a workspace of
zero bytes; the workspace grows with B and the row count in multiples of 256 bytes; the model switches are off by default, a CPU model
ignores them and the split functions set them for their own duration only; and ``CLAM_SB._bags_form`` routes by the truth table written
out below.  The exact envelope of a form, its workspace carves and the refusal texts that name its ranges are in that form's own file."""
import inspect
import itertools
import os
import re

import pytest
import torch

import clam_bags_util as U
from clam_bags_util import FORMS, W, cpu_model, entry_of, fake_weights
from conftest import ROOT
from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, _native as N
from hipt_abmil_atec23_amd import functional as Fn
from hipt_abmil_atec23_amd.evaluate import evaluate_split, validate_split


# ---- the registry and the C ABI ------------------------------------------------------------------------------------------------------
def test_the_registry_has_these_six_rows_in_routing_order():
    assert list(Fn._BAGS_FORMS) == list(FORMS) == ["sb", "narrow", "wide", "mb", "mb_many", "mb_wide"]
    for form, t in FORMS.items():
        f = Fn._BAGS_FORMS[form]
        assert f[:7] == (form, entry_of(form), t.ws_bytes, t.supported, t.multi, t.cls.__name__, t.switches)
        assert (f.name, f.entry, f.ws_bytes, f.supported, f.multi, f.kind, f.switches, f.heads) == tuple(f)
        assert getattr(Fn, f.entry[len("hipt_"):]) is t.call and f.entry in t.call.__doc__ and f.heads in t.call.__doc__
        assert list(inspect.signature(t.call).parameters) == ["w", "cat", "offsets", "attention_only", "out", "ws"]
        assert ("[B, K, S1]" in t.call.__doc__) == f.multi and ("M [B, S1]" in t.call.__doc__) == (not f.multi)
    assert set(Fn.BAGS_FORMS_K) == {"mb", "mb_many", "mb_wide"}
    w = fake_weights(**W(1024, 512, 256, 3))
    assert Fn.bags_shapes("mb", w, 7, 1000) == Fn.bags_shapes("mb_wide", w, 7, 1000) == ((3, 1000), (7, 3, 512), (7, 3))
    assert Fn.bags_shapes("wide", w, 7, 1000) == ((1000,), (7, 512), (7, 3))
    assert Fn.bags_shapes("mb_many", fake_weights(**W(384, 128, 64, 6)), 7, 1000) == ((6, 1000), (7, 6, 128), (7, 6))


@pytest.mark.parametrize("form", list(FORMS))
def test_symbols_are_exported_declared_mapped_and_bound(form):
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    declared = set(re.findall(r"\b(hipt_[a-z0-9_]+)\s*\(", hdr))
    vmap = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "hipt_abmil.map")).read()
    globs = re.search(r"global:\s*([^;]+);", vmap).group(1).split()
    lib = N.lib()
    names = lambda form: (FORMS[form].supported, FORMS[form].ws_bytes, entry_of(form))   # noqa: E731
    for name, like in zip(names(form), names("mb" if FORMS[form].multi else "sb")):      # (a form has the signatures of the first of its kind)
        assert name in declared and name in N.SIGNATURES and hasattr(lib, name), name
        assert any(re.fullmatch(g.replace("*", ".*"), name) for g in globs), (name, globs)     # the export map lets it out
        assert N.SIGNATURES[name] == N.SIGNATURES[like], name
    # the forms are additions beside the older symbols: the version stays where other tests of this suite pin it
    assert lib.hipt_abi_version() == N.ABI_VERSION == 6 and re.search(r"#define HIPT_ABI_VERSION 6\b", hdr)


# (clam_bags_util's check_* functions are the one statement of a check; a form's own host file runs them on the cases it has always had)
@pytest.mark.parametrize("case,kw", U.ARGUMENT_CASES)
@pytest.mark.parametrize("form", list(FORMS))
def test_argument_errors_come_back_before_any_device_work(form, case, kw):
    U.check_argument_error(form, case, kw)


@pytest.mark.parametrize("form", ["mb", "mb_many", "mb_wide"])      # (sb, narrow, wide: with their refusal texts, in their own files)
def test_attention_only_needs_no_pooled_outputs(form):
    U.check_attention_only_needs_no_pooled_outputs(form)


@pytest.mark.parametrize("form", list(FORMS))
def test_a_configuration_outside_the_form_is_unsupported_and_sizes_to_zero(form):
    U.check_outside(form)


@pytest.mark.parametrize("form", ["mb", "mb_many", "mb_wide"])      # (sb, narrow, wide: over their width tables, in their own files)
def test_workspace_grows_with_bags_and_rows(form):
    U.check_workspace_grows(form)


# ---- the model switches --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", list(FORMS))
def test_switches_are_off_by_default_and_a_cpu_model_ignores_them(form):
    switches, cls = FORMS[form].switches, FORMS[form].cls
    assert all(getattr(cls, s) is False for s in switches)
    m = cpu_model(form)
    assert not any(s in m.__dict__ for s in switches)
    assert m._bags_form(torch.device("cpu")) is None
    bags = [torch.randn(n, m._sizes[0]) for n in (1, 5, 3)]
    want = m.forward_bags(bags)
    assert m.bags_route == "per_bag"
    for s in switches:
        setattr(m, s, True)
    assert m._bags_form(torch.device("cpu")) is None
    before = N.calls
    got = m.forward_bags(bags)
    assert m.bags_route == "per_bag" and N.calls == before
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_the_keywords_have_their_defaults():
    want = {"narrow_one_call": True, "wide_one_call": False, "many_one_call": False}
    for fn in (evaluate_split, validate_split):
        assert {k: inspect.signature(fn).parameters[k].default for k in want} == want
    assert inspect.signature(validate_split).parameters["mb_one_call"].default is True


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


def test_many_one_call_sets_both_switches_and_overrides_mb_one_call():
    m = cpu_model("mb_many")
    seen = []
    real = m.forward_bags
    m.forward_bags = lambda *a, **kw: seen.append((m.bags_one_call, m.bags_many)) or real(*a, **kw)
    bags = [torch.randn(n, 64) for n in (9, 12, 8)]
    r1 = validate_split(m, bags, [0, 4, 2], 5, many_one_call=True, mb_one_call=False)
    assert "bags_many" not in m.__dict__ and "bags_one_call" not in m.__dict__
    r0 = validate_split(m, bags, [0, 4, 2], 5)
    evaluate_split(m, bags, [0, 4, 2], 5, many_one_call=True)
    evaluate_split(m, bags, [0, 4, 2], 5)
    assert seen == [(True, True), (True, False), (True, True), (False, False)]
    assert r1.prob.tobytes() == r0.prob.tobytes()               # on the CPU both are the loop
    m.bags_many = True                                          # the model's own switch stays in force, and stays
    validate_split(m, bags, [0, 4, 2], 5)
    assert seen[-1] == (True, True) and m.__dict__["bags_many"] is True and "bags_one_call" not in m.__dict__


def test_a_model_without_the_switches_is_left_alone():
    class Plain:
        def forward_bags(self, bags):
            logits = torch.stack([b[0, :2] for b in bags]).float()
            return logits, torch.softmax(logits, dim=1), torch.topk(logits, 1, dim=1)[1], [None] * len(bags), {}

    m = Plain()
    evaluate_split(m, [torch.randn(3, 4), torch.randn(2, 4)], [0, 1], 2, wide_one_call=True, many_one_call=True)
    assert m.__dict__ == {}


# ---- the routing truth table ---------------------------------------------------------------------------------------------------------
# CLAM_SB: bags_narrow bags_wide | answers of the sb, narrow, wide predicates | the form taken | the predicates asked, in order.
# From the rule: sb wherever its predicate says yes, whatever the switches; else narrow if bags_narrow and its predicate; else wide if
# bags_wide and its predicate; else the loop.  bags_one_call and bags_many do not matter to a CLAM_SB.
SB_TABLE = """
    0 0 | 0 0 0 | -       | sb
    0 0 | 0 0 1 | -       | sb
    0 0 | 0 1 0 | -       | sb
    0 0 | 0 1 1 | -       | sb
    0 0 | 1 0 0 | sb      | sb
    0 0 | 1 0 1 | sb      | sb
    0 0 | 1 1 0 | sb      | sb
    0 0 | 1 1 1 | sb      | sb
    0 1 | 0 0 0 | -       | sb wide
    0 1 | 0 0 1 | wide    | sb wide
    0 1 | 0 1 0 | -       | sb wide
    0 1 | 0 1 1 | wide    | sb wide
    0 1 | 1 0 0 | sb      | sb
    0 1 | 1 0 1 | sb      | sb
    0 1 | 1 1 0 | sb      | sb
    0 1 | 1 1 1 | sb      | sb
    1 0 | 0 0 0 | -       | sb narrow
    1 0 | 0 0 1 | -       | sb narrow
    1 0 | 0 1 0 | narrow  | sb narrow
    1 0 | 0 1 1 | narrow  | sb narrow
    1 0 | 1 0 0 | sb      | sb
    1 0 | 1 0 1 | sb      | sb
    1 0 | 1 1 0 | sb      | sb
    1 0 | 1 1 1 | sb      | sb
    1 1 | 0 0 0 | -       | sb narrow wide
    1 1 | 0 0 1 | wide    | sb narrow wide
    1 1 | 0 1 0 | narrow  | sb narrow
    1 1 | 0 1 1 | narrow  | sb narrow
    1 1 | 1 0 0 | sb      | sb
    1 1 | 1 0 1 | sb      | sb
    1 1 | 1 1 0 | sb      | sb
    1 1 | 1 1 1 | sb      | sb
"""
# CLAM_MB with bags_one_call SET: bags_many bags_wide | answers of the mb, mb_many, mb_wide predicates | the form | the predicates asked.
# From the rule: mb if its predicate says yes; else mb_many if bags_many and its predicate; else mb_wide if bags_wide and its predicate;
# else the loop.  With bags_one_call off: the loop, whatever else is set, nothing packed, nothing asked.  bags_narrow does not matter.
MB_TABLE = """
    0 0 | 0 0 0 | -       | mb
    0 0 | 0 0 1 | -       | mb
    0 0 | 0 1 0 | -       | mb
    0 0 | 0 1 1 | -       | mb
    0 0 | 1 0 0 | mb      | mb
    0 0 | 1 0 1 | mb      | mb
    0 0 | 1 1 0 | mb      | mb
    0 0 | 1 1 1 | mb      | mb
    0 1 | 0 0 0 | -       | mb mb_wide
    0 1 | 0 0 1 | mb_wide | mb mb_wide
    0 1 | 0 1 0 | -       | mb mb_wide
    0 1 | 0 1 1 | mb_wide | mb mb_wide
    0 1 | 1 0 0 | mb      | mb
    0 1 | 1 0 1 | mb      | mb
    0 1 | 1 1 0 | mb      | mb
    0 1 | 1 1 1 | mb      | mb
    1 0 | 0 0 0 | -       | mb mb_many
    1 0 | 0 0 1 | -       | mb mb_many
    1 0 | 0 1 0 | mb_many | mb mb_many
    1 0 | 0 1 1 | mb_many | mb mb_many
    1 0 | 1 0 0 | mb      | mb
    1 0 | 1 0 1 | mb      | mb
    1 0 | 1 1 0 | mb      | mb
    1 0 | 1 1 1 | mb      | mb
    1 1 | 0 0 0 | -       | mb mb_many mb_wide
    1 1 | 0 0 1 | mb_wide | mb mb_many mb_wide
    1 1 | 0 1 0 | mb_many | mb mb_many
    1 1 | 0 1 1 | mb_many | mb mb_many
    1 1 | 1 0 0 | mb      | mb
    1 1 | 1 0 1 | mb      | mb
    1 1 | 1 1 0 | mb      | mb
    1 1 | 1 1 1 | mb      | mb
"""
CUDA = torch.device("cuda", 0)     # only its type is read: nothing here touches a device


def table(text):
    """{(switch values, predicate answers): (form or None, [predicates asked])}"""
    out = {}
    for line in text.strip().splitlines():
        sw, ans, form, asked = (c.strip() for c in line.split("|"))
        out[tuple(map(int, sw.split())), tuple(map(int, ans.split()))] = (None if form == "-" else form, asked.split())
    assert len(out) == 32
    return out


def routed(monkeypatch, cls, forms, answers):
    """a CPU-built model of ``cls`` whose pack functions return a sentinel, the library's predicates of ``forms`` answering ``answers``:
    ``(model, sentinel, log of pack and predicate calls)``"""
    torch.manual_seed(0)
    m = cls(size_arg=[64, 128, 64]).eval()
    sentinel, log = N.ClamWeights(), []
    monkeypatch.setattr(m, "_pack", lambda device: log.append("_pack") or sentinel)
    monkeypatch.setattr(m, "_pack_stacked", lambda device: log.append("_pack_stacked") or sentinel, raising=False)
    for form, answer in zip(forms, answers):
        monkeypatch.setattr(N.lib(), FORMS[form].supported, lambda ref, form=form, answer=answer: log.append(form) or answer)
    for form in set(FORMS) - set(forms):        # a predicate of the other kind is never asked
        monkeypatch.setattr(N.lib(), FORMS[form].supported, lambda ref, form=form: log.append(form) or 1)
    return m, sentinel, log


@pytest.mark.parametrize("cls,forms,switches,free,text", [
    (CLAM_SB, ("sb", "narrow", "wide"), ("bags_narrow", "bags_wide"), ("bags_one_call", "bags_many"), SB_TABLE),
    (CLAM_MB, ("mb", "mb_many", "mb_wide"), ("bags_many", "bags_wide"), ("bags_narrow",), MB_TABLE)])
def test_bags_form_routes_by_the_truth_table(cls, forms, switches, free, text, monkeypatch):
    pack = "_pack_stacked" if cls is CLAM_MB else "_pack"
    for (values, answers), (form, asked) in table(text).items():
        for others in itertools.product((False, True), repeat=len(free)):
            m, sentinel, log = routed(monkeypatch, cls, forms, answers)
            if cls is CLAM_MB:
                m.bags_one_call = True
            for name, v in (*zip(switches, values), *zip(free, others)):
                setattr(m, name, bool(v))
            got = m._bags_form(CUDA)
            assert (got is None) if form is None else (got[0] is sentinel and got[1] == form), (values, answers, others, got)
            assert log == [pack, *asked], (values, answers, others, log)     # packed once, asked what the ladder asked, in its order


@pytest.mark.parametrize("many,wide,narrow", list(itertools.product((False, True), repeat=3)))
def test_clam_mb_without_bags_one_call_packs_and_asks_nothing(many, wide, narrow, monkeypatch):
    for answers in itertools.product((0, 1), repeat=3):
        m, _, log = routed(monkeypatch, CLAM_MB, ("mb", "mb_many", "mb_wide"), answers)
        m.bags_many, m.bags_wide, m.bags_narrow = many, wide, narrow
        assert m._bags_form(CUDA) is None and log == []
        m.bags_one_call = False
        assert m._bags_form(CUDA) is None and log == []


@pytest.mark.parametrize("cls", [CLAM_SB, CLAM_MB])
def test_an_ungated_head_or_a_cpu_device_never_reaches_the_library(cls, monkeypatch):
    forms = ("mb", "mb_many", "mb_wide") if cls is CLAM_MB else ("sb", "narrow", "wide")
    m, _, log = routed(monkeypatch, cls, forms, (1, 1, 1))
    m.bags_one_call = m.bags_many = m.bags_wide = m.bags_narrow = True
    monkeypatch.setattr(N, "lib", lambda: pytest.fail("the library was asked for"))
    assert m._bags_form(torch.device("cpu")) is None and log == []
    m._gate = False
    assert m._bags_form(CUDA) is None and log == []
