"""Host tests of the helpers every device-op front-end shares (hipt_abmil_atec23_amd/_frontend.py): each is exercised directly,
with CPU tensors and a device that is never touched.  No test here makes a native call."""
import types

import numpy as np
import pytest

from hipt_abmil_atec23_amd import _frontend as F
from hipt_abmil_atec23_amd import _native as N


def test_is_tensor_has_one_rule():
    import torch
    assert F.is_tensor(torch.zeros(2))
    assert not F.is_tensor(np.zeros(2)) and not F.is_tensor([1, 2])
    stranger = type("Stranger", (), {"data_ptr": lambda self: 0, "__module__": "elsewhere"})()
    lookalike = type("Tensor", (), {"data_ptr": lambda self: 0, "__module__": "torchfoo"})()
    assert hasattr(stranger, "data_ptr") and not F.is_tensor(stranger)
    assert type(lookalike).__module__.startswith("torch") and not F.is_tensor(lookalike)
    assert F.as_array(None) is None and isinstance(F.as_array([1, 2]), np.ndarray)
    t = torch.zeros(2)
    assert F.as_array(t) is t


def test_check_int():
    assert F.check_int("op", "k", np.int64(5), 0, 9) == 5 and type(F.check_int("op", "k", np.int64(5), 0, 9)) is int
    assert F.check_int("op", "k", -7) == -7 and F.check_int("op", "k", 3, 1) == 3
    for bad in (True, np.bool_(True), 1.0, np.float32(2.0), "3", None, -1, 10):
        with pytest.raises(ValueError, match=r"op: k must be an integer in 0 \.\. 9") as e:
            F.check_int("op", "k", bad, 0, 9)
        assert repr(bad) in str(e.value)   # (the offending value is named)
    with pytest.raises(ValueError, match=">= 1"):
        F.check_int("op", "k", 0, 1)


def test_rgb_layout():
    import torch
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8)
    assert F.rgb_layout("op", u8(2, 3, 5, 7)) == (False, 5, 7)
    assert F.rgb_layout("op", u8(2, 5, 7, 3)) == (True, 5, 7)
    assert F.rgb_layout("op", u8(2, 3, 5, 3)) == (False, 5, 3)   # planar, as HIPT_4K's test has it
    assert F.rgb_layout("op", u8(5, 7, 3)) == (True, 5, 7) and F.rgb_layout("op", u8(3, 5, 7)) == (False, 5, 7)
    with pytest.raises(ValueError, match=r"op: .*\[2, 4, 5, 7\]"):
        F.rgb_layout("op", u8(2, 4, 5, 7))
    with pytest.raises(ValueError, match="batch"):
        F.rgb_layout("op", u8(5, 7))
    with pytest.raises(ValueError, match="batch"):
        F.rgb_layout("op", u8(5, 7, 3), dims=(4,))          # an op that takes batches only
    with pytest.raises(ValueError, match="uint8"):
        F.rgb_layout("op", u8(2, 3, 5, 7).float())
    with pytest.raises(ValueError, match="uint8 tensor"):
        F.rgb_layout("op", np.zeros((2, 3, 5, 7), np.uint8))


def test_check_out_fails_one_clause_at_a_time():
    import torch
    dev, x = torch.device("cpu"), torch.zeros((4, 6), dtype=torch.uint8)
    good = torch.zeros((4, 6), dtype=torch.uint8)
    assert F.check_out("op", good, (4, 6), torch.uint8, dev, not_alias=(x,)) is good
    new = F.check_out("op", None, (4, 6), torch.float32, dev)
    assert tuple(new.shape) == (4, 6) and new.dtype == torch.float32 and new.device == dev
    elsewhere = types.SimpleNamespace(type="cuda", index=0)   # (a device nothing lives on; it is only compared)
    bad = {"not a tensor": (np.zeros((4, 6), np.uint8), dev), "dtype": (good.float(), dev), "shape": (torch.zeros((4, 5), dtype=torch.uint8), dev),
           "device": (good, elsewhere), "contiguous": (torch.zeros((6, 4), dtype=torch.uint8).t(), dev), "alias": (x, dev)}
    for clause, (out, where) in bad.items():
        with pytest.raises(ValueError, match=r"op: out must be a contiguous uint8 \[4, 6\] tensor on .*not the input"):
            F.check_out("op", out, (4, 6), torch.uint8, where, not_alias=(x,))
    assert F.check_out("op", x, (4, 6), torch.uint8, dev) is x   # (an op that can run in place names no input)
    with pytest.raises(ValueError, match=r"op: out\['256'\] must be"):
        F.check_out("op", good, (4, 7), torch.uint8, dev, name="out['256']")


def test_resolve_device_refuses_before_torch_cuda_is_asked(monkeypatch):
    import torch

    def asked(*a, **k):
        raise AssertionError("torch.cuda was asked")
    monkeypatch.setattr(torch.cuda, "is_available", asked)
    monkeypatch.setattr(torch.cuda, "current_device", asked)
    for exc in (RuntimeError, ValueError):
        with pytest.raises(exc, match="op: device cpu; .*HIP device") as e:
            F.resolve_device("op", "cpu", exc=exc)
        assert type(e.value) is exc
        with pytest.raises(exc, match="HIP device"):
            F.resolve_device("op", torch.device("cpu"), (torch.zeros(2),), exc=exc, staged=True)


def test_staging_refuses_on_the_host():
    import torch
    before = N.calls
    for bad in ([[1]], np.zeros((4, 6), np.float32), np.zeros((4, 6, 3), np.uint8), torch.zeros((0, 6), dtype=torch.uint8)):
        with pytest.raises(ValueError, match="op: "):
            F.as_device_u8("op", bad, None, dims=2)
    with pytest.raises(ValueError, match="C one of"):
        F.as_device_u8("op", np.zeros((4, 6, 2), np.uint8), None, dims=3, channels=(3, 4))
    with pytest.raises(ValueError, match="HIP device"):
        F.as_device_u8("op", np.zeros((4, 6), np.uint8), "cpu", dims=2)
    assert F.to_device(None, "cpu") is None
    m = F.to_device(np.array([[True, False]]), "cpu")
    assert m.dtype == torch.uint8 and m.tolist() == [[1, 0]]
    F.check_image("op", "mask", None, (4, 6), ("bool",))
    with pytest.raises(ValueError, match=r"op: mask must be bool \[4, 6\]"):
        F.check_image("op", "mask", np.zeros((6, 4), bool), (4, 6), ("bool",))
    with pytest.raises(ValueError, match="op: scores contain NaN"):
        F.check_no_nan("op", scores=np.array([1.0, np.nan]), ref=None)
    with pytest.raises(ValueError, match="op: ref contain NaN"):
        F.check_no_nan("op", scores=np.ones(2), ref=torch.tensor([float("nan")]))
    assert N.calls == before


def test_one_colour_table_cache_serves_both_builders():
    pytest.importorskip("matplotlib")
    from hipt_abmil_atec23_amd import heatmap as H
    from hipt_abmil_atec23_amd import hier_heatmap as HH
    for builder, entries in ((H.colour_table, 258), (HH.colour_table_n, 256)):
        first = F.table_host(builder, "coolwarm")
        assert F.table_host(builder, "coolwarm") is first                       # built once
        assert first.shape == (entries, 3) and np.array_equal(first, builder("coolwarm"))
        on_host = F.table_on(builder, "coolwarm", first, "cpu")
        assert F.table_on(builder, "coolwarm", first, "cpu") is on_host        # and copied to a device once
        assert np.array_equal(on_host.numpy(), first)
    assert F.table_host(H.colour_table, "coolwarm") is not F.table_host(HH.colour_table_n, "coolwarm")   # keyed by the builder
    assert HH.host_table("coolwarm") is F.table_host(HH.colour_table_n, "coolwarm")
    import matplotlib
    own = matplotlib.colormaps["jet"]
    assert F.table_host(H.colour_table, own) is not F.table_host(H.colour_table, own)   # a colormap object is not cached
    table = np.zeros((4, 3), np.uint8)
    assert HH.host_table(table) is table
    with pytest.raises(ValueError, match="patch_heatmap: a colour table"):
        HH.host_table(np.zeros((4, 4), np.uint8), "patch_heatmap")
