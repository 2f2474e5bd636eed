"""ResNet-50 baseline extractor, host side (no GPU): the reference's call surface and state dict, pretrained-weight loading
without a network, the drop-in mappings, and the fp64 restatement the GPU tests compare against."""
import importlib.util
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.utils.model_zoo  # noqa: F401  (patched below: must never be called)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref as R  # noqa: E402

from hipt_abmil_atec23_amd import synth  # noqa: E402
from hipt_abmil_atec23_amd import resnet_custom as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _keys_file():
    out = []
    with open(os.path.join(R.GOLDEN, "resnet50_baseline_keys.txt")) as f:
        for line in f:
            k, s = line.split()
            out.append((k, () if s == "-" else tuple(int(d) for d in s.split("x"))))
    return out


def test_state_dict_keys_and_shapes_match_reference():
    m = rc.resnet50_baseline(pretrained=False)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == _keys_file()
    assert rc.Bottleneck_Baseline.expansion == 4
    assert isinstance(m, rc.ResNet_Baseline) and len(m.layer3) == 6


def test_synth_specs_cover_every_learnable_tensor():
    m = rc.resnet50_baseline()
    learn = {k for k, _ in m.named_parameters()}
    assert set(synth.resnet_param_specs()) == learn
    missing, unexpected = m.load_state_dict(R.state_dict(), strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing)


def test_torchvision_checkpoint_loads_non_strict():
    # a torchvision resnet50 state dict: ResNet_Baseline's keys plus layer4.* and fc.*
    full = rc.ResNet_Baseline(rc.Bottleneck_Baseline, [3, 4, 6, 3])
    full.layer4 = full._make_layer(rc.Bottleneck_Baseline, 512, 3, stride=2)
    full.fc = torch.nn.Linear(2048, 1000)
    sd = full.state_dict()
    m = rc.resnet50_baseline()
    res = m.load_state_dict(sd, strict=False)
    assert res.missing_keys == []
    assert res.unexpected_keys and all(k.startswith(("layer4.", "fc.")) for k in res.unexpected_keys)
    assert torch.equal(m.layer3[5].conv3.weight, full.layer3[5].conv3.weight)


def _no_fetch(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a network fetch was attempted")
    monkeypatch.setattr(torch.utils.model_zoo, "load_url", boom)
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", boom)


def test_pretrained_missing_checkpoint_raises_without_fetch(monkeypatch, tmp_path):
    _no_fetch(monkeypatch)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    expect = os.path.join(str(tmp_path), "hub", "checkpoints", "resnet50-19c8e357.pth")
    assert rc.cached_checkpoint_path("resnet50") == expect
    with pytest.raises(FileNotFoundError, match="resnet50-19c8e357.pth"):
        rc.resnet50_baseline(pretrained=True)


def test_pretrained_reads_the_cached_checkpoint(monkeypatch, tmp_path):
    _no_fetch(monkeypatch)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    src = rc.resnet50_baseline()
    sd = src.state_dict()
    sd["fc.weight"] = torch.zeros(3, 2048)  # an extra key, as in a torchvision checkpoint
    path = rc.cached_checkpoint_path("resnet50")
    os.makedirs(os.path.dirname(path))
    torch.save(sd, path)
    m = rc.resnet50_baseline(pretrained=True)
    assert torch.equal(m.conv1.weight, src.conv1.weight) and torch.equal(m.layer2[0].downsample[0].weight, src.layer2[0].downsample[0].weight)


def test_resnet18_baseline_is_not_implemented():
    with pytest.raises(NotImplementedError, match="ResNet-18"):
        rc.resnet18_baseline(pretrained=False)


def test_forward_refuses_cpu_tensor():
    m = rc.resnet50_baseline().eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 3, 64, 64))


def test_input_normalization_setting():
    m = rc.resnet50_baseline()
    assert m._norm == rc.IMAGENET_MEAN + rc.IMAGENET_STD
    m.set_input_normalization(0.5, 0.5)
    assert m._norm == (0.5,) * 6
    with pytest.raises(ValueError):
        m.set_input_normalization((0.5, 0.5), (0.5, 0.5, 0.5))


@pytest.fixture
def clean_modules():
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.") or k.startswith("HIPT_4K")}
    yield
    from hipt_abmil_atec23_amd import dropin
    dropin.uninstall()
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.") or k.startswith("HIPT_4K")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_install_resnet_is_opt_in_and_uninstall_restores(clean_modules):
    from hipt_abmil_atec23_amd import dropin
    pkg = types.ModuleType("models")
    pkg.__path__ = []
    theirs = types.ModuleType("models.resnet_custom")
    pkg.resnet_custom = theirs
    sys.modules["models"], sys.modules["models.resnet_custom"] = pkg, theirs
    done = dropin.install()
    assert "models.resnet_custom" not in done and sys.modules["models.resnet_custom"] is theirs
    done = dropin.install(resnet=True)
    assert done["models.resnet_custom"] == "hipt_abmil_atec23_amd.resnet_custom"
    assert sys.modules["models.resnet_custom"] is rc and pkg.resnet_custom is rc
    from models.resnet_custom import resnet50_baseline  # noqa: F401  (the reference's import line)
    assert resnet50_baseline is rc.resnet50_baseline
    dropin.uninstall()
    assert sys.modules["models.resnet_custom"] is theirs and pkg.resnet_custom is theirs


def test_overlay_file_maps_resnet_custom():
    path = os.path.join(ROOT, "shims", "models", "resnet_custom.py")
    spec = importlib.util.spec_from_file_location("overlay_resnet_custom", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("ResNet_Baseline", "Bottleneck_Baseline", "resnet50_baseline", "resnet18_baseline", "load_pretrained_weights", "model_urls"):
        assert getattr(mod, name) is getattr(rc, name), name


def test_fp64_restatement_reproduces_golden():
    g = R.golden()
    sd = R.state_dict(g)
    for name, b, h, w, seed in R.CASES:
        x = R.normalized(synth.hash_u8_np((b, 3, h, w), seed))
        got = R.forward_fp64(sd, x).numpy()
        ref64, ref32 = g["out64_" + name], g["out_" + name].astype(np.float64)
        assert got.shape == ref64.shape == ref32.shape == (b, 1024)
        rel = np.linalg.norm(got - ref64) / np.linalg.norm(ref64)
        assert rel <= 1e-6, (name, rel)
        # the reference's fp32 run: fp32 rounding over 43 convolutions (2-4e-6 measured)
        rel = np.linalg.norm(got - ref32) / np.linalg.norm(ref32)
        assert rel <= 2e-5, (name, rel)


def test_bf16_emulation_is_near_the_reference():
    # the bf16 rounding points alone (no kernel involved): the size of the error the bf16 mode is held to
    g = R.golden()
    sd = R.state_dict(g)
    name, b, h, w, seed = R.CASES[0]
    x = R.normalized(synth.hash_u8_np((b, 3, h, w), seed))
    emu, ref = R.forward_bf16_emulated(sd, x).numpy(), g["out64_" + name]
    rel = np.linalg.norm(emu - ref) / np.linalg.norm(ref)
    cos = (emu * ref).sum(1) / (np.linalg.norm(emu, axis=1) * np.linalg.norm(ref, axis=1))
    assert 5e-3 < rel < 5e-2 and cos.min() >= 0.999, (rel, cos)
