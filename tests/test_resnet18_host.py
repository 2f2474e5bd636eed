"""HistoResNet-18 extractor, host side (no GPU): torchvision's state-dict contract, the reference's Histo checkpoint route, the
library's planning entry points (against the cross-compiled library), the drop-in switch, and the two restatements of the network
the GPU tests compare against (tests/resnet18_ref.py) held against each other."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet18_ref as R  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import resnet18 as r18  # noqa: E402
from hipt_abmil_atec23_amd import resnet_custom as rc  # noqa: E402
from hipt_abmil_atec23_amd import synth  # noqa: E402

FAKE = 1 << 20  # a non-null, aligned address that no call dereferences before its checks
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4


# ---- key contract --------------------------------------------------------------------------------------------------------
def test_state_dict_is_torchvisions_122_keys_in_order():
    m = r18.resnet18_baseline()
    assert list(m.state_dict().keys()) == R.key_list() and len(R.key_list()) == 122
    assert list(R.TorchResNet18().state_dict().keys()) == R.key_list()
    assert r18.BasicBlock_Baseline.expansion == 1 and isinstance(m.fc, torch.nn.Linear)
    assert m.fc.weight.shape == (1000, 512) and m.layer4[0].downsample[0].weight.shape == (512, 256, 1, 1)
    assert m.layer2[0].conv1.stride == (2, 2) and m.layer2[0].conv2.stride == (1, 1)   # the stride sits on conv1
    import hipt_abmil_atec23_amd as pkg
    assert pkg.ResNet18_Baseline is r18.ResNet18_Baseline and pkg.resnet18_baseline is r18.resnet18_baseline


def test_full_dict_loads_strict_and_a_resnet50_dict_does_not():
    src = R.TorchResNet18()
    m = r18.resnet18_baseline()
    m.load_state_dict(src.state_dict(), strict=True)
    assert torch.equal(m.layer4[1].conv2.weight, src.layer4[1].conv2.weight) and torch.equal(m.fc.bias, src.fc.bias)
    with pytest.raises(RuntimeError):
        m.load_state_dict(rc.resnet50_baseline().state_dict(), strict=True)


def test_synth_specs_cover_every_tensor_but_the_counters():
    m = r18.resnet18_baseline()
    sp = synth.resnet18_param_specs()
    assert list(sp) == [k for k in R.key_list() if not k.endswith("num_batches_tracked")]
    sd = synth.make_state_dict(sp)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(m.state_dict()[k].shape), k
        if k.endswith("running_var"):
            assert 0.5 <= float(v.min()) and float(v.max()) <= 1.5
        if k.endswith("running_mean"):
            assert float(v.abs().max()) <= 0.1
    # additive: the ResNet-50 specs are what they were
    assert len(synth.resnet_param_specs()) == 3 * 43 and "fc.weight" not in synth.resnet_param_specs()


# ---- the Histo route -----------------------------------------------------------------------------------------------------
def _write_ckpt(path, prefix="model.resnet.", keep=lambda k: True):
    sd = {prefix + k: v for k, v in R.state_dict().items() if keep(k)}
    sd["model.projection.weight"] = torch.full((7, 7), 123.0)
    torch.save({"state_dict": sd, "epoch": 3}, path)


def test_histo_checkpoint_loads_cleans_keys_and_empties_fc(tmp_path, capsys):
    path = str(tmp_path / "tenpercent_resnet18.ckpt")
    _write_ckpt(path, keep=lambda k: not k.startswith("fc."))
    m = r18.resnet18_baseline(pretrained=True, dataset="Histo", ckpt_path=path)
    assert "Loading histo-pretrained ResNet18" in capsys.readouterr().out
    ref = R.state_dict()
    got = m.state_dict()
    assert isinstance(m.fc, torch.nn.Sequential) and len(m.fc) == 0
    assert not any(k.startswith(("projection", "fc.")) for k in got)
    for k, v in ref.items():
        if not k.startswith("fc."):
            assert torch.equal(got[k], v), k


def test_histo_checkpoint_without_a_match_says_so_and_still_empties_fc(tmp_path, capsys):
    path = str(tmp_path / "other.ckpt")
    torch.save({"state_dict": {"encoder.conv1.weight": torch.zeros(64, 3, 7, 7)}}, path)
    m = r18.resnet18_baseline(pretrained=True, dataset="Histo", ckpt_path=path)
    assert "No weight could be loaded.." in capsys.readouterr().out
    assert isinstance(m.fc, torch.nn.Sequential) and len(m.fc) == 0


def test_histo_missing_file_raises_and_unpretrained_keeps_fc(tmp_path, monkeypatch):
    missing = str(tmp_path / "nope.ckpt")
    with pytest.raises(FileNotFoundError, match="nope.ckpt"):
        r18.resnet18_baseline(pretrained=True, dataset="Histo", ckpt_path=missing)
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match="tenpercent_resnet18.ckpt"):   # the reference's relative default
        r18.resnet18_baseline(pretrained=True, dataset="Histo")
    m = r18.resnet18_baseline(pretrained=False, dataset="Histo")
    assert isinstance(m.fc, torch.nn.Linear) and m.fc.out_features == 1000   # the reference's quirk, mirrored


def test_imagenet_pretrained_reads_the_hub_cache_and_never_fetches(tmp_path, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a network fetch was attempted")
    monkeypatch.setattr(torch.hub, "load_state_dict_from_url", boom)
    monkeypatch.setenv("TORCH_HOME", str(tmp_path))
    with pytest.raises(FileNotFoundError, match="resnet18-5c106cde.pth"):
        r18.resnet18_baseline(pretrained=True)
    path = rc.cached_checkpoint_path("resnet18")
    os.makedirs(os.path.dirname(path))
    torch.save(R.state_dict(), path)
    m = r18.resnet18_baseline(pretrained=True)
    assert torch.equal(m.layer3[0].downsample[0].weight, R.state_dict()["layer3.0.downsample.0.weight"])
    assert isinstance(m.fc, torch.nn.Linear)


def test_refusals_that_need_no_device():
    m = r18.resnet18_baseline().eval()
    with pytest.raises(RuntimeError, match="HIP device"):
        m(torch.zeros(1, 3, 64, 64))
    m.fc = torch.nn.Identity()
    with pytest.raises(NotImplementedError, match="fc"):
        m(torch.zeros(1, 3, 64, 64))
    assert m._norm == rc.IMAGENET_MEAN + rc.IMAGENET_STD and m.set_input_normalization(0.5, 0.5)._norm == (0.5,) * 6
    assert m.set_compute_dtype("bf16").compute_dtype == "bf16"
    assert m.set_tile_rows(128)._tile_rows == 128 and m.set_tile_rows()._tile_rows == 0
    with pytest.raises(ValueError):
        m.set_tile_rows(64)


# ---- library planning (the cross-compiled library; nothing is launched) -----------------------------------------------------
def basic_weights(dtype, layers=(2, 2, 2, 2)):
    names = synth.resnet18_conv_bn_names(layers)
    arr = (N.ConvBN * len(names))()
    for c, (_, _, cout, cin, k) in zip(arr, names):
        c.weight = c.bn_weight = c.bn_bias = c.bn_mean = c.bn_var = FAKE
        c.cin, c.cout, c.kh, c.kw, c.bn_eps = cin, cout, k, k, 1e-5
    w = N.ResnetBasicWeights(dtype=dtype, n_convs=len(names))
    w.layers[:] = list(layers) + [0] * (4 - len(layers))
    w.convs = C.cast(arr, C.POINTER(N.ConvBN))
    w._keep = arr
    return w


def _al(b):
    return (b + 255) // 256 * 256


@pytest.mark.parametrize("dtype,es", [(N.HIPT_F32, 4), (N.HIPT_BF16, 2)])
def test_packed_and_workspace_sizes_are_the_sums_of_their_carves(dtype, es):
    lib = N.lib()
    w = basic_weights(dtype)
    kb = 64 if es == 2 else 32
    packed = sum(_al(cout * (-(-cin * k * k // kb) * kb) * es) + _al(cout * 4) for _, _, cout, cin, k in synth.resnet18_conv_bn_names())
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) == packed
    for n, h, wd in ((1, 32, 32), (3, 96, 64), (32, 256, 256)):
        # block input / output: stem and maxpool outputs dominate; interior: the NHWC input copy or layer1's maps; downsample: layer2's
        a = n * (h // 2) * (wd // 2) * 64
        b = n * (h // 4) * (wd // 4) * 64
        t = max(n * h * wd * 3, b)
        d = n * (h // 8) * (wd // 8) * 128
        assert lib.hipt_resnet_basic_workspace_bytes(C.byref(w), n, h, wd) == sum(_al(x * es) for x in (a, b, t, d)), (n, h, wd)


def test_size_functions_return_zero_for_a_wrong_count_or_shape():
    lib = N.lib()
    w = basic_weights(N.HIPT_F32)
    assert lib.hipt_resnet_basic_packed_bytes(None) == 0 and lib.hipt_resnet_basic_workspace_bytes(None, 1, 32, 32) == 0
    assert lib.hipt_resnet_basic_workspace_bytes(C.byref(w), 0, 32, 32) == 0
    for h, wd in ((48, 48), (64, 80), (16, 32)):   # what the forward refuses has no size
        assert lib.hipt_resnet_basic_workspace_bytes(C.byref(w), 1, h, wd) == 0 and b"envelope" in lib.hipt_last_error()
    w.tile_rows = 64       # the struct's switch takes 0 or 128
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) == 0 and b"tile_rows" in lib.hipt_last_error()
    w.tile_rows = 128
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) > 0
    w.tile_rows = 0
    w.n_convs -= 1
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) == 0 and lib.hipt_resnet_basic_workspace_bytes(C.byref(w), 1, 32, 32) == 0
    w = basic_weights(N.HIPT_F32)
    w.convs[3].cin = 128   # layer1.1.conv1 is 64 -> 64
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) == 0 and b"conv 3" in lib.hipt_last_error()
    w = basic_weights(N.HIPT_F32)
    w.layers[1] = 0        # a hole in the layer table
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) == 0
    w = basic_weights(7)
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(w)) == 0
    # a shorter network is a valid one: layer1..layer3 of BasicBlocks
    assert lib.hipt_resnet_basic_packed_bytes(C.byref(basic_weights(N.HIPT_BF16, (2, 2, 2)))) > 0


def _forward(lib, w, h, wd, ws, nbytes):
    return lib.hipt_resnet_basic_forward(C.byref(w), FAKE, FAKE, N.RESNET_IN_F32, None, 1, h, wd, FAKE, ws, nbytes, None)


def test_forward_refuses_before_any_launch():
    """Every pointer is a fake address: a refusal that came after a launch or a dereference would not return."""
    lib = N.lib()
    w = basic_weights(N.HIPT_BF16)
    need = lib.hipt_resnet_basic_workspace_bytes(C.byref(w), 1, 32, 32)
    assert need > 0 and need % 256 == 0
    assert _forward(lib, w, 32, 32, FAKE, need - 1) == E_WORKSPACE
    msg = lib.hipt_last_error().decode()
    assert msg.startswith("resnet_basic_forward: workspace") and str(need) in msg and "too small / unaligned" in msg
    assert _forward(lib, w, 32, 32, FAKE + 16, need) == E_BADARG
    for h, wd in ((48, 48), (64, 80), (16, 32)):
        assert _forward(lib, w, h, wd, FAKE, 1 << 30) == E_UNSUPPORTED
        assert b"envelope" in lib.hipt_last_error()
    assert lib.hipt_resnet_basic_forward(C.byref(w), FAKE, FAKE, 9, None, 1, 32, 32, FAKE, FAKE, need, None) == E_BADARG
    if not torch.cuda.is_available():
        assert _forward(lib, w, 32, 32, FAKE, need) not in (E_WORKSPACE, E_BADARG, E_UNSUPPORTED)   # into the first launch: no device


def test_tile_rule_is_a_function_of_the_conv_shape():
    rows = N.lib().hipt_conv_tile_rows
    # batch 32 of 256 x 256 patches: layer1, layer2 fill the chip with 128-row tiles; layer3 (128 workgroups), layer4 (64) do not
    assert [rows(32 * s * s, c) for s, c in ((64, 64), (32, 128), (16, 256), (8, 512))] == [128, 128, 64, 64]
    # 64 rows only where they add a workgroup: one partial tile stays one tile
    assert rows(64, 128) == 128 and rows(65, 128) == 64 and rows(1, 512) == 128
    assert rows(0, 64) == 0 and rows(128, 96) == 0
    assert lib_refuses_tile_rows(96)


def lib_refuses_tile_rows(rows):
    rc_ = N.lib().hipt_conv2d_ex(FAKE, 1, 8, 8, 64, FAKE, FAKE, 64, 3, 3, 1, 1, None, 0, FAKE, N.HIPT_F32, rows, None)
    return rc_ == E_BADARG and b"tile_rows" in N.lib().hipt_last_error()


# ---- drop-in -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def clean_modules():
    saved = {k: v for k, v in sys.modules.items() if k == "models" or k.startswith("models.") or k.startswith("HIPT_4K")}
    yield
    from hipt_abmil_atec23_amd import dropin
    dropin.uninstall()
    for k in [k for k in sys.modules if k == "models" or k.startswith("models.") or k.startswith("HIPT_4K")]:
        del sys.modules[k]
    sys.modules.update(saved)


def test_install_resnet18_is_opt_in(clean_modules):
    from hipt_abmil_atec23_amd import dropin
    pkg = types.ModuleType("models")
    pkg.__path__ = []
    theirs = types.ModuleType("models.resnet_custom")
    theirs.resnet18_baseline = their_fn = lambda *a, **k: "theirs"
    pkg.resnet_custom = theirs
    sys.modules["models"], sys.modules["models.resnet_custom"] = pkg, theirs
    done = dropin.install()
    assert not any("resnet18" in k for k in done) and theirs.resnet18_baseline is their_fn
    done = dropin.install(resnet18=True)
    assert done["models.resnet_custom.resnet18_baseline"] == "hipt_abmil_atec23_amd.resnet18.resnet18_baseline"
    from models.resnet_custom import resnet18_baseline   # the reference's import line
    assert resnet18_baseline is r18.resnet18_baseline and sys.modules["models.resnet_custom"] is theirs
    dropin.uninstall()
    assert theirs.resnet18_baseline is their_fn
    # together with resnet=True: this package's resnet_custom names, the one function replaced, the package module untouched
    dropin.install(resnet=True, resnet18=True)
    import models.resnet_custom as both
    assert both.resnet18_baseline is r18.resnet18_baseline and both.resnet50_baseline is rc.resnet50_baseline
    assert both is not rc
    dropin.uninstall()
    assert sys.modules["models.resnet_custom"] is theirs and pkg.resnet_custom is theirs


def test_the_resnet_custom_stub_still_raises():
    # the feature lives in resnet18.py; the stub is another module's (and another test's) contract
    with pytest.raises(NotImplementedError, match="ResNet-18"):
        rc.resnet18_baseline(pretrained=False)


# ---- the two restatements against each other -------------------------------------------------------------------------------
def test_fp32_module_and_fp64_restatement_agree():
    sd = R.state_dict()
    net = R.TorchResNet18().eval()
    net.load_state_dict(sd, strict=False)
    for name, b, h, w, seed in R.CASES:
        x = R.normalized(R.pixels(b, h, w, seed))
        with torch.no_grad():
            got = net.features(x).double()
            logits = net(x).double()
        ref = R.forward_fp64(sd, x)
        assert got.shape == ref.shape == (b, 512)
        bar = 1e-5 * max(1.0, float(ref.abs().max()))
        assert float((got - ref).abs().max()) <= bar, (name, float((got - ref).abs().max()), bar)
        ref_fc = torch.nn.functional.linear(ref, sd["fc.weight"].double(), sd["fc.bias"].double())
        assert float((logits - ref_fc).abs().max()) <= 1e-5 * max(1.0, float(ref_fc.abs().max()))
        assert float(ref.abs().max()) > 1e-2 and float(ref.std()) > 1e-3   # a live signal, not a dead network


def test_bf16_emulation_is_near_the_fp64_restatement():
    sd = R.state_dict()
    name, b, h, w, seed = R.CASES[0]
    x = R.normalized(R.pixels(b, h, w, seed))
    emu, ref = R.forward_bf16_emulated(sd, x), R.forward_fp64(sd, x)
    rel = float((emu - ref).norm() / ref.norm())
    assert 1e-4 < rel < 5e-2, rel   # the rounding points alone: above fp32 noise, below the bar the kernels are held to
