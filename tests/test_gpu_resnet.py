"""ResNet-50 baseline extractor on the MI355X: every conv form of the fine-grained entry against fp64 ``F.conv2d``, the
pools, the whole network against the reference's stored outputs (tests/golden/resnet50_baseline.npz), input-format and
batch invariance, streams, DataParallel replicas, refusals, extract_slide and ResNet-ABMIL end to end."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref as R  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import resnet_custom as rc  # noqa: E402
from hipt_abmil_atec23_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DT = {"fp32": N.HIPT_F32, "bf16": N.HIPT_BF16}


class _Calls:
    def __enter__(self):
        self.before = N.calls
        return self

    def __exit__(self, *exc):
        if exc[0] is None:
            assert N.calls > self.before, "the native library was not called"


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def check(got, ref, dtype):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if dtype == "fp32":
        err = float(np.abs(got - ref).max())
        assert err <= 1e-4 * max(1.0, float(np.abs(ref).max())), err
    else:
        assert rel_l2(got, ref) <= 2e-2, rel_l2(got, ref)


@pytest.fixture(scope="module")
def golden():
    return R.golden()


@pytest.fixture(scope="module")
def model(golden):
    m = rc.resnet50_baseline()
    m.load_state_dict(R.state_dict(golden), strict=False)
    return m.eval().to(DEV)


def _pixels(b, h, w, seed):
    return synth.hash_u8_np((b, 3, h, w), seed)


# ---- a layer table whose block input / output parity differs from the default ------------------------------------------------
ODD_LAYERS = (1, 2, 1)   # a one-block layer flips which of the two buffers is "current" when the next layer starts


@pytest.fixture(scope="module")
def odd_net():
    """(model, state dict): hash weights and running statistics (means within +-0.1, variances in [0.5, 1.5])"""
    specs = synth.resnet_param_specs(ODD_LAYERS)
    for _, bn, cout, _, _ in synth.resnet_conv_bn_names(ODD_LAYERS):
        specs[bn + ".running_mean"], specs[bn + ".running_var"] = ((cout,), 0.1, 0.0), ((cout,), 0.5, 1.0)
    sd = synth.make_state_dict(specs)
    m = rc.ResNet_Baseline(rc.Bottleneck_Baseline, list(ODD_LAYERS))
    m.load_state_dict(sd, strict=False)
    return m.eval().to(DEV).set_compute_dtype("fp32"), sd


@pytest.mark.parametrize("b,h,w", [(1, 32, 32), (2, 64, 32)], ids=lambda v: str(v))
def test_other_layer_table_against_the_fp64_restatement(odd_net, b, h, w):
    m, sd = odd_net
    x = R.normalized(_pixels(b, h, w, 301 + h))
    with _Calls(), torch.no_grad():
        got = m(x.to(DEV)).cpu().numpy()
    ref = R.forward_fp64(sd, x, ODD_LAYERS).numpy()
    err = float(np.abs(got - ref).max())
    print(f"resnet {ODD_LAYERS} fp32 {b}x{h}x{w}: max|d| {err:.3e} (|ref|max {np.abs(ref).max():.3f})")
    assert got.shape == ref.shape == (b, 1024) and float(np.abs(ref).max()) > 1e-2
    assert err <= 1e-4 * max(1.0, float(np.abs(ref).max())), err


# ---- units -------------------------------------------------------------------------------------------------------------
def _conv_bn(cin, cout, k, stride, pad, seed):
    conv = torch.nn.Conv2d(cin, cout, k, stride, pad, bias=False)
    bn = torch.nn.BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(synth.hash_uniform_torch(conv.weight.shape, seed, (6.0 / (cout * k * k)) ** 0.5))
        bn.weight.copy_(synth.hash_uniform_torch((cout,), seed + 1, 0.1, 1.0))
        bn.bias.copy_(synth.hash_uniform_torch((cout,), seed + 2, 0.05))
        bn.running_mean.copy_(synth.hash_uniform_torch((cout,), seed + 3, 0.2))
        bn.running_var.copy_(synth.hash_uniform_torch((cout,), seed + 4, 0.5, 1.0))
    return conv.eval(), bn.eval()


# (cin, cout, k, stride, pad, n, h, w): the stem, 1x1 s1 / s2, 3x3 s1 / s2, with M odd, below and above one 128-row tile
CONV_FORMS = [
    (3, 64, 7, 2, 3, 2, 38, 30),
    (64, 256, 1, 1, 0, 1, 9, 7),
    (64, 128, 1, 2, 0, 2, 21, 17),
    (128, 64, 3, 1, 1, 1, 13, 11),
    (64, 128, 3, 2, 1, 3, 17, 23),
    (256, 64, 1, 1, 0, 2, 16, 16),
]


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("form", CONV_FORMS, ids=lambda f: "c{}-{}k{}s{}p{}_{}x{}x{}".format(*f))
@pytest.mark.parametrize("resid,relu", [(False, False), (True, True), (False, True)])
def test_conv_forms(dtype, form, resid, relu):
    cin, cout, k, s, p, n, h, w = form
    conv, bn = _conv_bn(cin, cout, k, s, p, 1000 + cin + cout + k)
    x = synth.hash_uniform_torch((n, h, w, cin), 7 + k)
    oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
    r = synth.hash_uniform_torch((n, oh, ow, cout), 9) if resid else None
    code = DT[dtype]
    with _Calls():
        wpk, b = rc.pack_conv_bn(conv.to(DEV), bn.to(DEV), code)
        out = rc.conv2d_nhwc(x.to(DEV), wpk, b, k, s, p, resid=None if r is None else r.to(DEV), relu=relu, dtype=code)
    assert out.shape == (n, oh, ow, cout) and out.dtype == (torch.float32 if dtype == "fp32" else torch.bfloat16)
    cast = (lambda t: t.double()) if dtype == "fp32" else (lambda t: t.bfloat16().double())
    xr = cast(x).permute(0, 3, 1, 2)
    ref = F.batch_norm(F.conv2d(xr, conv.weight.detach().cpu().double(), stride=s, padding=p), bn.running_mean.cpu().double(),
                       bn.running_var.cpu().double(), bn.weight.detach().cpu().double(), bn.bias.detach().cpu().double(), False, 0.0,
                       bn.eps).permute(0, 2, 3, 1)
    if r is not None:
        ref = ref + cast(r)
    if relu:
        ref = ref.clamp_min(0)
    check(out.float().cpu().numpy(), ref.numpy(), dtype)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pools(dtype):
    code = DT[dtype]
    x = synth.hash_uniform_torch((3, 33, 30, 64), 21)
    if dtype == "bf16":
        x = x.bfloat16()
    with _Calls():
        mp = rc.maxpool_nhwc(x.to(DEV), code)
        ap = rc.avgpool_nhwc(x.to(DEV), code)
    ref = F.max_pool2d(x.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.equal(mp.cpu().double(), ref)  # a max picks one of its inputs: exact
    refa = x.double().mean(dim=(1, 2))
    assert float((ap.cpu().double() - refa).abs().max()) <= 1e-6  # one fp32 sum over 990 values in [-1, 1)


# ---- the network ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c[0])
def test_network_against_golden(model, golden, dtype, case):
    name, b, h, w, seed = case
    model.set_compute_dtype(dtype)
    x = R.normalized(_pixels(b, h, w, seed)).to(DEV)
    with _Calls(), torch.no_grad():
        out = model(x)
    assert out.shape == (b, 1024) and out.dtype == torch.float32
    model.set_compute_dtype("fp32")
    got, ref = out.cpu().numpy(), golden["out_" + name]
    if dtype == "fp32":
        check(got, ref, dtype)
        return
    # bf16: the format itself costs 2.2-3.9 % rel-L2 on this 43-conv stack (the bf16 emulation below lands there too, mostly
    # from rounding the weights and the input: DESIGN.md 11.4).  The kernels are held to the emulation of the same rounding
    # points -- closer than the format's own error, not bitwise: this randomly initialised stack amplifies the few roundings
    # that fp32 accumulation order flips (0.9 % measured at 128 x 128) -- and the features to the fp32 reference's per-row direction
    emu = R.forward_bf16_emulated(R.state_dict(golden), R.normalized(_pixels(b, h, w, seed))).numpy()
    assert rel_l2(got, emu) <= 2e-2, rel_l2(got, emu)
    cos = (got * ref).sum(1) / (np.linalg.norm(got, axis=1) * np.linalg.norm(ref, axis=1))
    assert float(cos.min()) >= 0.999, cos
    assert rel_l2(got, ref) <= 5e-2, rel_l2(got, ref)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_uint8_inputs_give_the_same_bits(model, dtype):
    model.set_compute_dtype(dtype)
    u8 = torch.from_numpy(_pixels(3, 128, 96, 31))
    with _Calls(), torch.no_grad():
        a = model(R.normalized(u8).to(DEV))  # ToTensor + Normalize on the host, fp32 input
        b = model(u8.to(DEV))  # uint8 planar
        c = model(u8.permute(0, 2, 3, 1).contiguous().to(DEV))  # uint8 interleaved [B, H, W, 3]
        model.set_input_normalization(0.5, 0.5)
        d = model(u8.to(DEV))
        e = model(R.normalized(u8, (0.5,) * 3, (0.5,) * 3).to(DEV))
        model.set_input_normalization()
    model.set_compute_dtype("fp32")
    assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(d, e) and not torch.equal(a, d)


@pytest.mark.parametrize("dtype,size", [("fp32", 128), ("bf16", 256)])
def test_batch_invariance(model, dtype, size):
    model.set_compute_dtype(dtype)
    u8 = torch.from_numpy(_pixels(256, size, size, 41)).to(DEV)
    k = 19
    with _Calls(), torch.no_grad():
        alone = model(u8[100:101])
        in37 = model(torch.cat([u8[:k], u8[100:101], u8[k + 1:37]]))
        in256 = model(u8)
    model.set_compute_dtype("fp32")
    assert torch.equal(alone[0], in37[k]) and torch.equal(alone[0], in256[100])


def test_two_streams(model):
    model.set_compute_dtype("bf16")
    x1 = torch.from_numpy(_pixels(16, 256, 256, 51)).to(DEV)
    x2 = torch.from_numpy(_pixels(16, 256, 256, 52)).to(DEV)
    with torch.no_grad():
        r1, r2 = model(x1), model(x2)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        s1.wait_stream(torch.cuda.current_stream())
        s2.wait_stream(torch.cuda.current_stream())
        with _Calls():
            for _ in range(2):
                with torch.cuda.stream(s1):
                    a = model(x1)
                with torch.cuda.stream(s2):
                    b = model(x2)
        torch.cuda.synchronize()
    model.set_compute_dtype("fp32")
    assert torch.equal(a, r1) and torch.equal(b, r2)


def test_dataparallel_replica(model):
    x = torch.from_numpy(_pixels(4, 128, 128, 61)).to(DEV)
    with torch.no_grad():
        ref = model(x)
        rep = torch.nn.parallel.replicate(model, [0])[0]
        assert list(rep.parameters()) == [] and rep.weight_device == torch.device(DEV)
        with _Calls():
            got = rep(x)
        dp = torch.nn.DataParallel(model, device_ids=[0])
        got2 = dp(x)
    assert torch.equal(got, ref) and torch.equal(got2, ref)


def test_refusals(model):
    x = torch.from_numpy(_pixels(1, 64, 64, 71)).to(DEV)
    model.train()
    try:
        with pytest.raises(RuntimeError, match=r"\.eval\(\)"):
            model(x)
    finally:
        model.eval()
    for h, w in ((40, 64), (64, 72), (16, 64)):
        with pytest.raises(RuntimeError, match="envelope"):
            with torch.no_grad():
                model(torch.zeros(1, 3, h, w, device=DEV))
    with pytest.raises(RuntimeError, match="HIP device"):
        model(x.cpu())


def test_grad_warning_once(golden):
    m = rc.resnet50_baseline()
    m.load_state_dict(R.state_dict(golden), strict=False)
    m = m.eval().to(DEV)
    x = torch.from_numpy(_pixels(1, 64, 64, 72)).to(DEV)
    with pytest.warns(UserWarning, match="grad"):
        m(x)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        m(x)


def test_weight_changes_repack(golden):
    m = rc.resnet50_baseline()
    m.load_state_dict(R.state_dict(golden), strict=False)
    m = m.eval().to(DEV)
    x = torch.from_numpy(_pixels(2, 64, 64, 73)).to(DEV)
    with torch.no_grad():
        a = m(x)
        m.layer3[5].bn3.running_mean.add_(0.5)
        b = m(x)
    assert not torch.equal(a, b)


def test_extract_slide_host_batches(model, tmp_path):
    from hipt_abmil_atec23_amd.feature_store import extract_slide, load_coords
    model.set_compute_dtype("bf16")
    n, bs = 300, 32
    pix = torch.from_numpy(_pixels(n, 256, 256, 81))
    batches = [(pix[i:i + bs].pin_memory(), torch.stack([torch.arange(i, min(i + bs, n)) * 256, torch.arange(i, min(i + bs, n))], 1))
               for i in range(0, n, bs)]
    with _Calls():
        path = extract_slide(model, batches, str(tmp_path), "slide", coalesce=64)
    feats = torch.load(path)
    with torch.no_grad():
        direct = torch.cat([model(b.to(DEV)).cpu() for b, _ in batches])
    model.set_compute_dtype("fp32")
    assert os.path.basename(path) == "slide.pt" and feats.shape == (n, 1024)
    assert torch.equal(feats, direct)
    assert np.array_equal(load_coords(str(tmp_path), "slide"), torch.cat([c for _, c in batches]).numpy())


def test_resnet_abmil_end_to_end(model):
    from hipt_abmil_atec23_amd import CLAM_SB
    from oracle import hipt_oracle as O
    x = torch.from_numpy(_pixels(40, 256, 256, 91)).to(DEV)
    with torch.no_grad():
        h = model(x)
    sc = synth.clam_param_specs((1024, 64, 16))
    c = CLAM_SB(size_arg="tinier")
    c.load_state_dict(synth.make_state_dict(sc, 1024))
    c.relocate()
    c.eval()
    with _Calls(), torch.no_grad():
        logits, y_prob, y_hat, a_raw, _ = c(h)
    r = O.clam_sb_forward(h.cpu().numpy().astype(np.float64), synth.make_params_np(sc, 1024))
    e1 = float(np.abs(a_raw.cpu().numpy() - r["A_raw"]).max())
    e2 = float(np.abs(logits.cpu().numpy() - r["logits"]).max())
    assert e1 < 1e-4 and e2 < 1e-4 and int(y_hat.reshape(-1)[0]) == int(np.asarray(r["Y_hat"]).reshape(-1)[0]), (e1, e2)
