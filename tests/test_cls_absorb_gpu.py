"""The [CLS]-pruned last ViT-256 block without its K / V projection (csrc/cls_pool.hip) on the GPU: against the fp64
oracle at the bar of the bf16 `cls256` parity test (tests/test_gpu_parity.py, test_hipt4k_full_region_fp32_and_bf16: relative L2
1.3e-2, cosine 0.9999), against the old route (HIPT_NO_CLS_ABSORB=1, the fused kernel's [CLS]-only form, in a fresh child process)
within twice that bar, and bit for bit against itself: whatever shares the call, the stream count, the workgroup count, the run.
Measured on an MI355X (16 patches, relative L2 against the fp64 oracle): absorbed route 6.16e-3, old route 6.10e-3, the two 1.15e-3 apart."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from hipt_abmil_atec23_amd import synth
from oracle import hipt_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR_L2, BAR_COS = 1.3e-2, 0.9999  # the bf16 cls256 bar (module docstring)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def cosine(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))


@pytest.fixture(scope="module")
def vit256():
    from hipt_abmil_atec23_amd.vision_transformer import vit_small
    m = vit_small(patch_size=16, num_classes=0)
    m.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m = m.eval().to(DEV)
    m.set_compute_dtype("bf16")
    return m


@pytest.fixture(scope="module")
def hipt():
    from hipt_abmil_atec23_amd import HIPT_4K
    m = HIPT_4K(None, None, DEV, DEV)
    m.model256.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
    m.model4k.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit4k", embed_dim=192, depth=6), 4096))
    m = m.eval().to(DEV)
    m.set_compute_dtype("bf16")
    return m


CHILD = """
import sys, numpy as np, torch
from hipt_abmil_atec23_amd import synth
from hipt_abmil_atec23_amd.vision_transformer import vit_small
m = vit_small(patch_size=16, num_classes=0)
m.load_state_dict(synth.make_state_dict(synth.vit_param_specs("vit256"), 256))
m = m.eval().to("cuda:0")
m.set_compute_dtype("bf16")
x = synth.hash_uniform_torch((16, 3, 256, 256), 77, device="cuda:0")
np.save(sys.argv[1], m(x).float().cpu().numpy())
"""


def test_absorbed_route_vs_fp64_oracle_and_vs_the_old_route(vit256, tmp_path):
    """16 patches (whole 16-row fragments: the image path, the pruned block)."""
    x = synth.hash_uniform_torch((16, 3, 256, 256), 77, device=DEV)
    new = vit256(x).float().cpu().numpy()
    p = {k: v.astype(np.float64) for k, v in synth.make_params_np(synth.vit_param_specs("vit256"), 256).items()}
    want = O.vit256_forward(x.cpu().numpy().astype(np.float64), p, 6)
    assert want.dtype == np.float64
    out = str(tmp_path / "old.npy")
    env = dict(os.environ, HIPT_NO_CLS_ABSORB="1", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    subprocess.run([sys.executable, "-c", CHILD, out], check=True, env=env, cwd=ROOT, timeout=600)
    old = np.load(out)
    print(f"cls256 of 16 patches vs the fp64 oracle: absorbed route rel-L2 {rel_l2(new, want):.3e} cosine {cosine(new, want):.6f}; "
          f"old route rel-L2 {rel_l2(old, want):.3e} cosine {cosine(old, want):.6f}; new vs old rel-L2 {rel_l2(new, old):.3e}; "
          f"bitwise equal: {np.array_equal(new, old)}")
    assert rel_l2(new, want) < BAR_L2 and cosine(new, want) > BAR_COS
    assert rel_l2(old, want) < BAR_L2 and cosine(old, want) > BAR_COS
    assert rel_l2(new, old) < 2 * BAR_L2
    assert not np.array_equal(new, old)  # (the switch selected another route: the two round at different points)


def test_a_patch_does_not_depend_on_the_calls_other_patches(vit256):
    """256 patches alone (one region: the row GEMMs' small-M kernel) and inside a 2 048-patch call (their tiled kernel, four patches
    per workgroup); and a call whose patch count is not a multiple of the workgroup count."""
    x = synth.hash_uniform_torch((2048, 3, 256, 256), 78, device=DEV)
    big = vit256(x)
    alone = vit256(x[512:768])
    assert torch.equal(big[512:768], alone), float((big[512:768].float() - alone.float()).abs().max())
    ragged = vit256(x[:528])  # 528 = 2 x 256 + 16 work units
    assert torch.equal(ragged, big[:528])
    assert torch.equal(vit256(x[512:528]), big[512:528])
    assert bool(torch.isfinite(big).all())


def test_one_stream_and_three_streams_same_bits(hipt):
    """18 regions: the smallest call HIPT_4K spreads over THREE streams (a stream per six regions, HIPT_4K._parts); three distinct
    regions, each six times, so that every stream also holds every one of them."""
    x = synth.hash_uniform_torch((3, 3, 4096, 4096), 79, device=DEV).repeat(6, 1, 1, 1)
    old = hipt.streams
    try:
        hipt.streams = 1
        assert hipt._parts(x.shape[0]) == 1
        one = hipt(x)
        hipt.streams = 3
        assert hipt._parts(x.shape[0]) == 3  # (the call really is cut three ways)
        three = hipt(x)
        torch.cuda.synchronize()
        assert any(len(v) == 3 for v in hipt._side_streams.values())  # (and its three streams exist)
    finally:
        hipt.streams = old
    assert torch.equal(one, three)
    assert torch.equal(one[:3], one[3:6]) and torch.equal(three[:3], three[15:18])  # the same region, the same bits, wherever it sits


def test_two_stream_soak_same_bits_every_repeat(vit256):
    """A second stream runs a different kernel (a GEMM of another module) beside the pruned block, 30 repeats: identical bits."""
    x = synth.hash_uniform_torch((512, 3, 256, 256), 80, device=DEV)
    a = torch.randn(2048, 2048, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    ref = vit256(x).clone()
    torch.cuda.synchronize()
    for rep in range(30):
        with torch.cuda.stream(side):
            for _ in range(4):
                b = a @ a
        o = vit256(x)
        torch.cuda.synchronize()
        assert torch.equal(o, ref), rep
    del b
