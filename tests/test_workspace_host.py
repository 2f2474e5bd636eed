"""Host tests (no GPU) of the workspace carver (csrc/workspace.h): every *_workspace_bytes entry point returns the size the
hand-written layouts returned before they were replaced by carve functions (the literals below were read from a build of that
earlier commit), every converted forward refuses a short or misaligned buffer before it launches anything, and the source tree
holds no second description of a layout."""
import ctypes as C
import glob
import os
import re

import pytest
import torch

from conftest import ROOT
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd import synth

CSRC = os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc")
FAKE = 1 << 20            # a non-null, 4 KiB-aligned address that no call dereferences before its workspace check
E_BADARG, E_WORKSPACE = -1, -2
TR = 16                   # rows per workgroup of the training kernels (csrc/clam_train.hip)


# ---- the argument structs, filled with fake addresses --------------------------------------------------------------------------
def resnet_weights(dtype):
    """hipt_resnet_weights of the [3, 4, 6] layer table: stem, then conv1 / conv2 / conv3 (+ downsample) per bottleneck."""
    convs, inplanes = [(3, 64, 7)], 64
    for L, blocks in enumerate((3, 4, 6)):
        planes = 64 << L
        for b in range(blocks):
            convs += [(inplanes, planes, 1), (planes, planes, 3), (planes, planes * 4, 1)]
            if b == 0:
                convs.append((inplanes, planes * 4, 1))
            inplanes = planes * 4
    arr = (N.ConvBN * len(convs))()
    for c, (cin, cout, k) in zip(arr, convs):
        c.weight = c.bn_weight = c.bn_bias = c.bn_mean = c.bn_var = FAKE
        c.cin, c.cout, c.kh, c.kw, c.bn_eps = cin, cout, k, k, 1e-5
    w = N.ResnetWeights(dtype=dtype, n_convs=len(convs))
    w.layers[:] = [3, 4, 6]
    w.convs = C.cast(arr, C.POINTER(N.ConvBN))
    w._keep = arr
    return w


def vit_weights(dim, depth, heads, hidden, ntok, embed_k, dtype=N.HIPT_BF16):
    blocks = (N.BlockWeights * depth)()
    w = N.VitWeights(dtype=dtype, dim=dim, depth=depth, heads=heads, hidden=hidden, ntok=ntok, embed_k=embed_k, ln_eps=1e-6)
    w.blocks = C.cast(blocks, C.POINTER(N.BlockWeights))
    w._keep = blocks
    return w


def train_weights(s0, s1, s2, n_att):
    w = N.ClamTrainWeights(s0=s0, s1=s1, s2=s2, n_att=n_att, n_classes=n_att, multi_branch=int(n_att > 1))
    for name in ("w1", "b1", "wa", "ba", "wb", "bb", "wc", "bc", "wcls", "bcls"):
        setattr(w, name, FAKE)
    return w


# ---- sizes: what the earlier commit returned -----------------------------------------------------------------------------------
KNN_BYTES = {(300, 5, 7): 2304, (1000, 33, 64): 405504, (100000, 100, 20): 9384192}
UPDATE_BYTES = {1: 3072, 63: 3328, 64: 3328, 65: 4352, 100000: 2002432}
HEATMAP_BYTES = {(600, 5, 3, 67, 45): 10752, (100000, 64, 64, 10176, 10176): 15656448, (1, 1, 1, 1, 1): 1280, (750, 7, 5, 40, 40): 13056,
                 (20000, 8, 8, 1500, 1100): 398592}
RESNET_SHAPES = ((1, 32, 32), (2, 48, 80), (4, 224, 224))
RESNET_PACKED_BYTES = {"fp32": 34115328, "bf16": 17092352}
RESNET_BYTES = {"fp32": (245760, 1843200, 48168960), "bf16": (122880, 921600, 24084480)}   # at RESNET_SHAPES
VIT256 = dict(dim=384, depth=12, heads=6, hidden=1536, ntok=257, embed_k=768)
VIT_BYTES = {1: 2171136, 16: 34738176}                 # hipt_vit_workspace_bytes(ViT-256, nseq)
RANGE_BYTES = {(16, 0): 34738176, (3000, 0): 4446486528}   # hipt_vit256_range_workspace_bytes(ViT-256, nseq, chunk)
CLAM_BYTES = {1000: 1812992, 100000: 128532992}         # hipt_clam_workspace_bytes([384, 128, 64], N)
CLAM_MB_BYTES = {1: 278784, 70001: 18194688}          # hipt_clam_mb_workspace_bytes(N)
DTYPES = {"fp32": N.HIPT_F32, "bf16": N.HIPT_BF16}


def measured_sizes(lib):
    """Every pinned size, asked of `lib`, in the layout of the tables above."""
    vit = vit_weights(**VIT256)
    clam = N.ClamWeights(dtype=N.HIPT_BF16, s0=384, s1=128, s2=64, n_classes=2, n_att=1)
    rn = {name: resnet_weights(code) for name, code in DTYPES.items()}
    return dict(
        KNN_BYTES={k: lib.hipt_knn_workspace_bytes(*k) for k in KNN_BYTES},
        UPDATE_BYTES={n: lib.hipt_sampling_update_workspace_bytes(n) for n in UPDATE_BYTES},
        HEATMAP_BYTES={k: lib.hipt_heatmap_workspace_bytes(*k) for k in HEATMAP_BYTES},
        RESNET_PACKED_BYTES={name: lib.hipt_resnet_packed_bytes(C.byref(w)) for name, w in rn.items()},
        RESNET_BYTES={name: tuple(lib.hipt_resnet_workspace_bytes(C.byref(w), *s) for s in RESNET_SHAPES) for name, w in rn.items()},
        VIT_BYTES={n: lib.hipt_vit_workspace_bytes(C.byref(vit), n) for n in VIT_BYTES},
        RANGE_BYTES={k: lib.hipt_vit256_range_workspace_bytes(C.byref(vit), *k) for k in RANGE_BYTES},
        CLAM_BYTES={n: lib.hipt_clam_workspace_bytes(C.byref(clam), n) for n in CLAM_BYTES},
        CLAM_MB_BYTES={n: lib.hipt_clam_mb_workspace_bytes(C.byref(clam), n) for n in CLAM_MB_BYTES},
    )


def test_sizes_are_those_of_the_hand_written_layouts():
    got = measured_sizes(N.lib())
    for table, sizes in got.items():
        assert sizes == globals()[table], table
        flat = [v for s in sizes.values() for v in (s if isinstance(s, tuple) else (s,))]
        assert all(v > 0 and v % 256 == 0 for v in flat), table


def test_size_functions_keep_their_zero_for_bad_arguments():
    lib = N.lib()
    assert lib.hipt_knn_workspace_bytes(10, 4, 11) == 0 and lib.hipt_knn_workspace_bytes(0, 4, 1) == 0
    assert lib.hipt_sampling_update_workspace_bytes(0) == 0 and lib.hipt_heatmap_workspace_bytes(0, 8, 8, 100, 100) == 0
    w = resnet_weights(N.HIPT_F32)
    assert lib.hipt_resnet_workspace_bytes(C.byref(w), 0, 32, 32) == 0 and lib.hipt_resnet_workspace_bytes(None, 1, 32, 32) == 0
    w.n_convs -= 1
    assert lib.hipt_resnet_packed_bytes(C.byref(w)) == 0 and lib.hipt_resnet_packed_bytes(None) == 0
    assert lib.hipt_clam_train_workspace_bytes(None, 5) == 0 and lib.hipt_clam_train_workspace_bytes(C.byref(train_weights(32, 16, 8, 1)), 0) == 0
    assert lib.hipt_vit256_range_workspace_bytes(None, 4, 0) == 0


@pytest.mark.parametrize("n,sizes,n_att", [(1, (32, 16, 8), 1), (37, (32, 16, 8), 2), (5000, (1024, 512, 256), 1)])
def test_clam_train_workspace_is_the_sum_of_its_three_rounded_arrays(n, sizes, n_att):
    """duv [N, 2 S2] | dz [N, S1] | per-tile partials [ceil(N / TR), n_att S2 + n_att], fp32, each rounded up to 256 bytes."""
    s0, s1, s2 = sizes
    al = lambda b: (b + 255) // 256 * 256   # noqa: E731
    parts = (4 * n * 2 * s2, 4 * n * s1, 4 * -(-n // TR) * (n_att * s2 + n_att))
    got = N.lib().hipt_clam_train_workspace_bytes(C.byref(train_weights(s0, s1, s2, n_att)), n)
    assert got == sum(al(p) for p in parts)
    assert got % 256 == 0 and sum(parts) <= got < sum(parts) + 768
    assert f"TR = {TR};" in open(os.path.join(CSRC, "clam_train.hip")).read()


# ---- the ResNet drivers, layer tables other than the default ones ------------------------------------------------------------------
def net_weights(family, layers, dtype):
    """hipt_resnet_weights ("resnet") / hipt_resnet_basic_weights ("resnet_basic") of a layer table, fake addresses"""
    names = synth.resnet_conv_bn_names(layers) if family == "resnet" else synth.resnet18_conv_bn_names(layers)
    arr = (N.ConvBN * len(names))()
    for c, (_, _, cout, cin, k) in zip(arr, names):
        c.weight = c.bn_weight = c.bn_bias = c.bn_mean = c.bn_var = FAKE
        c.cin, c.cout, c.kh, c.kw, c.bn_eps = cin, cout, k, k, 1e-5
    w = (N.ResnetWeights if family == "resnet" else N.ResnetBasicWeights)(dtype=dtype, n_convs=len(names))
    w.layers[:] = list(layers) + [0] * (len(w.layers) - len(layers))
    w.convs = C.cast(arr, C.POINTER(N.ConvBN))
    w._keep = arr
    return w


NET_SHAPES = ((1, 32, 32), (2, 64, 96), (3, 224, 224))
# (family, layer table, dtype) -> (packed bytes, workspace bytes at NET_SHAPES), read from a build of the commit before the two
# drivers became one.  A block's output sizes both block input / output buffers, so the workspace does not follow the parity of the
# table ((1, 1, 1) needs what (3, 4, 6) needs), and a BasicBlock table without a downsample still carves 256 bytes for it.
NET_BYTES = {
    ("resnet", (1, 1, 1), "fp32"): (7890688, (245760, 2949120, 36126720)),
    ("resnet", (1, 1, 1), "bf16"): (3958528, (122880, 1474560, 18063360)),
    ("resnet", (2, 1, 3), "fp32"): (17095936, (245760, 2949120, 36126720)),
    ("resnet", (2, 1, 3), "bf16"): (8568064, (122880, 1474560, 18063360)),
    ("resnet", (3, 4, 6), "fp32"): (34115328, (245760, 2949120, 36126720)),
    ("resnet", (3, 4, 6), "bf16"): (17092352, (122880, 1474560, 18063360)),
    ("resnet_basic", (1,), "fp32"): (336640, (98560, 1179904, 14450944)),
    ("resnet_basic", (1,), "bf16"): (172800, (49408, 590080, 7225600)),
    ("resnet_basic", (1, 2, 1, 2), "fp32"): (39674112, (106496, 1277952, 15654912)),
    ("resnet_basic", (1, 2, 1, 2), "bf16"): (19849472, (53248, 638976, 7827456)),
    ("resnet_basic", (2, 2, 2), "fp32"): (11125504, (106496, 1277952, 15654912)),
    ("resnet_basic", (2, 2, 2), "bf16"): (5571328, (53248, 638976, 7827456)),
    ("resnet_basic", (3, 4, 6, 3), "fp32"): (85107968, (106496, 1277952, 15654912)),
    ("resnet_basic", (3, 4, 6, 3), "bf16"): (42575104, (53248, 638976, 7827456)),
}


@pytest.mark.parametrize("family,layers,dtype", sorted(NET_BYTES), ids=lambda v: str(v).replace(" ", ""))
def test_resnet_sizes_of_other_layer_tables_are_those_of_the_two_drivers(family, layers, dtype):
    lib = N.lib()
    w = net_weights(family, layers, DTYPES[dtype])
    packed, workspace = (getattr(lib, f"hipt_{family}_{what}_bytes") for what in ("packed", "workspace"))
    assert (packed(C.byref(w)), tuple(workspace(C.byref(w), *s) for s in NET_SHAPES)) == NET_BYTES[family, layers, dtype]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def _knn(lib, ws, nbytes):
    return lib.hipt_knn(FAKE, N.KNN_SPATIAL, 300, 2, FAKE, 5, 7, FAKE, FAKE, ws, nbytes, None)


def _update(lib, ws, nbytes):
    return lib.hipt_sampling_update(FAKE, 65, FAKE, 3, FAKE, 4, 4, FAKE, 5, 0.15, N.SAMPLING_AVERAGE, FAKE, ws, nbytes, None)


def _train_backward(lib, ws, nbytes):
    g = N.ClamTrainGrads()
    for name, _ in g._fields_:
        setattr(g, name, FAKE)
    w = train_weights(32, 16, 8, 2)
    return lib.hipt_clam_train_backward(C.byref(w), FAKE, 37, None, None, None, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, FAKE, None, None,
                                        0, C.byref(g), ws, nbytes, None)


def _overlay(lib, ws, nbytes):
    return lib.hipt_heatmap_overlay(FAKE, FAKE, None, 6, 3, 3, 70, 20, 0, FAKE, FAKE, None, ws, nbytes, None)


def _render(lib, ws, nbytes):
    return lib.hipt_heatmap_render(FAKE, FAKE, None, 6, 3, 3, 70, 20, 0, None, None, FAKE, 0.4, FAKE, None, ws, nbytes, None)


def _resnet(lib, ws, nbytes):
    w = resnet_weights(N.HIPT_BF16)
    return lib.hipt_resnet_forward(C.byref(w), FAKE, FAKE, N.RESNET_IN_F32, None, 1, 32, 32, FAKE, ws, nbytes, None)


def _need(lib, name):
    if name == "knn":
        return lib.hipt_knn_workspace_bytes(300, 5, 7)
    if name == "sampling_update":
        return lib.hipt_sampling_update_workspace_bytes(65)
    if name == "clam_train_backward":
        return lib.hipt_clam_train_workspace_bytes(C.byref(train_weights(32, 16, 8, 2)), 37)
    if name.startswith("heatmap"):
        return lib.hipt_heatmap_workspace_bytes(6, 3, 3, 70, 20)
    return lib.hipt_resnet_workspace_bytes(C.byref(resnet_weights(N.HIPT_BF16)), 1, 32, 32)


# entry point -> (the call, what a base address of 256 k + 16 returns: hipt_resnet_forward answers it from its argument check,
# as the earlier commit did -- read from a build of that commit, like the sizes)
REFUSALS = {"knn": (_knn, E_WORKSPACE), "sampling_update": (_update, E_WORKSPACE), "clam_train_backward": (_train_backward, E_WORKSPACE),
            "heatmap_overlay": (_overlay, E_WORKSPACE), "heatmap_render": (_render, E_WORKSPACE), "resnet_forward": (_resnet, E_BADARG)}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_forward_refuses_a_short_or_misaligned_workspace_before_any_launch(name):
    """Nothing is dereferenced, set or launched before the refusal: every pointer here is a fake address."""
    lib = N.lib()
    call, rc_misaligned = REFUSALS[name]
    need = _need(lib, name)
    assert need > 0
    assert call(lib, FAKE, need - 1) == E_WORKSPACE
    msg = lib.hipt_last_error().decode()
    assert msg.startswith(name + ": workspace") and str(need - 1) in msg and str(need) in msg and "too small / unaligned" in msg
    assert call(lib, FAKE + 16, need) == rc_misaligned
    assert call(lib, FAKE + 16, need + 4096) == rc_misaligned
    if not torch.cuda.is_available():
        # the accepted case: past the workspace check and into the first launch, which has no device to run on.  (With a device it
        # is tests/test_gpu_workspace_guard.py that runs it -- over real buffers.)
        assert call(lib, FAKE, need) != E_WORKSPACE


# ---- no second description left ------------------------------------------------------------------------------------------------
def test_csrc_holds_one_round_up_and_one_refusal():
    files = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    text = {os.path.basename(f): open(f).read() for f in files}
    assert "workspace.h" in text
    for f, s in text.items():
        assert not re.search(r"\bal256s\b|\balign256\b", s), f
    # augment.hip is the stated exception: its layout lives in its kernels, under an 8-byte alignment contract
    assert {f: s.count("too small") for f, s in text.items() if "too small" in s} == {"workspace.h": 1, "augment.hip": 1}
    assert sum(len(re.findall(r"size_t al256\(", s)) for s in text.values()) == 1
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^\$\(BUILD\)/%\.o:.*\bworkspace\.h\b", mk, re.M)
