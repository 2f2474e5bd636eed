"""GPU tests (-m gpu) of the carved workspaces (csrc/workspace.h): a carve that hands out more than it counted writes past the
buffer the caller was told to bring.  Every converted entry point runs through its Python wrapper over a workspace of EXACTLY
the size the library asks for, with a 4 KiB fence of 0xA5 on either side; the fences must survive and the outputs must equal,
bit for bit, those of the same call over a roomy buffer allocated on its own."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resnet_ref as R  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import functional as Fn  # noqa: E402
from hipt_abmil_atec23_amd import heatmap as H  # noqa: E402
from hipt_abmil_atec23_amd import resnet_custom as rc  # noqa: E402
from hipt_abmil_atec23_amd import sampling, synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FENCE, FILL, ROOMY = 4096, 0xA5, 65536


class _Scratch:
    """Stands in for the wrappers' workspace allocation: fenced and exact, or roomy and separate."""

    def __init__(self, fenced):
        self.fenced, self.handed = fenced, []

    def __call__(self, device, nbytes, slot=0, zero=False):
        nbytes = int(nbytes)
        if not self.fenced:
            return (torch.zeros if zero else torch.empty)(nbytes + ROOMY, dtype=torch.uint8, device=device)
        buf = torch.full((nbytes + 2 * FENCE,), FILL, dtype=torch.uint8, device=device)
        assert buf.data_ptr() % 256 == 0
        ws = buf[FENCE:FENCE + nbytes]
        if zero:
            ws.zero_()
        self.handed.append((buf, nbytes))
        return ws

    def fences_hold(self):
        return all(bool((buf[:FENCE] == FILL).all()) and bool((buf[FENCE + n:] == FILL).all()) for buf, n in self.handed)


def guarded(monkeypatch, need, run):
    """`run()` -> tensors, once over the fenced workspace of `need` bytes and once over the roomy one."""
    assert need > 0 and need % 256 == 0
    outs = []
    for fenced in (True, False):
        s = _Scratch(fenced)
        monkeypatch.setattr(Fn, "workspace", s)
        monkeypatch.setattr(H, "_workspace", lambda n, pw, ph, w, h, dev, s=s: s(dev, N.lib().hipt_heatmap_workspace_bytes(n, pw, ph, w, h)))
        outs.append([t.detach().clone() for t in run()])
        torch.cuda.synchronize()
        if fenced:
            assert [n for _, n in s.handed] == [need], "the wrapper did not bring exactly what the library asks for"
            assert s.fences_hold(), "a write outside the workspace"
    assert len(outs[0]) == len(outs[1]) > 0
    for a, b in zip(*outs):
        assert a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("kind,n,s,k", [("spatial", 300, 5, 7), ("textural", 300, 5, 7), ("spatial", 1000, 33, 64), ("textural", 1000, 33, 64)])
def test_knn(monkeypatch, kind, n, s, k):
    if kind == "spatial":
        X = (synth.hash_uniform_torch((n, 2), 41, device=DEV) * 5000).to(torch.int32)
    else:
        X = synth.hash_uniform_torch((n, 8), 42, device=DEV)
    q = torch.arange(s, dtype=torch.int64) * (n // s)
    guarded(monkeypatch, N.lib().hipt_knn_workspace_bytes(n, s, k), lambda: sampling.knn(X, q, k, kind))


@pytest.mark.parametrize("mode", ["max", "newest", "average"])
def test_sampling_update(monkeypatch, mode):
    n, s, neighbors = 65, 3, 4
    scores = synth.hash_uniform_torch((s,), 43, device=DEV).abs() + 0.01
    ids = torch.tensor([[0, 1, 2, 64], [2, 3, 63, 64], [64, 10, 2, 30]], dtype=torch.int64, device=DEV)   # shared targets: the fold of AVERAGE
    sampled = [5, 17, 33, 63, 64]

    def run():
        w = torch.full((n,), 0.25, dtype=torch.float64, device=DEV)
        return sampling.update_sampling_weights(w, scores, sampled, ids, neighbors, sampling_update=mode, return_sum=True)

    guarded(monkeypatch, N.lib().hipt_sampling_update_workspace_bytes(n), run)


@pytest.mark.parametrize("dbag", [False, True])
def test_clam_train_backward(monkeypatch, dbag):
    """(N; S0, S1, S2; n_att) = (37; 32, 16, 8; 2): duv takes 4 * 37 * 16 = 2 368 bytes, no multiple of 256, so dz and the per-tile
    partials do not start where plain pointer arithmetic would put them."""
    import ctypes as C
    from hipt_abmil_atec23_amd import CLAM_MB
    size, n = (32, 16, 8), 37
    m = CLAM_MB(size_arg=list(size), dropout=0.0, k_sample=4, n_classes=2, subtyping=True)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=2, multi=True, dropout=False), 32))
    m.relocate()
    m.train()
    h0 = synth.hash_uniform_torch((n, size[0]), 44, device=DEV)
    lab = torch.tensor([1], device=DEV)
    w = N.ClamTrainWeights(s0=32, s1=16, s2=8, n_att=2, n_classes=2, multi_branch=1)

    def run():
        m.zero_grad(set_to_none=True)
        h = h0.clone().requires_grad_(dbag)
        logits, _, _, a_raw, res = m(h, label=lab, instance_eval=True)
        (0.7 * F.cross_entropy(logits, lab) + 0.3 * res["instance_loss"]).backward()
        grads = [p.grad for p in m.parameters() if p.grad is not None]
        assert len(grads) >= 8 and (h.grad is not None) == dbag
        return [logits, a_raw, *grads] + ([h.grad] if dbag else [])

    guarded(monkeypatch, N.lib().hipt_clam_train_workspace_bytes(C.byref(w), n), run)


def test_heatmap_overlay(monkeypatch):
    scores = torch.tensor([40.0, 80.0, 20.0, 55.0, 90.0, 10.0], dtype=torch.float64, device=DEV)
    coords = torch.tensor([[0, 0], [1, 1], [30, 5], [31, 6], [67, 17], [69, 19]], dtype=torch.int64, device=DEV)   # overlaps; two clipped
    guarded(monkeypatch, N.lib().hipt_heatmap_workspace_bytes(6, 3, 3, 70, 20), lambda: H.heatmap_overlay(scores, coords, (3, 3), 1.0, (70, 20)))


@pytest.fixture(scope="module")
def resnet():
    m = rc.resnet50_baseline()
    m.load_state_dict(R.state_dict(), strict=False)
    return m.eval().to(DEV)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_resnet_forward(monkeypatch, resnet, dtype):
    x = torch.from_numpy(synth.hash_u8_np((1, 3, 32, 32), 45)).to(DEV)
    resnet.set_compute_dtype(dtype)
    try:
        with torch.no_grad():
            resnet(x)   # (packs the weight image, outside the guarded runs)
            need = N.lib().hipt_resnet_workspace_bytes(resnet._packed_for(x.device).ref, 1, 32, 32)
            guarded(monkeypatch, need, lambda: [resnet(x)])
    finally:
        resnet.set_compute_dtype("fp32")
