"""CPU tests (no GPU, no library call) of what the host-mirror modules share (hipt_abmil_atec23_amd/_host.py): the
compute-dtype setting and the weight-image cache, driven with a counting stand-in for the image builder."""
import copy
import pickle

import pytest
import torch
import torch.nn as nn

from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd._host import WeightImageCache
from test_host_and_abi import _replicate_like_data_parallel

CPU, META = torch.device("cpu"), torch.device("meta")


class Toy(WeightImageCache, nn.Module):
    def __init__(self, device=None):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(4, 3, device=device), nn.BatchNorm1d(3, device=device))
        self._init_host()
        self.builds = []

    def image(self, device, key_extra=()):
        def build(code):
            self.builds.append((device, code))
            return ("image", len(self.builds))
        return self._cached(device, key_extra, build)


class ToyWithStatistics(Toy):
    _image_buffers = True


def test_hit_and_the_three_ways_to_miss():
    m = Toy().set_compute_dtype("fp32")
    first = m.image(CPU)
    assert m.image(CPU) is first and len(m.builds) == 1                      # a second lookup is a hit
    with torch.no_grad():
        m.body[0].bias.add_(1)
    second = m.image(CPU)
    assert second is not first and len(m.builds) == 2 and m.image(CPU) is second   # an in-place update of one weight
    assert m.set_compute_dtype("bf16") is m and m.compute_dtype == "bf16"
    third = m.image(CPU)
    assert len(m.builds) == 3 and m.builds[-1] == (CPU, N.HIPT_BF16) and m.image(CPU) is third   # the other dtype
    assert m.image(CPU, key_extra=(7,)) is not third and len(m.builds) == 4   # whatever else the class keys on
    with pytest.raises(ValueError):
        m.set_compute_dtype("fp16")
    assert m.compute_dtype == "bf16"


def test_buffers_enter_the_key_only_where_the_class_says_so():
    plain, stats = Toy(), ToyWithStatistics()
    assert len(stats._tensors()) == len(plain._tensors()) + 2 == 6         # running_mean / running_var, not num_batches_tracked
    for m in (plain, stats):
        m.image(CPU)
        with torch.no_grad():
            m.body[1].running_mean.add_(1)
        m.image(CPU)
    assert len(plain.builds) == 1 and len(stats.builds) == 2


def test_two_devices_keep_separate_entries():
    a, b = Toy(), Toy(device=META)
    b._packed = a._packed  # what nn.DataParallel replicas do (shallow __dict__ copy): one dict, every replica on its own device
    ia, ib = a.image(CPU), b.image(META)
    assert set(a._packed) == {CPU, META} and a._packed[CPU][1] is ia and a._packed[META][1] is ib
    assert a.image(CPU) is ia and b.image(META) is ib and len(a.builds) == len(b.builds) == 1


def test_data_parallel_replica_has_the_key_of_its_source():
    m = Toy()
    r = _replicate_like_data_parallel(m)
    assert list(r.parameters()) == [] and len(r._tensors()) == len(list(m.parameters())) == 4
    assert len(r._version_key()) == 4 and all(ptr != 0 for ptr, _ in r._version_key())
    # the stand-in clones every parameter; on the source's own device the broadcast of nn.DataParallel hands the replica the source's
    # storage instead: give it that, and the replica has its source's key (and, through the shared dict, its image)
    for rm, sm in zip(r.modules(), m.modules()):
        for name, p in sm._parameters.items():
            if p is not None:
                setattr(rm, name, p.detach())
                rm._former_parameters[name] = getattr(rm, name)
    assert r._version_key() == m._version_key()
    assert r._packed is m._packed


def test_replica_key_follows_its_own_tensors():
    m = Toy()
    r = _replicate_like_data_parallel(m)
    key = r._version_key()
    assert key and key != m._version_key()      # its own copies: another image than the source's
    r.body[0].weight.add_(1)
    assert r._version_key() != key


def test_tensor_on_another_device_raises_and_stores_nothing():
    m = Toy()
    with pytest.raises(RuntimeError, match="expected all tensors on"):
        m.image(META)
    assert m._packed == {} and m.builds == []
    m.image(CPU)
    m.body[0].bias = nn.Parameter(torch.zeros(3, device=META))   # one stray tensor under an image that exists
    with pytest.raises(RuntimeError, match="expected all tensors on"):
        m.image(CPU)
    assert len(m.builds) == 1 and set(m._packed) == {CPU}


class _Unpicklable:
    def __reduce__(self):
        raise TypeError("ctypes objects containing pointers cannot be pickled")


def _families():
    from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, Attn_Net_Gated
    from hipt_abmil_atec23_amd.resnet_custom import Bottleneck_Baseline, ResNet_Baseline
    from hipt_abmil_atec23_amd.vision_transformer import VisionTransformer
    return [lambda: VisionTransformer(embed_dim=16, depth=1, num_heads=2), lambda: ResNet_Baseline(Bottleneck_Baseline, [1, 1, 1]),
            lambda: Attn_Net_Gated(L=8, D=4), lambda: CLAM_SB(size_arg=[8, 8, 4]), lambda: CLAM_MB(size_arg=[8, 8, 4], n_classes=3)]


@pytest.mark.parametrize("make", _families(), ids=["vit", "resnet", "attn_net_gated", "clam_sb", "clam_mb"])
def test_deepcopy_and_pickle_drop_the_caches(make):
    m = make().set_compute_dtype("bf16")
    assert isinstance(m, WeightImageCache) and all(getattr(m, name) == {} for name in m._caches)
    for name in m._caches:
        getattr(m, name)[CPU] = ("key", _Unpicklable())
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert all(getattr(twin, name) == {} for name in m._caches) and all(getattr(m, name) != {} for name in m._caches)
        assert twin.compute_dtype == "bf16"
        sd, sd2 = m.state_dict(), twin.state_dict()
        assert list(sd) == list(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
        for sub, sub2 in zip(m.modules(), twin.modules()):   # a CLAM module holds an Attn_Net_Gated with a cache of its own
            if isinstance(sub, WeightImageCache):
                assert all(getattr(sub2, name) == {} for name in sub._caches)
