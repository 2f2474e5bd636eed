"""GPU tests of what the device-op front-ends share (hipt_abmil_atec23_amd/_frontend.py), through every op that takes ``out=``:
the buffer handed in is the one that comes back, it holds the bytes of the call without it, and a buffer the kernel cannot
write -- strided, on the host, or the input itself -- is refused before any native call.  Two round trips pin the kind of the
result: numpy in, numpy out; device tensor in, device tensor out."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _u8(shape, seed):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)).to(DEV)


def _ops():
    """name -> (call(out=None), the input, the result's shape): small shapes, odd sizes"""
    import torch

    from hipt_abmil_atec23_amd import augment as AU
    from hipt_abmil_atec23_amd import macenko as MK
    from hipt_abmil_atec23_amd import patch_heatmap as PH
    from hipt_abmil_atec23_amd import resize as RZ
    from hipt_abmil_atec23_amd import segment as SG
    img, plane = _u8((5, 7, 3), 1), _u8((5, 7), 2)
    planar, inter = _u8((1, 3, 4, 6), 3), _u8((1, 4, 6, 3), 4)
    region, patch = _u8((1, 3, 8, 8), 5), _u8((1, 256, 256, 3), 6)
    colour = [AU.RegionParams(order=(AU.OP_BRIGHTNESS,), brightness=1.25)]
    a256 = torch.from_numpy(np.random.default_rng(7).random((1, 2, 1, 256), dtype=np.float32)).to(DEV)

    def heat(out=None):
        return PH.compose_patch_heatmaps(a256, patch, out=None if out is None else {"256": out})["256"]
    return {
        "tissue_mask": (lambda out=None: SG.tissue_mask(img, mthresh=3, close=2, out=out), img, (5, 7)),
        "median_blur_u8": (lambda out=None: SG.median_blur_u8(plane, 3, out=out), plane, (5, 7)),
        "morph_close_u8": (lambda out=None: SG.morph_close_u8(plane, 3, out=out), plane, (5, 7)),
        "macenko_normalize-planar": (lambda out=None: MK.macenko_normalize(planar, out=out), planar, (1, 3, 4, 6)),
        "macenko_normalize-interleaved": (lambda out=None: MK.macenko_normalize(inter, out=out), inter, (1, 4, 6, 3)),
        "resize_u8": (lambda out=None: RZ.resize_u8(img, (4, 3), out=out), img, (3, 4, 3)),
        "augment_regions": (lambda out=None: AU.augment_regions(region, colour, out=out), region, (1, 3, 8, 8)),
        "compose_patch_heatmaps": (heat, patch, (1, 1, 256, 256, 3)),
    }


OPS = ["tissue_mask", "median_blur_u8", "morph_close_u8", "macenko_normalize-planar", "macenko_normalize-interleaved", "resize_u8",
       "augment_regions", "compose_patch_heatmaps"]


@pytest.mark.parametrize("name", OPS)
def test_out_is_returned_filled_and_checked_before_any_native_call(name):
    import torch

    from hipt_abmil_atec23_amd import _native as N
    call, x, shape = _ops()[name]
    want = call()
    assert tuple(want.shape) == shape and want.dtype == torch.uint8 and want.device == x.device
    out = torch.full(shape, 0xA5, dtype=torch.uint8, device=DEV)
    got = call(out=out)
    assert got is out and torch.equal(out, want)
    assert torch.equal(call(), want)   # (and the input was left alone)
    strided = torch.empty(shape[:-1] + (2 * shape[-1],), dtype=torch.uint8, device=DEV)[..., ::2]
    on_host = torch.empty(shape, dtype=torch.uint8)
    alias = x.reshape(-1)[:want.numel()].view(shape)   # a well-formed buffer that begins where the input does
    assert tuple(strided.shape) == shape and not strided.is_contiguous() and alias.is_contiguous() and alias.data_ptr() == x.data_ptr()
    before = N.calls
    for bad in (strided, on_host, alias):   # (every op here refuses the input as its output: none of the kernels runs in place)
        with pytest.raises(ValueError, match="out.* must be a contiguous uint8"):
            call(out=bad)
    assert N.calls == before


def test_numpy_in_numpy_out_and_tensor_in_tensor_out():
    import torch

    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords = np.array([30.0, 80.0]), np.array([[0, 0], [4, 4]], dtype=np.int64)
    args = (4, 1.0, (8, 8))
    img = H.render_heatmap(scores, coords, *args)
    assert isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.shape == (8, 8, 3)
    img_t = H.render_heatmap(torch.from_numpy(scores).to(DEV), torch.from_numpy(coords).to(DEV), *args)
    assert torch.is_tensor(img_t) and img_t.device == torch.device(DEV) and img_t.dtype == torch.uint8
    assert np.array_equal(img_t.cpu().numpy(), img)
    assert (img[:4, :4] != 255).any() and (img[:4, 4:] == img[0, 7]).all()   # the first patch is painted, the corner beside it is canvas
