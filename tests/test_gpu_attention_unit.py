"""Per-unit bf16 parity of the attention unit of a LayerNorm-chained ViT-256 block through hipt_vit_attention_unit, on both routes:
fused = 1 ([CLS]-row gather + side GEMM + qkv_attn_kernel<0>, csrc/qkv_attention.hip) and fused = 0 (the QKV GEMM with head-major output +
attn64_kernel reading head-major and writing an activation image, csrc/seqgemm_pipe.hip + csrc/attention2.hip -- the combination the
forward uses), against the fp64 emulation tests/vit_bf16_ref.attention_unit (bf16 exactly where each route rounds).

Bars: R.ATT_BAR_FACTOR (4) x R.ATT_FLOOR, the emulation's own noise floor per (route, family, metric) -- the distance between its
fp64-product and fp32-product evaluations, measured on the CPU (tests/test_vit_bf16_ref.py).  The kernels' errors set nothing; they are
printed with -s beside floor and bar and tabulated in DESIGN.md 5.  The metrics (R.att_errors) look at the non-[CLS] and the [CLS] rows, the
worst head, the worst query wave, the worst patch class and the worst schedule position separately, so that a mistake confined to one of
them is not diluted by the rest.

Sizes: the smallest nseq (multiples of 16) at which the busiest workgroup of the fused kernel takes 1, 2 and 3 work units
(R.qkv_attn_schedule with the device's CU count; 16, 48 and 96 on the MI355X): with three, every state the kernel carries from unit to unit
(the weight ring, the prefetched operand rows, the two parity-indexed LDS slots, the merge behind the loop) is live.  Inputs: R.att_inputs
(plain / spiked-key / equal / near-equal patches; R.att_assert_edges says what they reach).  Every case also asserts its route from the
library's launch counts, NaN canaries behind the output image, bit-unchanged inputs and weights, and that every plausible wrong kernel
(R.ATT_VARIANTS) lands >= 3 x beyond a bar on these very inputs.

Out of scope: the two-kernel route's row-major q | k | v fallback (hm false in hipt_vit_attention_unit) is taken only beyond 4 GiB of
q | k | v, which no small shape reaches."""
import pytest
import torch

import vit_bf16_ref as R
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 32
E_BADARG, E_WORKSPACE, E_UNSUPPORTED = -1, -2, -4
FUSED = {"fused": 1, "two_kernel": 0}
# launches by category: [CLS]-row gather + side GEMM, the fused kernel | the QKV GEMM, the attention kernel
LAUNCHES = {"fused": {"qkv_cls_rows": 2, "qkv_attention_fused": 1}, "two_kernel": {"qkv_gemm": 1, "attention": 1}}

_models, _inputs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    """The models, the images and the emulation's float64 temporaries in the allocator's cache go back to the device when the module is
    done: the modules behind this one start from the memory state they had before it existed."""
    yield
    import gc
    _models.clear()
    _inputs.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def model(family="std"):
    if family not in _models:
        from hipt_abmil_atec23_amd.vision_transformer import vit_small
        specs = synth.vit_param_specs("vit256")
        m = vit_small(patch_size=16, num_classes=0)
        m.load_state_dict(synth.make_state_dict(specs, 256) if family == "std" else synth.make_vit_outlier_state_dict(specs, 256, 6))
        m = m.eval().to(DEV).set_compute_dtype("bf16")
        pk = m._tokens(synth.hash_uniform_torch((1, 3, 256, 256), 2, device=DEV))[0]
        _models[family] = (m, pk, {})
    return _models[family]


def params(family, blk):
    m, _, ps = model(family)
    if blk not in ps:
        ps[blk] = R.block_params(m, blk)
    return ps[blk]


def fenced(t):
    """t [M, 384] at the head of a buffer with CANARY more rows behind it (zeros: kernels that fetch ahead may read them)"""
    buf = torch.zeros(t.shape[0] + CANARY, 384, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def case_inputs(family, blk, nseq):
    """the inputs of a case, their image and the emulation of either route, built once per module"""
    if (family, blk, nseq) not in _inputs:
        for k in [k for k in _inputs if k[:2] != (family, blk)]:
            del _inputs[k]  # (the cases come grouped by weights: the images and emulations of the group before are spent)
        c = R.att_inputs(params(family, blk), nseq, R.att_seed(nseq), device=DEV, outlier_rows=family == "outlier")
        c["xn_img"] = fenced(R.to_image(c["xn"]))
        c["emu"] = {}
        _inputs[family, blk, nseq] = c
    return _inputs[family, blk, nseq]


def emulation(family, blk, nseq, route):
    c = case_inputs(family, blk, nseq)
    if route not in c["emu"]:
        c["emu"][route] = R.attention_unit(c["xn"], params(family, blk), nseq, route=route, ncu=ncu())
    return c["emu"][route]


def nan_image(nseq):
    return torch.full((nseq * 257 + CANARY, 384), float("nan"), dtype=torch.bfloat16, device=DEV)


def is_nan_fill(t):
    return torch.equal(t.view(torch.int16), torch.full_like(t, float("nan")).view(torch.int16))


def run_unit(pk, blk, xn_img, nseq, fused):
    """one hipt_vit_attention_unit call into a NaN-fenced image -> (rows [M, 384] bf16 row-major, the buffer)"""
    out = nan_image(nseq)
    ws = torch.zeros(N.lib().hipt_vit_workspace_bytes(pk.ref, nseq), dtype=torch.uint8, device=DEV)
    before = N.calls
    N.call("hipt_vit_attention_unit", pk.ref, blk, N.ptr(xn_img), nseq, N.ptr(out), fused, N.ptr(ws), ws.numel(), N.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert N.calls == before + 1
    return R.from_image(out[:nseq * 257]), out


def weight_buffers(pk, blk):
    """the device buffers of block blk that the library is handed and the two routes read: the bf16 qkv matrix, the fp32 bias and the
    packed images of the QKV GEMM and of the fused kernel (the tensors the packed-weights object keeps alive, found by address)"""
    b = pk.blocks[blk]
    by_ptr = {t.data_ptr(): t for t in pk.keep}
    bufs = [by_ptr[int(getattr(b, f))] for f in ("qkv_w", "qkv_b", "qkv_pk", "qkv_att_pk")]
    assert bufs[0].dtype == torch.bfloat16 and bufs[1].dtype == torch.float32 and bufs[2].dtype == bufs[3].dtype == torch.uint8
    return bufs


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def _fmt(e, keys=R.ATT_METRICS):
    return " ".join(f"{k} {e[k]:.2e}" for k in keys)


CASES = [(r, f, b, u) for r in R.ATT_ROUTES for f, b in (("std", 3), ("outlier", 3), ("outlier", 0)) for u in (1, 2, 3)]


@pytest.mark.parametrize("route,family,blk,units", CASES)
def test_attention_unit_vs_bf16_emulation(route, family, blk, units):
    sizes = R.att_schedule_sizes(ncu())
    nseq = sizes[units - 1]
    sched = R.qkv_attn_schedule(nseq, ncu())
    assert sched["max_units"] == units and (nseq == 16 or R.qkv_attn_schedule(nseq - 16, ncu())["max_units"] < units)
    if ncu() == 256:
        assert sizes == (16, 48, 96)
    assert bool(sched["carried"].any()) == (units == 3)
    m, pk, _ = model(family)
    p = params(family, blk)
    c = case_inputs(family, blk, nseq)
    xn0, w0 = c["xn_img"].clone(), [t.clone() for t in weight_buffers(pk, blk)]
    N.profile_enable(True)
    try:
        att, buf = run_unit(pk, blk, c["xn_img"], nseq, FUSED[route])
        pr = N.profile_read()
    finally:
        N.profile_enable(False)
    got = {k: n for k, (_, n) in pr.items()}
    tag = f"attention unit {route} {family} block {blk} nseq {nseq} ({units} units on the busiest workgroup)"
    print(f"\n{tag}: profile counts {got}")
    assert got == LAUNCHES[route], (tag, got)
    assert is_nan_fill(buf[nseq * 257:]), tag
    assert same_bits(c["xn_img"], xn0) and all(same_bits(a, b) for a, b in zip(weight_buffers(pk, blk), w0)), tag
    del xn0
    if blk == 3:  # (the edges are built for block 3; block 0 of the outlier family is there for its logits)
        print("   edges: " + " ".join(f"{k} {v:.3g}" for k, v in R.att_assert_edges(c, p, nseq, family).items()))
    else:
        smax = max(float(R.att_scores(c["xn"], p, nseq, i).abs().max()) for i in c["classes"].values())
        print(f"   largest |score| {smax:.0f}")
        assert smax > 89.0
    assert bool(torch.isfinite(att.float()).all()), tag
    ref = emulation(family, blk, nseq, route)
    e = R.att_errors(att, ref, nseq, c["classes"], sched)
    floor = R.ATT_FLOOR[route, R.att_floor_key(family, blk)[0]]
    bar = {k: R.ATT_BAR_FACTOR * v for k, v in floor.items()}
    print(f"   measured {_fmt(e)}\n   floor    {_fmt(floor)}\n   bar      {_fmt(bar)}")
    print("   x floor  " + " ".join(f"{k} {e[k] / floor[k]:.2f}" for k in R.ATT_METRICS))
    print("   per class (rows, [CLS]): " + " | ".join(f"{k} {a:.1e} {b:.1e}" for k, (a, b) in e["per_class"].items()))
    print("   per position (rows, [CLS]): " + " | ".join(f"{k} {a:.1e} {b:.1e}" for k, (a, b) in e["per_pos"].items()))
    for k in R.ATT_METRICS:
        assert e[k] < bar[k], (tag, k, e[k], bar[k])
    for v in R.ATT_VARIANTS[route]:
        if R.ATT_VARIANT_UNITS.get(v, 1) > units:
            continue  # (no workgroup has a unit the mistake would touch: the variant is the emulation itself)
        ev = R.att_errors(R.attention_unit(c["xn"], p, nseq, route=route, variant=v, ncu=ncu()), ref, nseq, c["classes"], sched)
        k = max(R.ATT_METRICS, key=lambda k: ev[k] / bar[k])
        pinned = (route, family, v) not in R.ATT_NOT_PINNED
        print(f"   variant {v}: {ev[k] / bar[k]:.3g} x the bar of {k}" + ("" if pinned else " (not pinned here)"))
        assert ev[k] / bar[k] >= 3.0 or not pinned, (tag, v, k, ev[k] / bar[k])


@pytest.mark.parametrize("route", R.ATT_ROUTES)
def test_attention_unit_patch_bits_do_not_depend_on_the_call(route):
    """The output of a patch depends neither on nseq nor on the unit's position in its workgroup's walk: the 16 patches of the smallest case
    (every workgroup has one unit) again as the last 16 patches of the largest one (carried and last units among them), bit for bit."""
    n1, _, n3 = R.att_schedule_sizes(ncu())
    m, pk, _ = model("std")
    small, big = case_inputs("std", 3, n1), case_inputs("std", 3, n3)
    s1, s3 = R.qkv_attn_schedule(n1, ncu()), R.qkv_attn_schedule(n3, ncu())
    assert bool((s1["first"] & s1["last"]).all()) and bool(s3["carried"][n3 - n1:].any()) and bool((s3["last"] & ~s3["first"])[n3 - n1:].any())
    rows = torch.cat([big["xn"][:(n3 - n1) * 257], small["xn"]])
    alone, _ = run_unit(pk, 3, small["xn_img"], n1, FUSED[route])
    inside, buf = run_unit(pk, 3, fenced(R.to_image(rows)), n3, FUSED[route])
    assert is_nan_fill(buf[n3 * 257:])
    assert torch.equal(inside[(n3 - n1) * 257:].view(torch.int16), alone.view(torch.int16)), route
    # (and the patches in front of them are those of the large case)
    full, _ = run_unit(pk, 3, big["xn_img"], n3, FUSED[route])
    assert torch.equal(inside[:(n3 - n1) * 257].view(torch.int16), full[:(n3 - n1) * 257].view(torch.int16)), route


def test_attention_unit_refusals():
    """HIPT_E_UNSUPPORTED: nseq * 257 off the 16-row grid; HIPT_E_WORKSPACE: a workspace one byte short of hipt_vit_workspace_bytes;
    HIPT_E_BADARG: out_img == xn_img.  Nothing is launched: the NaN-filled output, the input and the workspace keep their bits."""
    lib = N.lib()
    st = N.stream_ptr(torch.device(DEV))
    nseq = 16
    pk = model("std")[1]
    c = case_inputs("std", 3, nseq)
    xn0 = c["xn_img"].clone()
    out = nan_image(nseq)
    need = lib.hipt_vit_workspace_bytes(pk.ref, nseq)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    err = lambda: lib.hipt_last_error().decode()
    for fused in (1, 0):
        call = lambda n=nseq, o=out, nb=need: lib.hipt_vit_attention_unit(pk.ref, 3, N.ptr(c["xn_img"]), n, N.ptr(o), fused, N.ptr(ws), nb, st)
        assert call(n=8) == E_UNSUPPORTED and "nseq * 257 % 16 == 0" in err(), err()
        assert call(nb=need - 1) == E_WORKSPACE and "vit_attention_unit: workspace" in err() and "too small" in err(), err()
        assert call(o=c["xn_img"]) == E_BADARG and "vit_attention_unit: bad argument" in err(), err()
        torch.cuda.synchronize()
        assert is_nan_fill(out) and torch.equal(c["xn_img"].view(torch.int16), xn0.view(torch.int16)) and not bool(ws.any()), fused
    assert call() == 0  # (the same arguments with a whole workspace and an output of its own run)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out[:nseq * 257].float()).all()) and is_nan_fill(out[nseq * 257:])
