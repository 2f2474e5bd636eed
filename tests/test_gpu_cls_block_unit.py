"""Per-unit bf16 parity of the [CLS]-pruned last ViT-256 block (capi.hip run_last_block_cls: the [CLS]-row gather, the Q rows GEMM, u = q Wu^T,
cls_pool_kernel, o = z Wo^T + bv, the proj rows GEMM, the fused MLP on nseq rows) through hipt_vit_cls_block_unit, against the fp64 emulation
tests/vit_bf16_ref.cls_block (bf16 exactly where each route rounds), on the three routes the forward has: the default one, HIPT_NO_CLS_ABSORB=1
(the fused kernel's [CLS]-only form) and HIPT_NO_FUSED_ATTN=1 (K | V GEMM + the one-query attention kernel).

Bars: R.CLS_BAR_FACTOR (4) x R.CLS_FLOOR, the emulation's own noise floor per (route, family, metric) -- the distance between its fp64-product
and fp32-product evaluations, measured on the CPU (tests/test_vit_bf16_ref.py).  The kernel's errors do not set them; they are printed
with -s beside floor and bar and tabulated in DESIGN.md 5 (MEASURED below).  Every case also asserts its route from the library's
launch counts, NaN canaries behind both outputs, bit-unchanged inputs, that its inputs reach their edges (R.cls_assert_edges) and that
every plausible wrong kernel (R.CLS_VARIANTS) lands >= 3 x beyond a bar."""
import ctypes as C

import pytest
import torch

import vit_bf16_ref as R
from hipt_abmil_atec23_amd import _native as N
from hipt_abmil_atec23_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 32
E_WORKSPACE, E_UNSUPPORTED = -2, -4
ROUTE_ENV = {"absorb": {}, "fused_cls": {"HIPT_NO_CLS_ABSORB": "1"}, "two_kernel": {"HIPT_NO_FUSED_ATTN": "1"}}
# launches booked as last_block_cls: gather + Q + u + pool + o + proj + MLP | gather + q|k|v rows + fused [CLS] kernel + proj + MLP |
# gather + K|V GEMM + Q GEMM + one-query attention + proj + MLP; the [CLS] residual gather is booked as "other"
LAUNCHES = {"absorb": 7, "fused_cls": 5, "two_kernel": 6}
# patches the busiest workgroup of cls_pool_kernel takes (hipt_cls_pool_launch's split, restated in pool_split): 528 is the first size
# with two (66 per XCD > 64 workgroups per XCD: the prefetch across a patch's last block is live), 1 104 has three and takes the row
# GEMMs off the small-M kernel (> 1 088 rows)
PER_WG = {16: 1, 48: 1, 528: 2, 1104: 3}
# variants that do not reach 3 x on (route, family) would be listed here, printed with their multiple and named in DESIGN.md 5: none
# (the narrowest is u_one_bf16 at 3.2 .. 3.8 x)
NOT_PINNED = set()
# Measured on the MI355X beside the bars (largest over the sizes; floor / measured / bar; the full table is in DESIGN.md 5):
#   att rows rel-L2    absorb std 9.6e-5 / 1.0e-4 / 3.8e-4, outlier 1.4e-4 / 1.6e-4 / 5.6e-4; fused_cls 5.4e-5 / 7.3e-5 / 2.2e-4, 8.3e-5 / 1.0e-4 / 3.3e-4;
#                      two_kernel 4.4e-5 / 4.5e-5 / 1.7e-4, 8.9e-5 / 9.3e-5 / 3.6e-4
#   increment rel-L2   absorb 4.2e-4 / 5.3e-4 / 1.7e-3, 4.7e-4 / 4.5e-4 / 1.9e-3; fused_cls 2.9e-4 / 5.3e-4 / 1.1e-3, 3.4e-4 / 3.6e-4 / 1.4e-3;
#                      two_kernel 3.3e-4 / 4.8e-4 / 1.3e-3, 4.0e-4 / 4.4e-4 / 1.6e-3
# The kernels sit at 0.6 .. 1.8 x the floor; these figures do not set the bars.


def bars(route, family):
    return {k: R.CLS_BAR_FACTOR * v for k, v in R.CLS_FLOOR[route, family].items()}


_models, _inputs = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _release_module_state():
    """The models and the images (2.5 GB, and some ten GB of float64 temporaries of the emulation in the allocator's cache) go back to
    the device when the module is done: the modules behind this one start from the memory state they had before it existed."""
    yield
    import gc
    _models.clear()
    _inputs.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def model(family="std", dtype="bf16"):
    if (family, dtype) not in _models:
        from hipt_abmil_atec23_amd.vision_transformer import vit_small
        specs = synth.vit_param_specs("vit256")
        m = vit_small(patch_size=16, num_classes=0)
        m.load_state_dict(synth.make_state_dict(specs, 256) if family == "std" else synth.make_vit_outlier_state_dict(specs, 256, 6))
        m = m.eval().to(DEV).set_compute_dtype(dtype)
        pk = m._tokens(synth.hash_uniform_torch((1, 3, 256, 256), 2, device=DEV))[0]
        _models[family, dtype] = (m, pk, R.block_params(m, 11))
    return _models[family, dtype]


def fenced(t):
    """t [M, 384] at the head of a buffer with CANARY more rows behind it (zeros: kernels that fetch ahead may read them)"""
    buf = torch.zeros(t.shape[0] + CANARY, 384, dtype=t.dtype, device=DEV)
    buf[:t.shape[0]] = t
    return buf[:t.shape[0]]


def case_inputs(family, nseq):
    """the inputs of a case and their images, built once per module (1 104 patches: 0.65 GB of images)"""
    if (family, nseq) not in _inputs:
        c = R.cls_inputs(model(family)[2], nseq, R.cls_seed(nseq), device=DEV, outlier_rows=family == "outlier")
        c["x_img"], c["xn_img"] = fenced(R.to_image_f32(c["x"])), fenced(R.to_image(c["xn"]))
        del c["x"]
        _inputs[family, nseq] = c
    return _inputs[family, nseq]


def pool_split(nseq):
    """hipt_cls_pool_launch's split (cls_pool.hip): patches per XCD, workgroups per XCD, patches of the busiest workgroup"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    px = (nseq + 7) // 8
    per_xcd = max(2 * ncu // 8, 1)
    nslots = min(px, per_xcd)
    return px, nslots, -(-px // nslots)


def run_unit(pk, xn_img, x_img, nseq, want_att=True, ws=None):
    """one hipt_vit_cls_block_unit call into NaN-fenced outputs -> (att rows bf16 or None, xc fp32, buffers)"""
    ab = torch.full((nseq + CANARY, 384), float("nan"), dtype=torch.bfloat16, device=DEV) if want_att else None
    xb = torch.full((nseq + CANARY, 384), float("nan"), dtype=torch.float32, device=DEV)
    if ws is None:
        ws = torch.zeros(N.lib().hipt_vit_workspace_bytes(pk.ref, nseq), dtype=torch.uint8, device=DEV)
    before = N.calls
    N.call("hipt_vit_cls_block_unit", pk.ref, N.ptr(xn_img), N.ptr(x_img), nseq, N.ptr(xb), N.ptr(ab), N.ptr(ws), ws.numel(), N.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert N.calls == before + 1
    return (ab[:nseq] if want_att else None), xb[:nseq], (ab, xb)


def canaries_intact(buf, n):
    tail = buf[n:]
    it = torch.int16 if buf.dtype == torch.bfloat16 else torch.int32
    return torch.equal(tail.view(it), torch.full_like(tail, float("nan")).view(it))


def _fmt(e, keys=R.CLS_METRICS):
    return " ".join(f"{k} {e[k]:.2e}" for k in keys)


CASES = [(r, f, n) for r in R.CLS_ROUTES for f in ("std", "outlier") for n in (16, 48, 528)] + [("absorb", f, 1104) for f in ("std", "outlier")]


@pytest.mark.parametrize("route,family,nseq", CASES)
def test_cls_block_unit_vs_bf16_emulation(monkeypatch, route, family, nseq):
    px, nslots, per_wg = pool_split(nseq)
    if per_wg != PER_WG[nseq]:
        pytest.skip(f"{nseq} patches put {per_wg} patches on the busiest workgroup of this device ({px} per XCD, {nslots} workgroups per XCD), not {PER_WG[nseq]}")
    assert (nseq > 1088) == (nseq == 1104)  # (the row GEMMs' small-M kernel ends at 1 088 rows)
    m, pk, p = model(family)
    c = case_inputs(family, nseq)
    xn0, x0 = c["xn_img"].clone(), c["x_img"].clone()
    for k, v in ROUTE_ENV[route].items():
        monkeypatch.setenv(k, v)
    N.profile_enable(True)
    try:
        att, xc, bufs = run_unit(pk, c["xn_img"], c["x_img"], nseq)
        pr = N.profile_read()
    finally:
        N.profile_enable(False)
    got = {k: n for k, (_, n) in pr.items()}
    tag = f"cls block {route} {family} nseq {nseq} ({per_wg} patches on the busiest workgroup)"
    print(f"\n{tag}: profile counts {got}")
    assert got == {"last_block_cls": LAUNCHES[route], "other": 1}, (tag, got)
    assert canaries_intact(bufs[0], nseq) and canaries_intact(bufs[1], nseq), tag
    assert torch.equal(c["xn_img"].view(torch.int16), xn0.view(torch.int16)) and torch.equal(c["x_img"].view(torch.int32), x0.view(torch.int32)), tag
    del xn0, x0
    smax = R.cls_assert_edges(c, p, nseq, family)
    att_ref, xc_ref = R.cls_block(c["xn"], c["x_cls"], p, nseq, route)
    e = R.cls_errors(att, att_ref, xc, xc_ref, c["x_cls"], c["classes"])
    bar, floor = bars(route, family), R.CLS_FLOOR[route, family]
    print(f"   measured {_fmt(e)}\n   floor    {_fmt(floor)}\n   bar      {_fmt(bar)}" + (f"\n   largest |score| {smax:.1f}" if smax else ""))
    print("   per class (att rel-L2, increment rel-L2): " + " | ".join(f"{k} {a:.2e} {b:.2e}" for k, (a, b) in e["per_class"].items()))
    assert bool(torch.isfinite(att.float()).all()) and bool(torch.isfinite(xc).all()), tag
    for k in R.CLS_METRICS:
        assert e[k] < bar[k], (tag, k, e[k], bar[k])
    for v in R.CLS_VARIANTS[route]:
        av, xv = R.cls_block(c["xn"], c["x_cls"], p, nseq, route, variant=v)
        ev = R.cls_errors(av, att_ref, xv, xc_ref, c["x_cls"], c["classes"])
        worst = max(ev[k] / bar[k] for k in R.CLS_METRICS)
        pinned = (route, family, v) not in NOT_PINNED
        print(f"   variant {v}: {worst:.1f} x a bar" + ("" if pinned else " (not pinned here)"))
        assert worst >= 3.0 or not pinned, (tag, v, worst)
    missing = sorted(set(R.CLS_VARIANTS["absorb"]) - set(R.CLS_VARIANTS[route]))
    if missing:
        print(f"   no counterpart on this route: {missing}")


def test_cls_block_unit_invariants():
    """Bits that must not move on the default route: 16 patches alone and in front of 48; a workspace of 0xFF and one reused for a second
    call; att_out = NULL."""
    m, pk, p = model("std")
    c = case_inputs("std", 48)
    att, xc, _ = run_unit(pk, c["xn_img"], c["x_img"], 48)
    r = 16 * 257
    att16, xc16, _ = run_unit(pk, fenced(c["xn_img"][:r]), fenced(c["x_img"][:r]), 16)
    assert torch.equal(att16.view(torch.int16), att[:16].view(torch.int16)) and torch.equal(xc16, xc[:16])
    ws = torch.full((N.lib().hipt_vit_workspace_bytes(pk.ref, 48),), 0xFF, dtype=torch.uint8, device=DEV)
    for _ in range(2):
        a2, x2, _ = run_unit(pk, c["xn_img"], c["x_img"], 48, ws=ws)
        assert torch.equal(a2.view(torch.int16), att.view(torch.int16)) and torch.equal(x2, xc)
    a3, x3, _ = run_unit(pk, c["xn_img"], c["x_img"], 48, want_att=False)
    assert a3 is None and torch.equal(x3, xc)
    print("\ncls block invariants: 16 alone / in front of 48, 0xFF and reused workspace, att_out NULL: bit-identical")


def test_cls_block_unit_refusals(monkeypatch):
    """HIPT_E_UNSUPPORTED: fp32 weights, nseq * 257 off the 16-row grid, a call a forward would not prune (one patch: the small-call path;
    HIPT_NO_PRUNE=1).  HIPT_E_WORKSPACE: short, NULL, off the 256-byte grid.  Nothing is launched: the buffers keep their bits."""
    lib = N.lib()
    st = N.stream_ptr(torch.device(DEV))
    nseq = 16
    pk = model("std")[1]
    xn = fenced(torch.zeros(nseq * 257, 384, dtype=torch.bfloat16, device=DEV))
    x = fenced(torch.zeros(nseq * 257, 384, device=DEV))
    xc = torch.full((nseq, 384), float("nan"), device=DEV)
    att = torch.full((nseq, 384), float("nan"), dtype=torch.bfloat16, device=DEV)
    need = lib.hipt_vit_workspace_bytes(pk.ref, nseq)
    ws = torch.zeros(need + 512, dtype=torch.uint8, device=DEV)
    call = lambda w=pk, n=nseq, wp=N.ptr(ws), nb=need: lib.hipt_vit_cls_block_unit(w.ref, N.ptr(xn), N.ptr(x), n, N.ptr(xc), N.ptr(att), wp, nb, st)
    assert call(model("std", "fp32")[1]) == E_UNSUPPORTED
    assert call(n=17) == E_UNSUPPORTED and call(n=1) == E_UNSUPPORTED
    monkeypatch.setenv("HIPT_NO_PRUNE", "1")
    assert call() == E_UNSUPPORTED
    monkeypatch.delenv("HIPT_NO_PRUNE")
    assert call(nb=need - 256) == E_WORKSPACE
    assert call(wp=None) == E_WORKSPACE
    assert call(wp=C.c_void_p(ws.data_ptr() + 16)) == E_WORKSPACE
    torch.cuda.synchronize()
    assert bool(torch.isnan(xc).all()) and bool(torch.isnan(att.float()).all()) and not bool(ws.any())
    assert call() == 0  # (the same arguments with a valid workspace run)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xc).all()) and bool(torch.isfinite(att.float()).all())
