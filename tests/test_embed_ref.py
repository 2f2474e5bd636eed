"""Host checks (no GPU) of tests/embed_ref.py, the reference of the patch-embedding unit tests: the patchify agrees with
F.unfold / F.conv2d; the fp32 emulation of embed32.hip and of the [CLS]-row kernel stays inside both derived bounds on every case of the
table (the smallest size of each, at most 16 patches); every wrong kernel lands >= 3 x beyond a bound on the case named to catch it;
the edge family reaches its edges; ops_ref.layernorm_bound's chain parameter leaves the default untouched."""
import numpy as np
import pytest
import torch

import embed_ref as E
import ops_ref as P

_prm, _runs = {}, {}


def params(family):
    if family not in _prm:
        _prm[family] = E.make_params(family)[1]
    return _prm[family]


def run(name, kind):
    """(buffer, layout, seq0, nseq, operands, exact x, bound of x, emulated x) of a case, built once"""
    if (name, kind) not in _runs:
        case = E.CASES[name]
        buf, off, lay, seq0, nseq = E.build(case, kind, nseq=16)
        prm = params(case.family)
        a = E.gather(buf[off:], lay, seq0, nseq, kind)
        _runs[name, kind] = dict(buf=buf[off:], lay=lay, seq0=seq0, nseq=nseq, a=a, prm=prm, x=E.tokens_ref(a, prm), xb=E.tokens_bound(a, prm),
                                 xe=E.emulate_tokens(a, prm))
    return _runs[name, kind]


def test_patchify_agrees_with_unfold_and_conv2d():
    """a plain batch [3, 3, 256, 256] and a region [1, 3, 512, 768] cut 2 x 3 the reference's way (hipt_4k.py:64-65), every input kind"""
    prm = params("std")
    w4 = torch.from_numpy(prm["wb"]).reshape(E.D, 3, 16, 16)
    for shape, lay in (((3, 3, 256, 256), E.plain_layout(256, 256)), ((1, 3, 512, 768), E.region_layout(512, 768))):
        u8 = E.synth.hash_u8_np(shape, 17)
        f = torch.from_numpy(E.normalize_u8(u8))
        patches = f.unfold(2, 256, 256).unfold(3, 256, 256)                      # b c p1 p2 w h
        patches = patches.permute(0, 2, 3, 1, 4, 5).reshape(-1, 3, 256, 256)     # (b p1 p2) c w h
        nseq = patches.shape[0]
        cols = torch.nn.functional.unfold(patches, 16, stride=16).transpose(1, 2).numpy()   # [nseq, 256, 768], k = (c, y, x)
        ref = torch.nn.functional.conv2d(torch.from_numpy(P.bf16_round(patches.numpy())).double(), w4, stride=16).flatten(2).transpose(1, 2).numpy()
        for kind in (E.F32, E.U8_CHW, E.U8_HWC):
            buf, off = E.store(f.numpy() if kind == E.F32 else u8, kind, lay)
            raw = buf[E.patch_index(lay, 0, nseq, kind)]
            assert np.array_equal(raw if kind == E.F32 else E.normalize_u8(raw), cols), (shape, kind)
            a = E.gather(buf, lay, 0, nseq, kind)
            assert np.abs(a @ prm["wb"].T - ref).max() < 1e-12, (shape, kind)
            # a range inside the tensor: sequences 1 .. nseq - 1
            assert np.array_equal(E.gather(buf, lay, 1, nseq - 1, kind), a[1:])


def test_window_storage_round_trips():
    """the strided window (row_stride > width, chan_stride > plane, a lead) holds the pixels where the header's formula looks for them,
    NaN everywhere else"""
    case = E.CASES["window"]
    u8 = E.case_pixels(case)
    for kind in case.kinds:
        buf, off, lay, seq0, nseq = E.build(case, kind)
        assert off > 0 and lay.row_stride > 512 and lay.chan_stride > 512 * lay.row_stride and lay.batch_stride == 3 * lay.chan_stride
        assert lay.row_stride % 8 == 0 and lay.chan_stride % 8 == 0
        raw = buf[off:][E.patch_index(lay, 0, 8, kind)]
        ref = E.store(E.to_float(case, u8) if kind == E.F32 else u8, kind, E.region_layout(512, 512))[0][E.patch_index(E.region_layout(512, 512), 0, 8, kind)]
        assert np.array_equal(raw, ref)
        if kind == E.F32:
            assert np.isnan(buf).sum() == buf.size - u8.size


CASE_KINDS = [(c.name, k) for c in E.CASES.values() for k in c.kinds]


@pytest.mark.parametrize("name,kind", CASE_KINDS)
def test_emulation_inside_both_bounds(name, kind):
    r = run(name, kind)
    rx = P.ratio(r["xe"], r["x"], r["xb"])
    xn = E.emulate_xn(r["xe"], r["prm"])
    rn = P.ratio(xn, E.xn_ref(r["xe"], r["prm"]), E.xn_bound(r["xe"], r["prm"]))
    print(f"\n{name} kind {kind}: emulation / bound: x tokens {rx[:, 1:].max():.3f}, [CLS] {rx[:, 0].max():.3f}; xn tokens {rn[:, 1:].max():.3f}, [CLS] {rn[:, 0].max():.3f}")
    assert rx.max() < 1.0 and rn.max() < 1.0


@pytest.mark.parametrize("variant", E.VARIANTS_X + E.VARIANTS_XN)
def test_wrong_kernels_land_beyond_a_bound(variant):
    """each wrong kernel, as a float64 reference rounded like the output, against the exact one on the case named to catch it: >= 3 x the
    bound somewhere -- substituted for the reference in the GPU test, it would fail a kernel that is right"""
    name = E.CATCHES[variant]
    case = E.CASES[name]
    kind = case.kinds[0] if name != "plain16" else E.F32
    if variant == "no_eps":
        kind = E.F32   # (the near-constant rows need pixels that are exactly 0)
    r = run(name, kind)
    if variant in E.VARIANTS_X:
        v = E.variant_tokens(variant, r["buf"], r["lay"], r["seq0"], r["nseq"], kind, r["prm"])
        worst = P.ratio(P.rounded(v, False), r["x"], r["xb"])[:, 1:].max()
    else:
        x = r["xe"]
        rows = 1 + E.edge_tokens()["near_const"] if variant == "no_eps" else slice(1, None)
        v = E.xn_ref(x, r["prm"], variant)
        worst = P.ratio(P.rounded(v, True), E.xn_ref(x, r["prm"]), E.xn_bound(x, r["prm"]))[:, rows].max()
    print(f"\nvariant {variant} on {name} (kind {kind}): {worst:.1f} x the bound")
    assert worst >= 3.0


def test_edge_family_reaches_its_edges():
    r = run("edge", E.F32)
    reached = E.edge_reach(r["x"], r["prm"])
    print("\nedge family: " + ", ".join(f"{k} {v:.3g}" for k, v in reached.items()))


def test_background_patches_cancel():
    """all-white / all-black patches: every product of a token has the same sign pattern as the weights, |sum| << sum | |"""
    r = run("edge", E.U8_CHW)
    a, prm = r["a"], r["prm"]
    assert np.all(a[E.WHITE] == 1.0) and np.all(a[E.BLACK] == -1.0)
    y = np.abs(a[E.WHITE].reshape(-1, E.K) @ prm["wb"].T)
    S = np.abs(a[E.WHITE].reshape(-1, E.K)) @ np.abs(prm["wb"]).T
    print(f"\nwhite patch: median |sum| / sum|.| = {np.median(y / S):.3f}")
    assert np.median(y / S) < 0.1


def test_layernorm_bound_default_chain_is_unchanged():
    x, w, b, _ = P.ln_inputs(9, 384, 3)
    for out_bf16 in (False, True):
        assert np.array_equal(P.layernorm_bound(x, w, b, 1e-6, out_bf16), P.layernorm_bound(x, w, b, 1e-6, out_bf16, chain=384 / 64 + 7))
        assert np.all(P.layernorm_bound(x, w, b, 1e-6, out_bf16, chain=E.LN_CHAIN_TOKENS) > P.layernorm_bound(x, w, b, 1e-6, out_bf16))
    assert E.LN_CHAIN_CLS == 384 // 64 + 7 and E.LN_CHAIN_TOKENS == 194


def test_case_table_covers_the_issue():
    c = E.CASES
    assert set(c["plain16"].kinds) == {0, 1, 2} and set(c["plain16"].outs) == {"img", "rows"}
    assert len(np.unique(E.case_pixels(c["plain16"]))) == 256          # every byte value
    assert c["rows5"].nseq * E.NTOK % 16 != 0 and c["cross_2x3"].nseq * E.NTOK % 16 != 0
    assert (c["second_half"].seq0, c["second_half"].nseq) == (16, 16) and (c["cross_2x3"].seq0, c["cross_2x3"].nseq) == (3, 7)
    tok = E.edge_tokens()
    for k in E.EDGE_CLASSES:   # the first and the last token row of both tiles of a patch
        assert {int(v) // 16 for v in tok[k]} == {0, 7, 8, 15}
    assert {(ch >> 2) & 1 for ch in E.OUTLIER_CH} == {0, 1}
