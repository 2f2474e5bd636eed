"""GPU tests of the heat-map score ranks (csrc/percentile.hip through hipt_abmil_atec23_amd.heatmap).  Counts are
compared with array_equal and every float64 percentile as its int64 view against the numpy restatement tests/heatmap_scores_ref.py,
which tests/test_heatmap_scores_host.py holds against scipy.  Inputs are seeded.

test_percentile_heatmap_is_capturable_and_free_of_host_copies fails before this kernel existed: the ranks were numpy's, and the
``.cpu()`` in front of them cannot be captured into a graph."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import heatmap_ref as R  # noqa: E402
import heatmap_scores_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

T, QW = 512, 128   # the kernel's reference tile and its queries per workgroup


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def host(t):
    return t.detach().cpu().numpy()


def native_counts(q, ref, mode):
    """(less, leq, pct) as numpy from one call of the entry point with all three outputs."""
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    dev = torch.device("cuda")
    qt, rt = torch.from_numpy(np.ascontiguousarray(q)).to(dev), torch.from_numpy(np.ascontiguousarray(ref)).to(dev)
    less, leq, pct = H._counts_call(qt, rt, mode, counts=True, pct=True)
    return host(less), host(leq), host(pct)


def test_the_constants_are_the_launchers():
    from hipt_abmil_atec23_amd import _native as N
    assert (T, QW) == (N.PCT_REF_TILE, N.PCT_QUERIES_PER_WG)


@pytest.mark.parametrize("ties", [False, True], ids=["random", "ties"])
@pytest.mark.parametrize("mode", [S.RANKDATA, S.OF_SCORE], ids=["rankdata", "of_score"])
def test_counts_and_percentiles_are_bit_equal(mode, ties):
    from hipt_abmil_atec23_amd import _native as N
    before, cases = N.calls, 0
    for nref in (1, 2, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        for nq in (1, QW - 1, QW, QW + 1, 2 * QW + 3):
            q, ref = S.case(nq, nref, 1000 * nref + nq, ties)
            if ties and nref >= 4:
                assert np.signbit(ref[ref == 0]).any() and not np.signbit(ref[ref == 0]).all() and np.isinf(ref).sum() >= 2
            want_less, want_leq = S.counts(q, ref)
            want = S.pct_from_counts(want_less, want_leq, nref, mode)
            less, leq, pct = native_counts(q, ref, mode)
            assert less.dtype == np.int32 and leq.dtype == np.int32 and pct.dtype == np.float64
            assert np.array_equal(less, want_less) and np.array_equal(leq, want_leq), (nq, nref)
            assert np.array_equal(bits(pct), bits(want)), (nq, nref, int((bits(pct) != bits(want)).sum()))
            cases += 1
    assert N.calls == before + cases


def test_outputs_may_each_be_absent_and_the_public_functions_agree():
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    q, ref = S.case(300, 777, 4, True)
    want_less, want_leq = S.counts(q, ref)
    dev = torch.device("cuda")
    qt, rt = torch.from_numpy(q).to(dev), torch.from_numpy(ref).to(dev)
    less, leq, pct = H._counts_call(qt, rt, S.OF_SCORE, counts=True)
    assert pct is None and np.array_equal(host(less), want_less) and np.array_equal(host(leq), want_leq)
    less, leq, pct = H._counts_call(qt, rt, S.OF_SCORE, pct=True)
    assert less is None and leq is None and np.array_equal(bits(host(pct)), bits(S.percentiles(q, ref, S.OF_SCORE)))
    a, b = H.score_counts(qt, rt)
    assert a.is_cuda and a.dtype == torch.int32 and np.array_equal(host(a), want_less) and np.array_equal(host(b), want_leq)
    a, b = H.score_counts(q, ref)
    assert isinstance(a, np.ndarray) and np.array_equal(a, want_less) and np.array_equal(b, want_leq)
    a, b = H.score_counts(q.astype(np.float32), rt)   # mixed kinds: the result follows the scores
    w32 = S.counts(q.astype(np.float32), ref)
    assert isinstance(a, np.ndarray) and np.array_equal(a, w32[0]) and np.array_equal(b, w32[1])


@pytest.mark.parametrize("mode", [S.RANKDATA, S.OF_SCORE], ids=["rankdata", "of_score"])
def test_a_query_does_not_depend_on_its_company(mode):
    rng = np.random.default_rng(8)
    ref = np.round(rng.standard_normal(2 * T + 77), 1)
    q = np.round(rng.standard_normal(5000), 1)
    wl, we = S.counts(q, ref)
    mid = 2000 + int(np.flatnonzero((wl[2000:3000] > 0) & (wl[2000:3000] < we[2000:3000]))[0])   # in the middle, with ties in the reference
    alone = native_counts(q[mid:mid + 1], ref, mode)
    whole = native_counts(q, ref, mode)
    perm = rng.permutation(len(q))
    mixed = native_counts(q[perm], ref, mode)
    back = np.argsort(perm)
    for a, w, m in zip(alone, whole, mixed):
        assert a.tobytes() == w[mid:mid + 1].tobytes()
        assert w.tobytes() == np.ascontiguousarray(m[back]).tobytes()
    assert np.array_equal(whole[0], wl) and np.array_equal(whole[1], we)


@pytest.mark.parametrize("n", [1, 2, 257, 4099])
def test_to_percentiles_on_a_device_tensor_is_the_numpy_function(n):
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(n)
    s = rng.integers(0, max(2, n // 9), n).astype(np.float64) / 3.0   # heavy ties
    want = H.to_percentiles(s)
    assert np.array_equal(bits(want), bits(R.percentiles(s)))
    got = H.to_percentiles(torch.from_numpy(s).to("cuda"))
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (n,)
    assert np.array_equal(bits(host(got)), bits(want))
    got32 = H.to_percentiles(torch.from_numpy(s.astype(np.float32)).to("cuda").reshape(-1, 1))   # float32 scores, a column
    assert np.array_equal(bits(host(got32)), bits(H.to_percentiles(s.astype(np.float32))))


def test_score2percentile_float32_is_the_reference_loop():
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(9)
    a = rng.standard_normal((700, 1)).astype(np.float32)
    ref = np.concatenate([rng.standard_normal(1500), a[:60, 0].astype(np.float64), [0.0, -0.0]])
    want = S.score2percentile_loop_f32(a, ref)
    got = H.score2percentile(torch.from_numpy(a).to("cuda"), torch.from_numpy(ref).to("cuda"), out_dtype=torch.float32)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == (700, 1)
    assert np.array_equal(host(got).view(np.int32), want.view(np.int32))
    got_np = H.score2percentile(a, ref, out_dtype=np.float32)   # numpy in, numpy out
    assert isinstance(got_np, np.ndarray) and got_np.dtype == np.float32 and np.array_equal(got_np.view(np.int32), want.view(np.int32))
    full = H.score2percentile(a, ref)
    assert full.dtype == np.float64 and np.array_equal(bits(full), bits(S.percentiles(a, ref, S.OF_SCORE).reshape(700, 1)))


@pytest.mark.parametrize("multi", [False, True], ids=["CLAM_SB", "CLAM_MB"])
def test_compute_from_batches(multi):
    import torch
    from hipt_abmil_atec23_amd import CLAM_MB, CLAM_SB, synth
    from hipt_abmil_atec23_amd import heatmap as H
    size = (384, 128, 64)
    cls = CLAM_MB if multi else CLAM_SB
    m = cls(size_arg=list(size), n_classes=2)
    m.load_state_dict(synth.make_state_dict(synth.clam_param_specs(size, n_classes=2, multi=multi), 384), strict=True)
    m.relocate()
    m.eval()
    clam_pred = 1 if multi else None
    rows = (1, 130, 257)
    batches = [(synth.hash_uniform_torch((n, 384), 30 + i, device="cuda:0"), np.arange(2 * n).reshape(n, 2) + 1000 * i)
               for i, n in enumerate(rows)]
    want = []
    with torch.no_grad():
        for roi, _ in batches:
            a = m(roi, attention_only=True)
            assert a.shape == ((2 if multi else 1), len(roi))
            want.append(host(a[clam_pred] if multi else a).reshape(-1, 1))
    flat = np.concatenate(want).astype(np.float64).reshape(-1)
    rng = np.random.default_rng(31)
    ref = np.concatenate([flat[rng.permutation(len(flat))[:100]], rng.uniform(flat.min(), flat.max(), 200)])   # 300 values, 100 of them ties
    seen = []
    scores, coords = H.compute_from_batches(m, lambda roi: roi, batches, clam_pred=clam_pred, ref_scores=ref,
                                            on_batch=lambda s, c, f: seen.append((s, c, f)))
    assert scores.is_cuda and scores.dtype == torch.float32 and scores.shape == (sum(rows), 1)
    assert np.array_equal(coords, np.concatenate([c for _, c in batches]))
    want32 = np.concatenate([S.score2percentile_loop_f32(w, ref) for w in want])
    assert np.array_equal(host(scores).view(np.int32), want32.view(np.int32))
    assert [len(s) for s, _, _ in seen] == list(rows)
    for (s, c, f), (roi, bc), a in zip(seen, batches, np.split(want32, np.cumsum(rows)[:-1])):
        assert np.array_equal(host(s).view(np.int32), a.view(np.int32)) and np.array_equal(c, bc) and f is roi
    # float64 out, and without reference scores the attention itself comes back
    s64, _ = H.compute_from_batches(m, lambda roi: roi, batches, clam_pred=clam_pred, ref_scores=torch.from_numpy(ref).to("cuda:0"),
                                    out_dtype=torch.float64)
    assert np.array_equal(bits(host(s64)), bits(S.percentiles(flat, ref, S.OF_SCORE).reshape(-1, 1)))
    raw, _ = H.compute_from_batches(m, lambda roi: roi, batches, clam_pred=clam_pred)
    assert raw.dtype == torch.float32 and np.array_equal(host(raw), np.concatenate(want))
    if multi:
        with pytest.raises(ValueError, match="clam_pred"):
            H.compute_from_batches(m, lambda roi: roi, batches[:1])


def tied_case(seed):
    """200 patches of 6 x 4 on a 61 x 43 canvas, scores with ties."""
    rng = np.random.default_rng(seed)
    coords = np.stack([rng.integers(0, 58, 200), rng.integers(0, 41, 200)], axis=1)
    scores = rng.integers(0, 25, 200).astype(np.float64) * 1.5 - 4.0
    return scores, coords, (6, 4), 1.0, (61, 43)


def test_percentile_heatmap_is_capturable_and_free_of_host_copies():
    import torch
    from hipt_abmil_atec23_amd import heatmap as H
    scores, coords, patch, scale, region = tied_case(40)
    new_scores = tied_case(41)[0]
    assert len(np.unique(scores)) < 30 and not np.array_equal(scores, new_scores)
    dev = torch.device("cuda")
    rng = np.random.default_rng(42)
    canvas = rng.integers(0, 256, size=(43, 61, 3), dtype=np.uint8)
    kw = dict(convert_to_percentiles=True, binarize=False)
    rkw = dict(alpha=0.4, cmap="jet", canvas=canvas, **kw)
    s_t, c_t, cv_t = (torch.from_numpy(a).to(dev) for a in (scores, coords, canvas))
    tkw = dict(rkw, canvas=cv_t)
    H.render_heatmap(s_t, c_t, patch, scale, region, **tkw)   # (loads the library and puts the colour table on the device)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):   # one stream; a device-to-host copy in here raises
        ov, cnt = H.heatmap_overlay(s_t, c_t, patch, scale, region, **kw)
        img = H.render_heatmap(s_t, c_t, patch, scale, region, **tkw)
    for current in (scores, new_scores):
        s_t.copy_(torch.from_numpy(current))
        graph.replay()
        torch.cuda.synchronize()
        want_ov, want_cnt = H.heatmap_overlay(current, coords, patch, scale, region, **kw)   # the numpy-input route
        want_img = H.render_heatmap(current, coords, patch, scale, region, **rkw)
        assert np.array_equal(host(cnt), want_cnt)
        assert host(ov).tobytes() == want_ov.tobytes()
        assert np.array_equal(host(img), want_img)
        assert np.array_equal(want_img, R.render(current, coords, patch, scale, region, **rkw))
    assert not np.array_equal(want_img, H.render_heatmap(scores, coords, patch, scale, region, **rkw))


@pytest.mark.parametrize("mode,kw", [("topk", {}), ("reverse_topk", {}), ("range_sample", dict(score_start=40.0, score_end=60.0))])
def test_sample_rois_on_device_tensors_picks_what_the_numpy_route_picks(mode, kw):
    import torch
    from hipt_abmil_atec23_amd import _native as N
    from hipt_abmil_atec23_amd import heatmap as H
    rng = np.random.default_rng(50)
    n = 1000
    scores = rng.integers(0, 120, n).astype(np.float64) / 7.0
    coords = np.stack([rng.integers(0, 50, n) * 256, rng.integers(0, 40, n) * 256], axis=1)
    box = dict(top_left=(2560, 1024), bot_right=(9000, 8000))
    for extra in ({}, box):
        want = H.sample_rois(scores.reshape(-1, 1), coords, k=9, mode=mode, seed=13, **kw, **extra)
        before = N.calls
        got = H.sample_rois(torch.from_numpy(scores).to("cuda").reshape(-1, 1), torch.from_numpy(coords).to("cuda"), k=9, mode=mode,
                            seed=13, **kw, **extra)
        assert N.calls == before + 1
        assert len(want["sampled_scores"]) == 9
        assert np.array_equal(got["sampled_coords"], want["sampled_coords"])
        assert np.array_equal(bits(got["sampled_scores"]), bits(want["sampled_scores"]))
        ref = S.sample_rois_ref(scores, coords, k=9, mode=mode, seed=13, **kw, **extra)
        assert np.array_equal(ref["sampled_coords"], want["sampled_coords"])
