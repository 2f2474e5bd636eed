"""CPU tests of the device contour tracer: they pin the sequential restatement the device is compared with
(tests/contour_ref.py) -- literal examples, and on random and tissue-like masks the properties that follow from Suzuki and Abe's
definitions, checked against scipy.ndimage.label -- then the host glue of ``segment.trace_contours`` (order, hierarchy), the three
C entry points declared, exported and bound, and the refusals, which come before anything touches a device."""
import os
import re
import sys

import numpy as np
import pytest
from scipy import ndimage

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contour_ref as CR  # noqa: E402

from hipt_abmil_atec23_amd import _native as N  # noqa: E402
from hipt_abmil_atec23_amd import segment as SG  # noqa: E402

BADARG, WORKSPACE, UNSUPPORTED = -1, -2, -4
EIGHT = np.ones((3, 3), dtype=int)
_memo = {}


def case(name):
    """(mask, contours, hierarchy) of a property case; traced once"""
    if name not in _memo:
        mask = CR.smooth_mask(96, 128, seed=11, sigma=3.0) if name == "smooth" else CR.random_mask(37, 53, name, seed=int(name * 10))
        _memo[name] = (mask,) + CR.find_contours(mask)
    return _memo[name]


CASES = [0.3, 0.5, 0.7, "smooth"]


def pts(c):
    return c.reshape(-1, 2).tolist()


def signed_area(c):
    p = c.reshape(-1, 2).astype(np.int64)
    q = np.roll(p, 1, axis=0)
    return int(np.sum(q[:, 0] * p[:, 1] - p[:, 0] * q[:, 1]))


def test_literal_examples():
    m = np.zeros((4, 4), np.uint8)
    m[1:3, 1:3] = 255
    contours, hier = CR.find_contours(m)
    assert len(contours) == 1 and pts(contours[0]) == [[1, 1], [1, 2], [2, 2], [2, 1]] and hier.tolist() == [[[-1, -1, -1, -1]]]
    assert contours[0].dtype == np.int32 and contours[0].shape == (4, 1, 2) and hier.dtype == np.int32
    m = np.zeros((5, 5), np.uint8)
    m[1:4, 1:4] = 1
    m[2, 2] = 0
    contours, hier = CR.find_contours(m)
    assert len(contours) == 2 and pts(contours[1]) == [[1, 2], [2, 1], [3, 2], [2, 3]]
    assert pts(contours[0]) == [[1, 1], [1, 2], [1, 3], [2, 3], [3, 3], [3, 2], [3, 1], [2, 1]]
    assert hier.tolist() == [[[-1, -1, 1, -1], [-1, -1, -1, 0]]]
    assert signed_area(contours[0]) * signed_area(contours[1]) < 0
    m = np.zeros((3, 4), np.uint8)
    m[2, 3] = 9
    contours, hier = CR.find_contours(m)
    assert len(contours) == 1 and pts(contours[0]) == [[3, 2]] and hier.tolist() == [[[-1, -1, -1, -1]]]
    m = np.zeros((3, 6), np.uint8)
    m[1, 2:5] = 1
    assert pts(CR.find_contours(m)[0][0]) == [[2, 1], [3, 1], [4, 1], [3, 1]]
    assert CR.find_contours(np.zeros((3, 3), np.uint8)) == ((), None)
    p, o, hr = CR.trace(np.zeros((3, 3), np.uint8))
    assert p.shape == (0, 2) and o.tolist() == [0] and hr.shape == (0, 4)


def test_order_of_the_list_and_the_nesting():
    """two blobs, the lower one with two holes, one of which holds an island: top level in descending raster order of the starts, each
    followed by its holes in descending order; the island is top level again"""
    m = np.zeros((12, 12), np.uint8)
    m[0:2, 0:2] = 1                    # A: start (0, 0)
    m[3:12, 1:11] = 1                  # B: start (1, 3)
    m[4:6, 2:4] = 0                    # hole 1 of B: border starts at (1, 4)
    m[7:11, 4:9] = 0                   # hole 2 of B: border starts at (3, 7)
    m[8:10, 5:7] = 1                   # island C in hole 2: start (5, 8)
    contours, hier = CR.find_contours(m)
    assert [pts(c)[0] for c in contours] == [[5, 8], [1, 3], [3, 7], [1, 4], [0, 0]]
    assert hier[0].tolist() == [[1, -1, -1, -1], [4, 0, 2, -1], [3, -1, -1, 1], [-1, 2, -1, 1], [-1, 1, -1, -1]]


@pytest.mark.parametrize("name", CASES)
def test_borders_against_scipys_components(name):
    mask, contours, hier = case(name)
    h, w = mask.shape
    hier = hier[0]
    fg = np.pad(mask != 0, 1)
    lab, n_fg = ndimage.label(fg, structure=EIGHT)
    blab, n_bg = ndimage.label(~fg)
    outer = np.flatnonzero(hier[:, 3] == -1)
    holes = np.flatnonzero(hier[:, 3] >= 0)
    assert len(outer) == n_fg and len(holes) == n_bg - 1 and len(contours) == n_fg + n_bg - 1
    seen = set()
    for k, c in enumerate(contours):
        p = c.reshape(-1, 2)
        assert fg[p[:, 1] + 1, p[:, 0] + 1].all()                       # every point is foreground
        if len(p) > 1:
            d = np.abs(p - np.roll(p, 1, axis=0)).max(axis=1)
            assert (d == 1).all()                                       # consecutive points, cyclically, are 8-neighbours
        seen.update(map(tuple, p.tolist()))
        comp = lab[p[0, 1] + 1, p[0, 0] + 1]
        if hier[k, 3] == -1:     # an outer border starts at its component's raster-first pixel
            ys, xs = np.nonzero(lab == comp)
            assert (p[0, 1] + 1, p[0, 0] + 1) == (ys[0], xs[0])
        else:                    # a hole border: west of the hole's raster-first pixel; the parent is the outer border of the component
            hole = blab[p[0, 1] + 1, p[0, 0] + 2]
            assert hole != 0 and hole != blab[0, 0]
            ys, xs = np.nonzero(blab == hole)
            assert (p[0, 1] + 1, p[0, 0] + 2) == (ys[0], xs[0])
            q = contours[hier[k, 3]].reshape(-1, 2)[0]
            assert hier[hier[k, 3], 3] == -1 and lab[q[1] + 1, q[0] + 1] == comp
    # the union of all borders is the set of foreground pixels with a background 4-neighbour in the padded mask
    edge = fg & ~(np.roll(fg, 1, 0) & np.roll(fg, -1, 0) & np.roll(fg, 1, 1) & np.roll(fg, -1, 1))
    ys, xs = np.nonzero(edge)
    assert seen == set(zip((xs - 1).tolist(), (ys - 1).tolist()))
    # outer and hole borders turn opposite ways
    so = {np.sign(signed_area(contours[k])) for k in outer} - {0}
    sh = {np.sign(signed_area(contours[k])) for k in holes} - {0}
    assert len(so) == 1 and (not sh or (len(sh) == 1 and sh != so))


@pytest.mark.parametrize("name", CASES)
def test_hierarchy_links_are_consistent_and_ordered(name):
    mask, contours, hier = case(name)
    hier = hier[0]
    c = len(contours)
    start = [tuple(x.reshape(-1, 2)[0][::-1]) for x in contours]   # (y, x)
    for k in range(c):
        nxt, prv, child, parent = hier[k]
        assert hier[k, 2] == -1 or parent == -1                    # two levels
        if nxt >= 0:
            assert hier[nxt, 1] == k and hier[nxt, 3] == parent and start[nxt] < start[k]
        if prv >= 0:
            assert hier[prv, 0] == k
        if child >= 0:
            assert hier[child, 3] == k and hier[child, 1] == -1 and child == k + 1
        if parent >= 0 and prv == -1:
            assert hier[parent, 2] == k
    top = np.flatnonzero(hier[:, 3] == -1)
    assert top[0] == 0 and hier[0, 1] == -1 and [hier[k, 0] for k in top] == list(top[1:]) + [-1]
    for a, b in zip(top, list(top[1:]) + [c]):                     # its holes follow a top-level border at once
        assert (hier[a + 1:b, 3] == a).all()


@pytest.mark.parametrize("name", CASES)
def test_the_packages_order_and_hierarchy_functions_agree_with_the_restatement(name):
    """``segment._order_borders`` / ``_hierarchy`` (numpy, vectorised) from a table in raster order of the roots, as the library
    writes it, give the restatement's list"""
    mask, contours, hier = case(name)
    h, w = mask.shape
    hier = hier[0]
    first = np.array([x.reshape(-1, 2)[0] for x in contours], dtype=np.int64)
    start = first[:, 1] * w + first[:, 0]
    kind = (hier[:, 3] >= 0).astype(np.int64)
    parent = np.where(kind == 1, start[np.maximum(hier[:, 3], 0)], -1)
    shuffle = np.random.default_rng(3).permutation(len(contours))   # any table order gives the same list
    order = SG._order_borders(start[shuffle], kind[shuffle], parent[shuffle])
    assert np.array_equal(shuffle[order], np.arange(len(contours)))
    got = SG._hierarchy(kind)
    assert got.dtype == np.int32 and np.array_equal(got, hier)


def test_entry_points_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "hipt_abmil.h")).read()
    want = {"hipt_contours_workspace_bytes": ["h", "w"],
            "hipt_contours_trace": ["mask", "h", "w", "table", "ws", "ws_bytes", "stream"],
            "hipt_contours_emit": ["h", "w", "table", "offsets", "n_borders", "n_points", "points", "ws", "ws_bytes", "stream"]}
    lib = N.lib()
    for name, args in want.items():
        decl = re.search(r"^(?:int|size_t) %s\((.*?)\);" % name, hdr, re.S | re.M).group(1)
        assert [a.split()[-1].lstrip("*") for a in decl.split(",")] == args, name
        assert len(N.SIGNATURES[name][1]) == len(args) and hasattr(lib, name), name
    assert lib.hipt_abi_version() == N.ABI_VERSION   # additive: the version stays
    for macro, value in (("HIPT_CONTOURS_MAX_PLANE", N.CONTOURS_MAX_PLANE), ("HIPT_CONTOURS_MAX_BORDER_PIXELS", N.CONTOURS_MAX_BORDER_PIXELS),
                         ("HIPT_CONTOURS_MAX_BORDERS", N.CONTOURS_MAX_BORDERS)):
        assert f"#define {macro} {value}\n" in hdr
    assert "global: hipt_*;" in open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "hipt_abmil.map")).read()
    mk = open(os.path.join(ROOT, "hipt_abmil_atec23_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*=.*\bcontours\.hip\b", mk, re.M)
    import hipt_abmil_atec23_amd as amd
    for name in ("trace_contours", "find_contours"):
        assert getattr(amd, name) is getattr(SG, name)
    assert SG.find_contours.takes_device_mask is True


def al256(v):
    return (v + 255) & ~255


def test_workspace_bytes_is_the_carve():
    lib = N.lib()
    for h, w in [(1, 1), (37, 53), (256, 320), (4096, 4096), (8192, 8192)]:
        n, nb = (h + 2) * (w + 2), min(h * w, N.CONTOURS_MAX_BORDER_PIXELS)
        want = (al256(256) + al256(n) + 2 * al256(4 * n) + al256(8 * ((n + 255) // 256)) + 2 * al256(4 * nb) + 2 * al256(64 * nb)
                + al256(32 * nb))
        assert lib.hipt_contours_workspace_bytes(h, w) == want
    for h, w in [(0, 8), (8, 0), (-1, 8), (16384, 8192), (1, 1 << 27)]:
        assert lib.hipt_contours_workspace_bytes(h, w) == 0
    assert lib.hipt_contours_workspace_bytes(1, (1 << 27) // 3 - 2) > 0   # (h + 2) (w + 2) just inside 2^27


def test_library_refuses_without_launching():
    """Every pointer below is a made-up address: a check that let one through would launch on it."""
    lib = N.lib()
    mask, table, ws, offs, points = 0x10000, 0x20000, 0x70000, 0x30000, 0x40000
    need = lib.hipt_contours_workspace_bytes(64, 64)

    def trace(hw=(64, 64), mask=mask, table=table, ws=ws, ws_bytes=need):
        return lib.hipt_contours_trace(mask, hw[0], hw[1], table, ws, ws_bytes, None)

    def emit(hw=(64, 64), table=table, offs=offs, c=3, p=40, points=points, ws=ws, ws_bytes=need):
        return lib.hipt_contours_emit(hw[0], hw[1], table, offs, c, p, points, ws, ws_bytes, None)
    assert trace(mask=None) == BADARG and trace(table=None) == BADARG and trace(table=table + 4) == BADARG
    assert trace(hw=(0, 64)) == BADARG and trace(hw=(64, -3)) == BADARG
    assert trace(hw=(16384, 8192)) == UNSUPPORTED and b"2^27" in lib.hipt_last_error()
    assert trace(ws_bytes=need - 1) == WORKSPACE and trace(ws=ws + 16) == WORKSPACE and trace(ws=None, ws_bytes=0) == WORKSPACE
    assert trace(ws=None) == BADARG
    assert emit(table=None) == BADARG and emit(offs=None) == BADARG and emit(points=None) == BADARG and emit(points=points + 4) == BADARG
    assert emit(c=0) == BADARG and emit(c=64 * 64 + 1) == BADARG and emit(p=2) == BADARG and emit(p=8 * 64 * 64 + 4) == BADARG
    assert emit(hw=(0, 64)) == BADARG and emit(hw=(16384, 8192)) == UNSUPPORTED
    assert emit(ws_bytes=need - 1) == WORKSPACE and emit(ws=None) == BADARG


def test_python_layer_refuses_bad_requests_before_any_native_call():
    import torch
    before = N.calls
    for fn in (SG.trace_contours, SG.find_contours):
        for bad in (np.zeros((8, 8), np.float32), np.zeros((8, 8), np.int32), np.zeros((8, 8), bool), np.zeros((8, 8, 1), np.uint8),
                    np.zeros((8,), np.uint8), np.zeros((0, 8), np.uint8), [[1]], torch.zeros((8, 8), dtype=torch.float32),
                    torch.zeros((2, 8, 8), dtype=torch.uint8)):
            with pytest.raises(ValueError):
                fn(bad)
        big = np.broadcast_to(np.zeros((1, 1), np.uint8), (16384, 8192))   # beyond the envelope; no memory behind it
        with pytest.raises(ValueError, match="8192 x 8192"):
            fn(big)
        with pytest.raises(ValueError, match="HIP device"):     # a CPU tensor: there is no CPU path
            fn(torch.zeros((8, 8), dtype=torch.uint8))
        with pytest.raises(ValueError, match="HIP device"):
            fn(np.zeros((8, 8), np.uint8), device="cpu")
    assert N.calls == before


def test_segment_tissue_without_a_tracer_still_asks_for_cv2(monkeypatch):
    import torch

    class Slide:
        class wsi:
            @staticmethod
            def read_region(origin, level, size):
                return np.zeros((8, 8, 4), np.uint8)
        level_dim = [(8, 8)]
        level_downsamples = [(1.0, 1.0)]
    monkeypatch.setattr(SG, "tissue_mask", lambda *a: torch.zeros((8, 8), dtype=torch.uint8))
    monkeypatch.setitem(sys.modules, "cv2", None)
    with pytest.raises(ImportError, match="find_contours=") as e:
        SG.segment_tissue(Slide())
    assert "segment.find_contours" in str(e.value)
    # a tracer that finds nothing may return cv2's (.., None)
    slide = Slide()
    SG.segment_tissue(slide, find_contours=lambda mask: ((), None))
    assert slide.contours_tissue == [] and slide.holes_tissue == []
