"""Regenerates tests/golden/tiling_*.npz from the reference's own code (run where a checkout of scjjb/HIPT_ABMIL_ATEC23 is at hand:
``python tests/golden/make_golden_tiling.py /path/to/reference``; the tests never run this).

What executes is the reference's text: ``wsi_core/util_classes.py`` is loaded as a module, and the bodies of ``isInHoles``,
``isInContours``, ``process_contour`` and ``process_coord_candidate`` are taken out of ``wsi_core/WholeSlideImage.py`` by name (its
syntax tree) and compiled into a class of their own, because the module itself imports openslide, h5py, cv2 and matplotlib, none of
which is installed here.  Stand-ins fill the gaps: a ``cv2`` module whose ``pointPolygonTest`` / ``boundingRect`` / ``contourArea``
are tests/tiling_ref.py's, empty ``openslide`` and ``h5py`` modules, and a serial stand-in for ``multiprocessing.Pool``.  So the
files pin this package's glue -- shifts, ``// 2`` against ``/ 2``, candidate order, clamps, result dtype -- to the reference's code;
they do NOT pin cv2's own return values (cv2 is absent, that agreement is argued and not measured).
Only data is written: inputs and the resulting coordinates of a handful of small cases, a few KB each."""
import ast
import contextlib
import importlib.util
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import tiling_ref as TR  # noqa: E402

WANTED = ("isInHoles", "isInContours", "process_contour", "process_coord_candidate")


class _SerialPool:
    def __init__(self, n):
        pass

    def starmap(self, fn, iterable):
        return [fn(*a) for a in iterable]

    def close(self):
        pass


def load_reference(ref_root):
    cv2 = types.ModuleType("cv2")
    cv2.pointPolygonTest, cv2.boundingRect, cv2.contourArea = TR.pointPolygonTest, TR.boundingRect, TR.contourArea
    sys.modules["cv2"] = cv2
    for name in ("openslide", "h5py"):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location("ref_util_classes", os.path.join(ref_root, "wsi_core", "util_classes.py"))
    uc = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(uc)
    path = os.path.join(ref_root, "wsi_core", "WholeSlideImage.py")
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "WholeSlideImage")
    fns = [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in WANTED]
    assert sorted(f.name for f in fns) == sorted(WANTED)
    mod = ast.Module(body=[ast.ClassDef(name="WholeSlideImage", bases=[], keywords=[], body=fns, decorator_list=[])], type_ignores=[])
    ast.fix_missing_locations(mod)
    mp = types.SimpleNamespace(cpu_count=lambda: 1, Pool=_SerialPool)
    ns = {"cv2": cv2, "np": np, "mp": mp, "Contour_Checking_fn": uc.Contour_Checking_fn}
    for n in ("isInContourV1", "isInContourV2", "isInContourV3_Easy", "isInContourV3_Hard"):
        ns[n] = getattr(uc, n)
    exec(compile(mod, path, "exec"), ns)
    return ns["WholeSlideImage"], uc


def cases():
    """name -> (cont, holes, level_dim, level_downsamples, patch_level, kwargs of process_contour, dataset-route (name, center_shift) or None)"""
    big = TR.blob(3, 2100, 1900, 900, 120)
    holes = [TR.blob(5, 1900, 1800, 150, 24), TR.blob(6, 2500, 2200, 90, 12), TR.blob(7, 2100, 2500, 60, 9)]
    chain = TR.pixel_chain(TR.blob(9, 300, 260, 120, 40))
    dims1 = [(6000, 5000)]
    dims2 = [(6000, 5000), (3000, 2500)]
    out = {}
    for fn in ("four_pt", "four_pt_hard", "center", "basic"):
        out[f"blob_{fn}"] = (big, holes, dims1, [(1.0, 1.0)], 0, dict(patch_size=256, step_size=256, contour_fn=fn), None)
    out["blob_overlap_odd"] = (big, holes, dims1, [(1.0, 1.0)], 0, dict(patch_size=255, step_size=100, contour_fn="four_pt"), None)
    out["blob_level1"] = (big, holes, dims2, [(1.0, 1.0), (2.0, 2.0)], 1, dict(patch_size=128, step_size=96, contour_fn="four_pt_hard"), None)
    out["blob_roi"] = (big, holes, dims1, [(1.0, 1.0)], 0,
                       dict(patch_size=256, step_size=128, contour_fn="center", top_left=(1500, 1400), bot_right=(2600, 2300)), None)
    out["blob_roi_miss"] = (big, holes, dims1, [(1.0, 1.0)], 0,
                            dict(patch_size=256, step_size=128, contour_fn="center", top_left=(4000, 4000), bot_right=(4500, 4500)), None)
    edge = TR.blob(11, 5700, 4700, 280, 60)
    out["border_nopad"] = (np.clip(edge, 0, [5999, 4999]).astype(np.int32), [], dims1, [(1.0, 1.0)], 0,
                           dict(patch_size=256, step_size=64, contour_fn="four_pt", use_padding=False), None)
    out["chain_tiny_patch"] = (chain, [], [(700, 600)], [(1.0, 1.0)], 0, dict(patch_size=3, step_size=7, contour_fn="four_pt"), None)
    out["dataset_hard_0375"] = (big, holes, dims1, [(1.0, 1.0)], 0, dict(patch_size=256, step_size=224), ("four_pt_hard", 0.375))
    out["dataset_hard_0"] = (big, holes, dims1, [(1.0, 1.0)], 0, dict(patch_size=256, step_size=256), ("four_pt_hard", 0.0))
    out["dataset_easy"] = (big, holes, dims1, [(1.0, 1.0)], 0, dict(patch_size=256, step_size=256), ("four_pt_easy", 0.625))
    return out


def main(ref_root):
    W, uc = load_reference(ref_root)
    for name, (cont, holes, level_dim, level_ds, level, kw, route) in cases().items():
        w = W.__new__(W)
        w.level_dim, w.level_downsamples, w.name = level_dim, level_ds, name
        kwargs = dict(kw)
        contour_fn, center_shift = kw.get("contour_fn", "four_pt"), 0.5
        if route is not None:   # datasets/wsi_dataset.py:18-29: an instance, built as get_contour_check_fn builds it
            contour_fn, center_shift = route
            ref_ps = kw["patch_size"] * int(level_ds[level][0])
            if contour_fn == "four_pt_hard":
                kwargs["contour_fn"] = uc.isInContourV3_Hard(contour=cont, patch_size=ref_ps, center_shift=center_shift)
            else:
                kwargs["contour_fn"] = uc.isInContourV3_Easy(contour=cont, patch_size=ref_ps, center_shift=0.5)
        with contextlib.redirect_stdout(io.StringIO()):
            asset, attr = w.process_contour(cont, holes, level, "", **kwargs)
        coords = asset["coords"] if asset else np.zeros((0, 2), np.int64)
        assert coords.dtype == np.int64 and (not asset or sorted(attr["coords"]) == sorted(
            ["patch_size", "patch_level", "downsample", "downsampled_level_dim", "level_dim", "name", "save_path"]))
        hole_off = np.cumsum([0] + [len(h) for h in holes]).astype(np.int64)
        np.savez_compressed(
            os.path.join(HERE, f"tiling_{name}.npz"), cont=cont, hole_verts=np.concatenate(holes) if holes else np.zeros((0, 2), np.int32),
            hole_off=hole_off, level_dim0=np.array(level_dim[0]), downsample=np.array(level_ds[level]), patch_size=kw["patch_size"],
            step_size=kw["step_size"], contour_fn=contour_fn, center_shift=center_shift, use_padding=kw.get("use_padding", True),
            top_left=np.array(kw.get("top_left") or (-1, -1)), bot_right=np.array(kw.get("bot_right") or (-1, -1)),
            has_roi=("top_left" in kw), coords=coords)
        print(f"{name}: {len(cont)} vertices, {len(holes)} holes -> {len(coords)} coordinates")


if __name__ == "__main__":
    main(sys.argv[1])
