"""Drop-in hook: make the reference's scripts import this package's classes.

The reference imports the hot-path classes by module path:
  ``from HIPT_4K.hipt_4k import HIPT_4K``, ``from HIPT_4K.hipt_model_utils import eval_transforms``
  (extract_features_fp.py:15-16, create_heatmaps.py:23), ``import HIPT_4K.vision_transformer as vits``
  (hipt_4k.py:25-26) and ``from models.model_clam import CLAM_MB, CLAM_SB`` (utils/core_utils.py:7,
  utils/eval_utils.py:6).  ``install()`` registers this package's modules in ``sys.modules`` under
  exactly those names BEFORE the reference scripts import them; the reference's ``models`` package
  (which also holds model_mil.py / resnet_custom.py) is left alone — only the ``model_clam``
  sub-module is replaced.  ``install(resnet=True)`` also replaces ``models.resnet_custom`` (the ResNet-50 baseline route,
  extract_features_fp.py:19,210-211).  ``install(sampling=True)`` makes ``utils.sampling_utils.generate_sample_idxs`` and
  ``update_sampling_weights`` (what ``summary_sampling`` calls, utils/eval_utils.py:18,298-467) this package's: where the
  reference's module imports, the two names are rebound ON it (eval_utils.py takes its plotting helpers from the same module);
  where it does not, a module is registered whose plotting names raise.  ``install(heatmaps=True)`` binds this package's
  ``vis_heatmap`` as ``wsi_core.WholeSlideImage.WholeSlideImage.visHeatmap`` (what create_heatmaps.py draws with) where the
  reference's ``wsi_core`` imports (it needs openslide and cv2); elsewhere it does nothing.  ``install(resnet18=True)`` binds
  ``models.resnet_custom.resnet18_baseline`` to this package's HistoResNet-18 (``resnet18.resnet18_baseline``).
  ``install(heatmap_scores=True)`` binds ``wsi_core.wsi_utils.to_percentiles`` and ``sample_rois`` to ``heatmap``'s where the
  reference's module imports (it needs h5py and cv2); elsewhere it does nothing.  ``install(hier_heatmaps=True)`` binds
  ``HIPT_4K.hipt_heatmap_utils.create_hierarchical_heatmaps_indiv`` to ``hier_heatmap``'s where the reference's module imports
  (it needs cv2, h5py and webdataset); elsewhere it does nothing.  ``install(tiling=True)`` binds ``tiling.process_contour_like`` as
  ``wsi_core.WholeSlideImage.WholeSlideImage.process_contour`` (what ``process_contours`` and ``Wsi_Region`` call per contour) where
  the reference's ``wsi_core`` imports; elsewhere it does nothing.  The alternative is the overlay files under ``shims/``.
"""
from __future__ import annotations

import importlib
import importlib.util
import sys
import types

_MAP = {
    "HIPT_4K.hipt_4k": "hipt_4k",
    "HIPT_4K.hipt_model_utils": "hipt_model_utils",
    "HIPT_4K.vision_transformer": "vision_transformer",
    "HIPT_4K.vision_transformer4k": "vision_transformer4k",
    "models.model_clam": "model_clam",
}


# opt-in (install(resnet=True)): the reference's ResNet-50 baseline extractor (extract_features_fp.py:19,210-211)
_RESNET_MAP = {"models.resnet_custom": "resnet_custom"}
_saved = {}  # ref name -> the module it replaced (restored by uninstall())


_SAMPLING_MOD = "utils.sampling_utils"
_SAMPLING_NAMES = {"generate_sample_idxs": "generate_sample_idxs", "update_sampling_weights": "update_sampling_weights_np"}
_PLOTTING = ("plot_sampling", "plot_sampling_gif", "plot_weighting", "plot_weighting_gif", "generate_features_array")


def _install_sampling(verbose: bool):
    """Bind the two sampling functions under ``utils.sampling_utils`` (opt-in)."""
    from . import sampling
    if _SAMPLING_MOD in _saved:
        return
    mod = None
    try:
        if importlib.util.find_spec(_SAMPLING_MOD) is not None:
            mod = importlib.import_module(_SAMPLING_MOD)   # needs openslide / matplotlib, as the reference does
    except Exception:   # no reference checkout on sys.path, or one of its imports is missing
        mod = None
    if mod is not None and not getattr(mod, "__hipt_amd_stub__", False):
        _saved[_SAMPLING_MOD] = ("rebound", {n: getattr(mod, n) for n in _SAMPLING_NAMES})
    else:
        _saved[_SAMPLING_MOD] = ("stub", sys.modules.get(_SAMPLING_MOD))
        mod = types.ModuleType(_SAMPLING_MOD)
        mod.__hipt_amd_stub__ = True

        def _absent(name):
            def fn(*a, **k):
                raise RuntimeError(f"utils.sampling_utils.{name}: the reference's module is not importable here (no checkout on "
                                   f"sys.path, or openslide / matplotlib missing); hipt_abmil_atec23_amd provides the sampling functions only")
            return fn
        for name in _PLOTTING:
            setattr(mod, name, _absent(name))
        if "utils" not in sys.modules:
            parent = types.ModuleType("utils")
            parent.__path__ = []
            parent.__hipt_amd_stub__ = True
            sys.modules["utils"] = parent
        sys.modules[_SAMPLING_MOD] = mod
        setattr(sys.modules["utils"], "sampling_utils", mod)
    for ref_name, ours in _SAMPLING_NAMES.items():
        setattr(mod, ref_name, getattr(sampling, ours))
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_SAMPLING_MOD}.{{{', '.join(_SAMPLING_NAMES)}}} -> {sampling.__name__} ({_saved[_SAMPLING_MOD][0]})")


def _uninstall_sampling():
    if _SAMPLING_MOD not in _saved:
        return
    how, prev = _saved.pop(_SAMPLING_MOD)
    if how == "rebound":
        for n, fn in prev.items():
            setattr(sys.modules[_SAMPLING_MOD], n, fn)
        return
    parent = sys.modules.get("utils")
    if prev is None:
        sys.modules.pop(_SAMPLING_MOD, None)
        if parent is not None and hasattr(parent, "sampling_utils"):
            delattr(parent, "sampling_utils")
    else:
        sys.modules[_SAMPLING_MOD] = prev
        if parent is not None:
            parent.sampling_utils = prev
    if getattr(parent, "__hipt_amd_stub__", False):
        sys.modules.pop("utils", None)


_WSI_MOD = "wsi_core.WholeSlideImage"


def _install_heatmaps(verbose: bool) -> bool:
    """Bind ``vis_heatmap`` as the reference class's ``visHeatmap`` (opt-in).  False, and nothing done, where the reference's
    ``wsi_core.WholeSlideImage`` does not import: there is no class to bind to, and the reading, segmenting and contour code of
    that module is not this package's."""
    from . import heatmap
    if _WSI_MOD in _saved:
        return True
    try:
        if _WSI_MOD not in sys.modules and importlib.util.find_spec(_WSI_MOD) is None:
            return False
        cls = importlib.import_module(_WSI_MOD).WholeSlideImage
    except Exception:   # no reference checkout on sys.path, or openslide / cv2 missing
        return False
    _saved[_WSI_MOD] = cls.__dict__.get("visHeatmap")
    cls.visHeatmap = heatmap.vis_heatmap
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_WSI_MOD}.WholeSlideImage.visHeatmap -> {heatmap.__name__}.vis_heatmap")
    return True


def _uninstall_heatmaps():
    if _WSI_MOD not in _saved:
        return
    prev = _saved.pop(_WSI_MOD)
    cls = sys.modules[_WSI_MOD].WholeSlideImage
    if prev is None:
        del cls.visHeatmap
    else:
        cls.visHeatmap = prev


_TILING_KEY = _WSI_MOD + ".process_contour"


def _install_tiling(verbose: bool) -> bool:
    """Bind ``tiling.process_contour_like`` as the reference class's ``process_contour`` (opt-in).  False, and nothing done, where
    the reference's ``wsi_core.WholeSlideImage`` does not import."""
    from . import tiling
    if _TILING_KEY in _saved:
        return True
    try:
        if _WSI_MOD not in sys.modules and importlib.util.find_spec(_WSI_MOD) is None:
            return False
        cls = importlib.import_module(_WSI_MOD).WholeSlideImage
    except Exception:   # no reference checkout on sys.path, or openslide / cv2 missing
        return False
    _saved[_TILING_KEY] = cls.__dict__.get("process_contour")
    cls.process_contour = tiling.process_contour_like
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_WSI_MOD}.WholeSlideImage.process_contour -> {tiling.__name__}.process_contour_like")
    return True


def _uninstall_tiling():
    if _TILING_KEY not in _saved:
        return
    prev = _saved.pop(_TILING_KEY)
    mod = sys.modules.get(_WSI_MOD)
    if mod is None:
        return
    if prev is None:
        del mod.WholeSlideImage.process_contour
    else:
        mod.WholeSlideImage.process_contour = prev


_WSI_UTILS_MOD = "wsi_core.wsi_utils"
_WSI_UTILS_NAMES = ("to_percentiles", "sample_rois")


def _install_heatmap_scores(verbose: bool) -> bool:
    """Bind ``heatmap.to_percentiles`` and ``heatmap.sample_rois`` on the reference's ``wsi_core.wsi_utils`` (opt-in).  False, and
    nothing done, where that module does not import."""
    from . import heatmap
    if _WSI_UTILS_MOD in _saved:
        return True
    try:
        if _WSI_UTILS_MOD not in sys.modules and importlib.util.find_spec(_WSI_UTILS_MOD) is None:
            return False
        mod = importlib.import_module(_WSI_UTILS_MOD)
    except Exception:   # no reference checkout on sys.path, or h5py / cv2 missing
        return False
    _saved[_WSI_UTILS_MOD] = {n: mod.__dict__.get(n) for n in _WSI_UTILS_NAMES}
    for n in _WSI_UTILS_NAMES:
        setattr(mod, n, getattr(heatmap, n))
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_WSI_UTILS_MOD}.{{{', '.join(_WSI_UTILS_NAMES)}}} -> {heatmap.__name__}")
    return True


def _uninstall_heatmap_scores():
    if _WSI_UTILS_MOD not in _saved:
        return
    prev = _saved.pop(_WSI_UTILS_MOD)
    mod = sys.modules.get(_WSI_UTILS_MOD)
    if mod is None:
        return
    for n, fn in prev.items():
        if fn is None:
            delattr(mod, n)
        else:
            setattr(mod, n, fn)


_HIER_MOD, _HIER_NAME = "HIPT_4K.hipt_heatmap_utils", "create_hierarchical_heatmaps_indiv"


def _install_hier_heatmaps(verbose: bool) -> bool:
    """Bind ``hier_heatmap.create_hierarchical_heatmaps_indiv_like`` (the reference's signature) as
    ``HIPT_4K.hipt_heatmap_utils.create_hierarchical_heatmaps_indiv`` (opt-in).  False, and nothing done, where the reference's
    module does not import: the patch-level and concatenated pictures of that module are not this package's."""
    from . import hier_heatmap
    if _HIER_MOD in _saved:
        return True
    try:
        if _HIER_MOD not in sys.modules and importlib.util.find_spec(_HIER_MOD) is None:
            return False
        mod = importlib.import_module(_HIER_MOD)
    except Exception:   # no reference checkout on sys.path, or cv2 / h5py / webdataset missing
        return False
    _saved[_HIER_MOD] = mod.__dict__.get(_HIER_NAME)
    setattr(mod, _HIER_NAME, hier_heatmap.create_hierarchical_heatmaps_indiv_like)
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_HIER_MOD}.{_HIER_NAME} -> {hier_heatmap.__name__}")
    return True


def _uninstall_hier_heatmaps():
    if _HIER_MOD not in _saved:
        return
    prev = _saved.pop(_HIER_MOD)
    mod = sys.modules.get(_HIER_MOD)
    if mod is None:
        return
    if prev is None:
        delattr(mod, _HIER_NAME)
    else:
        setattr(mod, _HIER_NAME, prev)


_EVAL_MOD = "utils.eval_utils"


def _install_evaluation(verbose: bool) -> bool:
    """Bind ``evaluate.summary_like`` as ``utils.eval_utils.summary`` (opt-in): the split goes through ``forward_bags`` in a few
    calls instead of one forward per slide.  False, and nothing done, where the reference's module does not import (its AUC, data
    frame and logger come from that module's own imports)."""
    from . import evaluate
    if _EVAL_MOD in _saved:
        return True
    try:
        if _EVAL_MOD not in sys.modules and importlib.util.find_spec(_EVAL_MOD) is None:
            return False
        mod = importlib.import_module(_EVAL_MOD)
    except Exception:   # no reference checkout on sys.path, or sklearn / pandas / ... missing
        return False
    _saved[_EVAL_MOD] = mod.__dict__.get("summary")
    mod.summary = evaluate.summary_like(mod)
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_EVAL_MOD}.summary -> {evaluate.__name__}.evaluate_split")
    return True


_VAL_MOD = "utils.core_utils"


def _install_validation(verbose: bool) -> bool:
    """Bind ``evaluate.validate_clam_like`` as ``utils.core_utils.validate_clam`` (opt-in): the per-epoch validation goes through
    ``forward_bags(..., instance_eval=True)`` in a few calls.  False, and nothing done, where the reference's module does not import."""
    from . import evaluate
    if _VAL_MOD in _saved:
        return True
    try:
        if _VAL_MOD not in sys.modules and importlib.util.find_spec(_VAL_MOD) is None:
            return False
        mod = importlib.import_module(_VAL_MOD)
    except Exception:   # no reference checkout on sys.path, or one of its imports is missing
        return False
    _saved[_VAL_MOD] = mod.__dict__.get("validate_clam")
    mod.validate_clam = evaluate.validate_clam_like(mod)
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_VAL_MOD}.validate_clam -> {evaluate.__name__}.validate_split")
    return True


def _uninstall_validation():
    if _VAL_MOD not in _saved:
        return
    prev = _saved.pop(_VAL_MOD)
    mod = sys.modules.get(_VAL_MOD)
    if mod is None:
        return
    if prev is None:
        del mod.validate_clam
    else:
        mod.validate_clam = prev


def _uninstall_evaluation():
    if _EVAL_MOD not in _saved:
        return
    prev = _saved.pop(_EVAL_MOD)
    mod = sys.modules.get(_EVAL_MOD)
    if mod is None:
        return
    if prev is None:
        del mod.summary
    else:
        mod.summary = prev


_RESNET18_MOD, _RESNET18_NAME = "models.resnet_custom", "resnet18_baseline"
_RESNET18_KEY = _RESNET18_MOD + "." + _RESNET18_NAME


def _install_resnet18(verbose: bool) -> bool:
    """Bind ``resnet18.resnet18_baseline`` as ``models.resnet_custom.resnet18_baseline`` (opt-in).  On the reference's own module
    the name is rebound; where ``install(resnet=True)`` mapped this package's ``resnet_custom``, whose stub of that name keeps
    raising, a module with its names and this one function is registered in its place (a snapshot: names added to ``resnet_custom``
    later do not appear in it).  That second form, and its branch of ``_uninstall_resnet18``, exist only because the stub must keep
    raising: delete both when the stub returns ``resnet18.resnet18_baseline``.  False, and nothing done, where no
    ``models.resnet_custom`` imports."""
    from . import resnet18, resnet_custom
    _uninstall_resnet18()
    try:
        if _RESNET18_MOD not in sys.modules and importlib.util.find_spec(_RESNET18_MOD) is None:
            return False
        mod = importlib.import_module(_RESNET18_MOD)
    except Exception:   # no reference checkout on sys.path, or one of its imports (torchvision) is missing
        return False
    if mod is resnet_custom:
        view = types.ModuleType(_RESNET18_MOD)
        view.__dict__.update({k: v for k, v in vars(mod).items() if not k.startswith("__")})
        setattr(view, _RESNET18_NAME, resnet18.resnet18_baseline)
        sys.modules[_RESNET18_MOD] = view
        setattr(sys.modules["models"], "resnet_custom", view)
        _saved[_RESNET18_KEY] = ("view", view, mod)
    else:
        _saved[_RESNET18_KEY] = ("rebound", mod, mod.__dict__.get(_RESNET18_NAME))
        setattr(mod, _RESNET18_NAME, resnet18.resnet18_baseline)
    if verbose:
        print(f"[hipt_abmil_atec23_amd] {_RESNET18_KEY} -> {resnet18.__name__}.resnet18_baseline")
    return True


def _uninstall_resnet18():
    if _RESNET18_KEY not in _saved:
        return
    how, mod, prev = _saved.pop(_RESNET18_KEY)
    if how == "view":
        if sys.modules.get(_RESNET18_MOD) is mod:
            sys.modules[_RESNET18_MOD] = prev
            if "models" in sys.modules:
                setattr(sys.modules["models"], "resnet_custom", prev)
    elif prev is None:
        delattr(mod, _RESNET18_NAME)
    else:
        setattr(mod, _RESNET18_NAME, prev)


def install(verbose: bool = False, resnet: bool = False, sampling: bool = False, heatmaps: bool = False, resnet18: bool = False,
            evaluation: bool = False, validation: bool = False, heatmap_scores: bool = False, hier_heatmaps: bool = False,
            tiling: bool = False):
    """Register the HIP-backed modules under the reference's import paths. Returns the mapping.  ``resnet=True`` also maps
    ``models.resnet_custom`` (ResNet_Baseline / resnet50_baseline); without it the reference's resnet_custom is left alone.
    ``sampling=True`` also binds ``utils.sampling_utils.generate_sample_idxs`` / ``update_sampling_weights`` (eval.py --sampling).
    ``heatmaps=True`` also binds ``WholeSlideImage.visHeatmap`` where the reference's ``wsi_core`` imports (else a no-op).
    ``resnet18=True`` also binds ``models.resnet_custom.resnet18_baseline`` to ``resnet18.resnet18_baseline`` (the HistoResNet-18
    extractor), on the module ``resnet=True`` mapped or on the reference's own.
    ``evaluation=True`` also binds ``utils.eval_utils.summary`` to ``evaluate.evaluate_split`` where that module imports (else a no-op).
    ``validation=True`` also binds ``utils.core_utils.validate_clam`` to ``evaluate.validate_split`` where that module imports (else a no-op).
    ``heatmap_scores=True`` also binds ``wsi_core.wsi_utils.to_percentiles`` / ``sample_rois`` to ``heatmap``'s where that module imports
    (else a no-op).
    ``hier_heatmaps=True`` also binds ``HIPT_4K.hipt_heatmap_utils.create_hierarchical_heatmaps_indiv`` to ``hier_heatmap``'s where
    that module imports (else a no-op).
    ``tiling=True`` also binds ``WholeSlideImage.process_contour`` to ``tiling.process_contour_like`` where the reference's ``wsi_core``
    imports (else a no-op)."""
    done = {}
    if tiling and _install_tiling(verbose):
        done[_WSI_MOD + ".WholeSlideImage.process_contour"] = f"{__name__.rsplit('.', 1)[0]}.tiling.process_contour_like"
    if hier_heatmaps and _install_hier_heatmaps(verbose):
        done[f"{_HIER_MOD}.{_HIER_NAME}"] = f"{__name__.rsplit('.', 1)[0]}.hier_heatmap.create_hierarchical_heatmaps_indiv_like"
    if heatmap_scores and _install_heatmap_scores(verbose):
        for n in _WSI_UTILS_NAMES:
            done[f"{_WSI_UTILS_MOD}.{n}"] = f"{__name__.rsplit('.', 1)[0]}.heatmap.{n}"
    if heatmaps and _install_heatmaps(verbose):
        done[_WSI_MOD + ".WholeSlideImage.visHeatmap"] = f"{__name__.rsplit('.', 1)[0]}.heatmap.vis_heatmap"
    if sampling:
        _install_sampling(verbose)
        done[_SAMPLING_MOD] = f"{__name__.rsplit('.', 1)[0]}.sampling"
    pkg = __name__.rsplit(".", 1)[0]
    for ref_name, ours in list(_MAP.items()) + (list(_RESNET_MAP.items()) if resnet else []):
        mod = importlib.import_module(f"{pkg}.{ours}")
        parent_name = ref_name.split(".")[0]
        if parent_name not in sys.modules:
            # HIPT_4K/: a directory of four files we replace entirely -> always a stub namespace.
            # models/: the reference's real package (model_mil.py, resnet_custom.py ...) must keep working,
            # so it is imported if it is on sys.path and only stubbed when there is no reference checkout.
            spec = None
            if parent_name != "HIPT_4K":
                try:
                    spec = importlib.util.find_spec(parent_name)
                except (ImportError, ValueError):
                    spec = None
            if spec is not None:
                importlib.import_module(parent_name)
            else:
                parent = types.ModuleType(parent_name)
                parent.__path__ = []
                parent.__hipt_amd_stub__ = True
                sys.modules[parent_name] = parent
        if ref_name in _RESNET_MAP and ref_name not in _saved:
            _saved[ref_name] = sys.modules.get(ref_name)
        sys.modules[ref_name] = mod
        parent = sys.modules.get(parent_name)
        if parent is not None:
            setattr(parent, ref_name.split(".")[1], mod)
        done[ref_name] = mod.__name__
        if verbose:
            print(f"[hipt_abmil_atec23_amd] {ref_name} -> {mod.__name__}")
    if resnet18 and _install_resnet18(verbose):
        done[_RESNET18_KEY] = f"{pkg}.resnet18.resnet18_baseline"
    if evaluation and _install_evaluation(verbose):
        done[_EVAL_MOD + ".summary"] = f"{pkg}.evaluate.evaluate_split"
    if validation and _install_validation(verbose):
        done[_VAL_MOD + ".validate_clam"] = f"{pkg}.evaluate.validate_split"
    return done


def uninstall():
    _uninstall_validation()
    _uninstall_evaluation()
    _uninstall_resnet18()
    _uninstall_sampling()
    _uninstall_heatmaps()
    _uninstall_heatmap_scores()
    _uninstall_hier_heatmaps()
    _uninstall_tiling()
    for ref_name in _MAP:
        sys.modules.pop(ref_name, None)
    for ref_name in _RESNET_MAP:
        if ref_name not in _saved:
            continue
        prev = _saved.pop(ref_name)
        parent = sys.modules.get(ref_name.split(".")[0])
        if prev is None:
            sys.modules.pop(ref_name, None)
            if parent is not None and hasattr(parent, ref_name.split(".")[1]):
                delattr(parent, ref_name.split(".")[1])
        else:
            sys.modules[ref_name] = prev
            if parent is not None:
                setattr(parent, ref_name.split(".")[1], prev)
    for parent in ("HIPT_4K", "models"):
        if getattr(sys.modules.get(parent), "__hipt_amd_stub__", False):
            sys.modules.pop(parent, None)
