"""Feature store either side of the hot path.

Writer = what ``compute_w_loader`` + ``save_hdf5`` + the ``.pt`` export do in the reference
(``extract_features_fp.py:159-171,248-255``, ``utils/file_utils.py:16-35``): per slide, ``features [n, 192]``
fp32 and ``coords [n, 2]`` appended batch by batch, then ``pt_files/{slide}.pt`` = ``torch.save(features)``.
Reader = the bag loader of ``datasets/dataset_generic.py:505-528``: ``torch.load`` of that file and, when the slide
has more than ``max_patches_per_slide`` rows, ``np.random.choice(n, max)`` (WITH replacement, as the reference)
rows of it.

``coords`` are integer data and pass through bit for bit: whatever integer dtype the loader hands over
(the reference's h5 ``coords`` dataset: int64, or int32 from older patch files) is what is stored.  The reference keeps them
in ``h5_files/{slide}.h5`` beside the features; ``h5py`` is not part of every host (this image has none), so the coordinates
are ALWAYS written to a sidecar ``coords_files/{slide}.npy`` (plain ``numpy.save`` of the ``[n, 2]`` array, same row order as
``pt_files/{slide}.pt``; ``load_coords`` reads it back) and the ``.h5`` twin (datasets ``features`` / ``coords``, chunks
``(1, .)``, resizable first axis: ``utils/file_utils.py:16-35``) in addition where ``h5py`` is importable.  The directory is a
sibling of ``pt_files/`` because the reference lists that directory to find finished slides
(``extract_features_fp.py:231-238``) and loads bags from it by name: nothing else may live there.
"""
from __future__ import annotations

import os
from typing import Iterable, Optional, Tuple

import numpy as np
import torch


class FeatureWriter:
    """Accumulates one slide's region features / coordinates; ``close()`` writes the files."""

    def __init__(self, feat_dir: str, slide_id: str, write_h5: Optional[bool] = None):
        self.feat_dir, self.slide_id = feat_dir, slide_id
        self._feats, self._coords = [], []
        if write_h5 is None:
            try:
                import h5py  # noqa: F401
                write_h5 = True
            except ImportError:
                write_h5 = False
        self.write_h5 = write_h5

    def append(self, features, coords) -> None:
        f = features.detach().float().cpu() if torch.is_tensor(features) else torch.as_tensor(np.asarray(features), dtype=torch.float32)
        c = coords.detach().cpu().numpy() if torch.is_tensor(coords) else np.asarray(coords)
        if f.dim() != 2 or c.ndim != 2 or f.shape[0] != c.shape[0]:
            raise ValueError(f"features {tuple(f.shape)} / coords {tuple(c.shape)}: expected [n, d] and [n, 2]")
        if c.dtype.kind not in "iu":
            raise TypeError(f"slide {self.slide_id}: coords must be integers (got {c.dtype}); they are stored bit for bit, never rounded")
        if self._coords and (c.dtype != self._coords[0].dtype or c.shape[1:] != self._coords[0].shape[1:]):
            # (the reference's resizable h5 dataset keeps the dtype of the first batch and would cast silently: refuse instead)
            raise TypeError(f"slide {self.slide_id}: coords {c.dtype}{list(c.shape[1:])} after {self._coords[0].dtype}{list(self._coords[0].shape[1:])}")
        self._feats.append(f)
        self._coords.append(np.array(c, copy=True))  # (the caller may reuse its buffer)

    def __len__(self) -> int:
        return sum(f.shape[0] for f in self._feats)

    def close(self) -> str:
        if not self._feats:
            raise ValueError(f"slide {self.slide_id}: nothing was appended")
        feats, coords = torch.cat(self._feats, 0), np.concatenate(self._coords, 0)
        for d in ("pt_files", "coords_files"):
            os.makedirs(os.path.join(self.feat_dir, d), exist_ok=True)
        # coordinates first: a slide counts as finished when its .pt exists (the auto-skip looks at pt_files only), so the .pt is
        # written last and both files go through a rename -- a run killed in between leaves no half-written finished slide
        cpath = coords_path(self.feat_dir, self.slide_id)
        with open(cpath + ".tmp", "wb") as fh:
            np.save(fh, coords, allow_pickle=False)
        os.replace(cpath + ".tmp", cpath)
        if self.write_h5:
            import h5py
            os.makedirs(os.path.join(self.feat_dir, "h5_files"), exist_ok=True)
            with h5py.File(os.path.join(self.feat_dir, "h5_files", self.slide_id + ".h5"), "w") as fh:
                for key, val in (("features", feats.numpy()), ("coords", coords)):
                    fh.create_dataset(key, data=val, maxshape=(None,) + val.shape[1:], chunks=(1,) + val.shape[1:])
        pt = os.path.join(self.feat_dir, "pt_files", self.slide_id + ".pt")
        torch.save(feats, pt + ".tmp")  # extract_features_fp.py:255: the tensor itself, nothing else
        os.replace(pt + ".tmp", pt)
        return pt


def coords_path(feat_dir: str, slide_id: str) -> str:
    return os.path.join(feat_dir, "coords_files", slide_id + ".npy")


def load_coords(feat_dir: str, slide_id: str) -> np.ndarray:
    """The slide's ``coords [n, 2]`` exactly as they were appended (dtype and bits); row i belongs to row i of
    ``pt_files/{slide}.pt``.  Reads the sidecar, or the reference's ``h5_files/{slide}.h5`` where only that exists."""
    p = coords_path(feat_dir, slide_id)
    if os.path.isfile(p):
        return np.load(p, allow_pickle=False)
    h5 = os.path.join(feat_dir, "h5_files", slide_id + ".h5")
    if os.path.isfile(h5):
        try:
            import h5py
        except ImportError as e:
            raise FileNotFoundError(f"{p} is missing and {h5} needs h5py, which this host lacks") from e
        with h5py.File(h5, "r") as fh:
            return fh["coords"][:]
    raise FileNotFoundError(f"no coordinates for slide {slide_id} under {feat_dir} (coords_files/ or h5_files/)")


class _HostFeed:
    """The H2D hop of the driver loop (extract_features_fp.py:162-166: ``batch = batch.to(device, non_blocking=True)`` from whatever memory
    the loader hands over; HIPT_4K/hipt_4k.py:69).  Loader batches that live in HOST memory are copied into one of two device gather
    buffers on a COPY stream while the previous gathered call computes: pinned sources (``DataLoader(pin_memory=True)``) straight from
    where they lie, pageable ones through a pinned staging buffer of the same shape (one host memcpy, then the same asynchronous copy).
    Events order the three parties: a gather buffer is refilled only after the call that read it has finished (``free``), a call starts only
    after its copies have landed (``ready``), a staging buffer is rewritten only after its last copy out has completed.  No extra device
    copy: the gather buffer IS the tensor the model call reads."""

    SLOTS = 2

    def __init__(self, device: torch.device):
        self.device = device
        # HIGH-PRIORITY streams: HIP multiplexes a process's streams over a few hardware queues (four by default), and a copy whose stream shares
        # an in-order hardware queue with a compute stream starts only behind the ~26 ms of kernels already enqueued there -- measured in
        # bench.py's process (14 streams alive): 33.3 ms per gathered call against 27.3 for the same loop in a fresh process.  Priority
        # streams get hardware queues of their own.
        self.copy_stream = torch.cuda.Stream(device=device, priority=-1)
        self.buf = [None] * self.SLOTS       # device gather buffers [cap, ...]
        self.stage = [None] * self.SLOTS     # pinned staging twins (allocated only when a pageable batch arrives)
        self.free = [None] * self.SLOTS      # event: the call that read buf[s] has finished
        self.staged = [None] * self.SLOTS    # event: the last copy out of stage[s] has completed
        self.slot = self.fill = 0
        self.stage_waited = False            # the open gather has waited for staged[slot]

    def begin(self, cap: int, like: torch.Tensor):
        """start gathering up to `cap` regions shaped like `like` ([r, ...]) into the current slot"""
        s = self.slot
        shape = (cap,) + tuple(like.shape[1:])
        if self.buf[s] is None or self.buf[s].shape != shape or self.buf[s].dtype != like.dtype:
            self.buf[s] = torch.empty(shape, dtype=like.dtype, device=self.device)
            self.stage[s] = None
            # the block comes from the compute stream's pool: it may be one that work still enqueued there has just freed (the
            # augmented copy of the previous call, which is exactly this size); the copy stream writes it only after that work
            self.copy_stream.wait_stream(torch.cuda.current_stream(self.device))
        if self.free[s] is not None:
            self.copy_stream.wait_event(self.free[s])  # the compute that read this buffer two calls ago
        self.fill, self.stage_waited = 0, False

    def add(self, r: torch.Tensor):
        s, o, n = self.slot, self.fill, r.shape[0]
        dst = self.buf[s][o:o + n]
        src = r
        if not r.is_pinned():
            if self.stage[s] is None:
                self.stage[s] = torch.empty(self.buf[s].shape, dtype=self.buf[s].dtype, pin_memory=True)
            if self.staged[s] is not None and not self.stage_waited:  # the FIRST pageable batch of this gather, at whatever offset
                self.staged[s].synchronize()  # (long complete: its call has been launched and usually finished)
            self.stage_waited = True
            src = self.stage[s][o:o + n]
            src.copy_(r)  # host memcpy: pageable -> pinned
        with torch.cuda.stream(self.copy_stream):
            dst.copy_(src, non_blocking=True)
        self.fill = o + n

    def finish(self) -> torch.Tensor:
        """the gathered regions as a device tensor the CURRENT stream may read"""
        self.staged[self.slot] = ev = torch.cuda.Event()
        ev.record(self.copy_stream)
        torch.cuda.current_stream(self.device).wait_event(ev)
        return self.buf[self.slot][:self.fill]

    def release(self):
        """the call that read the finished gather has been enqueued on the current stream; the next gather takes the other slot"""
        self.free[self.slot] = ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self.slot = (self.slot + 1) % self.SLOTS


class _ResidentFeed:
    """The same four calls for loader batches that already lie where ``model`` reads them (and for any model that is not on a HIP device): a
    lone batch passes through as the tensor it is; several are gathered in ONE buffer, each loader batch dropped as soon as it is copied --
    the peak is the gathered batch plus one loader batch (8 fp32 4096 x 4096 regions: 1.6 GB + 0.2 GB), not two copies of everything."""

    def begin(self, cap: int, like: torch.Tensor):
        self.parts = []

    def add(self, r: torch.Tensor):
        self.parts.append(r)

    def finish(self) -> torch.Tensor:
        parts, self.parts = self.parts, None
        if len(parts) == 1:
            return parts.pop()
        out = torch.empty((sum(r.shape[0] for r in parts),) + tuple(parts[0].shape[1:]), dtype=parts[0].dtype, device=parts[0].device)
        o = 0
        while parts:
            r = parts.pop(0)
            out[o:o + r.shape[0]].copy_(r)
            o += r.shape[0]
        return out

    def release(self):
        pass


class _ReadBack:
    """Features of a finished call as a host tensor, without waiting for anything enqueued after that call (a `.cpu()` on the compute stream
    would wait for the NEXT call too, and the host could not feed the one after it meanwhile).  Everything is taken from the tensor it is
    given: the copy runs on a high-priority read stream of ``feats.device`` (one per device seen), behind ``done`` -- an event the caller
    recorded on THAT device's current stream once the call was enqueued -- so a model whose two ViTs sit on two devices needs no special case."""

    def __init__(self):
        self.streams = {}
        self.hbuf = None

    def __call__(self, outs: list, done: "torch.cuda.Event") -> list:
        return [self.one(feats, done) for feats in outs]

    def one(self, feats: torch.Tensor, done: "torch.cuda.Event") -> torch.Tensor:
        n = feats.shape[0]
        if self.hbuf is None or self.hbuf.shape[1:] != feats.shape[1:] or self.hbuf.shape[0] < n or self.hbuf.dtype != feats.dtype:
            self.hbuf = torch.empty((max(n, 8),) + tuple(feats.shape[1:]), dtype=feats.dtype, pin_memory=True)
        if feats.device not in self.streams:
            self.streams[feats.device] = torch.cuda.Stream(device=feats.device, priority=-1)
        rs = self.streams[feats.device]
        rs.wait_event(done)
        with torch.cuda.stream(rs):
            self.hbuf[:n].copy_(feats, non_blocking=True)
        feats.record_stream(rs)
        rs.synchronize()
        return self.hbuf[:n].clone()


class _CallPlan:
    """Which loader batches share a model call -- by their facts alone (no tensor, no device): ``add`` takes a batch's key
    ``(shape[1:], dtype, device)``, its region count, whether its shape is gathered (``gathers_bit_exactly``) and whether it is fed from the
    host to a HIP device, and answers (close the open call BEFORE this batch?, close it AFTER?).  Loader batches are never split."""

    def __init__(self, coalesce: int):
        self.coalesce = coalesce
        self.calls = 0   # closed so far
        self.n = 0       # regions in the open call (0: none open)
        self.key = None
        self.cap = 0     # what the open call's gather may hold

    def add(self, key, n: int, gatherable: bool, host_fed: bool):
        # a different shape / type / device cannot share a call, nor a host-fed batch that would overrun the open gather (a large one behind small ones)
        before = self.n > 0 and (key != self.key or (host_fed and self.n + n > self.cap))
        if before:
            self.calls, self.n = self.calls + 1, 0
        gathers = self.coalesce > 1 and gatherable
        if self.n == 0:
            # capacity: what a gathered call reaches with loader batches of this size, so that ragged tails re-use the host feed's buffer
            self.key, self.cap = key, (self.coalesce + n - 1 if gathers else n)
        self.n += n
        # host-fed: the FIRST call of a slide is a short one -- a quarter of `coalesce` -- so that the GPU starts behind 2 regions' copies instead
        # of 8; nothing hides the first call's copy, every later one lands under the call before it
        want = max(1, self.coalesce // 4) if (host_fed and self.calls == 0) else self.coalesce
        after = not gathers or self.n >= want
        if after:
            self.calls, self.n = self.calls + 1, 0
        return before, after


def extract_slide(model, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], feat_dir: str, slide_id: str, coalesce: int = 8) -> str:
    """The loop of ``compute_w_loader`` (extract_features_fp.py:159-171): ``batches`` yields ``(regions, coords)``;
    regions are whatever ``model`` takes — here ``[R, 3, W, H]`` float or raw ``uint8`` (planar or interleaved), R >= 1.

    The reference's loader yields ONE region per batch (``batch_size = 1``, extract_features_fp.py:128), and one region per
    call leaves the GPU a third idle (tile quantisation + launch latency of the small kernels: 175 regions/s against 285 at
    8+ regions per call).  Consecutive loader batches of the same shape and type are therefore gathered until ``coalesce``
    regions are at hand and go through ``model`` in ONE call; features and coordinates are appended in loader order, and a
    region's features do not depend on what else is in the call (rows are independent through every kernel), so the saved
    files are the ones the one-by-one loop writes -- bit for bit: only regions whose patch count is a multiple of 16 (4096 x 4096:
    256) are gathered, because both calls then take the same kernels (tested); other sizes go one loader batch per call.
    ``coalesce <= 1`` restores the one-by-one loop for everything.  Peak memory of a gathered call: the gathered batch plus one
    loader batch.

    **Host batches** (round 6; the reference's loader yields CPU tensors and moves each to the device inside the loop,
    extract_features_fp.py:162-166): when ``model`` is a ``HIPT_4K`` on a HIP device and a loader batch is not there, the batch
    is copied host -> device AS IT ARRIVES, on a copy stream, into one of two gather buffers while the previous call computes (``_HostFeed``),
    and the features of call k are read back (on a stream of their own) only after call k + 1 has been enqueued -- the link, the GPU and the host loop overlap.  Same
    gathered tensor, same kernels, same bits as with resident batches.

    ``model`` may also be a ``ResNet_Baseline`` (``--model_type resnet50``: patches ``[B, 3, H, W]``, features ``[B, 1024]``) or a
    ``ResNet18_Baseline`` (``--model_type resnet18``, features ``[B, 512]`` on the Histo route): host
    batches take the same copy-stream path (keyed on the model's ``weight_device``), and loader batches of any patch size are gathered
    up to ``coalesce`` patches per call -- bit-exact, since every output row depends on its own patch only."""
    w = FeatureWriter(feat_dir, slide_id)
    return _extract(model, batches, [w], lambda regions, first: [model(regions)], coalesce)[0]


def extract_slide_augmented(model, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], feat_dir: str, slide_id: str, policy: str,
                            n_augs: int, seed: int = 0, include_original: bool = True, coalesce: int = 8) -> list:
    """``extract_features_fp.py --use_transforms <policy>`` run ``n_augs`` times, plus the plain run, in ONE pass over the loader:
    every (gathered) call of ``extract_slide`` goes through ``model`` as it is -> ``pt_files/{slide}.pt`` (bit for bit what
    ``extract_slide`` writes; skipped when ``include_original`` is False) and then, for k = 1..n_augs, augmented on the device
    (``augment.RegionAugment(policy, seed)``: region i of the slide gets the parameters seeded by (seed, slide_id, k, i)) and
    through ``model`` again -> ``pt_files/{slide}aug{k}.pt``, the files ``Generic_MIL_Dataset(use_augs=True)`` reads
    (datasets/dataset_generic.py:497-507).  Each file has its coords sidecar.  Regions must be raw uint8 RGB (the reference
    augments before eval_transforms): float regions raise ``ValueError``.  Returns the written ``.pt`` paths, original first.

    ``policy`` ``"all"`` / ``"spatial"`` (the ResNet routes' two policies, ``tensor_augment.TensorAugment``) augment in tensor
    space: the augmented copy reaches ``model`` as the normalised float32 planar tensor the reference's Compose ends in, and the
    un-augmented file is still the model's plain run on the uint8 regions."""
    from .augment import POLICIES, RegionAugment
    from .tensor_augment import TENSOR_POLICIES, TensorAugment

    if policy not in POLICIES and policy not in TENSOR_POLICIES:
        raise ValueError(f"unknown augmentation policy {policy!r}; known: {sorted(POLICIES)} (uint8, before eval_transforms) and "
                         f"{sorted(TENSOR_POLICIES)} (tensor space, normalised float32 out)")
    if n_augs < 0 or (n_augs == 0 and not include_original):
        raise ValueError(f"n_augs={n_augs}, include_original={include_original}: nothing to write")
    aug = TensorAugment(policy, seed) if policy in TENSOR_POLICIES else RegionAugment(policy, seed)
    writers = ([FeatureWriter(feat_dir, slide_id)] if include_original else []) + \
              [FeatureWriter(feat_dir, f"{slide_id}aug{k}") for k in range(1, n_augs + 1)]

    def run(regions, first):
        if regions.dtype != torch.uint8:
            raise ValueError(f"extract_slide_augmented: regions must be raw uint8 RGB (got {regions.dtype}); the reference augments "
                             f"before eval_transforms")
        out = [model(regions)] if include_original else []
        for k in range(1, n_augs + 1):
            out.append(model(aug(regions, slide_id, k, first)))
        return out

    return _extract(model, batches, writers, run, coalesce)


class NormalisedSlide(str):
    """The ``.pt`` path ``extract_slide_normalised`` wrote (a ``str``), with ``fallbacks``: how many regions had no stain plane."""
    fallbacks = 0


def extract_slide_normalised(model, batches: Iterable[Tuple[torch.Tensor, torch.Tensor]], feat_dir: str, slide_id: str, coalesce: int = 8,
                             reference_input: bool = True, **macenko_kw) -> str:
    """``extract_features_fp.py --use_transforms macenko``: the loop of ``extract_slide`` with every (gathered) call
    Macenko-normalised on the device (``macenko.macenko_normalize``) before it goes through ``model``.  Regions
    must be raw uint8 RGB (the stain model is fitted to the bytes): float regions raise ``ValueError``.

    ``reference_input=True`` feeds ``model`` what the reference's route feeds it: the planar float32 tensor ``normalised / 255``
    in [0, 1], with no mean / std normalisation after it.  ``False`` feeds the normalised uint8 images, which then take the
    model's usual eval transforms.  ``macenko_kw``: ``Io``, ``alpha``, ``beta``, ``target`` of ``macenko_normalize``.  An image's
    normalisation does not depend on the call it shares, so the file is the same for every ``coalesce``.

    Returns the ``.pt`` path as a ``NormalisedSlide``: a ``str`` whose attribute ``fallbacks`` is the number of regions that fell
    back (no stain plane: passed on unchanged, as the reference's ``except`` does) -- counted on the device, read once after the
    loop.  Nothing is kept outside the returned value."""
    from .macenko import macenko_normalize

    bad = set(macenko_kw) - {"Io", "alpha", "beta", "target"}
    if bad:
        raise TypeError(f"extract_slide_normalised: unknown arguments {sorted(bad)}")
    counts = []

    def run(regions, first):
        if regions.dtype != torch.uint8:
            raise ValueError(f"extract_slide_normalised: regions must be raw uint8 RGB (got {regions.dtype}); the reference normalises "
                             f"the image before any other transform")
        x, status = macenko_normalize(regions, out_dtype=torch.float32 if reference_input else torch.uint8, return_status=True, **macenko_kw)
        counts.append(status.sum())
        return [model(x)]

    path = NormalisedSlide(_extract(model, batches, [FeatureWriter(feat_dir, slide_id)], run, coalesce)[0])
    path.fallbacks = int(torch.stack(counts).sum()) if counts else 0
    return path


def _is_resnet(model) -> bool:
    from .resnet18 import ResNet18_Baseline
    from .resnet_custom import ResNet_Baseline
    return isinstance(model, (ResNet_Baseline, ResNet18_Baseline))


def gathers_bit_exactly(regions: torch.Tensor, is_resnet: bool) -> bool:
    """whole 16-row fragments in every call (patch count a multiple of 16): the gathered call and the one-by-one call take the same kernels
    and write the same bits; other region sizes are NOT gathered (they would agree to the bf16 bar only)"""
    if is_resnet:
        return True  # every output row of hipt_resnet_forward depends on its own patch only, whatever the batch
    if regions.dim() != 4:
        return False
    hw = regions.shape[2:] if regions.shape[1] == 3 else regions.shape[1:3]  # planar [R,3,W,H] or interleaved [R,W,H,3]
    return ((hw[0] // 256) * (hw[1] // 256)) % 16 == 0


def _fed_calls(batches, plan: _CallPlan, dev: Optional[torch.device], resnet: bool):
    """Feeds the loader's batches to where the model reads them AS THEY ARRIVE and yields ``(feed, held)`` each time the plan closes a
    call: the feed whose ``finish()`` is the call's regions, and the ``(coords, count)`` of its loader batches."""
    resident, host = _ResidentFeed(), None  # (the _HostFeed is made when the first host batch for a HIP model arrives)
    feed, held = None, []
    for regions, coords in batches:
        host_fed = dev is not None and dev.type == "cuda" and regions.device.type == "cpu"
        before, after = plan.add((tuple(regions.shape[1:]), regions.dtype, regions.device), regions.shape[0],
                                 gathers_bit_exactly(regions, resnet), host_fed)
        if before:
            yield feed, held
            held = []
        if not held:
            if host_fed and host is None:
                host = _HostFeed(dev)
            feed = host if host_fed else resident
            feed.begin(plan.cap, regions)
        feed.add(regions)  # (a host batch's copy starts NOW)
        held.append((coords, regions.shape[0]))
        if after:
            yield feed, held
            held = []
    if held:
        yield feed, held


def _append_call(writers, held, outs) -> None:
    for w, feats in zip(writers, outs):
        o = 0
        for coords, n in held:  # one append per loader batch, as the reference's loop does
            w.append(feats[o:o + n], coords)
            o += n


def _extract(model, batches, writers, run, coalesce: int) -> list:
    """the loop of ``extract_slide``; ``run(regions, first)`` -> one feature tensor per writer for a call whose regions are
    regions ``first, first+1, ...`` of the slide (in loader order).  Three owners: ``_CallPlan`` says which loader batches share a call,
    a feed (``_ResidentFeed`` / ``_HostFeed``) brings them to the device, ``_ReadBack`` brings a host-fed call's features home one call late."""
    resnet = _is_resnet(model)
    # HIPT_4K: where its first-level ViT's weights live NOW (.to() may have moved it since construction)
    dev = model.weight_device if resnet else getattr(getattr(model, "model256", None), "weight_device", None)
    read_back = _ReadBack()
    pending = None  # (held, features on their device, done) of a host-fed call: read back after the NEXT call is enqueued
    first = 0
    with torch.no_grad():
        for feed, held in _fed_calls(batches, _CallPlan(coalesce), torch.device(dev) if dev is not None else None, resnet):
            regions = feed.finish()
            outs = run(regions, first)
            feed.release()
            del regions
            first += sum(n for _, n in held)
            late, pending = pending, None
            if isinstance(feed, _HostFeed):  # the GPU never waits for the host
                # `done` goes where the FEATURES are, which need not be where the regions went (every output of `run` is on ONE device)
                pending = (held, outs, torch.cuda.Event())
                pending[2].record(torch.cuda.current_stream(outs[0].device))
            if late is not None:
                _append_call(writers, late[0], read_back(*late[1:]))
            if pending is None:
                _append_call(writers, held, outs)
        if pending is not None:
            _append_call(writers, pending[0], read_back(*pending[1:]))
    return [w.close() for w in writers]


def load_bag(data_dir: str, slide_id: str, max_patches_per_slide: Optional[int] = None, rng=None, number_of_augs: int = 0,
             perturb_variance: Optional[float] = None) -> torch.Tensor:
    """``datasets/dataset_generic.py:497-526``: the slide's ``[n, d]`` features, sub-sampled WITH replacement to
    ``max_patches_per_slide`` rows when it has more (``rng``: a ``numpy.random.Generator`` / ``RandomState`` for
    reproducible draws; default ``np.random`` as the reference).

    ``number_of_augs > 0`` (``use_augs``): first draws k uniformly in ``[0, number_of_augs]`` (``rng`` or, by default, Python's
    ``random.randint`` as the reference) and reads ``{slide}aug{k}.pt`` for k > 0, the plain file for k = 0.
    ``perturb_variance`` (``use_perturbs``): adds ``torch.randn_like(features) * perturb_variance`` after the sub-sampling."""
    if number_of_augs > 0:
        if rng is None:
            import random
            k = random.randint(0, number_of_augs)
        else:
            k = int(rng.integers(0, number_of_augs + 1)) if hasattr(rng, "integers") else int(rng.randint(0, number_of_augs + 1))
        if k > 0:
            slide_id = f"{slide_id}aug{k}"
    path = os.path.join(data_dir, "pt_files", f"{slide_id}.pt")
    try:
        features = torch.load(path)
    except Exception as e:  # the reference asserts with the slide name
        raise AssertionError(f"Error caused by slide {slide_id}") from e
    if max_patches_per_slide is not None and max_patches_per_slide < len(features):
        idx = (rng if rng is not None else np.random).choice(len(features), max_patches_per_slide)
        features = features[torch.as_tensor(np.asarray(idx), dtype=torch.int64)]
    if perturb_variance is not None:
        features = features + torch.randn_like(features) * perturb_variance
    return features
