"""fp64 reference, derived error bound, pixel classes and wrong-kernel variants for the implicit-GEMM convolution of
``csrc/resnet.hip`` (CPU only; tests/test_conv_ref.py tests it, and a per-launch GPU test is to compare the kernels with it: DESIGN.md 11.6).

The model of the kernel
-----------------------
One output element is ``relu?(sum_k x[k] * w[k] + bias + resid)`` with k over the K = kh * kw * cin taps in (ky, kx, ci) order.
The operands are taken AS THE KERNEL READS THEM: ``x`` and ``resid`` already in the compute dtype, ``w`` the packed [cout, kp] image
(BN folded, rounded to the compute dtype, zero in [K, kp)), ``bias`` the packed fp32 bias.  Given those, the kernel has two error
sources only:

* accumulation in fp32: the K products and the two epilogue adds (bias, residual).  A product of two bf16 values is exact in fp32;
  a product of two fp32 values costs one rounding.  Each add may lose one fp32 ulp of the running magnitude, which is at most
  ``S = sum_k |x[k]| |w[k]| + |bias| + |resid|``.  Whether the matrix unit's adder rounds or truncates has not been measured on this
  part, so an ulp is taken as 2^-23 (truncation) and not 2^-24 (round to nearest); that factor of two also pays for the fp32
  products, and the ``+ 4`` for the epilogue adds and the second-order terms.
* one rounding of the result to the compute dtype, and nothing in fp32 (the accumulator is fp32).  bf16 has 8 significand bits, so
  its ulp in [2^e, 2^(e+1)) is 2^(e-7) and half of it is at most 2^-8 |y| (reached at the bottom of the binade; 2^-9 |y| is what it
  falls to at the top, and as a bound it fails for the correctly rounding kernel: tests/test_conv_ref.py).  2^-133 is the smallest
  bf16 subnormal.

Hence, per element, with ``y`` the unrounded fp64 result:

    bf16: |got - y| <= 2^-8 |y| + (K + 4) 2^-23 S + 2^-133
    fp32: |got - y| <=            (K + 4) 2^-23 S

``emulate`` is the right kernel in NumPy (fp32 accumulation slab by slab, fp32 epilogue, one rounding); tests/test_conv_ref.py holds
it to the bound on every form, which is the check that the model is not too tight, and holds every entry of ``VARIANTS`` (a wrong
kernel written the same way) to exceed it at least threefold, which is the check that it is not too loose.
"""
import numpy as np

SLAB = {"fp32": 32, "bf16": 64}   # elements of one 128-byte K slab


# ---- rounding ---------------------------------------------------------------------------------------------------------------
def round_bf16(a):
    """fp64 -> nearest bf16 (ties to even, 8 significand bits, subnormals down to 2^-133), returned as fp64; one rounding"""
    a = np.asarray(a, np.float64)
    _, e = np.frexp(a)
    q = np.ldexp(1.0, np.maximum(e, -125) - 8)
    return np.rint(a / q) * q


def round_to(a, dtype):
    """fp64 -> the compute dtype, returned as fp64"""
    return round_bf16(a) if dtype == "bf16" else np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def ulp(a, dtype):
    """the spacing of the compute dtype at ``a``"""
    a = np.abs(np.asarray(a, np.float64))
    if dtype == "fp32":
        return np.spacing(a.astype(np.float32)).astype(np.float64)
    _, e = np.frexp(a)
    return np.ldexp(1.0, np.maximum(e, -125) - 8)


# ---- the fold rule -------------------------------------------------------------------------------------------------------
def fold(weight, gamma, beta, mean, var, eps):
    """The BN fold in fp64: (w * scale, beta - mean * scale) with scale = gamma / sqrt(var + eps), every operand the fp32 value the
    pack kernel is given (eps included)."""
    f = lambda t: np.asarray(t, np.float32).astype(np.float64)
    scale = f(gamma) / np.sqrt(f(var) + float(np.float32(eps)))
    return f(weight) * scale[:, None, None, None], f(beta) - f(mean) * scale


def pack(weight, gamma, beta, mean, var, eps, dtype):
    """The fold rule, stated once: the packed image is the fp64 fold rounded once to fp32 and, for bf16, once more to bf16, laid out
    [cout, kp] in (ky, kx, ci) order with zeros in [K, kp); the bias is the fp64 fold rounded once to fp32.  Returns both as fp64."""
    wf, bf = fold(weight, gamma, beta, mean, var, eps)
    cout, cin, kh, kw = wf.shape
    K, kb = cin * kh * kw, SLAB[dtype]
    kp = (K + kb - 1) // kb * kb
    img = np.zeros((cout, kp))
    w32 = wf.astype(np.float32).astype(np.float64)
    img[:, :K] = (round_bf16(w32) if dtype == "bf16" else w32).transpose(0, 2, 3, 1).reshape(cout, K)
    return img, bf.astype(np.float32).astype(np.float64)


def check_packed(img, bias, op, dtype):
    """what a pack kernel wrote (``img`` [cout, kp], ``bias`` [cout], as fp64) against the fold rule of ``op``'s tensors"""
    want_w, want_b = pack(op["weight"], op["gamma"], op["beta"], op["mean"], op["var"], op["eps"], dtype)
    img, bias = np.asarray(img, np.float64), np.asarray(bias, np.float64)
    assert img.shape == want_w.shape and bias.shape == want_b.shape, (img.shape, want_w.shape)
    bad = np.argwhere(img != want_w)
    assert not len(bad), f"{len(bad)} packed weights off the fold rule, first at {tuple(bad[0])}: {img[tuple(bad[0])]!r} != {want_w[tuple(bad[0])]!r}"
    _, fb = fold(op["weight"], op["gamma"], op["beta"], op["mean"], op["var"], op["eps"])
    assert bool((np.abs(bias - fb) <= 2.0 ** -24 * np.abs(fb) + 2.0 ** -149).all()), float(np.abs(bias - fb).max())
    dead = np.asarray(op["gamma"]) == 0
    assert not img[dead].any(), "a dead channel's packed weights are not exactly 0"


# ---- the reference -----------------------------------------------------------------------------------------------------------
def out_hw(h, w, kh, kw, stride, pad):
    return (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1


def _unpack(w_stored, cin, kh, kw):
    w_stored = np.asarray(w_stored, np.float64)
    K = cin * kh * kw
    assert w_stored.ndim == 2 and w_stored.shape[1] >= K, w_stored.shape
    assert not w_stored[:, K:].any(), "the packed image is not zero beyond K"
    return w_stored[:, :K]


def gather(x, kh, kw, stride, pad, mode="right", swap=False):
    """The loader as a matrix: A [M, K] fp64, row m the K operands of output pixel m in (ky, kx, ci) order, 0 for a padding tap.
    ``mode``: "right"; "wrap_x" (no horizontal bounds check: the tap lands on the neighbouring row's pixel); "bleed_y" (no vertical
    check: the tap lands in the adjacent image; zero only outside the whole batch).  ``swap``: tap t read with (ky, kx) transposed, at (t % kh, t // kh)
    instead of (t // kw, t % kw); on a 1 x k or k x 1 kernel that is the same tap (ky or kx is always 0) and no wrong kernel at all,
    so there the swap is the decode with kh and kw exchanged, (t // kh, t % kh): the kernel read along the other axis."""
    x = np.asarray(x, np.float64)
    n, h, w, cin = x.shape
    oh, ow = out_hw(h, w, kh, kw, stride, pad)
    b, oy, ox = np.meshgrid(np.arange(n), np.arange(oh), np.arange(ow), indexing="ij")
    b, oy, ox = b.reshape(-1), oy.reshape(-1), ox.reshape(-1)
    flat = x.reshape(n * h * w, cin)
    A = np.zeros((n * oh * ow, kh * kw, cin))
    for t in range(kh * kw):
        ky, kx = (t // kw, t % kw)
        if swap:
            ky, kx = (t % kh, t // kh) if kh == kw else (t // kh, t % kh)
        iy, ix = oy * stride - pad + ky, ox * stride - pad + kx
        lin = (b * h + iy) * w + ix
        inside = (lin >= 0) & (lin < n * h * w)
        yok, xok = (iy >= 0) & (iy < h), (ix >= 0) & (ix < w)
        ok = {"right": yok & xok, "wrap_x": yok & inside, "bleed_y": xok & inside}[mode]
        A[ok, t] = flat[lin[ok]]
    return A.reshape(n * oh * ow, kh * kw * cin)


def conv_exact(x, w_stored, bias, resid, relu, kh, kw, stride, pad):
    """(y, S), both [n, oh, ow, cout] fp64: y the unrounded ``relu?(conv + bias + resid)`` of the operands as the kernel reads them
    (``w_stored`` the packed [cout, kp] image), S the sum of the magnitudes of all its terms at the same element."""
    x = np.asarray(x, np.float64)
    n, h, w, cin = x.shape
    W = _unpack(w_stored, cin, kh, kw)
    bias = np.asarray(bias, np.float64)
    oh, ow = out_hw(h, w, kh, kw, stride, pad)
    A = gather(x, kh, kw, stride, pad)
    y = (A @ W.T + bias).reshape(n, oh, ow, -1)
    S = (np.abs(A) @ np.abs(W).T + np.abs(bias)).reshape(n, oh, ow, -1)
    if resid is not None:
        r = np.asarray(resid, np.float64)
        y, S = y + r, S + np.abs(r)
    return (np.maximum(y, 0.0) if relu else y), S


def bound(y, S, K, dtype):
    """the per-element bound on |got - y| of the module docstring"""
    acc = (K + 4) * 2.0 ** -23 * np.asarray(S, np.float64)
    return acc if dtype == "fp32" else 2.0 ** -8 * np.abs(y) + acc + 2.0 ** -133


def emulate(x, w_stored, bias, resid, relu, kh, kw, stride, pad, dtype):
    """What the RIGHT kernel stores: fp32 accumulation slab by slab over the zero-padded K in (ky, kx, ci) order, fp32 bias and
    residual adds, ReLU, one rounding to the compute dtype.  Returned as fp64."""
    x = np.asarray(x, np.float64)
    n, h, w, cin = x.shape
    W = np.asarray(w_stored, np.float64).astype(np.float32)
    kp, kb = W.shape[1], SLAB[dtype]
    assert kp % kb == 0
    G = gather(x, kh, kw, stride, pad).astype(np.float32)
    A = np.zeros((G.shape[0], kp), np.float32)
    A[:, :G.shape[1]] = G
    acc = np.zeros((A.shape[0], W.shape[0]), np.float32)
    for k0 in range(0, kp, kb):
        acc = acc + A[:, k0:k0 + kb] @ W[:, k0:k0 + kb].T
    acc = acc + np.asarray(bias, np.float32)
    if resid is not None:
        acc = acc + np.asarray(resid, np.float64).astype(np.float32).reshape(acc.shape)
    if relu:
        acc = np.maximum(acc, np.float32(0))
    oh, ow = out_hw(h, w, kh, kw, stride, pad)
    return round_to(acc.astype(np.float64), dtype).reshape(n, oh, ow, -1)


# ---- pixel classes --------------------------------------------------------------------------------------------------------------
def pixel_classes(n, oh, ow, h, w, kh, kw, stride, pad):
    """Boolean masks over the M = n * oh * ow output pixels (row-major in (image, oy, ox), the kernel's row order):
    interior   no padding tap
    edge       at least one padding tap
    corner     a vertical and a horizontal padding tap
    seam       a vertical padding tap that, addressed without the bounds check, lands in the NEIGHBOURING image: the top rows of
               every image but the first, the bottom rows of every image but the last
    tile_tail64 / tile_tail128   the rows of the ragged last tile under that tile height (empty if M is a multiple of it)
    tile_seam  the rows within +-1 of each multiple of 64 inside (0, M): the first and last rows of neighbouring tiles
    """
    b, oy, ox = np.meshgrid(np.arange(n), np.arange(oh), np.arange(ow), indexing="ij")
    b, oy, ox = b.reshape(-1), oy.reshape(-1), ox.reshape(-1)
    M = n * oh * ow
    top, bottom = oy * stride - pad < 0, oy * stride - pad + kh - 1 >= h
    left, right = ox * stride - pad < 0, ox * stride - pad + kw - 1 >= w
    edge = top | bottom | left | right
    m = np.arange(M)
    near = np.zeros(M, bool)
    for j in range(64, M, 64):
        near |= np.abs(m - j) <= 1
    cls = {"interior": ~edge, "edge": edge, "corner": (top | bottom) & (left | right),
           "seam": (top & (b > 0)) | (bottom & (b < n - 1)), "tile_seam": near}
    for bm in (64, 128):
        cls["tile_tail%d" % bm] = (m >= M // bm * bm) & (M % bm != 0)
    return cls


# ---- forms -------------------------------------------------------------------------------------------------------------------------
class Form:
    """One launch shape: (cin, cout, kh, kw, stride, pad, n, h, w), the operand families it runs beyond ``plain`` and ``relu_map``,
    and the pixel classes it must populate."""

    def __init__(self, shape, classes, extra=(), why=""):
        self.cin, self.cout, self.kh, self.kw, self.stride, self.pad, self.n, self.h, self.w = shape
        self.shape, self.classes, self.why = tuple(shape), tuple(classes), why
        self.families = ("plain", "relu_map") + tuple(extra)
        self.oh, self.ow = out_hw(self.h, self.w, self.kh, self.kw, self.stride, self.pad)
        self.M, self.K = self.n * self.oh * self.ow, self.cin * self.kh * self.kw
        self.id = "c{}-{}k{}x{}s{}p{}_{}x{}x{}".format(*shape)
        self.geom = (self.kh, self.kw, self.stride, self.pad)

    def pixel_classes(self):
        return pixel_classes(self.n, self.oh, self.ow, self.h, self.w, *self.geom)

    def bn_cols(self):
        """output channels per workgroup tile (launch_conv's rule)"""
        return 128 if self.cout % 128 == 0 else 64


_EIS = ("interior", "edge", "corner", "seam")
FORMS = [
    Form((3, 64, 7, 7, 2, 3, 2, 38, 30), _EIS + ("tile_tail64", "tile_tail128", "tile_seam"), why="stem: gather, K = 147 padded to 160 / 192"),
    Form((3, 64, 7, 7, 2, 3, 1, 32, 32), ("interior", "edge", "corner", "tile_seam"), why="stem on the smallest envelope"),
    Form((3, 64, 3, 3, 1, 1, 2, 9, 7), _EIS + ("tile_tail64", "tile_tail128", "tile_seam"), why="gather, K = 27, under one slab"),
    Form((96, 64, 1, 1, 1, 0, 2, 9, 7), ("interior", "tile_tail64", "tile_tail128", "tile_seam"), why="bf16 gathers with cin != 3"),
    Form((64, 192, 1, 1, 1, 0, 1, 13, 11), ("interior", "tile_tail64", "tile_tail128", "tile_seam"), extra=("bn_edges",),
         why="BN = 64, three column tiles"),
    Form((128, 384, 1, 1, 1, 0, 1, 9, 15), ("interior", "tile_tail64", "tile_tail128", "tile_seam"), why="BN = 128, three column tiles"),
    Form((64, 64, 3, 3, 1, 1, 1, 1, 1), ("edge", "corner", "tile_tail64", "tile_tail128"), why="M = 1"),
    Form((64, 64, 3, 3, 1, 1, 1, 7, 9), ("interior", "edge", "corner", "tile_tail64", "tile_tail128"), why="M = 63"),
    Form((64, 64, 3, 3, 1, 1, 1, 8, 8), ("interior", "edge", "corner", "tile_tail128"), why="M = 64"),
    Form((64, 64, 3, 3, 1, 1, 1, 5, 13), ("interior", "edge", "corner", "tile_tail64", "tile_tail128", "tile_seam"), why="M = 65"),
    Form((64, 64, 3, 3, 1, 1, 1, 1, 127), ("edge", "corner", "tile_tail64", "tile_tail128", "tile_seam"), why="M = 127"),
    Form((64, 64, 3, 3, 1, 1, 2, 8, 8), _EIS + ("tile_seam",), extra=("cancel", "bn_edges"), why="M = 128, the seam on a tile edge too"),
    Form((64, 64, 3, 3, 1, 1, 1, 3, 43), ("interior", "edge", "corner", "tile_tail64", "tile_tail128", "tile_seam"), why="M = 129"),
    Form((64, 128, 3, 3, 2, 1, 3, 8, 8), _EIS + ("tile_tail64", "tile_tail128"), why="stride 2, even map: no bottom / right padding tap"),
    Form((64, 128, 3, 3, 2, 1, 3, 17, 23), _EIS + ("tile_tail64", "tile_tail128", "tile_seam"), why="stride 2, odd map"),
    Form((64, 128, 1, 1, 2, 0, 2, 21, 17), ("interior", "tile_tail64", "tile_tail128", "tile_seam"), why="strided 1x1"),
    Form((1024, 256, 1, 1, 1, 0, 2, 5, 5), ("interior", "tile_tail64", "tile_tail128"), extra=("cancel",), why="K = 1024"),
    Form((256, 1024, 1, 1, 1, 0, 1, 5, 5), ("interior", "tile_tail64", "tile_tail128"), extra=("cancel",), why="eight column tiles"),
    Form((512, 512, 3, 3, 1, 1, 3, 2, 2), ("edge", "corner", "seam", "tile_tail64", "tile_tail128"), why="K = 4608, every pixel a corner"),
    Form((64, 64, 1, 3, 1, 1, 2, 6, 10), _EIS + ("tile_tail64", "tile_tail128", "tile_seam"), why="kh != kw"),
    Form((64, 64, 3, 1, 1, 1, 2, 6, 10), _EIS + ("tile_tail64", "tile_tail128", "tile_seam"), why="kh != kw"),
]
FORM = {f.id: f for f in FORMS}
# residual / ReLU combinations: none, c3 behind the identity, conv1 / conv2, the downsample-fed c3 before its ReLU
COMBOS = [(False, False), (True, True), (False, True), (True, False)]


# ---- operands -----------------------------------------------------------------------------------------------------------------
def _hash():
    from hipt_abmil_atec23_amd import synth
    return synth.hash_uniform_np


def operands(form, family, dtype):
    """The operands of one (form, family) as the caller hands them over: ``weight`` [cout, cin, kh, kw], the BN tensors and eps (all
    fp32), ``x`` [n, h, w, cin] and ``resid`` [n, oh, ow, cout] already in the compute dtype (as fp64).  The ``cancel`` residual
    depends on the packed image and comes from :func:`cancel_resid`.

    plain     everything uniform in [-1, 1) (the existing conv tests' operands)
    relu_map  x = max(0, u + 0.1), about 45 % exact zeros, four channels (as many as there are) scaled by 40; the residual a
              non-negative map of the conv result's size; weights as plain
    cancel    x and weights as plain
    bn_edges  x as relu_map; gains with every eighth channel negative and every sixteenth exactly 0, running_var 0 on channels
              3 mod 16 and 1e-12 on channels 5 mod 16 (eps decides the scale), running_mean up to +-50
    """
    u = _hash()
    f = form
    seed = 3000 + f.cin + f.cout + 7 * f.kh + 11 * f.kw + f.stride + f.M
    op = {"weight": u((f.cout, f.cin, f.kh, f.kw), seed, (6.0 / (f.cout * f.kh * f.kw)) ** 0.5), "gamma": u((f.cout,), seed + 1, 0.1, 1.0),
          "beta": u((f.cout,), seed + 2, 0.05), "mean": u((f.cout,), seed + 3, 0.2), "var": u((f.cout,), seed + 4, 0.5, 1.0),
          "eps": 1e-5}
    x, r = u((f.n, f.h, f.w, f.cin), seed + 5), u((f.n, f.oh, f.ow, f.cout), seed + 6)
    if family in ("relu_map", "bn_edges"):
        x = np.maximum(x + np.float32(0.1), np.float32(0))
        x[..., sorted({1 % f.cin, 5 % f.cin, 17 % f.cin, f.cin - 1})] *= np.float32(40)
        r = np.maximum(r + np.float32(0.1), np.float32(0)) * np.float32(2)
    if family == "bn_edges":
        c = np.arange(f.cout)
        op["gamma"] = np.where(c % 16 == 0, 0.0, np.where(c % 8 == 4, -op["gamma"], op["gamma"])).astype(np.float32)
        op["var"] = np.where(c % 16 == 3, 0.0, np.where(c % 16 == 5, 1e-12, op["var"])).astype(np.float32)
        op["mean"] = u((f.cout,), seed + 3, 50.0)
    op["x"], op["resid"] = round_to(x, dtype), round_to(r, dtype)
    return op


def cancel_resid(form, x, w_stored, bias, dtype):
    """``-(conv + bias rounded to the compute dtype) + 1e-3 u``, in the compute dtype: the stored result is about 1e-3 of its terms, so
    an epilogue that rounds before it adds the residual is off by far more than the result's own rounding"""
    c, _ = conv_exact(x, w_stored, bias, None, False, *form.geom)
    return round_to(-round_to(c, dtype) + 1e-3 * _hash()(c.shape, 4000 + form.M + form.cout).astype(np.float64), dtype)


# ---- wrong kernels ----------------------------------------------------------------------------------------------------------------
def _finish(acc, bias, resid, relu, dtype, shape):
    y = acc + np.asarray(bias, np.float64)
    if resid is not None:
        y = y + np.asarray(resid, np.float64).reshape(y.shape)
    if relu:
        y = np.maximum(y, 0.0)
    return round_to(y, dtype).reshape(shape)


def _variant(name, form, x, w_stored, bias, resid, relu, dtype, bm=128):
    """what the wrong kernel ``name`` stores for this call, as fp64 [n, oh, ow, cout]"""
    f = form
    W = _unpack(w_stored, f.cin, *f.geom[:2])
    bias = np.asarray(bias, np.float64)
    shape = (f.n, f.oh, f.ow, f.cout)
    A = gather(x, *f.geom, mode=name if name in ("wrap_x", "bleed_y") else "right", swap=name == "swap_taps")
    if name == "drop_last_slab":
        keep = (f.K - 1) // SLAB[dtype] * SLAB[dtype]
        A = np.concatenate([A[:, :keep], np.zeros_like(A[:, keep:])], 1)
    if name == "tail_row_pixel0":
        A = A.copy()
        A[f.M // bm * bm if f.M % bm else f.M:] = A[0]
    if name == "col_tile_zero":
        W = W[np.arange(f.cout) % f.bn_cols()]
    if name == "bias_fragment":
        bias = bias.copy()
        bias[-16:] = 0.0
    acc = A @ W.T
    if name == "round_before_resid":
        return _finish(round_to(acc + bias, dtype), 0.0, resid, relu, dtype, shape)
    if name == "relu_before_resid":
        return _finish(np.maximum(acc + bias, 0.0) if relu else acc + bias, 0.0, resid, False, dtype, shape)
    return _finish(acc, bias, resid, relu, dtype, shape)


VARIANTS = ("wrap_x", "bleed_y", "drop_last_slab", "tail_row_pixel0", "bias_fragment", "round_before_resid", "relu_before_resid",
            "swap_taps", "col_tile_zero")


def variant(name, *args, **kw):
    assert name in VARIANTS, name
    return _variant(name, *args, **kw)


# variant -> [(form id, family, (resid, relu), class it corrupts, tile height or None)]: where tests/test_conv_ref.py proves the catch
# (at least 3x the bound at some element of that class, in both dtypes).  ``all`` is every pixel.  round_before_resid is a different
# kernel in bf16 only: in fp32 the accumulator already is the compute dtype, so there the variant IS the right kernel and the host
# test holds it to the bound instead.
CATCHES = {
    "wrap_x": [("c64-64k3x3s1p1_2x8x8", "plain", (False, False), "edge", None),
               ("c3-64k7x7s2p3_2x38x30", "relu_map", (False, True), "edge", None),
               ("c64-64k1x3s1p1_2x6x10", "plain", (False, False), "edge", None)],
    "bleed_y": [("c64-64k3x3s1p1_2x8x8", "plain", (False, False), "seam", None),
                ("c64-128k3x3s2p1_3x17x23", "relu_map", (True, True), "seam", None),
                ("c64-64k3x1s1p1_2x6x10", "plain", (False, False), "seam", None)],
    "drop_last_slab": [("c3-64k7x7s2p3_2x38x30", "plain", (False, False), "interior", None),
                       ("c3-64k3x3s1p1_2x9x7", "relu_map", (False, True), "interior", None),
                       ("c1024-256k1x1s1p0_2x5x5", "plain", (False, False), "interior", None)],
    "tail_row_pixel0": [("c64-64k3x3s1p1_1x5x13", "plain", (False, False), "tile_tail64", 64),
                        ("c64-64k3x3s1p1_1x3x43", "relu_map", (True, True), "tile_tail128", 128),
                        ("c128-384k1x1s1p0_1x9x15", "plain", (False, False), "tile_tail128", 128)],
    "bias_fragment": [("c64-192k1x1s1p0_1x13x11", "plain", (False, False), "all", None),
                      ("c256-1024k1x1s1p0_1x5x5", "relu_map", (True, False), "all", None)],
    "round_before_resid": [("c256-1024k1x1s1p0_1x5x5", "cancel", (True, False), "all", None),
                           ("c1024-256k1x1s1p0_2x5x5", "cancel", (True, False), "all", None),
                           ("c64-64k3x3s1p1_2x8x8", "cancel", (True, True), "all", None)],
    "relu_before_resid": [("c64-64k3x3s1p1_2x8x8", "plain", (True, True), "all", None),
                          ("c256-1024k1x1s1p0_1x5x5", "cancel", (True, True), "all", None)],
    "swap_taps": [("c64-64k3x3s1p1_2x8x8", "plain", (False, False), "interior", None),
                  ("c64-64k1x3s1p1_2x6x10", "plain", (False, False), "all", None),
                  ("c64-64k3x1s1p1_2x6x10", "relu_map", (False, True), "all", None)],
    "col_tile_zero": [("c64-192k1x1s1p0_1x13x11", "plain", (False, False), "all", None),
                      ("c128-384k1x1s1p0_1x9x15", "relu_map", (False, True), "all", None),
                      ("c256-1024k1x1s1p0_1x5x5", "plain", (False, False), "all", None)],
}


# ---- pools -----------------------------------------------------------------------------------------------------------------------
def avgpool_bound(x):
    """AdaptiveAvgPool2d(1) as one fp32 sum in pixel order: hw adds of half an fp32 ulp of a running magnitude of at most
    hw * mean|x| each, then the division by hw: ``hw * 2^-24 * mean|x|`` per (image, channel); ``x`` [n, hw, c] fp64"""
    x = np.abs(np.asarray(x, np.float64))
    return x.shape[1] * 2.0 ** -24 * x.mean(1)
