"""Per-launch tests of the three base operators through the C ABI -- hipt_layernorm, hipt_linear, hipt_attention -- against the float64
references and the derived per-element bounds of tests/ops_ref.py.  Every operand and every output sits in a buffer
with 32 rows of NaN behind it and NaN in its stride gaps; every element of every case is held to its bound, every output must be
finite and every fence intact.  The launch lists name the branch each shape reaches (ops_ref.LN_LAUNCHES, linear_launches,
attention_launches).  Worst ratios are printed with -s."""
import numpy as np
import pytest
import torch

import ops_ref as R
from hipt_abmil_atec23_amd import _native as N

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY = 32  # rows of NaN behind every buffer
EPS = 1e-6
TDT = {R.F32: torch.float32, R.BF16: torch.bfloat16}


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


class Fenced:
    """rows x cols values at `stride` elements per row, `off` elements into a NaN-filled buffer that goes on for CANARY more rows.
    .view is the window a kernel may touch; intact() says that everything else still holds the NaN it was filled with."""

    def __init__(self, rows, cols, dtype, stride=None, off=0, data=None):
        stride = cols if stride is None else stride
        self.buf = torch.full((off + (rows + CANARY) * stride,), float("nan"), dtype=dtype, device=DEV)
        self.view = torch.as_strided(self.buf, (rows, cols), (stride, 1), off)
        inside = torch.zeros(self.buf.numel(), dtype=torch.bool, device=DEV)
        torch.as_strided(inside, (rows, cols), (stride, 1), off).fill_(True)
        self.outside = ~inside
        if data is not None:
            self.view.copy_(torch.from_numpy(np.ascontiguousarray(data)).to(DEV).to(dtype))
        self.before = self.buf.clone()

    def intact(self):
        o = _bits(self.buf)[self.outside]
        return torch.equal(o, _bits(torch.full_like(self.buf[:1], float("nan"))).expand_as(o))

    def unchanged(self):  # (operands: not one bit of the whole buffer moved)
        return torch.equal(_bits(self.buf), _bits(self.before))

    def numpy(self):
        return self.view.float().cpu().numpy().astype(np.float64)


def _stream():
    return N.stream_ptr(torch.device(DEV))


def _held(tag, got, ref, bound, classes=None):
    """every element finite and inside its bound; prints the worst ratio overall and per class"""
    assert np.isfinite(got).all(), f"{tag}: non-finite output"
    r = R.ratio(got, ref, bound)
    per = "" if not classes else "; " + ", ".join(f"{k} {r[m].max():.3f}" for k, m in classes.items() if m.any())
    print(f"\n{tag}: worst |err| / bound {r.max():.3f}{per}")
    i = np.unravel_index(r.argmax(), r.shape)
    assert r.max() <= 1.0, f"{tag}: element {i} is {r.max():.3f} x its bound (got {got[i]!r}, reference {ref[i]!r}, bound {bound[i]:.3e})"
    return float(r.max())


# =====================================================================================================================
# LayerNorm
# =====================================================================================================================
def run_layernorm(x, w, b, out_dtype, x_stride, x_off=0):
    rows, D = x.shape
    xf = Fenced(rows, D, torch.float32, x_stride, x_off, x)
    wf, bf = Fenced(1, D, torch.float32, data=w[None]), Fenced(1, D, torch.float32, data=b[None])
    of = Fenced(rows, D, TDT[out_dtype], D)
    before = N.calls
    N.call("hipt_layernorm", N.ptr(xf.view), x_stride, N.ptr(wf.view), N.ptr(bf.view), N.ptr(of.view), out_dtype, D, rows, D, EPS, _stream())
    torch.cuda.synchronize()
    assert N.calls == before + 1
    assert of.intact() and xf.unchanged() and wf.unchanged() and bf.unchanged(), "a fence or an operand was written"
    return of


@pytest.mark.parametrize("out_dtype", [R.F32, R.BF16], ids=["f32out", "bf16out"])
@pytest.mark.parametrize("i", range(len(R.LN_LAUNCHES)), ids=[f"D{D}-rows{r}-{s}-off{o}-{br}" for D, r, s, o, br in R.LN_LAUNCHES])
def test_layernorm_launch(i, out_dtype):
    D, rows, smode, xoff, branch = R.LN_LAUNCHES[i]
    xs = R.ln_stride(D, smode)
    assert f"V{R.ln_vector_width(D, xs, D, xoff)}" == branch
    x, w, b, cls = R.ln_inputs(rows, D, 100 + i)
    of = run_layernorm(x, w, b, out_dtype, xs, xoff)
    obf = out_dtype == R.BF16
    _held(f"layernorm D={D} rows={rows} x_stride={smode} off={xoff} {branch} {'bf16' if obf else 'fp32'}", of.numpy(),
          R.layernorm_ref(x, w, b, EPS), R.layernorm_bound(x, w, b, EPS, obf), {n: cls == k for k, n in enumerate(R.LN_CLASSES)})


@pytest.mark.parametrize("out_dtype", [R.F32, R.BF16], ids=["f32out", "bf16out"])
def test_layernorm_bits_do_not_depend_on_position_or_stream(out_dtype):
    D = 384
    x, w, b, _ = R.ln_inputs(6, D, 7)
    full = run_layernorm(x, w, b, out_dtype, D).view.clone()
    shifted = run_layernorm(x[1:], w, b, out_dtype, D).view  # every row one place earlier in its 4-row block
    assert torch.equal(_bits(shifted), _bits(full[1:]))
    s = torch.cuda.Stream(device=DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(s):
        again = run_layernorm(x, w, b, out_dtype, D).view
    assert torch.equal(_bits(again), _bits(full))
    # V = 1 (x one float into its buffer) against V = 2: both are held to the bound above; their summation orders differ
    v1 = run_layernorm(x, w, b, out_dtype, D, 1).view
    print(f"\nlayernorm V=1 against V=2, {'bf16' if out_dtype else 'fp32'} out: bit-equal {torch.equal(_bits(v1), _bits(full))}, "
          f"max |d| {float((v1.float() - full.float()).abs().max()):.3e}")
    obf = out_dtype == R.BF16
    _held("layernorm V=1 row block", v1.float().cpu().numpy().astype(np.float64), R.layernorm_ref(x, w, b, EPS), R.layernorm_bound(x, w, b, EPS, obf))


# =====================================================================================================================
# Linear
# =====================================================================================================================
def run_linear(a, w, bias, resid, dtype, flags, lds=None, out_bf16=False):
    M, K = a.shape
    Nn = w.shape[0]
    lda, ldw, ldc = lds or (K, K, Nn)
    af, wf = Fenced(M, K, TDT[dtype], lda, data=a), Fenced(Nn, K, TDT[dtype], ldw, data=w)
    bf = Fenced(1, Nn, torch.float32, data=bias[None])
    rf = Fenced(M, Nn, torch.float32, ldc, data=resid) if resid is not None else None
    of = Fenced(M, Nn, torch.bfloat16 if out_bf16 else torch.float32, ldc)
    before = N.calls
    N.call("hipt_linear", N.ptr(af.view), lda, N.ptr(wf.view), ldw, N.ptr(bf.view), N.ptr(rf.view if rf else None), N.ptr(of.view), ldc, M, Nn, K,
           dtype, flags, _stream())
    torch.cuda.synchronize()
    assert N.calls == before + 1
    assert of.intact() and af.unchanged() and wf.unchanged() and bf.unchanged() and (rf is None or rf.unchanged()), "a fence or an operand was written"
    return of


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("epi", list(R.EPILOGUES))
def test_linear_launches(epi, dtype):
    flags, act, res, obf = R.EPILOGUES[epi]
    obf = obf and dtype == R.BF16
    e = list(R.EPILOGUES).index(epi)
    worst = {}
    for i, (M, Nn, K, padded, branch) in enumerate(R.linear_launches(epi, dtype)):
        assert R.linear_branch(M, K, dtype) == branch
        a, w, bias, r, cancel = R.linear_inputs(M, Nn, K, 1000 * e + i, dtype == R.BF16, gelu=act == "gelu", resid=res)
        a = a[:-1]
        of = run_linear(a, w, bias, r, dtype, flags, R.linear_lds(Nn, K, dtype, padded), obf)
        h = R.linear_ref(a, w, bias)
        rows = np.broadcast_to(cancel[:, None], h.shape)
        classes = {"cancelling": rows, "ordinary": ~rows}
        if act == "gelu":
            classes.update({"|h|>8": np.abs(h) > 8, "h in [-8,-2]": (h >= -8) & (h <= -2)})
        tag = f"linear {epi} {'bf16' if dtype else 'fp32'} M={M} N={Nn} K={K}{' padded-ld' if padded else ''} {branch}"
        worst[branch] = max(worst.get(branch, 0.0), _held(tag, of.numpy(), R.linear_ref(a, w, bias, r, act), R.linear_bound(a, w, bias, r, act, obf), classes))
    assert set(worst) == {"ring", "guarded", "tiled"}
    print(f"\nlinear {epi} {'bf16' if dtype else 'fp32'}: worst per kernel {worst}")


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["fp32", "bf16"])
def test_linear_refuses_what_it_cannot_run(dtype):
    a, w, bias, _, _ = R.linear_inputs(16, 8, 64, 3, dtype == R.BF16)
    A, W = Fenced(17, 64, TDT[dtype], data=a), Fenced(8, 64, TDT[dtype], data=w)
    Bv, O = Fenced(1, 8, torch.float32, data=bias[None]), Fenced(16, 8, torch.float32)
    one = torch.as_strided(A.buf, (16, 64), (64, 1), 4 // A.buf.element_size())  # A four bytes off
    for args, text in (((N.ptr(A.view), 64, N.ptr(W.view), 64, N.ptr(Bv.view), None, N.ptr(O.view), 8, 16, 8, 48), "K=48 must be a multiple of"),
                       ((N.ptr(A.view), 64, N.ptr(W.view), 64, N.ptr(Bv.view), None, N.ptr(O.view), 8, 16, 6, 64), "N=6 must be a multiple of 4"),
                       ((N.ptr(one), 64, N.ptr(W.view), 64, N.ptr(Bv.view), None, N.ptr(O.view), 8, 16, 8, 64), "16-byte aligned")):
        with pytest.raises(RuntimeError, match=text):
            N.call("hipt_linear", *args, dtype, R.EPI_OUT_F32, _stream())
    torch.cuda.synchronize()
    assert O.unchanged() and A.unchanged()


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["fp32", "bf16"])
def test_linear_bits_do_not_depend_on_the_call_or_stream(dtype):
    """a row alone against the same row inside a larger call of the same kernel (ring, guarded, tiled); the same call on a second stream"""
    for K in ((192, 64) if dtype == R.F32 else (384, 128)):
        a, w, bias, _, _ = R.linear_inputs(1361, 132, K, 9, dtype == R.BF16)
        big = run_linear(a[:273], w, bias, None, dtype, R.EPI_OUT_F32).view.clone()
        for row in (0, 100, 272):
            alone = run_linear(a[row:row + 1], w, bias, None, dtype, R.EPI_OUT_F32).view
            assert torch.equal(_bits(alone[0]), _bits(big[row])), (K, row)
        tiled = run_linear(a[:1361], w, bias, None, dtype, R.EPI_OUT_F32).view.clone()
        head = run_linear(a[:1089], w, bias, None, dtype, R.EPI_OUT_F32).view
        assert torch.equal(_bits(head), _bits(tiled[:1089])), K
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            again = run_linear(a[:273], w, bias, None, dtype, R.EPI_OUT_F32).view
        assert torch.equal(_bits(again), _bits(big)), K


def gelu_sweep():
    """2^16 fp32 pre-activations: [-12, 12] evenly, and the 256 fp32 neighbours on either side of 0, +-8 and +-1e-4"""
    pts = []
    for c in (0.0, 8.0, -8.0, 1e-4, -1e-4):
        v = np.full(513, c, np.float32)
        for k in range(1, 257):
            v[256 + k] = np.nextafter(v[256 + k - 1], np.float32(np.inf))
            v[256 - k] = np.nextafter(v[256 - k + 1], np.float32(-np.inf))
        pts.append(v)
    pts = np.concatenate(pts)
    return np.concatenate([np.linspace(-12.0, 12.0, 65536 - len(pts)).astype(np.float32), pts])


def test_gelu_epilogue_constant():
    """measures c_g -- |gelu_device(h) - gelu(h)| / (2^-23 max(|h|, |gelu(h)|)) over the sweep, through hipt_linear with K = 32, W the
    identity and the GELU epilogue (h reaches the epilogue exactly) -- and holds it to ops_ref.C_G = 2 x the recorded measurement"""
    h = np.ascontiguousarray(gelu_sweep().reshape(32, 2048).T)  # (every row block spans the whole range)
    for M in (1024, 2048):  # the small kernel, the tiled kernel: one epilogue
        of = run_linear(h[:M], np.eye(32, dtype=np.float32), np.zeros(32, np.float32), None, R.F32, R.EPI_GELU | R.EPI_OUT_F32)
        got, h64 = of.numpy(), h[:M].astype(np.float64)
        g = R.gelu64(h64)
        c = np.abs(got - g) / (R.U * np.maximum(np.maximum(np.abs(h64), np.abs(g)), 2.0 ** -100))
        i = np.unravel_index(c.argmax(), c.shape)
        print(f"\ngelu epilogue M={M}: c_g measured {c.max():.3f} at h = {h64[i]!r} (recorded {R.C_G_MEASURED}, bar C_G = {R.C_G}); "
              f"per range: |h|<1e-3 {c[np.abs(h64) < 1e-3].max():.3f}, h<-2 {c[h64 < -2].max():.3f}, |h|<=2 {c[np.abs(h64) <= 2].max():.3f}, h>2 {c[h64 > 2].max():.3f}")
        assert np.isfinite(got).all() and c.max() <= R.C_G
    assert R.C_G <= 16.0  # (a measurement beyond 8 is a finding, not a bar)


# =====================================================================================================================
# Attention
# =====================================================================================================================
def run_attention(qkv, heads, dh, dtype, want_probs):
    B, ntok, C3 = qkv.shape
    qf = Fenced(B * ntok, C3, TDT[dtype], data=qkv.reshape(B * ntok, C3))
    of = Fenced(B * ntok, heads * dh, TDT[dtype])
    pf = Fenced(B * heads * ntok, ntok, torch.float32) if want_probs else None
    before = N.calls
    N.call("hipt_attention", N.ptr(qf.view), N.ptr(of.view), N.ptr(pf.view if pf else None), B, ntok, heads, dh, dh ** -0.5, dtype, _stream())
    torch.cuda.synchronize()
    assert N.calls == before + 1
    assert of.intact() and qf.unchanged() and (pf is None or pf.intact()), "a fence or an operand was written"
    return of, pf


_ATT = [(dh, bf, i) for dh in (32, 64) for bf in (False, True) for i in range(len(R.ATTN_NTOK))]


def _att_id(c):
    dh, bf, i = c
    B, ntok, heads, fam = R.attention_launches(dh, bf)[i]
    return f"dh{dh}-{'bf16' if bf else 'fp32'}-B{B}h{heads}-ntok{ntok}-{fam}-{R.attention_branch(ntok, dh, B, heads, bf, True)}|{R.attention_branch(ntok, dh, B, heads, bf, False)}"


@pytest.mark.parametrize("case", _ATT, ids=[_att_id(c) for c in _ATT])
def test_attention_launch(case):
    dh, bf, i = case
    B, ntok, heads, fam = R.attention_launches(dh, bf)[i]
    dtype, scale = (R.BF16 if bf else R.F32), dh ** -0.5
    qkv, key = R.attn_inputs(B, ntok, heads, dh, 300 + i, fam, bf)
    o_ref, p_ref = R.attention_ref(qkv, heads, scale)
    bo, bp = R.attention_bound(qkv, heads, scale, bf)
    rows = {"spiked rows": R.spike_rows(qkv, heads, scale, key)} if key is not None else None
    tag = f"attention dh={dh} {'bf16' if bf else 'fp32'} B={B} heads={heads} ntok={ntok} {fam}"
    of, pf = run_attention(qkv, heads, dh, dtype, True)
    _held(tag + " probs [" + R.attention_branch(ntok, dh, B, heads, bf, True) + "]", pf.numpy().reshape(p_ref.shape), p_ref, bp,
          {k: np.broadcast_to(m[..., None], p_ref.shape) for k, m in rows.items()} if rows else None)
    sums = pf.numpy().reshape(p_ref.shape).sum(-1)
    assert np.abs(sums - 1).max() <= (ntok + 4) * R.U, f"{tag}: a row of probabilities sums to 1 {np.abs(sums - 1).max():+.3e}"
    _held(tag + " out with probs", of.numpy().reshape(o_ref.shape), o_ref, bo)
    of2, _ = run_attention(qkv, heads, dh, dtype, False)
    branch = R.attention_branch(ntok, dh, B, heads, bf, False)
    _held(tag + " out alone [" + branch + "]", of2.numpy().reshape(o_ref.shape), o_ref, bo)
    same = torch.equal(_bits(of.view), _bits(of2.view))
    if branch.startswith("attn64"):  # its own exponent arithmetic: the same bits would mean the call took attention.hip's kernel
        ndiff = int((_bits(of.view) != _bits(of2.view)).sum())
        print(f"\n{tag}: the 64-wide-head kernel differs from attention.hip's in {ndiff} of {of.view.numel()} output values")
        assert B * heads < 48 or not same
    else:
        assert same, f"{tag}: out depends on whether probs is asked for"


@pytest.mark.parametrize("dtype", [R.F32, R.BF16], ids=["fp32", "bf16"])
def test_attention_refuses_289_tokens_and_second_stream_bits(dtype):
    qkv, _ = R.attn_inputs(1, 289, 2, 64, 5, "ordinary", dtype == R.BF16)
    qf, of = Fenced(289, 384, TDT[dtype], data=qkv[0]), Fenced(289, 128, TDT[dtype])
    with pytest.raises(RuntimeError, match=rf"code {R.E_UNSUPPORTED}: attention: ntok=289 exceeds"):
        N.call("hipt_attention", N.ptr(qf.view), N.ptr(of.view), None, 1, 289, 2, 64, 0.125, dtype, _stream())
    torch.cuda.synchronize()
    assert of.unchanged()
    for probs in (True, False):
        first, _ = run_attention(qkv[:, :273], 2, 64, dtype, probs)
        s = torch.cuda.Stream(device=DEV)
        s.wait_stream(torch.cuda.current_stream(DEV))
        with torch.cuda.stream(s):
            again, _ = run_attention(qkv[:, :273], 2, 64, dtype, probs)
        assert torch.equal(_bits(first.view), _bits(again.view))
