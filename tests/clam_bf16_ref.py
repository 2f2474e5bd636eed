"""fp64 restatement of the CLAM inference forward (models/model_clam.py:147-191, 226-264) with the bf16 mode's rounding points made
explicit, per ROUTE of the library: a reference for per-route parity tests of the CLAM kernels, with structured inputs, wrong-kernel
variants and the comparison statistics for them.  tests/test_clam_bf16_ref.py holds it to the oracle and to the restatements of the
ragged-bag GPU tests, on the CPU.

Arithmetic is float64 on whatever device the inputs live on; a value is rounded to bf16 (``vit_bf16_ref.bf16``) exactly where the
route's kernels round it, and nowhere else:

  stream  csrc/abmil32.hip abmil32_kernel<KS, 1> (CLAM_SB, bf16 [384 | 192, 128, 64], sum |wc| < 60).  The bag and W1 / Wa / Wb are bf16;
          the biases ride in the GEMMs as three bf16 pieces whose sum is the fp32 value (:94-101), wc is fp32 (:131-137): all exact.
          h1 = ReLU(W1 x + b1) is rounded to bf16 ONLY as the operand of the gate product (pack8, :391-392); the pooling adds
          p * Hp with the unrounded h1 (:386) and p = e^(A - bc) against the fixed shift (:349).  tanh's argument is clamped to
          +-15 (:362); tanh(x) sigmoid(y) = (E - 1) / (E (1 + F) + (1 + F)), which is 0 where F = e^-y overflows.
  mb      abmil32_kernel<KS, NB> + clam_mb_pool_kernel (CLAM_MB, 2 ... 4 branches): the logits as `stream`, one per branch; the
          pooling kernel reads h1 as the bf16 image the first pass left (:511, :868-871).
  fused   csrc/abmil.hip abmil_fused_kernel<bf16_t, ..> (a bf16 model whose logit bound is >= 60 or unknown): h1 -> bf16 once
          (store4, :166), operand of the gate product AND of the pooling; no clamp (tanh_f / sigmoid_f); the softmax weights
          p = exp(A - m) against the workgroup's RUNNING maximum m (tile t of 128 rows belongs to workgroup t mod min(tiles, 512))
          are rounded to bf16 and summed as rounded (:246-256).

``rnd=False`` switches every rounding point and the clamp off: oracle.hipt_oracle.clam_sb_forward, which the CPU tests hold it to.

``variant`` names a plausible wrong kernel (for sensitivity self-checks): the emulation with that one mistake.
The ones that depend on how the launcher deals the 32-row blocks to the waves take the compute-unit count ``ncu``."""
import numpy as np
import torch

from hipt_abmil_atec23_amd import synth
from vit_bf16_ref import bf16

S1, S2 = 128, 64
ROUTES = ("stream", "mb", "fused")
# the wrong kernels.  Every route: a bias never added (no_bc: to A_raw; no_b1 / no_ba / no_bb: in the GEMMs), two wc entries exchanged,
# the bag's last block (fused: last 128-row tile) never pooled, the rows past N of the last block pooled (stream / mb: as the zero rows the
# range-checked buffer returns; fused: as the copies of row N - 1 its clamped loads return), the pooling's h1 operand in the other
# route's precision.  stream / mb: the biases as ONE bf16 piece (mid / lo lost), every wave's drained (= last) block never finished,
# a block's weights meeting the h1 of the same wave's NEXT block.
VARIANTS = ("no_bc", "no_ba", "no_bb", "no_b1", "bias_hi", "wc_swap", "drop_last_block", "tail_rows", "drop_drain", "pool_prev_block",
            "pool_bf16_h1", "pool_f32_h1")
WC_SWAP = (3, 40)


def _id(t):
    return t


# ---- the launcher's block arithmetic (abmil32.hip launch<KS>: :717-723, the kernel's nstep :249) -------------------------------------
def launch_geometry(N: int, ncu: int = 256):
    """(nblocks, rounds, grid, nwaves): every wave gets ceil(nblocks / (4 min(CUs, 256))) blocks, to within one"""
    nblocks = (N + 31) // 32
    maxg = min(ncu, 256)
    rounds = (nblocks + 4 * maxg - 1) // (4 * maxg)
    grid = ((nblocks + rounds - 1) // rounds + 3) // 4
    return nblocks, rounds, grid, 4 * grid


def wave_steps(N: int, ncu: int = 256) -> np.ndarray:
    """blocks of wave gw = 0 .. nwaves - 1 (its blocks: gw, gw + nwaves, ..)"""
    nblocks, _, _, nwaves = launch_geometry(N, ncu)
    gw = np.arange(nwaves)
    return np.where(gw < nblocks, (nblocks - gw + nwaves - 1) // nwaves, 0)


def step_mix(N: int, ncu: int = 256) -> dict:
    """{blocks per wave: number of waves}.  A wave with s blocks runs the pipelined carry (gates + pooling of the block before under the
    MFMAs of the next) s - 1 times and the drain once; its re-requests one block ahead are live for s >= 2, two ahead for s >= 3."""
    s, c = np.unique(wave_steps(N, ncu), return_counts=True)
    return {int(a): int(b) for a, b in zip(s, c)}


def drained_rows(N: int, ncu: int = 256) -> torch.Tensor:
    """bool [32 nblocks]: rows of the blocks that are some wave's last"""
    nblocks, _, _, nwaves = launch_geometry(N, ncu)
    steps = wave_steps(N, ncu)
    last = np.zeros(nblocks, dtype=bool)
    gw = np.nonzero(steps > 0)[0]
    last[gw + (steps[gw] - 1) * nwaves] = True
    return torch.from_numpy(np.repeat(last, 32))


# ---- weights -----------------------------------------------------------------------------------------------------------------------
def params(sd, device="cpu", rnd: bool = True) -> dict:
    """fp64 tensors of a CLAM_SB / CLAM_MB state dict (torch or numpy values; no dropout: the gated head is attention_net.2): the
    matrices as the bf16 the kernels read, biases / wc / the bag classifier as fp32 -> fp64.  wc [K, 64], bc [K]; CLAM_SB: wcls [C, 128];
    CLAM_MB: wcls [K, 128] (row k = classifiers.k)."""
    t = lambda k: torch.as_tensor(sd[k]).detach().to(device).double()
    m = (lambda k: bf16(t(k))) if rnd else t
    g = "attention_net.2."
    p = {"w1": m("attention_net.0.weight"), "b1": t("attention_net.0.bias"), "wa": m(g + "attention_a.0.weight"), "ba": t(g + "attention_a.0.bias"),
         "wb": m(g + "attention_b.0.weight"), "bb": t(g + "attention_b.0.bias"), "wc": t(g + "attention_c.weight"), "bc": t(g + "attention_c.bias")}
    p["multi"] = "classifiers.0.weight" in sd
    if p["multi"]:
        K = p["wc"].shape[0]
        p["wcls"] = torch.cat([t(f"classifiers.{k}.weight") for k in range(K)], 0)
        p["bcls"] = torch.cat([t(f"classifiers.{k}.bias") for k in range(K)], 0)
    else:
        p["wcls"], p["bcls"] = t("classifiers.weight"), t("classifiers.bias")
    p["logit_bound"] = float(p["wc"].abs().sum(1).max())
    return p


# ---- the forward ---------------------------------------------------------------------------------------------------------------------
def forward(bag, p, route, rnd=True, variant=None, ncu=256, rows=16384) -> dict:
    """bag [N, S0] (any float dtype; read as the bf16 the kernels read) -> dict(A_raw [K, N], M [K, 128], logits [C], Y_prob [C], Y_hat,
    plus what the tests' coverage assertions need: neff [K], the effective row count (sum p)^2 / sum p^2 of each branch's softmax,
    frac_clamp, the fraction of tanh pre-activations beyond +-15, and frac_far, the fraction of sigmoid pre-activations below -88.8,
    where e^-y overflows fp32).  Row blocks of `rows` keep the fp64 temporaries small."""
    assert route in ROUTES and (variant is None or variant in VARIANTS), (route, variant)
    r = bf16 if rnd else _id
    v = variant
    x = r(bag.double())
    N, dev = x.shape[0], x.device
    unit = 128 if route == "fused" else 32  # the rows a workgroup / wave handles together
    npad = (N + unit - 1) // unit * unit
    if npad > N:  # what the kernels see past the bag: zeros (range-checked buffer) / row N - 1 again (clamped row index)
        pad = x[-1:].expand(npad - N, -1) if route == "fused" else torch.zeros(npad - N, x.shape[1], dtype=x.dtype, device=dev)
        x = torch.cat([x, pad])
    hi = (lambda b: bf16(b)) if v == "bias_hi" else _id
    b1 = torch.zeros_like(p["b1"]) if v == "no_b1" else hi(p["b1"])
    ba = torch.zeros_like(p["ba"]) if v == "no_ba" else hi(p["ba"])
    bb = torch.zeros_like(p["bb"]) if v == "no_bb" else hi(p["bb"])
    wc = p["wc"].clone()
    if v == "wc_swap":
        wc[:, list(WC_SWAP)] = wc[:, list(WC_SWAP[::-1])]
    pool_rounded = route != "stream"
    if v == "pool_bf16_h1":
        pool_rounded = True
    if v == "pool_f32_h1":
        pool_rounded = False
    gs, hps, n_clamp, n_far = [], [], 0, 0
    for s in range(0, npad, rows):
        h1 = torch.relu(x[s:s + rows] @ p["w1"].t() + b1)
        h1b = r(h1)  # the gate product's operand
        a, b = h1b @ p["wa"].t() + ba, h1b @ p["wb"].t() + bb
        n_clamp += int((a[:max(0, N - s)].abs() > 15).sum())
        n_far += int((b[:max(0, N - s)] < -88.8).sum())
        if rnd and route != "fused":
            a = a.clamp(-15.0, 15.0)
        gs.append((torch.tanh(a) * torch.sigmoid(b)) @ wc.t())  # A - bc [rows, K]
        hps.append(h1b if pool_rounded else h1)
    g, hp = torch.cat(gs), torch.cat(hps)
    K = wc.shape[0]
    A = g + (0.0 if v == "no_bc" else p["bc"])
    live = torch.arange(npad, device=dev) < N  # rows that weigh something
    if v == "tail_rows":
        live = torch.ones_like(live)
    if v == "drop_last_block":
        live = live & (torch.arange(npad, device=dev) < npad - unit)
    if v == "drop_drain" and route != "fused":
        drained = drained_rows(N, ncu).to(dev)
        if route == "stream":
            live = live & ~drained
        else:
            # several branches: the drain finishes the LOGITS of a wave's last block; without it those rows of A_raw are never written.  What a
            # real kernel would then pool is stale workspace; the model here is a zeroed A_raw whose rows weigh nothing
            A = torch.where(drained[:, None], torch.zeros_like(A), A)
            live = live & ~drained
    if v == "pool_prev_block" and route != "fused":
        sh = 32 * launch_geometry(N, ncu)[3]
        hp = torch.cat([hp[sh:], torch.zeros(min(sh, npad), hp.shape[1], dtype=hp.dtype, device=dev)])[:npad]
        hp = torch.where((torch.arange(npad, device=dev) + sh < N)[:, None], hp, torch.zeros_like(hp))
    if route == "fused" and rnd:
        # running maximum of the workgroup: tile t is step t // grid of workgroup t % grid
        ntiles = npad // 128
        grid = min(ntiles, 512)
        tmax = torch.where(live[:, None], A, torch.full_like(A, -float("inf"))).view(ntiles, 128, K).amax(1)
        steps = (ntiles + grid - 1) // grid
        tm = torch.full((steps * grid, K), -float("inf"), dtype=A.dtype, device=dev)
        tm[:ntiles] = tmax
        run = tm.view(steps, grid, K).cummax(0)[0].view(steps * grid, K)[:ntiles]
        shift = run.repeat_interleave(128, 0)
        top = run.amax(0)
        w = bf16(torch.exp(A - shift)) * torch.exp(shift - top)
    else:
        w = torch.exp(g - g[:N].amax(0))  # (fp64: the shift is a common factor)
    w = torch.where(live[:, None], w, torch.zeros_like(w))
    M = (w.t() @ hp) / w.sum(0)[:, None]
    logits = (M * p["wcls"]).sum(1) + p["bcls"] if p["multi"] else p["wcls"] @ M[0] + p["bcls"]
    prob = torch.softmax(logits, 0)
    wn = w[:N]
    return {"A_raw": A[:N].t().contiguous(), "M": M, "logits": logits, "Y_prob": prob, "Y_hat": int(logits.argmax()),
            "neff": (wn.sum(0) ** 2 / (wn * wn).sum(0)), "frac_clamp": n_clamp / (N * S2), "frac_far": n_far / (N * S2)}


# ---- structured inputs -------------------------------------------------------------------------------------------------------
CLASS_SCALE = (0.25, 1.0, 2.0, 3.0)
SPECIAL = {"zero": (5,), "outlier": (2, 11, 17), "heavy": (8,)}  # offsets inside the head, middle and last 32-row block (heavy: and row N - 1)
OUTLIER_CH = ((7, 30.0), (100, -30.0), (150, 30.0), (-1, -30.0))


def row_layout(N: int):
    """(cls int64 [N]: 0 ... 3 the scale classes 0.25 / 1 / 2 / 3 by a hash of the row index, 4 the special rows; zero rows; outlier rows;
    heavy rows)"""
    cls = (synth.hash_u32_np(N, 4242) % np.uint32(4)).astype(np.int64)
    nblocks = (N + 31) // 32
    starts = sorted({0, 32 * (nblocks // 2), 32 * (nblocks - 1)})
    zero = [b + o for b in starts for o in SPECIAL["zero"] if b + o < N]
    outl = [b + o for b in starts for o in SPECIAL["outlier"] if b + o < N]
    heavy = sorted({b + o for b in starts for o in SPECIAL["heavy"] if b + o < N} | {N - 1})
    cls[zero + outl + heavy] = 4
    return cls, zero, outl, heavy


def structured_bag(N: int, s0: int, seed: int, device="cpu", heavy=None) -> torch.Tensor:
    """bf16 [N, s0]: hash-uniform rows times a per-row class scale (rows of different classes have different h1 norms, so the softmax
    concentrates on a few hundred rows and which weight meets which row matters), one all-zero row and three rows with four channels at
    +-30 in the head, the middle and the last block; `heavy` [s0], where given, is written into one row of each of these blocks and into
    the bag's last row (case_bag: the row the softmax weighs most, so that a block which is not pooled is missed)"""
    cls, zero, outl, hv = row_layout(N)
    x = synth.hash_uniform_torch((N, s0), seed, device=device)
    scale = torch.tensor(CLASS_SCALE + (1.0,), device=device)[torch.from_numpy(cls).to(device)]
    x = x * scale[:, None]
    for ch, val in OUTLIER_CH:
        x[outl, ch] = val
    x[zero] = 0.0
    x = x.bfloat16()
    if heavy is not None:
        x[hv] = heavy.to(x.dtype)
    return x


def case_bag(N: int, s0: int, seed: int, p: dict, route: str, device="cpu") -> torch.Tensor:
    """The structured bag with its own most-attended row (branch 0 of the emulation) as the heavy row"""
    x = structured_bag(N, s0, seed, device)
    top = int(forward(x, p, route)["A_raw"][0].argmax())
    return structured_bag(N, s0, seed, device, heavy=x[top])


def state_dict(family: str, s0: int, n_classes: int = 2, multi: bool = False, base: int = 384, wc_scale: float = 1.0):
    """The standard synthetic weights (synth.clam_param_specs) or the EDGE family: every bias x 8, the rows of every eighth gate unit
    of Wa / Wb x 48 (tanh pre-activations beyond the +-15 clamp, sigmoid pre-activations out to about -100, where e^-y overflows fp32
    and the gate's reciprocal must give 0).  wc is left alone (sum |wc| < 60) unless wc_scale says otherwise (x 4: the fused route)."""
    sd = synth.make_state_dict(synth.clam_param_specs((s0, S1, S2), n_classes=n_classes, multi=multi), base)
    g = "attention_net.2."
    if family == "edge":
        for k in sd:
            if k.endswith(".bias"):
                sd[k] = sd[k] * 8.0
        sel = torch.from_numpy((synth.hash_u32_np(S2, 901) % np.uint32(8) == 0))
        for k in (g + "attention_a.0.weight", g + "attention_b.0.weight"):
            sd[k][sel] *= 48.0
    else:
        assert family == "std", family
    if wc_scale != 1.0:
        sd[g + "attention_c.weight"] = sd[g + "attention_c.weight"] * wc_scale
    return sd


# ---- comparison ----------------------------------------------------------------------------------------------------------------------------
def stats(got: dict, ref: dict, cls) -> dict:
    """The statistics a parity test holds to a bar: A_raw max abs and rel-L2 over all rows (A_max, A_rel) and the largest of each over the
    row classes (Ac_max, Ac_rel); M rel-L2 and its worst 16-column tile (M_rel, M_tile: the reductions and the merge write in tiles);
    logits max abs (L_max)"""
    A, Ar = got["A_raw"].double(), ref["A_raw"].double()
    d = A - Ar
    out = {"A_max": float(d.abs().max()), "A_rel": float(d.norm() / Ar.norm()), "Ac_max": 0.0, "Ac_rel": 0.0}
    cls = torch.as_tensor(cls, device=A.device)
    for c in range(5):
        sel = cls == c
        if bool(sel.any()):
            dc, rc = d[:, sel], Ar[:, sel]
            out["Ac_max"] = max(out["Ac_max"], float(dc.abs().max()))
            if float(rc.norm()) > 0:
                out["Ac_rel"] = max(out["Ac_rel"], float(dc.norm() / rc.norm()))
    M, Mr = got["M"].double(), ref["M"].double()
    dm = M - Mr
    out["M_rel"] = float(dm.norm() / Mr.norm())
    out["M_tile"] = float((dm.reshape(-1, 8, 16).square().sum((0, 2)) / Mr.reshape(-1, 8, 16).square().sum((0, 2))).sqrt().max())
    out["L_max"] = float((got["logits"].double().reshape(-1) - ref["logits"].double().reshape(-1)).abs().max())
    return {k: (float("inf") if v != v else v) for k, v in out.items()}  # (a NaN is beyond every bar)
