"""LayerNorm test kit shared by tests/test_gpu_layernorm.py (the HIP kernels) and tests/test_layernorm_ref_cpu.py (an fp32
emulation of them and its mutants): the inputs, ONE fp64 reference of the forward and the backward, and the assertion
helpers.  Everything here runs on the CPU; a caller hands in what the code under test produced.

Reference (reference models/heads.py:178-185, nn.LayerNorm: biased variance, eps inside the root):
    y  = (x - mean) * rstd * gamma + beta
    dx = rstd * (g - mean(g) - xhat * mean(g * xhat)) + dres,  g = dy * gamma
    dgamma = sum_r dy * xhat,  dbeta = sum_r dy,  colsum = sum_r f * dx   (f: dropout factors, 1 without dropout)
Operands that are bf16 on the device are generated in bf16 and enter the reference as those very values.

Bounds
  fp32 element (y, mean, rstd, dx): |got - ref| <= atol + rtol |ref| with the figures of tests/test_gpu_ops.py.  In the
      "constant_row" / "large_offset" families y, rstd and dx get the per-row factor max(1, rstd |mean|): the fp32
      rounding of the mean (2^-24 |mean|) is amplified by rstd in xhat, which the fp64 reference does not suffer.
  bf16 element (y, dx_lo, dx_m): 2^-8 |ref| on top of the fp32 bound - the unit round-off of round-to-nearest bf16.
  column sums: in units of u T_c (u = 2^-24, T_c = sum_r |term_rc|) the kernel may need 2 k_seq + 4, where k_seq is what
      a SEQUENTIAL fp32 accumulation in row order of the fp32-rounded fp64 terms needs (measured here, per check).  The
      "+ 4" covers the roundings INSIDE a term, which the sequential baseline does not have.  A term that is itself a
      cancelling expression is measured THERE by the magnitudes that enter it (its T_inner):
        colsum: sum_r f (rstd (|g| + |mean g| + |xhat mean(g xhat)|) + |dres|)   (this is also its T_c in the k_seq part)
        dgamma: sum_r |dy| rstd (|x| + |mean|) - the term is dy (x - mean) rstd and the kernels' mean is an fp32 value: an
                error of 2^-24 |mean| in it moves xhat by 2^-24 rstd |mean| however small |xhat| is.  With the plain
                sum_r |dy xhat| an honest fp32 evaluation (emulate() below) misses the bound where few rows meet a column
                with xhat ~ 0: 215 units against 5.9 at 1 row x 512 columns of the general family, 143 against 6.5 at
                5 x 40 of large_offset.  The k_seq part of dgamma keeps the plain T_c.
        colsum, T_inner only: mean g and mean(g xhat) are sums over a row that cancel too, and their fp32 error follows
                mean |g| and mean |g xhat|, which replace |mean g| and |mean(g xhat)|.  It shows where gamma_c = 0 (g_rc = 0,
                so T_c holds little else): ln_bwd_reg_kernel at 1 row x 516 columns needed 6.42 units of T_c against
                2 k_seq + 4 = 5.7 at such a column with an error of 0.4 x 2^-24 x mean |g| - honest arithmetic.
      In the two special families xhat in the colsum magnitudes is taken as rstd (|x| + |mean|) for the same reason.
"""
import numpy as np
import torch

EPS = 1e-5
U24 = 2.0 ** -24
U8 = 2.0 ** -8
# (atol, rtol) of tests/test_gpu_ops.py::test_layernorm_fwd / test_layernorm_bwd
TOL = {"y": (2e-5, 1e-4), "mean": (2e-5, 1e-4), "rstd": (1e-5, 1e-4), "dx": (5e-5, 1e-4)}
FAMILIES = ("general", "constant_row", "large_offset")


def make_inputs(rows, D, seed, x_dtype=torch.float32, dy_dtype=torch.float32, dres_dtype=None, family="general"):
    """CPU tensors in their device storage types.  dres_dtype None = no residual gradient."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    ru = lambda *s: torch.rand(*s, generator=g)
    if family == "large_offset":  # |x| ~ 1e3, small variance: cancellation in x - mean (bf16 spacing at 1e3 is 4)
        sign = torch.where(ru(rows, 1) < 0.5, -1.0, 1.0)
        x = sign * 1000.0 + rn(rows, D) * (6.0 if x_dtype == torch.bfloat16 else 0.5)
    else:
        scale = 10.0 ** (ru(rows, 1) - 0.5)
        offset = 10.0 ** (ru(rows, 1) - 0.5) * torch.where(ru(rows, 1) < 0.5, -1.0, 1.0)
        x = (2.0 * rn(rows, D) + 0.5) * scale + offset
        if family == "constant_row":  # variance 0: rstd = eps^-1/2
            x[0] = 3.0
            x[rows - 1] = -0.75
            if rows > 2:
                x[rows // 2] = 0.0
    gamma = 1.0 + 0.5 * rn(D)
    gamma[1 % D] = -gamma[1 % D].abs() - 0.25
    gamma[D // 2] = -gamma[D // 2].abs() - 0.25
    gamma[3 % D] = 0.0
    gamma[D - 1] = 0.0
    if D > 512:  # the chunk boundaries of both layouts
        gamma[512] = -1.5
        gamma[D - 2] = -0.5
    beta = rn(D)
    dy = rn(rows, D) * 10.0 ** (ru(1, D) - 0.5)
    dres = rn(rows, D).to(dres_dtype) if dres_dtype is not None else None
    return dict(x=x.to(x_dtype).contiguous(), gamma=gamma, beta=beta, dy=dy.to(dy_dtype).contiguous(), dres=dres,
                family=family, rows=rows, D=D)


def reference(inp, f=None, eps=EPS):
    """fp64 forward and backward of the stored operand values; f: dropout factors [rows, D] or None."""
    x, gamma, beta, dy = inp["x"].double(), inp["gamma"].double(), inp["beta"].double(), inp["dy"].double()
    dres = inp["dres"].double() if inp["dres"] is not None else torch.zeros_like(x)
    f = torch.ones_like(x) if f is None else f.double()
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True) + eps)
    xhat = (x - mean) * rstd
    g = dy * gamma
    m1 = g.mean(1, keepdim=True)
    m2 = (g * xhat).mean(1, keepdim=True)
    dx = rstd * (g - m1 - xhat * m2) + dres
    special = inp["family"] != "general"
    xh_mag = rstd * (x.abs() + mean.abs()) if special else xhat.abs()
    terms = dict(dgamma=dy * xhat, dbeta=dy, colsum=f * dx)
    mags = dict(dgamma=(dy * xhat).abs(), dbeta=dy.abs(),
                colsum=f * (rstd * (g.abs() + m1.abs() + xh_mag * m2.abs()) + dres.abs()))
    ma1 = g.abs().mean(1, keepdim=True)
    ma2 = (g.abs() * xh_mag).mean(1, keepdim=True)
    inner = dict(dgamma=dy.abs() * rstd * (x.abs() + mean.abs()), dbeta=dy.abs(),
                 colsum=f * (rstd * (g.abs() + ma1 + xh_mag * ma2) + dres.abs()))
    sums = {}
    for k, t in terms.items():
        ref = t.sum(0)
        T = mags[k].sum(0)
        seq = torch.from_numpy(np.cumsum(t.float().numpy(), axis=0, dtype=np.float32)[-1]).double()
        unit = (U24 * T).clamp_min(1e-300)
        k_seq = float(((seq - ref).abs() / unit).max())
        sums[k] = dict(ref=ref, T=T, inner=inner[k].sum(0), k_seq=k_seq)
    amp = torch.clamp(rstd * mean.abs(), min=1.0) if special else torch.ones_like(rstd)
    return dict(y=xhat * gamma + beta, mean=mean[:, 0], rstd=rstd[:, 0], dx=dx, dx_masked=f * dx, f=f, amp=amp, sums=sums,
                special=special)


def _fail(what, got, ref, bound, extra=""):
    err = (got - ref).abs()
    bad = ~(err <= bound)  # (a NaN fails)
    n = int(bad.sum())
    if n:
        i = int(torch.argmax(torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err)).flatten()))
        idx = np.unravel_index(i, tuple(got.shape))
        raise AssertionError(f"{what}: {n} of {got.numel()} elements ({100.0 * n / got.numel():.3g} %) outside the bound; worst at "
                             f"{tuple(int(v) for v in idx)}: got {float(got.flatten()[i])!r} ref {float(ref.flatten()[i])!r} "
                             f"bound {float(bound.flatten()[i]):.3g} {extra}")


def check_f32(what, got, ref, kind, amp=None):
    """element by element, fp32 output `got` against fp64 `ref`; kind picks (atol, rtol); amp: per-row factor [rows, 1]"""
    assert got.dtype == torch.float32 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    atol, rtol = TOL[kind]
    bound = atol + rtol * ref.abs()
    if amp is not None:
        bound = bound * (amp if ref.dim() == 2 else amp[:, 0])
    _fail(what, got.double(), ref, bound)


def check_bf16(what, got, ref, kind, amp=None):
    """bf16 output: 2^-8 |ref| (round-to-nearest) on top of the fp32 bound.  -> share of elements within 2^-9 |ref|"""
    assert got.dtype == torch.bfloat16 and got.shape == ref.shape, (what, got.dtype, got.shape, ref.shape)
    atol, rtol = TOL[kind]
    fb = atol + rtol * ref.abs()
    if amp is not None:
        fb = fb * amp
    got = got.double()
    _fail(what, got, ref, U8 * ref.abs() + fb, "(bf16 by round-to-nearest: 2^-8 |ref| + the fp32 bound)")
    return float(((got - ref).abs() <= 2.0 ** -9 * ref.abs()).double().mean())


def check_colsum(what, got, s, stats=None):
    """got fp32 [D] against s = reference(...)['sums'][name]: |got - ref| <= 2 k_seq u T + 4 u T_inner.  -> the kernel's ratio in
    units of u T (its largest over the columns)"""
    assert got.dtype == torch.float32 and got.shape == s["ref"].shape, (what, got.dtype, got.shape)
    got = got.double()
    err = (got - s["ref"]).abs()
    ratio = float((err / (U24 * s["T"]).clamp_min(1e-300)).max()) if bool(torch.isfinite(err).all()) else float("inf")
    bound = 2.0 * s["k_seq"] * U24 * s["T"] + 4.0 * U24 * s["inner"]
    _fail(what, got, s["ref"], bound, f"(k_seq = {s['k_seq']:.3g}, kernel ratio = {ratio:.3g} in units of 2^-24 T_c)")
    if stats is not None:
        stats[what.split(":")[-1] + "_ratio"] = ratio
        stats[what.split(":")[-1] + "_kseq"] = s["k_seq"]
    return ratio


def check_finite(what, **outs):
    for k, t in outs.items():
        if t is not None:
            assert bool(torch.isfinite(t.float()).all()), f"{what}:{k}: not finite"


def check_forward(what, ref, y, mean, rstd):
    """-> stats.  y fp32 or bf16 [rows, D]; mean, rstd fp32 [rows]"""
    stats = {}
    amp = ref["amp"] if ref["special"] else None
    if ref["special"]:
        check_finite(what, y=y, mean=mean, rstd=rstd)
    check_f32(what + ":mean", mean, ref["mean"], "mean")
    check_f32(what + ":rstd", rstd, ref["rstd"], "rstd", amp)
    if y.dtype == torch.float32:
        check_f32(what + ":y", y, ref["y"], "y", amp)
    else:
        stats["y_within_2^-9"] = check_bf16(what + ":y", y, ref["y"], "y", amp)
    return stats


def check_backward(what, ref, dx, dx_lo, dx_m, dgamma, dbeta, colsum, dropout):
    """The output contract of avf_layernorm_bwd_ex (include/avformer_hip.h): dx is never masked; with dx_m (row8 form) dx_lo
    is unmasked and dx_m masked; without it (register form) dx_lo is the masked image; the column sums are always those of
    the masked values.  Outputs that were not requested are None.  -> stats"""
    stats = {}
    amp = ref["amp"] if ref["special"] else None
    if ref["special"]:
        check_finite(what, dx=dx, dx_lo=dx_lo, dx_m=dx_m, dgamma=dgamma, dbeta=dbeta, colsum=colsum)
    if dx is not None:
        check_f32(what + ":dx", dx, ref["dx"], "dx", amp)
    if dx_m is not None:
        assert dropout and dx_lo is not None, what + ": a separate masked image only exists under dropout, next to dx_lo"
    lo_ref = ref["dx"] if (dx_m is not None or not dropout) else ref["dx_masked"]
    for name, img, r in (("dx_lo", dx_lo, lo_ref), ("dx_m", dx_m, ref["dx_masked"])):
        if img is None:
            continue
        stats[name + "_within_2^-9"] = check_bf16(f"{what}:{name}", img, r, "dx", amp)
        if r is ref["dx_masked"] and dropout:
            dropped = ref["f"] == 0
            assert bool((img[dropped].float() == 0).all()), f"{what}:{name}: a dropped element is not exactly 0"
    check_colsum(what + ":dgamma", dgamma, ref["sums"]["dgamma"], stats)
    check_colsum(what + ":dbeta", dbeta, ref["sums"]["dbeta"], stats)
    if colsum is not None:
        check_colsum(what + ":colsum", colsum, ref["sums"]["colsum"], stats)
    return stats


# ---- an fp32 emulation of what the kernels do (test_layernorm_ref_cpu.py): fp32 statistics and arithmetic, bf16 on store,
# ---- per-block partial column sums of `rpb` rows folded one after the other; and its mutants ---------------------------------
MUTANTS = ("drop_row_from_sums", "last_row_from_previous", "s1_s2_swapped", "bf16_truncation", "colsum_unmasked",
           "gamma_chunk0_everywhere")


def _to_bf16(t, truncate=False):
    if not truncate:
        return t.to(torch.bfloat16)
    bits = t.contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(torch.bfloat16)


def _block_sums(t, rpb, skip_row=None):
    rows, D = t.shape
    if skip_row is not None:
        t = t.clone()
        t[skip_row] = 0.0
    nb = -(-rows // rpb)
    pad = torch.zeros(nb * rpb, D, dtype=torch.float32)
    pad[:rows] = t
    partial = pad.view(nb, rpb, D).sum(1, dtype=torch.float32)
    return torch.from_numpy(np.cumsum(partial.numpy(), axis=0, dtype=np.float32)[-1].copy())


def emulate(inp, f=None, form="reg", rpb=16, y_dtype=torch.bfloat16, want_dx=True, mutant=None, eps=EPS):
    """-> dict(y, mean, rstd, dx, dx_lo, dx_m, dgamma, dbeta, colsum) as a kernel of the given form would return them.
    form "row8": dx_lo unmasked + dx_m masked under dropout; "reg": dx_lo masked under dropout, no dx_m."""
    assert mutant is None or mutant in MUTANTS
    x, gamma, beta, dy = inp["x"].float(), inp["gamma"].float(), inp["beta"].float(), inp["dy"].float()
    rows, D = x.shape
    if mutant == "gamma_chunk0_everywhere":
        gamma = gamma[torch.arange(D) % 512]
    trunc = mutant == "bf16_truncation"
    mean = x.mean(1, keepdim=True, dtype=torch.float32)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(1, keepdim=True, dtype=torch.float32) + eps)
    xhat = (x - mean) * rstd
    y = xhat * gamma + beta
    g = dy * gamma
    s1 = g.mean(1, keepdim=True, dtype=torch.float32)
    s2 = (g * xhat).mean(1, keepdim=True, dtype=torch.float32)
    if mutant == "s1_s2_swapped":
        s1, s2 = s2, s1
    dx = rstd * (g - s1 - xhat * s2)
    if inp["dres"] is not None:
        dx = dx + inp["dres"].float()
    masked = dx if f is None else dx * f.float()
    skip = rows // 2 if mutant == "drop_row_from_sums" else None
    out = dict(mean=mean[:, 0].contiguous(), rstd=rstd[:, 0].contiguous(), dx=dx if want_dx else None, dx_m=None,
               y=y if y_dtype == torch.float32 else _to_bf16(y, trunc),
               dgamma=_block_sums(dy * xhat, rpb, skip), dbeta=_block_sums(dy, rpb, skip),
               colsum=_block_sums(dx if mutant == "colsum_unmasked" else masked, rpb, skip))
    if form == "row8":
        out["dx_lo"] = _to_bf16(dx, trunc)
        if f is not None:
            out["dx_m"] = _to_bf16(masked, trunc)
    else:
        out["dx_lo"] = _to_bf16(masked, trunc)
    if mutant == "last_row_from_previous" and rows > 1:
        for k in ("y", "dx_lo", "dx_m", "dx"):
            if out[k] is not None:
                out[k] = out[k].clone()
                out[k][rows - 1] = out[k][rows - 2]
    return out
