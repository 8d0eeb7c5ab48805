"""fp64 reference, bf16 emulation, group-wise bounds and mutants for the UNMASKED bf16 attention kernels: csrc/attn_bf16.hip
(attn_fwd_res_kernel<8 | 12 | 8,multi>, attn_fwd_bf16_kernel, attn_dq/dkv_res_kernel, attn_dq/dkv_bf16_kernel) and
csrc/attn_bwd_merged.hip (attn_bwd_m4_kernel<KB, RAGGED, MXO>).  CPU only: tests/test_gpu_attn_bf16.py hands in what the device
returned, tests/test_attn_bf16_ref_cpu.py shows without a device that the bounds pass a correct rounding and refuse the mutants.

Everything lives in HEAD FORM [B, H, N, dh] (heads() / packed() convert from and to the [B N, k H dh] projection layout).

Reference (reference models/heads.py:222-237), fp64 on the stored bf16 operands (a pre-scaled q' = bf16(q log2(e)/sqrt(dh)) is
divided by the factor in fp64, so the reference sees the very numbers the kernels see):
    s = q k^T dh^-1/2 ; p = softmax(s) ; o = p v ; lse2 = log2(e) logsumexp(s) ; dq, dk, dv by autograd with d_o
and the magnitudes of the same sums, taken over absolute values (none is zero where the reference is: at N = 1 dq = dk = 0):
    Mag_o = p |v|        Mag_dv = p^T |dO|        dSmag = p (|dP| + sum_d |dO| |o|),  dP = dO v^T
    Mag_dq = dSmag |k| dh^-1/2                     Mag_dk = dSmag^T |q| dh^-1/2
The backward is checked on REFERENCE-MADE inputs o_in = bf16(o_ref), lse2_in = fp32(lse2_ref): a forward fault cannot hide one.

Emulation: the fp64 arithmetic again with the bf16 rounding points of the kernels (attn_bwd_merged.hip:13-26 and the header of
attn_bf16.hip, :20-26):
    forward   P rounded to bf16 before P V; o rounded once.  assoc = "normalised": bf16(softmax) V; assoc = "unnormalised" (what
              the kernels do): pu = exp2(s2 - rowmax), bf16(pu) V / l with l = sum of the ROUNDED pu, lse2 = rowmax + log2(l).
    backward  P = exp2(s2 - lse2_in); delta = fp32(sum_d dO bf16(o)); dS = P (dP - delta) rounded to bf16 (from the UNROUNDED P:
              attn_bwd_merged.hip:370-377, attn_bf16.hip:892-905); dV = bf16(P)^T dO, dQ = bf16(dS) K dh^-1/2,
              dK = bf16(dS)^T Q dh^-1/2, each rounded once.  assoc = "unnormalised": dS from the rounded P instead.
    Scores and lse2 are fp32 in the kernels: fp64 here, their fp32 error is the second term of the bounds.

Groups: one part (o | dq | dk | dv), one clip, one head, 16 rows, 16 columns; a tail block of fewer than 8 rows joins the block
before it; every element lies in exactly one group (a wave owns 32 keys or 32 queries, the merged kernel's dQ job 16 columns,
the dim_head 128 streaming kernels give a wave 16 rows).

Bounds, per group g, || . || the Frobenius norm over g, U = 2^-24, K = max(N, dh):
    random operands   ||got - ref||_g <= 2 ||emu - ref||_g + 2 K U ||Mag||_g
        the emulation carries every bf16 rounding point; what it leaves out (summation order, v_exp_f32) is 2^-15 of that; the
        rms of >= 128 roundings fluctuates by a few percent; a kernel may round the same quantities in another association.
        2 K U Mag is the fp32 summation term of tests/gemm_nt_util.py.  If a correct kernel exceeds it, the cure is a rounding
        point the kernel demonstrably performs, added to the emulation - never a larger factor.
    score regimes     ||got - ref||_g <= (3 * 2^-8 + 2 K U) ||Mag||_g
        at most three bf16 roundings on any path, each at most 2^-8 relative: the worst case; the lazy rescaling of the
        head-resident forward cannot be emulated without copying it.  A rescale fault is a factor 2^k.
    lse2, per element |got - ref| <= 2 [(dh + N/64 + 8) U S_i + log2(e) (N + 16) U]  +  log2(e) 2^-8 where l sums ROUNDED P
        S_i = max_j sum_d |q'_id| |k_jd| (log2 units) bounds every score of the row and so the running maximum m and lse2
        itself; (dh + ..) U S_i: the fp32 accumulation of a score (an error of all scores of a row by at most e moves lse2 by at
        most e), the N/64 additions m += shift of the lazy rescaling and m + log2(l); log2(e) (N + 16) U: an fp32 sum of N
        positive terms in any order, v_exp_f32 and v_log_f32; factor 2 as in gemm_nt_util.  The head-resident forward takes l
        from the MFMA of a ones row with the bf16 P (attn_bf16.hip:719-720): each term is off by at most 2^-8 relative, so is l,
        and lse2 by log2(1 + 2^-8) < log2(e) 2^-8.  The streaming forward sums the unrounded P (attn_bf16.hip:260-264): no
        such term.
    sign statistic, per part over all clips and heads: T = sum (got - ref) sign(ref), R_r = sum_d |got - ref| of token row r:
        |T| <= 8 sqrt(sum_r R_r^2).  Round-to-nearest errors have mean zero; errors of one token row may be fully coherent
        (they share l, a probability or delta; with q = small noise + one large vector, as in the score regimes, a row of dK
        IS one rounding error times that vector), rows are taken as independent: the right side is eight standard deviations
        of T in that worst case - six for the tail of a sum of hundreds of bounded terms, a third more for the coupling of
        the rows of dK through delta (one delta error enters every key's row, with weights p whose signed sum is small: the
        rows of dS sum to zero).  Truncation pulls every stored value toward zero: T = -sum_r (its share of R_r), which
        grows like the number of rows, not its root - visible from about 200 rows (N >= 33 at B H = 6).

Mutants, applied to the emulation (check() must refuse each): the table MUTANTS below and the emulate_* functions.

The two run_* functions at the end are the only device code: the launches of the GPU file, on
NaN-filled outputs, twice, compared bit for bit.

ATTNSTAT maxima on an MI355X - the worst error / bound of each kernel family by part, with the case and the group (clip, head,
row block, column block) that came closest to its bound - are ATTNSTAT_MAXIMA at the end of this file.  In short: every
backward family sits at 0.44 .. 0.51 of the random-operand bound (its kernels round exactly where the emulation does), the
forward families at 0.47 .. 0.58 (unnormalised P, l from the rounded P), the regimes at or below 0.07 of the worst-case bound,
lse2 at or below 0.29 of its tolerance, the sign statistic at or below 0.19."""
import functools
import math

import torch

from mask_attn_util import LOG2E, REGIMES, prescale_q, regime_qk

U = 2.0 ** -24
U_BF16 = 2.0 ** -8  # largest relative error of one round-to-nearest to bf16 (8 significand bits)
FACTOR = 2.0
SIGN_SIGMAS = 8.0
PARTS_FWD = ("o",)
PARTS_BWD = ("dq", "dk", "dv")
B_, H_ = 2, 3
REGIME_NAMES = ("ramp", "small_steps", "descending", "very_negative")


# ---------------------------------------------------------------------------------------------- layout and rounding
def heads(x, B, N, H, dh):
    """[B N, k H dh] -> k tensors [B, H, N, dh] (one, not a list, for k = 1)"""
    k = x.shape[1] // (H * dh)
    out = [t.reshape(B, N, H, dh).permute(0, 2, 1, 3) for t in x.split(H * dh, dim=-1)]
    assert len(out) == k
    return out[0] if k == 1 else out


def packed(*ts):
    """tensors [B, H, N, dh] -> [B N, k H dh]"""
    B, H, N, dh = ts[0].shape
    return torch.cat([t.permute(0, 2, 1, 3).reshape(B * N, H * dh) for t in ts], dim=-1)


def bf(x):
    """round to nearest even to bf16, back in fp64"""
    return x.float().to(torch.bfloat16).double()


def bf_trunc(x):
    """bf16 by truncation (the low 16 bits of the fp32 pattern dropped), back in fp64"""
    return (x.float().contiguous().view(torch.int32) & -65536).view(torch.float32).double()


def f32(x):
    return x.float().double()


# ---------------------------------------------------------------------------------------------- operands
def make_operands(B, N, H, dh, seed, qs, regime=None):
    """-> (qkv bf16 [B N, 3 H dh], pre-scaled q when qs; d_o bf16 [B N, H dh]; the fp64 projection (q | k | v) those stand for).
    Distinct data per clip and head."""
    g = torch.Generator().manual_seed(seed)
    I = H * dh
    if regime is None:
        qkv = torch.randn(B * N, 3 * I, generator=g)
    else:
        qkv = torch.empty(B, N, 3, H, dh)
        for b in range(B):
            for h in range(H):
                q, k, v, u = (torch.randn(N, dh, generator=g), torch.randn(N, dh, generator=g), torch.randn(N, dh, generator=g),
                              torch.randn(dh, generator=g))
                q, k = regime_qk(regime, q, k, u / u.norm())
                qkv[b, :, 0, h], qkv[b, :, 1, h], qkv[b, :, 2, h] = q, k, v
        qkv = qkv.reshape(B * N, 3 * I)
    d_o = torch.randn(B * N, I, generator=g).to(torch.bfloat16)
    qkv = qkv.to(torch.bfloat16)
    if qs:
        qkv = prescale_q(qkv, H, dh)[0]
    proj = qkv.double()
    if qs:
        proj[:, :I] = proj[:, :I] / (LOG2E / math.sqrt(dh))
    return qkv, d_o, proj


# ---------------------------------------------------------------------------------------------- reference
def reference(proj, d_o, B, N, H, dh):
    """fp64 -> dict(o, lse2 [B, H, N], dq, dk, dv, and Mag_o, Mag_dq, Mag_dk, Mag_dv; S: the score bound of the lse2 tolerance)"""
    x = proj.clone().requires_grad_(True)
    q, k, v = heads(x, B, N, H, dh)
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    p = s.softmax(-1)
    o = p @ v
    g = heads(d_o.double(), B, N, H, dh)
    o.backward(g)
    dq, dk, dv = [t.contiguous() for t in heads(x.grad, B, N, H, dh)]
    with torch.no_grad():
        lse2 = torch.logsumexp(s, dim=-1) * LOG2E
        dP = g @ v.transpose(-1, -2)
        dsmag = p * (dP.abs() + (g.abs() * o.abs()).sum(-1, keepdim=True))
        mag = dict(o=p @ v.abs(), dv=p.transpose(-1, -2) @ g.abs(), dq=(dsmag @ k.abs()) * dh ** -0.5,
                   dk=(dsmag.transpose(-1, -2) @ q.abs()) * dh ** -0.5)
        S = (q.abs() @ k.abs().transpose(-1, -2)).amax(-1) * dh ** -0.5 * LOG2E
    return dict(o=o.detach().contiguous(), lse2=lse2, dq=dq, dk=dk, dv=dv, mag=mag, S=S)


def backward_inputs(ref):
    """the reference-made inputs of the backward: o_in bf16 [B, H, N, dh], lse2_in fp32 [B, H, N]"""
    return ref["o"].float().to(torch.bfloat16), ref["lse2"].float()


# ---------------------------------------------------------------------------------------------- mutants
def _where(N):
    """the places a mutant touches at N tokens (clip B - 1, head H - 1): a 16-row query block in the middle, one key, a 16-key
    block, the second 32-row slice, the first key of the last 64-key tile (where a skipped rescale leaves the most weight)"""
    nb = max(1, N // 16)
    r0 = 16 * (nb // 2)
    return dict(rows=slice(r0, min(r0 + 16, N)), key=(2 * N) // 3, keys=slice(r0, min(r0 + 16, N)), query=N // 3,
                sl=slice(32, min(64, N)), prev=slice(0, min(64, N) - 32), tile=64 * ((N - 1) // 64))


# name -> (passes it touches, smallest N it applies to, needs: None | "ragged" (N % 64 != 0) | "ramp")
MUTANTS = {
    "drop_key": (("fwd", "bwd"), 2, None),        # one key dropped for one 16-row block of queries (o, dq)
    "drop_query": (("bwd",), 2, None),            # one query dropped for one 16-key block (dk, dv)
    "last_row_lse": (("bwd",), 2, None),          # the last row computed with row N - 2's lse2 (every clip and head)
    # one padded key (K = 0, V = 0: score 0) left unmasked in the last key block.  With random operands it takes a weight of
    # about 0.6 / N from every row: where l sums the rounded P (head-resident kernels) o and lse2 must be allowed 2 * 2.3e-3 and
    # log2(e) 2^-8 = 5.6e-3, so the fault is resolved up to N = 129 only; beyond, the `very_negative` regime shows it (every
    # real score is about -360 in log2 units, the padded key takes all the weight).  The streaming kernel's lse2 is held to the
    # fp32 terms alone and shows it at every N.
    "padded_key": (("fwd",), 1, "ragged"),
    "dq_stale_slice": (("bwd",), 33, None),       # one 16-column block of dQ built from the previous 32-row slice's dS
    "delta_stale_slice": (("bwd",), 33, None),    # delta of one 32-row slice taken from the previous slice
    "skip_rescale": (("fwd",), 65, "ramp"),       # the rescale of one 64-key tile skipped for one 16-row block
    "swap_heads": (("fwd", "bwd"), 1, None),      # two heads of one clip swapped
    "truncate": (("fwd", "bwd"), 33, None),       # an output stored by truncation instead of round-to-nearest
}


def mutant_applies(name, what, N, regime=None, rounded_l=True):
    """is the mutant defined at N tokens, and can the bound of this case (random operands, or `regime`) resolve it"""
    passes, nmin, needs = MUTANTS[name]
    if what not in passes or N < nmin:
        return False
    if regime is not None and name not in ("skip_rescale", "padded_key", "swap_heads"):
        return False  # the other mutants are for the random-operand bound
    if needs == "ragged":
        return N % 64 != 0 and (N <= 129 or not rounded_l or regime == "very_negative")
    if needs == "ramp":
        return regime == "ramp"
    return True


# ---------------------------------------------------------------------------------------------- emulation
def _scores2(proj, B, N, H, dh):
    q, k, v = heads(proj, B, N, H, dh)
    return q, k, v, (q @ k.transpose(-1, -2)) * (dh ** -0.5 * LOG2E)


def emulate_forward(proj, B, N, H, dh, assoc="normalised", mutant=None, rounding=True, rounded_l=True):
    """-> dict(o [B, H, N, dh], lse2 [B, H, N]); rounding=False: the same arithmetic without a rounding point (= reference);
    rounded_l (assoc "unnormalised"): l sums the rounded P (head-resident kernels), else the unrounded (streaming kernel)"""
    rnd = bf if rounding else (lambda t: t)
    q, k, v, s2 = _scores2(proj, B, N, H, dh)
    w = _where(N)
    b, h = B - 1, H - 1
    m = s2.amax(-1, keepdim=True)
    pu = torch.exp2(s2 - m)
    if mutant == "drop_key":
        pu[b, h, w["rows"], w["key"]] = 0.0
    if mutant == "skip_rescale":  # the accumulators of the tiles before `tile` keep the scale of the old maximum
        t = w["tile"]
        shift = (s2[b, h, w["rows"], :t + 64].amax(-1) - s2[b, h, w["rows"], :t].amax(-1)).clamp_min(0.0)
        pu[b, h, w["rows"], :t] = pu[b, h, w["rows"], :t] * torch.exp2(shift)[:, None]
    extra = torch.zeros_like(m)
    if mutant == "padded_key":  # a key with K = 0 scores 0; V = 0 adds nothing to the numerator
        extra[b, h] = torch.exp2(-m[b, h])
    if assoc == "normalised":
        l = pu.sum(-1, keepdim=True) + extra
        o = rnd(pu / l) @ v
    else:
        assert assoc == "unnormalised", assoc
        pb = rnd(pu)
        l = (pb if rounded_l else pu).sum(-1, keepdim=True) + extra
        o = (pb @ v) / l
    lse2 = (m + torch.log2(l)).squeeze(-1)
    if mutant == "swap_heads":
        o[b, [0, 1]] = o[b, [1, 0]]
        lse2[b, [0, 1]] = lse2[b, [1, 0]]
    if rounding:
        o = bf_trunc(o) if mutant == "truncate" else bf(o)
        lse2 = f32(lse2)
    return dict(o=o, lse2=lse2)


def emulate_backward(proj, d_o, o_in, lse2_in, B, N, H, dh, assoc="normalised", mutant=None, rounding=True):
    """o_in [B, H, N, dh], lse2_in [B, H, N] -> dict(dq, dk, dv)"""
    rnd = bf if rounding else (lambda t: t)
    q, k, v, s2 = _scores2(proj, B, N, H, dh)
    g = heads(d_o.double(), B, N, H, dh)
    w = _where(N)
    b, h = B - 1, H - 1
    L = lse2_in.double().clone()
    if mutant == "last_row_lse":  # in every clip and head, as a kernel would: how far two neighbouring rows' lse2 lie apart is chance
        L[:, :, N - 1] = L[:, :, N - 2]
    p = torch.exp2(s2 - L[..., None])
    if mutant == "drop_key":
        p[b, h, w["rows"], w["key"]] = 0.0
    if mutant == "drop_query":
        p[b, h, w["query"], w["keys"]] = 0.0
    delta = (g * o_in.double()).sum(-1, keepdim=True)
    if rounding:
        delta = f32(delta)
    if mutant == "delta_stale_slice":
        n = w["sl"].stop - w["sl"].start
        delta[b, h, w["sl"]] = delta[b, h, w["prev"]][:n].clone()
    dP = g @ v.transpose(-1, -2)
    pb = rnd(p)
    ds = rnd((pb if assoc == "unnormalised" else p) * (dP - delta))
    dv = pb.transpose(-1, -2) @ g
    dq = (ds @ k) * dh ** -0.5
    dk = (ds.transpose(-1, -2) @ q) * dh ** -0.5
    if mutant == "dq_stale_slice":
        n = w["sl"].stop - w["sl"].start
        dq[b, h, w["sl"], 16:32] = dq[b, h, w["prev"], 16:32][:n].clone()
    out = dict(dq=dq, dk=dk, dv=dv)
    for name in out:
        if mutant == "swap_heads":
            out[name][b, [0, 1]] = out[name][b, [1, 0]]
        if rounding:
            out[name] = bf_trunc(out[name]) if mutant == "truncate" else bf(out[name])
    return out


# ---------------------------------------------------------------------------------------------- groups
def row_blocks(N):
    """-> (block index of every row [N], number of blocks): 16-row blocks, a tail of fewer than 8 rows joins the block before"""
    nblk = max(1, (N + 8) // 16)
    return torch.clamp(torch.arange(N) // 16, max=nblk - 1), nblk


def group_sq(x):
    """x [B, H, N, dh] -> the sums of squares of its groups [B, H, row blocks, dh / 16]"""
    B, H, N, dh = x.shape
    assert dh % 16 == 0
    rb, nblk = row_blocks(N)
    cols = (x.double() ** 2).reshape(B, H, N, dh // 16, 16).sum(-1)
    return torch.zeros(B, H, nblk, dh // 16, dtype=torch.float64).index_add_(2, rb, cols)


def group_ids(B, H, N, dh):
    """the group number of every element [B, H, N, dh] (the partition the bounds are taken over)"""
    rb, nblk = row_blocks(N)
    cb = torch.arange(dh) // 16
    bh = (torch.arange(B)[:, None] * H + torch.arange(H)[None, :])[:, :, None, None]
    return (bh * nblk + rb[None, None, :, None]) * (dh // 16) + cb[None, None, None, :]


# ---------------------------------------------------------------------------------------------- checks
def group_ratio(got, ref, emu, mag, N, dh, regime=False):
    """-> (error / bound of every group [B, H, row blocks, dh / 16])"""
    K = max(N, dh)
    err = group_sq(got.double() - ref).sqrt()
    gm = group_sq(mag).sqrt()
    if regime:
        bound = (3 * U_BF16 + 2 * K * U) * gm
    else:
        bound = FACTOR * group_sq(emu - ref).sqrt() + 2 * K * U * gm
    assert bool((bound > 0).all()), "a group's bound is 0"
    return err / bound


def sign_ratio(got, ref):
    """|T| / (SIGN_SIGMAS sqrt(sum_r R_r^2)) of one part (0 where nothing was rounded)"""
    e = got.double() - ref
    T = float((e * torch.sign(ref)).sum().abs())
    R = float((e.abs().sum(-1) ** 2).sum().sqrt())
    return 0.0 if R == 0.0 else T / (SIGN_SIGMAS * R)


def lse2_tolerance(ref, N, dh, rounded_l):
    fp32 = (dh + N / 64.0 + 8) * U * ref["S"] + LOG2E * (N + 16) * U
    return FACTOR * fp32 + (LOG2E * U_BF16 if rounded_l else 0.0)


def check(tag, got, ref, emu, N, dh, parts, regime=False, rounded_l=None):
    """got: {part: [B, H, N, dh]} (+ "lse2" [B, H, N] with rounded_l given); emu: the clean emulation (None under the regime
    bound).  Asserts every group bound, the sign statistic and the lse2 tolerance; -> {part: dict(ratio, group, sign)} with
    the worst error / bound and the group (clip, head, row block, column block) that gave it."""
    stats, bad = {}, []
    for part in parts:
        g = got[part].detach().double().cpu()
        assert g.shape == ref[part].shape, (part, g.shape, ref[part].shape)
        assert bool(torch.isfinite(g).all()), f"{tag}:{part}: not finite"
        r = group_ratio(g, ref[part], None if regime else emu[part], ref["mag"][part], N, dh, regime)
        worst = int(r.argmax())
        idx = [int(i) for i in torch.unravel_index(torch.tensor(worst), r.shape)]
        sg = sign_ratio(g, ref[part])
        stats[part] = dict(ratio=round(float(r.max()), 4), group=idx, sign=round(sg, 4))
        if float(r.max()) > 1.0:
            bad.append(f"{part}: error / bound {float(r.max()):.3f} in group (clip, head, rows, cols) {idx}")
        if sg > 1.0:
            bad.append(f"{part}: sign statistic {sg:.3f} x its {SIGN_SIGMAS:g}-sigma bound (truncation?)")
    if rounded_l is not None:
        g = got["lse2"].detach().double().cpu()
        assert bool(torch.isfinite(g).all()), f"{tag}:lse2: not finite"
        r = (g - ref["lse2"]).abs() / lse2_tolerance(ref, N, dh, rounded_l)
        worst = int(r.argmax())
        idx = [int(i) for i in torch.unravel_index(torch.tensor(worst), r.shape)]
        stats["lse2"] = dict(ratio=round(float(r.max()), 4), group=idx)
        if float(r.max()) > 1.0:
            bad.append(f"lse2: error / tolerance {float(r.max()):.3f} at (clip, head, row) {idx}")
    assert not bad, f"{tag}: " + "; ".join(bad)
    return stats


# ---------------------------------------------------------------------------------------------- the cases of the GPU file
FWD_QS = {"res8": (1, 15, 16, 17, 33, 255, 256), "res12": (257, 383, 384), "res_multi": (385, 511, 512, 513, 575, 576),
          "stream": (577, 640, 641)}
FWD_DH = ((32, 12), (32, 129), (32, 200), (128, 17), (128, 129), (128, 257))   # (dim_head, N), qs = 1, streaming
FWD_RAW = ((64, 33, "res8"), (64, 256, "res8"), (64, 324, "res12"), (64, 385, "res_multi"), (64, 576, "res_multi"),
           (64, 577, "stream"), (32, 200, "stream"), (128, 129, "stream"))      # (dim_head, N, kernel), qs = 0
BWD_MERGED = {1: (1, 31, 32, 33, 97, 127, 128), 2: (129, 255, 256), 3: (257, 324, 383, 384), 4: (385, 500, 511, 512)}
MXO_LENGTHS = (128, 129, 256, 384)
# dim_head 64 on the streaming backward where the forward is still head-resident: past the merged kernel's 512 tokens with
# pre-scaled q (qs = 1), and with raw q (qs = 0) from a single ragged 64-row tile (33) to the last resident length (576)
BWD_STREAM64_RES_FWD = {1: (513, 575, 576), 0: (33, 256, 257, 384, 385, 576)}
BWD_STREAM = (tuple((64, N, qs) for N in (577, 640, 641) for qs in (1, 0)) + tuple((dh, N, 1) for dh, N in FWD_DH) +
              tuple((64, N, qs) for qs in (1, 0) for N in BWD_STREAM64_RES_FWD[qs]))
# ... and `very_negative` at two ragged multi-pass lengths: the only operands that show an unmasked padded key past N = 129
REGIME_CASES = tuple((r, N) for r in REGIME_NAMES for N in (324, 512)) + (("very_negative", 511), ("very_negative", 575))


def all_cases():
    """every (N, dh, qs, regime) the GPU file runs"""
    out = set()
    for ns in FWD_QS.values():
        out |= {(N, 64, 1, None) for N in ns}
    out |= {(N, dh, 1, None) for dh, N in FWD_DH}
    out |= {(N, dh, 0, None) for dh, N, _ in FWD_RAW}
    for ns in BWD_MERGED.values():
        out |= {(N, 64, 1, None) for N in ns}
    out |= {(N, 64, 1, None) for N in MXO_LENGTHS}
    out |= {(N, dh, qs, None) for dh, N, qs in BWD_STREAM}
    out |= {(N, 64, 1, r) for r, N in REGIME_CASES}
    return sorted(out, key=lambda c: (c[3] or "", c[1], c[2], c[0]))


class Case:
    """operands, fp64 reference, reference-made backward inputs and clean emulations of one case (B = 2, H = 3); read-only"""

    def __init__(self, N, dh, qs, regime=None):
        self.N, self.dh, self.qs, self.regime, self.B, self.H = N, dh, qs, regime, B_, H_
        seed = 200000 + 131 * N + dh + 7 * qs + (1000 * (1 + REGIMES.index(regime)) if regime else 0)
        self.qkv, self.d_o, self.proj = make_operands(B_, N, H_, dh, seed, qs, regime)
        self.ref = reference(self.proj, self.d_o, B_, N, H_, dh)
        self.o_in, self.lse2_in = backward_inputs(self.ref)
        self.dims = (B_, N, H_, dh)
        self.emu_fwd = None if regime else emulate_forward(self.proj, *self.dims)
        self.emu_bwd = None if regime else emulate_backward(self.proj, self.d_o, self.o_in, self.lse2_in, *self.dims)

    def forward(self, assoc="normalised", mutant=None, rounding=True, rounded_l=True):
        return emulate_forward(self.proj, *self.dims, assoc=assoc, mutant=mutant, rounding=rounding, rounded_l=rounded_l)

    def backward(self, assoc="normalised", mutant=None, rounding=True):
        return emulate_backward(self.proj, self.d_o, self.o_in, self.lse2_in, *self.dims, assoc=assoc, mutant=mutant,
                                rounding=rounding)

    def check_forward(self, tag, got, rounded_l):
        return check(tag, got, self.ref, self.emu_fwd, self.N, self.dh, PARTS_FWD, self.regime is not None, rounded_l)

    def check_backward(self, tag, got):
        return check(tag, got, self.ref, self.emu_bwd, self.N, self.dh, PARTS_BWD, self.regime is not None)


@functools.lru_cache(maxsize=4)
def case(N, dh, qs, regime=None):
    return Case(N, dh, qs, regime)


# ---------------------------------------------------------------------------------------------- device launches
def _twice(tag, launch, make_outputs):
    """launch(outputs) on fresh NaN-filled outputs, twice -> the outputs on the CPU, all finite and equal bit for bit"""
    runs = []
    for _ in range(2):
        outs = make_outputs()
        launch(*outs)
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in outs])
    for a, b in zip(*runs):
        if a.dtype != torch.uint8:
            assert bool(torch.isfinite(a.float()).all()), f"{tag}: an output holds NaN or inf (not written?)"
        assert torch.equal(a, b), f"{tag}: two calls differ"
    return runs[0]


def run_forward(A, qkv, B, N, H, dh, qs, tag="fwd"):
    """avf_attn_fwd_qs / avf_attn_fwd on bf16 -> (o [B, H, N, dh] bf16, lse2 [B, H, N] fp32) on the CPU"""
    ops, lib = A.ops, A._lib.load()
    q = qkv.cuda().contiguous()

    def outputs():
        return (torch.full((B * N, H * dh), float("nan"), dtype=torch.bfloat16, device="cuda"),
                torch.full((B, H, N), float("nan"), dtype=torch.float32, device="cuda"))

    def launch(o, lse2):
        if qs:
            rc = lib.avf_attn_fwd_qs(ops._ptr(q), ops._ptr(o), ops._ptr(lse2), B, N, H, dh, ops._stream())
        else:
            rc = lib.avf_attn_fwd(A._lib.BF16, ops._ptr(q), ops._ptr(o), ops._ptr(lse2), B, N, H, dh, ops._stream())
        A._lib.check(rc, "attn_fwd")

    o, lse2 = _twice(tag, launch, outputs)
    return heads(o, B, N, H, dh), lse2


def run_backward(A, qkv, o_in, lse2_in, d_o, B, N, H, dh, qs, mx8=False, tag="bwd"):
    """avf_attn_bwd_qs / avf_attn_bwd on bf16 (mx8: avf_attn_bwd_mx8) with o_in [B, H, N, dh] bf16 and lse2_in [B, H, N] fp32
    -> dict(dq, dk, dv [B, H, N, dh] bf16, dqkv [B N, 3 I]) on the CPU (+ image, scales with mx8)"""
    ops, lib = A.ops, A._lib.load()
    q, g, o, L = qkv.cuda().contiguous(), d_o.cuda().contiguous(), packed(o_in).cuda().contiguous(), lse2_in.cuda().contiguous()
    I = H * dh
    ws = ops._bytes(lib.avf_attn_bwd_workspace_bytes(B, N, H, dh), q.device)

    def outputs():
        out = (torch.full((B * N, 3 * I), float("nan"), dtype=torch.bfloat16, device="cuda"),)
        if mx8:  # 0xFF is NaN in e4m3 and in E8M0
            out += (torch.full((B * N, 3 * I), 255, dtype=torch.uint8, device="cuda"),
                    torch.full((B * N, 3 * I // 32), 255, dtype=torch.uint8, device="cuda"))
        return out

    def launch(dqkv, img=None, scales=None):
        args = (ops._ptr(q), ops._ptr(o), ops._ptr(g), ops._ptr(L), ops._ptr(dqkv))
        if mx8:
            rc = lib.avf_attn_bwd_mx8(*args, ops._ptr(img), ops._ptr(scales), B, N, H, dh, ops._stream())
        elif qs:
            rc = lib.avf_attn_bwd_qs(*args, ops._ptr(ws), B, N, H, dh, ops._stream())
        else:
            rc = lib.avf_attn_bwd(A._lib.BF16, *args, ops._ptr(ws), B, N, H, dh, ops._stream())
        A._lib.check(rc, "attn_bwd")

    outs = _twice(tag, launch, outputs)
    dq, dk, dv = heads(outs[0], B, N, H, dh)
    res = dict(dq=dq, dk=dk, dv=dv, dqkv=outs[0])
    if mx8:
        res.update(image=outs[1], scales=outs[2])
    return res


# ---------------------------------------------------------------------------------------------- measured
# Worst error / bound of the ATTNSTAT lines of tests/test_gpu_attn_bf16.py on an MI355X, per kernel family and part
# (the group that came closest to its bound: case, (clip, head, row block, column block)).
ATTNSTAT_MAXIMA = {
    # family: {part: (error / bound, N, regime, group)}
    "fwd_res8": {"o": (0.5829, 255, None, (1, 1, 4, 0)), "lse2": (0.2893, 15, None, (1, 0, 5))},
    "fwd_res12": {"o": (0.5597, 257, None, (0, 1, 12, 3)), "lse2": (0.1816, 384, None, (0, 0, 343))},
    "fwd_res_multi": {"o": (0.5593, 513, None, (0, 0, 26, 1)), "lse2": (0.1871, 513, None, (0, 0, 431))},
    "fwd_stream": {"o": (0.4655, 641, None, (1, 0, 8, 2)), "lse2": (0.0057, 577, None, (1, 2, 490))},
    "fwd_stream32": {"o": (0.5308, 129, None, (1, 2, 5, 0)), "lse2": (0.0158, 129, None, (1, 0, 41))},
    "fwd_stream128": {"o": (0.5231, 129, None, (1, 1, 7, 7)), "lse2": (0.0043, 257, None, (1, 1, 112))},
    "fwd_raw_res": {"o": (0.5549, 256, None, (0, 0, 9, 3)), "lse2": (0.2151, 33, None, (1, 0, 14))},
    "fwd_raw_stream": {"o": (0.5679, 200, None, (1, 0, 12, 1)), "lse2": (0.0152, 200, None, (1, 0, 198))},
    "bwd_merged_kb1": {"dq": (0.4956, 31, None, (1, 0, 0, 0)), "dk": (0.4959, 31, None, (1, 1, 0, 1)), "dv": (0.4983, 32, None, (1, 2, 0, 1))},
    "bwd_merged_kb2": {"dq": (0.4923, 129, None, (1, 0, 5, 3)), "dk": (0.4894, 129, None, (1, 0, 6, 2)), "dv": (0.4919, 129, None, (1, 0, 7, 3))},
    "bwd_merged_kb3": {"dq": (0.4809, 257, None, (0, 1, 7, 0)), "dk": (0.4818, 257, None, (0, 1, 10, 0)), "dv": (0.4845, 257, None, (1, 1, 13, 2))},
    "bwd_merged_kb4": {"dq": (0.4624, 385, None, (1, 1, 10, 3)), "dk": (0.4620, 385, None, (1, 1, 21, 3)), "dv": (0.4645, 385, None, (1, 1, 21, 3))},
    "bwd_merged_mx8": {"dq": (0.4923, 129, None, (1, 0, 5, 3)), "dk": (0.4911, 128, None, (1, 2, 1, 1)), "dv": (0.4934, 128, None, (1, 2, 4, 1))},
    "bwd_stream64": {"dq": (0.4499, 513, None, (1, 2, 8, 0)), "dk": (0.4507, 513, None, (1, 0, 10, 3)), "dv": (0.4544, 513, None, (0, 0, 11, 2))},
    "bwd_stream64_raw": {"dq": (0.4955, 33, None, (1, 2, 0, 0)), "dk": (0.4952, 33, None, (0, 0, 0, 3)), "dv": (0.4977, 33, None, (1, 2, 0, 0))},
    "bwd_stream32": {"dq": (0.4986, 12, None, (1, 2, 0, 0)), "dk": (0.4985, 12, None, (1, 2, 0, 1)), "dv": (0.4993, 12, None, (0, 2, 0, 1))},
    "bwd_stream128": {"dq": (0.4882, 17, None, (1, 1, 0, 7)), "dk": (0.4905, 17, None, (1, 1, 0, 6)), "dv": (0.5133, 129, None, (1, 1, 3, 5))},
    "masked_f32": {"o": (0.3974, 40, None, (1, 0, 2, 0)), "lse2": (0.0172, 40, None, (1, 1, 24)), "dq": (0.4466, 40, None, (0, 0, 2, 0)),
                   "dk": (0.4619, 40, None, (0, 0, 2, 1)), "dv": (0.4175, 40, None, (0, 0, 2, 1))},
    "regime_fwd": {"o": (0.0669, 324, "descending", (0, 0, 4, 1)), "lse2": (0.2781, 324, "ramp", (0, 2, 183))},
    "regime_bwd": {"dq": (0.0339, 324, "descending", (0, 1, 15, 0)), "dk": (0.0233, 512, "very_negative", (1, 2, 13, 1)),
                   "dv": (0.0307, 512, "descending", (1, 2, 30, 0))},
}
