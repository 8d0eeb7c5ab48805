"""Masked-attention test kit shared by tests/test_gpu_mask_core.py (the HIP kernels a bf16 layer runs under a token mask) and
tests/test_mask_attn_ref_cpu.py (the kit itself, without a device).  Everything here runs on the CPU; a caller hands in what
the code under test produced.

Reference (reference models/heads.py:222-237 with the mask of 225-232), in fp64 on the stored bf16 operands:
    dots = q k^T dh^-0.5 ; dots.masked_fill_(~(keep_q & keep_k), -FLT_MAX) ; attn = softmax(dots) ; out = attn v
A kept query gives dropped keys exactly zero weight; a dropped query's row is one constant, so it attends uniformly to ALL N
keys (out = mean of v) and passes no gradient to q or k - only d_o / N to every row of dv.

The device operand is the bf16 projection with PRE-SCALED q (q' = bf16(q log2(e)/sqrt(dh)), what a bf16 layer's Wqkv image
produces); the reference undoes the factor in fp64, so it sees the very numbers the kernels see.

Grouped error: relative Frobenius error of o, dq, dk, dv separately over the rows of KEPT tokens and over the rows of DROPPED
ones - a dropped query's output row has about 1/sqrt(N) of a kept row's norm, so a whole-tensor norm cannot see it - and the
same two groups once more for clip 0 alone, which carries the named pattern (clip 1 is always random).
"""
import math

import torch

LOG2E = math.log2(math.e)
FLT_MAX = torch.finfo(torch.float32).max

# the caps of tests/test_gpu_mask.py::test_masked_attention_core_vs_fp64 (o; 2 x for each gradient), of
# tests/test_gpu_ops.py::test_attention_bf16 (lse2) and ::test_attention_bf16_rescale_paths (lse2 and dqkv under the score regimes)
CAP_O = 1.2e-2
CAP_GRAD = 2.4e-2
LSE_TOL = dict(atol=2e-2, rtol=1e-3)
LSE_TOL_REGIME = dict(atol=5e-2, rtol=2e-3)
# DERIVED, not measured: test_attention_bf16_rescale_paths allows 3e-2 for the unmasked dqkv, and the masked core test allows
# 1.2 x the unmasked cap of test_attention_bf16 (1.2e-2 against 1e-2) - the same ratio here
CAP_DQKV_REGIME = 3e-2 * 1.2
ZERO_REF_MAX_ABS = 1e-2  # where the reference's group is exactly 0 (tests/test_gpu_ops.py::test_attention_bf16_dh64_lengths at N = 1)


# ---------------------------------------------------------------------------------------------- operands
def prescale_q(qkv, H, dh):
    """bf16 projection with q' = bf16(q * log2(e)/sqrt(dh)) in the q columns, and the fp32 projection it stands for:
    (q'/c | k | v) exactly, so that the reference sees the very numbers the kernels see"""
    c = LOG2E / math.sqrt(dh)
    I = H * dh
    dev = qkv.float().clone()
    dev[:, :I] = (dev[:, :I] * c).to(torch.bfloat16).float()
    ref = dev.clone()
    ref[:, :I] = ref[:, :I] / c
    return dev.to(torch.bfloat16), ref


REGIMES = ("ramp", "small_steps", "huge", "descending", "very_negative")


def regime_qk(mode, q, k, u):
    """q [N, dh], k [N, dh] ~ randn and a unit vector u -> (q, k) whose scores exercise one rescale path of the head-resident
    forward (tests/test_gpu_ops.py::test_attention_bf16_rescale_paths describes them)"""
    N = q.shape[0]
    t = torch.arange(N).float()[:, None] / 64.0
    if mode == "ramp":      # score(q_i, k_j) ~ 8 * 6 * j/64 / 8 ... grows ~6 nats per 64 keys
        return q * 0.2 + 8.0 * u, k * 0.2 + u[None, :] * t * 6.0
    if mode == "small_steps":  # ~2.5 nats (3.6 in log2) per tile: below the threshold of 6
        return q * 0.2 + 8.0 * u, k * 0.2 + u[None, :] * t * 2.5
    if mode == "descending":  # the first tile holds the row maxima; later tiles fall by ~6 nats per 64 keys
        return q * 0.2 + 8.0 * u, k * 0.2 - u[None, :] * t * 6.0
    if mode == "very_negative":  # every score ~ -250 nats: the first tile must centre the maximum far below zero
        return q * 0.2 + 40.0 * u, k * 0.2 - 50.0 * u[None, :]
    assert mode == "huge", mode
    return q * 30.0, k * 30.0


def make_operands(B, N, H, dh, seed, regime=None):
    """-> (qkv bf16 [B N, 3 H dh] with pre-scaled q, d_o bf16 [B N, H dh])"""
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
    return prescale_q(qkv.to(torch.bfloat16), H, dh)[0], d_o


def hide_dropped(qkv, keep, H, dh):
    """the q and k columns of every dropped token replaced by x * 40 + 7 (v stays: a dropped token's v IS read, by dropped
    queries): scores that the mask discards then reach thousands of nats, far above any kept row's lse"""
    I = H * dh
    out = qkv.float().clone()
    rows = ~keep.reshape(-1)
    out[rows, :2 * I] = out[rows, :2 * I] * 40.0 + 7.0
    return out.to(qkv.dtype)


# ---------------------------------------------------------------------------------------------- reference
def reference(qkv, keep, B, N, H, dh, d_o=None):
    """fp64.  qkv: the bf16 device operand (pre-scaled q); keep bool [B, N]
    -> dict(o [B N, I], lse2 [B, H, N] (meaningful for kept queries), dqkv [B N, 3 I] or None, max_discarded: the largest
    score, in nats, that the mask threw away)"""
    I = H * dh
    x = qkv.double()
    x[:, :I] = x[:, :I] / (LOG2E / math.sqrt(dh))
    x.requires_grad_(True)
    q, k, v = [t.reshape(B, N, H, dh).permute(0, 2, 1, 3) for t in x.split(I, dim=-1)]
    s = (q @ k.transpose(-1, -2)) * dh ** -0.5
    pair = keep[:, None, :, None] & keep[:, None, None, :]
    discarded = s.detach()[(~pair).expand_as(s)]
    s = s.masked_fill(~pair, -FLT_MAX)
    o = (s.softmax(-1) @ v).permute(0, 2, 1, 3).reshape(B * N, I)
    lse2 = torch.logsumexp(s.detach(), dim=-1) * LOG2E
    dqkv = None
    if d_o is not None:
        o.backward(d_o.double())
        dqkv = x.grad
    return dict(o=o.detach(), lse2=lse2, dqkv=dqkv, max_discarded=float(discarded.max()) if discarded.numel() else None)


# ---------------------------------------------------------------------------------------------- masks
def _all_kept(N, g):
    return torch.ones(N, dtype=torch.bool)


def _random30(N, g):
    return torch.rand(N, generator=g) > 0.3


def _token0_dropped(N, g):
    m = torch.rand(N, generator=g) > 0.3
    m[0] = False
    return m


def _first_tile_dropped(N, g):
    m = torch.rand(N, generator=g) > 0.3
    m[:64] = False
    m[64] = True
    return m


def _middle_tile_dropped(N, g):
    m = torch.rand(N, generator=g) > 0.3
    m[64:128] = False
    m[0] = m[128] = True
    return m


def _last_only(N, g):
    m = torch.zeros(N, dtype=torch.bool)
    m[N - 1] = True
    return m


def _one_in_the_middle(N, g):
    m = torch.zeros(N, dtype=torch.bool)
    m[N // 2] = True
    return m


def _none_kept(N, g):
    return torch.zeros(N, dtype=torch.bool)


def _alternating(N, g):
    return torch.arange(N) % 2 == 1  # (token 0 dropped)


# name -> (builder of one clip's keep [N], smallest N it fits)
PATTERNS = {
    "all_kept": (_all_kept, 1), "random30": (_random30, 1), "token0_dropped": (_token0_dropped, 1),
    "first_tile_dropped": (_first_tile_dropped, 65), "middle_tile_dropped": (_middle_tile_dropped, 129),
    "last_only": (_last_only, 1), "one_in_the_middle": (_one_in_the_middle, 1), "none_kept": (_none_kept, 1),
    "alternating": (_alternating, 1),
}


def fits(pattern, N):
    return N >= PATTERNS[pattern][1]


def patterns_for(N, names=None):
    return [p for p in (names or PATTERNS) if fits(p, N)]


def make_keep(pattern, B, N, seed=0):
    """keep bool [B, N]: clip 0 carries the named pattern, every further clip random30 with token 0 dropped"""
    assert fits(pattern, N), (pattern, N)
    g = torch.Generator().manual_seed(7919 * seed + N)
    rows = [PATTERNS[pattern][0](N, g)] + [_token0_dropped(N, g) for _ in range(B - 1)]
    return torch.stack(rows)


# ---------------------------------------------------------------------------------------------- the cases of the GPU file
B_, H_ = 2, 2
LENGTHS_MFMA = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 383, 384, 385, 511, 512)
CASES_MFMA = [(N, p) for N in LENGTHS_MFMA for p in patterns_for(N)]
SHAPES_VEC = ((513, 64), (576, 64), (577, 64), (40, 32), (100, 32), (40, 128), (130, 128))
CASES_VEC = [(N, dh, p) for N, dh in SHAPES_VEC for p in ("random30", "token0_dropped", "none_kept")]
CASES_REGIME = [(N, r, p) for N in (324, 512) for r in ("ramp", "small_steps", "descending", "very_negative")
                for p in ("first_tile_dropped", "middle_tile_dropped", "random30")]
CASES_HIDDEN = [(N, p) for N in (65, 200, 324, 512) for p in ("random30", "first_tile_dropped")]
LENGTHS_ALL_KEPT = (64, 324, 512)


def case_inputs(N, dh, pattern, regime=None):
    """the operands of one GPU case (B = 2, H = 2) -> (qkv, d_o, keep)"""
    seed = 100000 + 131 * N + dh + 17 * list(PATTERNS).index(pattern) + (1000 * (1 + REGIMES.index(regime)) if regime else 0)
    qkv, d_o = make_operands(B_, N, H_, dh, seed, regime)
    return qkv, d_o, make_keep(pattern, B_, N, seed)


# ---------------------------------------------------------------------------------------------- grouped error
def row_groups(keep):
    """-> {name: bool [B N]} - kept / dropped token rows of all clips and of clip 0 alone; empty groups are left out"""
    B, N = keep.shape
    flat = keep.reshape(-1)
    clip0 = torch.zeros(B, N, dtype=torch.bool)
    clip0[0] = True
    clip0 = clip0.reshape(-1)
    groups = {"kept": flat, "dropped": ~flat, "kept0": flat & clip0, "dropped0": ~flat & clip0}
    return {k: v for k, v in groups.items() if bool(v.any())}


def grouped_errors(got, ref, keep, parts):
    """got, ref [B N, C]; parts: {name: column slice} -> {(part, group): ("rel", relative Frobenius error) or, where the
    reference's group is exactly 0, ("abs", largest absolute value)}"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    out = {}
    for gname, rows in row_groups(keep).items():
        for pname, sl in parts.items():
            a, b = got[rows][:, sl], ref[rows][:, sl]
            nb = float(b.norm())
            if nb == 0.0:
                out[(pname, gname)] = ("abs", float(a.abs().max()))
            else:
                out[(pname, gname)] = ("rel", float((a - b).norm()) / nb)
    return out


def grad_parts(H, dh):
    I = H * dh
    return {"dq": slice(0, I), "dk": slice(I, 2 * I), "dv": slice(2 * I, 3 * I)}


def assert_grouped(tag, errs, cap, check=None):
    """every group within its cap (check(tag, err, cap): gpu_util.check, which also holds the calibrated bound; None: the cap
    alone); a group whose reference is 0 within ZERO_REF_MAX_ABS.  -> the largest relative error"""
    worst = 0.0
    for (pname, gname), (kind, e) in sorted(errs.items()):
        assert math.isfinite(e), f"{tag}:{pname}:{gname}: not finite"
        if kind == "abs":
            assert e <= ZERO_REF_MAX_ABS, f"{tag}:{pname}:{gname}: reference is 0, got max |x| = {e:.3e} > {ZERO_REF_MAX_ABS:g}"
            continue
        c = cap[pname] if isinstance(cap, dict) else cap
        if check is not None:
            check(f"{tag}:{pname}:{gname}", e, c)
        else:
            assert e <= c, f"{tag}:{pname}:{gname}: {e:.3e} > cap {c:.1e}"
        worst = max(worst, e)
    return worst
