"""Test kit of the short-sequence fused layer kernels (csrc/layer_small.hip: layer_fwd_small, layer_bwd_small_a, layer_bwd_small_b
with and without the fused attention backward), shared by tests/test_gpu_small_layer.py (the kernels) and
tests/test_small_layer_ref_cpu.py (the kit itself, without a device).  Everything here runs on the CPU in fp64; a caller hands in
what the code under test produced.

Three things live here:

  CASES      the shapes: every (dim, inner, mlp) triple the kernels are built for, token counts at and around the 16-row block,
             1 / 3 / 130 clips, one and two layers, dropout off and on, both residual-gradient streams.
  model()    ONE hand-written forward + backward of the stack in fp64.  With rounding off it IS the reference
             (tests/test_small_layer_ref_cpu.py holds it against oracle.transformer_forward + autograd); with rounding on it
             rounds to bf16 exactly where layer_small.hip stores bf16 - the rounded model, from which every group bound below is
             derived; with a fault switched on it is a wrong kernel, which the bounds must catch.
  grouped_errors() / CAPS   relative Frobenius error per token row, per 16-column block (one wavefront's share of a GEMM), per
             16-row block and q / k / v part of a weight gradient, against whole-tensor caps that are the project's own.

Nothing in CAPS comes from what the kernels produce: MODEL_WORST is the rounded model against the fp64 reference on the CPU
(`python tests/small_layer_util.py` prints it), and a group cap is BOUND_FACTOR x that figure.
"""
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import oracle  # noqa: E402

LOG2E = math.log2(math.e)
DH = 32
BOUND_FACTOR = 3.0  # the margin the project gives a measured low-precision error (tests/gpu_util.py)

# ---------------------------------------------------------------------------------------------- cases
# (B, N, D, H, M, depth, dropout p, residual-gradient stream); inner = 32 H.  With live dropout a short-sequence layer always
# runs the fp32 gradient stream (Transformer._grad_stream_bf16), so "bf16" appears at p = 0 only; "f32" at p = 0 is
# AVF_GRAD_STREAM=f32.
CASES = [
    (3, 12, 256, 4, 128, 1, 0.0, "bf16"),     # D > inner: the LDS operand stride comes from D, o has width inner
    (3, 16, 256, 4, 256, 1, 0.0, "bf16"),     # D > inner, the full 16-row block
    (3, 2, 256, 4, 128, 1, 0.0, "f32"),       # D > inner, the two-token VA shape
    (3, 15, 256, 4, 256, 1, 0.25, "f32"),     # D > inner, one padded row
    (130, 16, 256, 4, 128, 1, 0.0, "bf16"),   # 130 per-clip partial rows in the bias / LayerNorm gradient fold
    (3, 12, 128, 8, 128, 2, 0.25, "f32"),     # D < inner; two layers with dropout: hand-off image under layer 0's site-2 mask
    (3, 16, 128, 8, 256, 1, 0.0, "f32"),      # D < inner
    (3, 2, 128, 8, 256, 2, 0.0, "bf16"),      # D < inner; the two-layer, two-token VA former
    (1, 15, 128, 8, 128, 1, 0.0, "bf16"),     # D < inner
    (130, 12, 128, 8, 256, 1, 0.25, "f32"),
    (3, 13, 256, 8, 256, 1, 0.0, "bf16"),
    (3, 7, 128, 4, 128, 1, 0.0, "bf16"),
    (3, 1, 256, 8, 128, 1, 0.0, "bf16"),      # one token: dq = dk = 0 exactly
    (1, 1, 128, 4, 256, 1, 0.25, "f32"),
    (3, 12, 256, 8, 256, 2, 0.25, "f32"),     # former_AU_head's widths, two layers, dropout
    (130, 7, 256, 8, 128, 1, 0.0, "f32"),
    (3, 13, 128, 4, 256, 2, 0.0, "f32"),      # two layers on the fp32 stream: fp32 dx beside the bf16 hand-off image
    (1, 16, 128, 4, 128, 1, 0.25, "f32"),
    (3, 2, 256, 4, 256, 1, 0.25, "f32"),      # D > inner
    (130, 2, 128, 8, 128, 1, 0.0, "bf16"),
    (1, 13, 128, 8, 256, 1, 0.25, "f32"),
    (3, 12, 128, 8, 256, 1, 0.0, "bf16"),     # AU_former's widths
    (130, 15, 256, 4, 128, 1, 0.25, "f32"),
    (3, 7, 256, 4, 256, 2, 0.0, "bf16"),      # D > inner, two layers on the bf16 stream (the hand-off image is all there is)
]


def case_id(c):
    B, N, D, H, M, L, p, gs = c
    return f"B{B}_N{N}_D{D}_I{32 * H}_M{M}_L{L}_p{int(100 * p)}_{gs}"


def case_seed(c):
    B, N, D, H, M, L, p, gs = c
    return 1000 + 7 * B + 131 * N + D + 3 * H + 5 * M + 11 * L + (17 if p else 0) + (29 if gs == "f32" else 0)


# ---------------------------------------------------------------------------------------------- inputs
# With init_transformer_state weights the attention branch is a tenth of the residual it is added to and the softmax is nearly
# uniform: a wrong attention core then moves y by less than its cap (test_default_init_hides_the_attention_core keeps the
# figures).  GAIN_QK multiplies the q and k rows of to_qkv.weight (scores x GAIN_QK^2); GAIN_OUT multiplies to_out.0.weight and
# net.3.weight of layer 0, GAIN_OUT_DEEP those of layer 1.  Conditions (test_inputs_make_every_phase_count), in the fp64 reference
# of every case: for N >= 7 the median over (clip, head, query) of the largest softmax probability in PMAX_RANGE; attention
# branch and MLP branch of every layer with rms in BRANCH_RANGE x rms(x), x the stack's input.
# Achieved (`python tests/small_layer_util.py` prints them per case): largest probability 0.33 .. 0.52 over the cases with
# N >= 7 (0.75 .. 1 below); attention branch 0.52 .. 1.25, MLP branch 0.51 .. 0.93; at the AU head's shape (3 x 12, D = I = M = 256,
# two layers, p = 0.25): 0.40 / 0.70 / 0.85 in layer 0, 0.38 / 0.61 / 0.70 in layer 1.
# How the gains were chosen.  Every fault of test_small_layer_ref_cpu.py is caught at 2.6 x its cap or more anywhere between
# gains 2 / 3 and 2.5 / 3.5 (2.6 x at the gains chosen), so sensitivity does not decide; the rounded model's error does.  It grows with GAIN_QK (a sharper
# softmax amplifies the bf16 rounding of P and dS: at 3 / 3 the worst dx row of a 130-clip case errs by 4.7e-2 against the 2e-2 that
# a group cap of at most twice the whole-tensor cap leaves a model that must keep a third of it) and with the branch / residual
# ratio.  2.2 is the smallest GAIN_QK that keeps the largest probability above 0.3 with margin, 3.3 the smallest GAIN_OUT that keeps the
# attention branch of a 15- or 16-token clip (which averages about three values per query) above 0.5.  A second layer's branches come
# out of a LayerNorm, so at equal gain they have layer 0's rms while the residual they join has grown by layer 0's two branches:
# two layers of rounding then exceed a third of the caps on y and dx (5.2e-3 / 1.08e-2 at 3.3 / 3.3).  GAIN_OUT_DEEP = 2.6 keeps
# layer 1's branches above 0.5 x rms(x); against its OWN input (rms 1.3 .. 1.5) they are 0.36 .. 0.6.
GAIN_QK = 2.2
GAIN_OUT = 3.3
GAIN_OUT_DEEP = 2.6
PMAX_RANGE = (0.3, 0.8)
BRANCH_RANGE = (0.5, 2.0)


def make_inputs(case, default_init=False):
    """-> (sd: fp32 state dict, x: fp32 [B, N, D]); default_init: the inputs of test_transformer_vs_oracle (no gains)"""
    B, N, D, H, M, L, p, gs = case
    g = torch.Generator().manual_seed(123 if default_init else case_seed(case))
    sd = oracle.init_transformer_state(D, L, H, DH, M, generator=g)
    for k in sd:  # non-trivial LayerNorm affine, as test_transformer_vs_oracle
        if k.endswith("norm.weight"):
            sd[k] = 1 + 0.1 * torch.randn(D, generator=g)
        if k.endswith("norm.bias"):
            sd[k] = 0.1 * torch.randn(D, generator=g)
    if not default_init:
        I = H * DH
        for l in range(L):
            sd[f"layers.{l}.0.fn.fn.to_qkv.weight"][:2 * I] *= GAIN_QK
            sd[f"layers.{l}.0.fn.fn.to_out.0.weight"] *= GAIN_OUT if l == 0 else GAIN_OUT_DEEP
            sd[f"layers.{l}.1.fn.fn.net.3.weight"] *= GAIN_OUT if l == 0 else GAIN_OUT_DEEP
    x = torch.randn(B, N, D, generator=g)
    return sd, x


def cpu_drop_factors(case, seed=0):
    """keep / (1 - p) factors of the three sites of every layer from a torch generator (the CPU tests; the GPU test replays the
    kernels' own masks through ops.dropout_factors) -> [(f0 [B,N,D], f1 [B,N,M], f2 [B,N,D])] * depth, or None at p = 0"""
    B, N, D, H, M, L, p, gs = case
    if p == 0.0:
        return None
    g = torch.Generator().manual_seed(case_seed(case) + 77 + seed)
    mk = lambda cols: (torch.rand(B, N, cols, generator=g) >= p).double() / (1.0 - p)
    return [(mk(D), mk(M), mk(D)) for _ in range(L)]


# ---------------------------------------------------------------------------------------------- the model
FAULTS = ("pad_keys", "scale_10pct", "copy_last_row", "head0_reads_head1_k", "bwd_lse_shift", "site1_next_row",
          "handoff_mask_missing", "db1_last_clip", "ln2_last_clip", "ln1_last_clip")


def _r(t, on):
    """round to bf16 (through fp32, as the kernels do) when `on`"""
    return t.float().to(torch.bfloat16).double() if on else t


def _gelu(u):
    c = math.sqrt(2.0 / math.pi)
    return 0.5 * u * (1 + torch.tanh(c * (u + 0.044715 * u ** 3)))


def _dgelu(u):
    c = math.sqrt(2.0 / math.pi)
    t = torch.tanh(c * (u + 0.044715 * u ** 3))
    return 0.5 * (1 + t) + 0.5 * u * (1 - t * t) * c * (1 + 3 * 0.044715 * u * u)


def _ln_fwd(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt((x - mu).pow(2).mean(-1, keepdim=True) + eps)
    xh = (x - mu) * rs
    return xh * w + b, xh, rs


def _ln_bwd(dy, xh, rs, w):
    g = dy * w
    return rs * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))


def _heads(t, H):  # [B, N, H * dh] -> [B, H, N, dh]
    B, N, _ = t.shape
    return t.reshape(B, N, H, DH).permute(0, 2, 1, 3)


def _unheads(t):  # [B, H, N, dh] -> [B, N, H * dh]
    B, H, N, _ = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * DH)


def _names(l):
    p = f"layers.{l}"
    return dict(ln1_w=f"{p}.0.fn.norm.weight", ln1_b=f"{p}.0.fn.norm.bias", wqkv=f"{p}.0.fn.fn.to_qkv.weight",
                wo=f"{p}.0.fn.fn.to_out.0.weight", bo=f"{p}.0.fn.fn.to_out.0.bias", ln2_w=f"{p}.1.fn.norm.weight",
                ln2_b=f"{p}.1.fn.norm.bias", w1=f"{p}.1.fn.fn.net.0.weight", b1=f"{p}.1.fn.fn.net.0.bias",
                w2=f"{p}.1.fn.fn.net.3.weight", b2=f"{p}.1.fn.fn.net.3.bias")


def model(case, sd, x, drop=None, rounded=False, round_dh=False, stream=None, faults=(), stats=None):
    """Forward and backward (loss = y.pow(2).mean()) of the stack in fp64 -> (y [B N, D], dx [B N, D], {state-dict key: gradient}).

    rounded   round to bf16 where layer_small.hip stores bf16.  Forward: the four weight images (the q rows of to_qkv.weight
              pre-multiplied by log2(e)/sqrt(dh), as attn_q_prescale), h1, qkv, the un-normalised probabilities, o, h2, the saved
              pre-activation u and g - g from the UNROUNDED pre-activation.  Backward: gy, du, the masked dx_mid image, d_o, P, dS,
              dqkv and the hand-off image; the bias / LayerNorm column sums are taken of the unrounded fp32 values, as the kernels do.
    round_dh  also round dh2 and dh1, which the per-operator path stores in bf16 and the fused kernels keep in fp32.
    stream    "f32" / "bf16" residual-gradient stream (default: the case's).  On "bf16" the residual gradient a LayerNorm backward
              adds is the bf16 image, and no fp32 dx passes between layers.
    drop      [(f0, f1, f2)] * depth of keep/(1-p) factors, or None.
    faults    names out of FAULTS: the model then computes what a kernel with that defect would.
    stats     optional dict: receives per-layer input figures (median largest probability, branch rms ratios)."""
    B, N, D, H, M, L, p, gs = case
    stream = stream or gs
    gs16 = stream == "bf16"
    assert not (gs16 and drop is not None), "the short-sequence layer runs dropout on the fp32 gradient stream"
    assert all(f in FAULTS for f in faults), faults
    I = H * DH
    rd = rounded
    c = LOG2E / math.sqrt(DH)
    x = x.double()
    x0_rms = float(x.pow(2).mean().sqrt())
    P = {k: v.double() for k, v in sd.items()}
    one = torch.ones((), dtype=torch.float64)
    sv = []
    for l in range(L):  # ---------------------------------------------------------------- forward
        n = _names(l)
        f0, f1, f2 = drop[l] if drop is not None else (one, one, one)
        if "site1_next_row" in faults and drop is not None:
            f1 = torch.roll(f1.reshape(B * N, M), -1, 0).reshape(B, N, M)
        wqkv = P[n["wqkv"]]
        wq_img = _r(torch.cat([wqkv[:I] * c, wqkv[I:]], 0), rd)
        wqkv_t, wo, w1, w2 = _r(wqkv, rd), _r(P[n["wo"]], rd), _r(P[n["w1"]], rd), _r(P[n["w2"]], rd)
        y1, xh1, rs1 = _ln_fwd(x, P[n["ln1_w"]], P[n["ln1_b"]])
        h1 = _r(y1, rd)
        qkv = _r(h1 @ wq_img.t(), rd)
        q, k, v = (_heads(t, H) for t in qkv.split(I, -1))
        if "head0_reads_head1_k" in faults:
            k = k.clone()
            k[:, 0] = k[:, 1]
        s2 = q @ k.transpose(-1, -2)  # log2 domain: q carries log2(e)/sqrt(dh)
        if "scale_10pct" in faults:
            s2 = s2 * 1.1
        mx = s2.max(-1, keepdim=True).values
        npad = 16 - N if "pad_keys" in faults else 0  # zero-padded keys: score 0, v = 0
        if npad:
            mx = mx.clamp_min(0.0)
        pt = torch.exp2(s2 - mx)
        ssum = pt.sum(-1, keepdim=True) + npad * torch.exp2(-mx)
        o = _r((_r(pt, rd) @ v) / ssum, rd)
        lse2 = mx + torch.log2(ssum)
        if "copy_last_row" in faults and N >= 2:
            o = o.clone()
            o[:, :, N - 1] = o[:, :, N - 2]
        o = _unheads(o)
        a = (o @ wo.t() + P[n["bo"]]) * f0
        x_mid = a + x
        y2, xh2, rs2 = _ln_fwd(x_mid, P[n["ln2_w"]], P[n["ln2_b"]])
        h2 = _r(y2, rd)
        u = h2 @ w1.t() + P[n["b1"]]
        g = _r(_gelu(u) * f1, rd)
        m = (g @ w2.t() + P[n["b2"]]) * f2
        x_out = m + x_mid
        if stats is not None:
            rms = lambda t: float(t.pow(2).mean().sqrt())
            stats[l] = dict(pmax=float((pt / ssum).max(-1).values.median()), attn=rms(a) / x0_rms, mlp=rms(m) / x0_rms,
                            attn_own=rms(a) / rms(x), mlp_own=rms(m) / rms(x))
        sv.append(dict(xh1=xh1, rs1=rs1, h1=h1, q=q, k=k, v=v, s2=s2, lse2=lse2, o=o, xh2=xh2, rs2=rs2, h2=h2, u=_r(u, rd), g=g,
                       wqkv_t=wqkv_t, wo=wo, w1=w1, w2=w2, f=(f0, f1, f2)))
        x = x_out
    y = x
    grads = {}
    dxo = 2.0 * y / y.numel()  # fp32 stream entering the top layer
    lo = None                  # bf16 hand-off image from the layer above (carries THIS layer's site-2 mask)
    db2 = None                 # ... and its column sums
    cut = lambda t, name: (t[:-1] if name in faults and B > 1 else t).sum((0, 1))  # per-clip partial rows, last clip lost
    for l in reversed(range(L)):  # ------------------------------------------------------- backward
        n, s = _names(l), sv[l]
        f0, f1, f2 = s["f"]
        # kernel A: gy -> du -> dh2 -> LayerNorm-2 backward -> dx_mid, gm -> d_o
        if lo is None:
            gy = _r(dxo * f2, rd)
            db2 = (gy if drop is not None else dxo).sum((0, 1))
        else:
            gy = lo
        res2 = gy if gs16 else dxo
        du_f = (gy @ s["w2"]) * f1 * _dgelu(s["u"])
        du = _r(du_f, rd)
        dh2 = _r(du @ s["w1"], rd and round_dh)
        dx_mid = _ln_bwd(dh2, s["xh2"], s["rs2"], P[n["ln2_w"]]) + res2
        gm_f = dx_mid * f0
        gm = _r(gm_f, rd)
        d_o = _heads(_r(gm @ s["wo"], rd), H)
        # kernel B: attention backward from the saved projection, dh1, LayerNorm-1 backward
        q, k, v = s["q"], s["k"], s["v"]
        pr = torch.exp2(s["s2"] - (s["lse2"] + (0.1 if "bwd_lse_shift" in faults else 0.0)))
        dp = d_o @ v.transpose(-1, -2)
        delta = (d_o * _heads(s["o"], H)).sum(-1, keepdim=True)
        ds = _r(pr * (dp - delta), rd)
        dv = _r(pr, rd).transpose(-1, -2) @ d_o
        dk = ds.transpose(-1, -2) @ q / LOG2E
        dq = ds @ k / math.sqrt(DH)
        dqkv = _r(torch.cat([_unheads(dq), _unheads(dk), _unheads(dv)], -1), rd)
        dh1 = _r(dqkv @ s["wqkv_t"], rd and round_dh)
        res1 = gm if gs16 else dx_mid
        dx_in = _ln_bwd(dh1, s["xh1"], s["rs1"], P[n["ln1_w"]]) + res1
        grads[n["w2"]] = gy.reshape(-1, D).t() @ s["g"].reshape(-1, M)
        grads[n["b2"]] = db2
        grads[n["w1"]] = du.reshape(-1, M).t() @ s["h2"].reshape(-1, D)
        grads[n["b1"]] = cut(du_f, "db1_last_clip")
        grads[n["ln2_w"]] = cut(dh2 * s["xh2"], "ln2_last_clip")
        grads[n["ln2_b"]] = cut(dh2, "ln2_last_clip")
        grads[n["wo"]] = gm.reshape(-1, D).t() @ s["o"].reshape(-1, I)
        grads[n["bo"]] = gm_f.sum((0, 1))
        grads[n["wqkv"]] = dqkv.reshape(-1, 3 * I).t() @ s["h1"].reshape(-1, D)
        grads[n["ln1_w"]] = cut(dh1 * s["xh1"], "ln1_last_clip")
        grads[n["ln1_b"]] = cut(dh1, "ln1_last_clip")
        if l > 0:
            prev2 = one if "handoff_mask_missing" in faults else sv[l - 1]["f"][2]
            lo_f = dx_in * prev2
            lo, db2 = _r(lo_f, rd), lo_f.sum((0, 1))
        dxo = dx_in
    return y.reshape(B * N, D), dxo.reshape(B * N, D), grads


def reference_autograd(case, sd, x, drop=None):
    """the fp64 reference the GPU test compares against: oracle.transformer_forward on double tensors, autograd"""
    B, N, D, H, M, L, p, gs = case
    xd = x.double().clone().requires_grad_(True)
    ps = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    y = oracle.transformer_forward(xd, ps, L, H, drop=drop)
    y.pow(2).mean().backward()
    return y.detach().reshape(B * N, D), xd.grad.reshape(B * N, D), {k: v.grad for k, v in ps.items()}


# ---------------------------------------------------------------------------------------------- grouped errors
def _rel(a, b):
    return float((a - b).norm() / b.norm())


def _blocks(a, b, dim, out, kind, scale, zero_tol=1e-12):
    """relative error of every 16-wide block along `dim`; a block whose reference is exactly zero goes to `kind + ':zero'` with
    its largest |value| relative to the rms of the whole reference tensor"""
    for i in range(0, b.shape[dim], 16):
        ga, gb = a.narrow(dim, i, min(16, b.shape[dim] - i)), b.narrow(dim, i, min(16, b.shape[dim] - i))
        _group(ga, gb, out, kind, scale, zero_tol)


def _group(ga, gb, out, kind, scale, zero_tol=1e-12):
    # "exactly zero": the fp64 reference leaves rounding dust of 1e-16 of the tensor's scale where the value is 0
    if float(gb.abs().max()) <= zero_tol * scale:
        out[kind + ":zero"] = max(out.get(kind + ":zero", 0.0), float(ga.abs().max()) / scale)
    else:
        out[kind] = max(out.get(kind, 0.0), _rel(ga, gb))


def grouped_errors(y, dx, grads, ref, zero_tol=1e-12):
    """(y, dx [B N, D], {key: gradient}) against ref = (y, dx, grads) -> {kind: worst error of that kind}, the kinds of CAPS.
    Per-tensor detail for a failure message: grouped_errors_detail.  zero_tol: a group of `ref` within zero_tol x the rms of its
    tensor counts as exactly zero (path against path, where `ref` is itself a kernel's output: ZERO_REF_MAX)."""
    out = {}
    for name, err in grouped_errors_detail(y, dx, grads, ref, zero_tol).items():
        kind = name.split("|")[0]
        out[kind] = max(out.get(kind, 0.0), err)
    return out


def grouped_errors_detail(y, dx, grads, ref, zero_tol=1e-12):
    """-> {"kind|tensor": worst error of that kind within that tensor}"""
    y_ref, dx_ref, g_ref = ref
    res = {}
    for nm, a, b in (("y", y, y_ref), ("dx", dx, dx_ref)):
        a, b = a.detach().double().cpu(), b.detach().double().cpu()
        res[f"{nm}.whole|{nm}"] = _rel(a, b)
        res[f"{nm}.row|{nm}"] = float(((a - b).norm(dim=1) / b.norm(dim=1)).max())
        o = {}
        _blocks(a, b, 1, o, f"{nm}.col", 1.0)
        res[f"{nm}.col|{nm}"] = o[f"{nm}.col"]
    for k, b in g_ref.items():
        a, b = grads[k].detach().double().cpu(), b.detach().double().cpu()
        if b.dim() == 1:
            res[f"vec.whole|{k}"] = _rel(a, b)
            continue
        scale = float(b.pow(2).mean().sqrt())
        o = {}
        _group(a, b, o, "g.whole", scale, zero_tol)
        _blocks(a, b, 0, o, "g.block", scale, zero_tol)
        _blocks(a, b, 1, o, "g.block", scale, zero_tol)
        if k.endswith("to_qkv.weight"):
            for part_a, part_b in zip(a.chunk(3, 0), b.chunk(3, 0)):
                _group(part_a, part_b, o, "g.qkv_part", scale, zero_tol)
        for kind, v in o.items():
            res[f"{kind}|{k}"] = v
    return res


# ---------------------------------------------------------------------------------------------- caps
# Whole-tensor caps: the project's own (test_transformer_vs_oracle: 1.5e-2 y, 3e-2 dx, 4e-2 gradients;
# test_shape_sweep_bf16_vs_parity_mode: 6e-2 for vectors of at most 2048 elements - every vector here has at most 256).
WHOLE_CAPS = {"y.whole": 1.5e-2, "dx.whole": 3e-2, "g.whole": 4e-2, "vec.whole": 6e-2}
GROUP_OF = {"y.row": "y.whole", "y.col": "y.whole", "dx.row": "dx.whole", "dx.col": "dx.whole", "g.block": "g.whole",
            "g.qkv_part": "g.whole"}
# The rounded model against the fp64 reference, worst over CASES, on the CPU at GAIN_QK / GAIN_OUT above
# (`python tests/small_layer_util.py`; test_model_figures_are_the_recorded_ones recomputes them).  No kernel output enters.
# (rounded up in the fourth digit; the CPU test wants the recomputed figure within [0.9, 1] x the recorded one)
#                                       cap = min(3 x figure, 2 x whole-tensor cap)
MODEL_WORST = {
    "y.whole": 4.777e-3,    # whole-tensor cap 1.5e-2
    "y.row": 9.176e-3,      # 2.75e-2
    "y.col": 5.227e-3,      # 1.57e-2
    "dx.whole": 9.859e-3,   # whole-tensor cap 3e-2
    "dx.row": 1.750e-2,     # 5.25e-2
    "dx.col": 1.103e-2,     # 3.31e-2
    "g.whole": 9.234e-3,    # whole-tensor cap 4e-2
    "g.block": 2.049e-2,    # 6.15e-2
    "g.qkv_part": 1.361e-2,  # 4.08e-2
    "vec.whole": 8.728e-3,  # whole-tensor cap 6e-2
}
# A group whose reference is exactly zero (at N = 1 the q and k rows of to_qkv.weight's gradient: a single key has probability 1
# and dS = P (dP - delta) = 0): largest |value| over the rms of the whole reference tensor.  The kernels form dP (an MFMA) and delta
# (an fma chain) separately from bf16 operands in fp32, so the difference is fp32 rounding of two 32-term sums, 2^-24 x a few,
# times bf16 factors of order one: 1e-5 of the tensor's scale is two decades above that and three below a real dq.
ZERO_REF_MAX = 1e-5
# Path against path (test_gpu_small_layer.py part c).  Forward: results two bf16 roundings apart, the project's figure
# (tests/test_gpu_mask.py::test_all_kept_equals_no_mask).  Backward: BOUND_FACTOR x the difference between the rounded model's two
# variants - dh2 / dh1 kept in fp32 (the fused kernels) or rounded to bf16 (the per-operator path) - worst over CASES:
PATH_FWD_BOUND = 4e-3
MODEL_VARIANT_DIFF = {     # bound = 3 x figure
    "dx.whole": 4.770e-3,   # 1.43e-2
    "dx.row": 6.876e-3,     # 2.06e-2
    "dx.col": 5.558e-3,     # 1.67e-2
    "g.whole": 4.532e-3,    # 1.36e-2
    "g.block": 9.144e-3,    # 2.74e-2
    "g.qkv_part": 5.307e-3,  # 1.59e-2
    "vec.whole": 4.665e-3,  # 1.40e-2
}


def _caps():
    caps = dict(WHOLE_CAPS)
    for kind, whole in GROUP_OF.items():
        caps[kind] = min(BOUND_FACTOR * MODEL_WORST[kind], 2.0 * WHOLE_CAPS[whole])
    for kind in ("g.whole", "g.block", "g.qkv_part"):
        caps[kind + ":zero"] = ZERO_REF_MAX
    return caps


def _path_bounds():
    b = {k: BOUND_FACTOR * v for k, v in MODEL_VARIANT_DIFF.items()}
    for kind in ("g.whole", "g.block", "g.qkv_part"):
        b[kind + ":zero"] = ZERO_REF_MAX
    for kind in ("y.whole", "y.row", "y.col"):
        b[kind] = PATH_FWD_BOUND
    return b


CAPS = _caps()
PATH_BOUNDS = _path_bounds()


# ---------------------------------------------------------------------------------------------- on the device
def set_grad_stream(case, setenv, delenv):
    """AVF_GRAD_STREAM for a case (read per call by Transformer._grad_stream_bf16): "f32" where the case asks for the fp32 stream
    without dropout (with dropout the short-sequence layer takes it by itself), unset otherwise"""
    if case[7] == "f32" and case[6] == 0.0:
        setenv("AVF_GRAD_STREAM", "f32")
    else:
        delenv("AVF_GRAD_STREAM")


def gpu_run(case, index):
    """one forward + backward of the case on the HIP path -> dict(y, dx [B N, D], grads, seed, path); the caller has set
    AVF_GRAD_STREAM.  torch.manual_seed and the module's seed salt are fixed per case, so two processes that run the same case
    draw the same dropout seed (the caller compares `seed`)."""
    import avformer_amd as A
    B, N, D, H, M, L, p, gs = case
    sd, x = make_inputs(case)
    torch.manual_seed(case_seed(case))
    t = A.Transformer(D, L, H, DH, M, dropout=p, compute_dtype="bf16")
    t._seed_salt = 1 + index  # (construction order otherwise: other tests of the process have built modules before this one)
    t.load_state_dict(sd)
    t = t.to("cuda").train()
    cfg = t._cfg(B, N)
    assert bool(cfg.grad_stream_bf16) == (gs == "bf16"), (case, cfg.grad_stream_bf16)
    path = A.ops.layer_small_path(cfg)
    xg = x.to("cuda").requires_grad_(True)
    y = t(xg)
    y.pow(2).mean().backward()
    torch.cuda.synchronize()
    return dict(y=y.detach().reshape(B * N, D).cpu(), dx=xg.grad.reshape(B * N, D).cpu(),
                grads={k: v.grad.cpu() for k, v in t.named_parameters()}, seed=t.last_seed if p > 0.0 else 0, path=path)


def device_drop_factors(case, seed):
    """the masks the kernels drew under `seed`, through the C ABI (as tests/test_gpu_dropout.py::test_mask_replay_against_oracle)"""
    import avformer_amd as A
    B, N, D, H, M, L, p, gs = case
    return [tuple(A.ops.dropout_factors(seed, l, s, p, B * N, cols).cpu().double().view(B, N, cols)
                  for s, cols in ((0, D), (1, M), (2, D))) for l in range(L)]


def child_main(outdir, expect_path):
    """body of a child process of test_gpu_small_layer.py part (c): every case once under the tuning switch of the environment"""
    for i, case in enumerate(CASES):
        set_grad_stream(case, os.environ.__setitem__, lambda k: os.environ.pop(k, None))
        r = gpu_run(case, i)
        assert r["path"] == expect_path, (case_id(case), r["path"], expect_path)
        torch.save(r, os.path.join(outdir, f"{i}.pt"))
    print("SMALL_LAYER_CHILD_OK")


# ---------------------------------------------------------------------------------------------- figures
def measure(cases=CASES, verbose=False):
    """-> (MODEL_WORST, MODEL_VARIANT_DIFF, per-case input figures) recomputed on the CPU"""
    worst, diff, figs = {}, {}, {}
    for case in cases:
        sd, x = make_inputs(case)
        drop = cpu_drop_factors(case)
        st = {}
        ref = model(case, sd, x, drop, stats=st)
        fused = model(case, sd, x, drop, rounded=True)
        perop = model(case, sd, x, drop, rounded=True, round_dh=True)
        e = grouped_errors(*fused, ref)
        d = grouped_errors(*perop, fused)
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        for k, v in d.items():
            diff[k] = max(diff.get(k, 0.0), v)
        figs[case_id(case)] = st
        if verbose:
            print(case_id(case), " ".join(f"L{l}: pmax {s['pmax']:.2f} attn {s['attn']:.2f} mlp {s['mlp']:.2f}" for l, s in st.items()))
            print("    model  ", " ".join(f"{k} {v:.2e}" for k, v in sorted(e.items())))
            print("    variant", " ".join(f"{k} {v:.2e}" for k, v in sorted(d.items())))
    return worst, diff, figs


if __name__ == "__main__":
    w, d, _ = measure(verbose=True)
    print("MODEL_WORST", {k: float(f"{v:.2e}") for k, v in sorted(w.items())})
    print("MODEL_VARIANT_DIFF", {k: float(f"{v:.2e}") for k, v in sorted(d.items())})
