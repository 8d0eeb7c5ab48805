#!/usr/bin/env python3
"""Per-operator micro-benchmarks on the MI355X (tuning aid; not part of the product path).
usage: python tools/bench_ops.py [gemm_nt|gemm_tn|attn|ln|all] [--rows R]
       python tools/bench_ops.py eval --batch ROWS     (the evaluation metrics; not part of "all")"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import avformer_amd as A  # noqa: E402

ops = A.ops


def timeit(fn, iters=30, warm=5):
    """seconds per call, from the library's HIP-event brackets around the kernel launches (host overhead excluded)"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    A._lib.timing_enable(True)
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    A._lib.timing_enable(False)
    tm = A._lib.timing_read()
    ms = sum(v["ms"] for v in tm.values())
    return ms / iters * 1e-3


def gemm_nt(R):
    D, I, M = 512, 512, 1024
    shapes = [("qkv", R, 3 * I, D, ops.EPI_NONE, torch.bfloat16), ("out+res", R, D, I, ops.EPI_BIAS_RES, torch.float32),
              ("mlp1+gelu", R, M, D, ops.EPI_BIAS_GELU, torch.bfloat16), ("mlp2+res", R, D, M, ops.EPI_BIAS_RES, torch.float32),
              ("dX_w2+dgelu", R, M, D, ops.EPI_DGELU, torch.bfloat16), ("dX_w1", R, D, M, ops.EPI_NONE, torch.bfloat16),
              ("dX_qkv", R, D, 3 * I, ops.EPI_NONE, torch.bfloat16)]
    for name, m, n, k, epi, cdt in shapes:
        a = torch.randn(m, k, device="cuda").bfloat16()
        b = (torch.randn(n, k, device="cuda") / k ** 0.5).bfloat16()
        bias = torch.randn(n, device="cuda") if epi in (ops.EPI_BIAS_RES, ops.EPI_BIAS_GELU) else None
        res = torch.randn(m, n, device="cuda") if epi == ops.EPI_BIAS_RES else None
        aux = torch.randn(m, n, device="cuda").bfloat16() if epi in (ops.EPI_DGELU, ops.EPI_BIAS_GELU) else None
        fn = lambda: ops.gemm(a, b, out_dtype=cdt, epilogue=epi, bias=bias, residual=res, aux=aux)
        t = timeit(fn)
        print(f"gemm_nt {name:12s} M={m} N={n} K={k}: {t * 1e6:8.1f} us  {2.0 * m * n * k / t / 1e12:7.1f} TF/s")


def gemm_tn(R):
    D, I, M = 512, 512, 1024
    for name, m, n in [("dWqkv", 3 * I, D), ("dWo", D, I), ("dW1", M, D), ("dW2", D, M)]:
        a = torch.randn(R, m, device="cuda").bfloat16()
        b = torch.randn(R, n, device="cuda").bfloat16()
        fn = lambda: ops.gemm(a, b, trans_a=True, trans_b=False, out_dtype=torch.float32)
        t = timeit(fn)
        print(f"gemm_tn {name:12s} M={m} N={n} K={R}: {t * 1e6:8.1f} us  {2.0 * m * n * R / t / 1e12:7.1f} TF/s")


def gemm_tn_group(R):
    """the layer's four weight gradients as the grouped launch the backward uses"""
    D, I, M = 512, 512, 1024
    shapes = [(3 * I, D), (M, D), (D, M), (D, I)]
    pairs = [(torch.randn(R, m, device="cuda").bfloat16(), torch.randn(R, n, device="cuda").bfloat16()) for m, n in shapes]
    t = timeit(lambda: ops.gemm_tn_group(pairs))
    fl = sum(2.0 * m * n * R for m, n in shapes)
    print(f"gemm_tn_group (4 dW of a d=512 layer) K={R}: {t * 1e6:8.1f} us (GEMM + fold)  {fl / t / 1e12:7.1f} TF/s")


def attn(B, N, H=8, dh=64):
    qkv = torch.randn(B * N, 3 * H * dh, device="cuda").bfloat16()
    d_o = torch.randn(B * N, H * dh, device="cuda").bfloat16()
    o, lse = ops.attn_fwd(qkv, B, N, H, dh)
    t = timeit(lambda: ops.attn_fwd(qkv, B, N, H, dh))
    fl = 4.0 * B * H * N * N * dh
    print(f"attn_fwd B={B} N={N} H={H} dh={dh}: {t * 1e6:8.1f} us  {fl / t / 1e12:7.1f} TF/s")
    if N <= 576 and dh == 64:  # (the MX-FP8 output image exists on the dim_head-64 head-resident kernel only)
        t = timeit(lambda: ops.attn_fwd_mx8(qkv, B, N, H, dh))
        print(f"attn_fwd+mx8 image B={B} N={N}: {t * 1e6:8.1f} us")
    t = timeit(lambda: ops.attn_bwd(qkv, o, d_o, lse, B, N, H, dh))
    print(f"attn_bwd B={B} N={N} H={H} dh={dh}: {t * 1e6:8.1f} us  {2.5 * fl / t / 1e12:7.1f} TF/s (nominal 2.5x fwd flops)"
          f"  {2.0 * fl / t / 1e12:7.1f} TF/s (strict 2x)")


def ln(R):
    D = 512
    x = torch.randn(R, D, device="cuda")
    w = torch.randn(D, device="cuda")
    b = torch.randn(D, device="cuda")
    y, mean, rstd = ops.layernorm_fwd(x, w, b, 1e-5, torch.bfloat16)
    t = timeit(lambda: ops.layernorm_fwd(x, w, b, 1e-5, torch.bfloat16))
    print(f"ln_fwd R={R}: {t * 1e6:8.1f} us  {R * D * 6 / t / 1e9:7.1f} GB/s")
    dy = torch.randn(R, D, device="cuda").bfloat16()
    t = timeit(lambda: ops.layernorm_bwd(dy, x, w, mean, rstd, dres=x, want_lo=True, want_colsum=True))
    print(f"ln_bwd R={R}: {t * 1e6:8.1f} us  {R * D * 16 / t / 1e9:7.1f} GB/s")


def _profiled(fn, iters=20, warm=3):
    """(kernel launches, device microseconds, wall microseconds) per call of fn, from the torch profiler's device events"""
    import time
    from torch.profiler import ProfilerActivity, profile
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / iters * 1e6
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
          and "Memset" not in e.name]
    return len(ev) / iters, sum(e.time_range.elapsed_us() for e in ev) / iters, wall


def eval_metrics(rows):
    """one validation batch of `rows` rows: (a) EvalMetrics.update - the fused kernel; (b) the same statistics as plain torch ops
    on the device: MultiLabelAccF1.update_from_logits plus the EX and VA parts of update_torch; (c) the reference's host recipe of
    train.py:150-155 with its three device-to-host copies (wall time; the sklearn scoring at the end of the epoch is not in it)"""
    import numpy as np
    g = torch.Generator().manual_seed(0)
    out = torch.randn(rows, 21, generator=g).cuda()
    labels = {"EX": torch.randint(0, 8, (rows,), generator=g).cuda(), "AU": (torch.rand(rows, 12, generator=g) > 0.6).float().cuda(),
              "VA": (torch.rand(rows, 2, generator=g) * 2 - 1).cuda()}
    loss = torch.tensor(0.5, device="cuda")
    fused = A.EvalMetrics(device="cuda")
    M = A.metrics
    au, st = M.MultiLabelAccF1(ignore_index=-1), torch.zeros(128, dtype=torch.float64, device="cuda")

    def plain():
        au.update_from_logits(out, labels["AU"])
        st[M.EX_CONF:M.AU_STATS] += M.ex_confusion(torch.argmax(out[:, 12:19], dim=1), labels["EX"], 7).reshape(-1)
        st[M.VA_MOMENTS:M.LOSS_SUM] += M.va_moments(torch.tanh(out[:, 19:21]), labels["VA"], -5.0).reshape(-1)
        st[M.LOSS_SUM] += loss.double()
        st[M.LOSS_STEPS] += 1.0

    host = {"ex": [], "va": [], "au": [], "loss": 0.0}

    def reference():
        host["loss"] += loss.item()
        host["ex"].append((torch.argmax(out[:, 12:19], dim=1).detach().cpu().numpy().reshape(-1), labels["EX"].detach().cpu().numpy()))
        host["va"].append((torch.tanh(out[:, 19:21]).detach().cpu().numpy(), labels["VA"].detach().cpu().numpy()))
        host["au"].append((np.round(torch.sigmoid(out[:, :12]).detach().cpu().numpy()), labels["AU"].detach().cpu().numpy()))
        for v in (host["ex"], host["va"], host["au"]):
            del v[:-1]

    for name, fn in (("fused update", lambda: fused.update(out, labels, loss)), ("plain torch on the device", plain),
                     ("reference host recipe", reference)):
        n, dev_us, wall_us = _profiled(fn)
        print(f"eval rows={rows} {name:26s}: {n:5.1f} launches  {dev_us:8.1f} us device  {wall_us:8.1f} us wall per batch")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="?", default="all")
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--tokens", type=int, default=324)
    ap.add_argument("--heads", type=int, default=8, help="attn: heads")
    ap.add_argument("--dim-head", type=int, default=64, help="attn: head width (32, 64 or 128)")
    a = ap.parse_args()
    R = a.batch * a.tokens
    if a.what in ("gemm_nt", "all"):
        gemm_nt(R)
    if a.what in ("gemm_tn", "all"):
        gemm_tn(R)
    if a.what in ("gemm_tn_group", "all"):
        gemm_tn_group(R)
    if a.what in ("attn", "all"):
        attn(a.batch, a.tokens, a.heads, a.dim_head)
    if a.what in ("ln", "all"):
        ln(R)
    if a.what == "eval":
        eval_metrics(a.batch)
