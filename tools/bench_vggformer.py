"""The S-Former of the vggformer model (vggface2.VGGFormer: the frozen VGGFace2 ResNet-50, the 1x1 conv, one transformer layer)
forward on a batch of frames, the HIP path against the only path there was before it, on one box, in one process, the arms
alternated.

    python tools/bench_vggformer.py [--frames 1024] [--size 112] [--groups 7] [--calls 3] [--warmup 2]

  torch   VGGFormer(backend="torch"): the extractor as torch ops in fp32, NCHW - the yardstick
  hip     VGGFormer(backend="hip", stem="hip", conv_dtype="bf16"): the stem kernel in its ceil-mode pool geometry, 52 launches of
          the NHWC conv kernel, the 1x1 conv on the library's GEMM
The token section is this package's Transformer (compute_dtype="bf16") in both arms.  A timed window is --calls calls between two
device events under torch.no_grad(); the groups alternate over the arms after --warmup calls of each; the result is the median of
the groups.  Device operations per call are counted with torch.profiler, and the hip arm's stages - stem, layer1 .. layer4, the
1x1 conv with the positional add, the transformer - are profiled one by one for the sum of their kernels' device time.  This is a
record, no threshold: where the 1x1 convolutions of the Bottlenecks stand against the vendor library is what it is for.  Writes
<out-dir>/<name>.json (default profiles/ab/vggformer_backbone.json)."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_sum_ms(fn):
    """-> (sum of the device time of the kernels one call of fn enqueues in ms, their count), or (None, reason)"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
        if not ev:
            return None, "the profiler recorded no device event"
        us = sum(float(getattr(e, "device_time", None) or getattr(e, "cuda_time", 0.0) or e.time_range.elapsed_us()) for e in ev)
        return round(us / 1e3, 5), len(ev)
    except Exception as e:  # a by-product: the timing stands without it
        return None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--name", default="vggformer_backbone")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import device_ops, shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_vggformer.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m_t = A.VGGFormer(backend="torch").to(dev).eval()
    for p in m_t.parameters():
        p.requires_grad_(False)
    m_h = copy.deepcopy(m_t).set_backend("hip", stem="hip")
    x = torch.randn(args.frames, 3, args.size, args.size, device=dev)
    arms = {"torch": lambda: m_t(x), "hip": lambda: m_h(x)}
    clock_before = shader_clock()
    with torch.no_grad():
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        want = m_t(x)
        err = float((m_h(x) - want).norm() / want.norm())
        runs = {k: [] for k in arms}
        for r in range(args.groups):
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fn()
                e1.record()
                e1.synchronize()
                runs[name].append(round(e0.elapsed_time(e1) / args.calls, 5))
            print(f"group {r + 1}: " + "  ".join(f"{k} {v[-1]:.3f}" for k, v in runs.items()) + " ms", flush=True)
        med = {k: statistics.median(v) for k, v in runs.items()}
        ops_count = {k: device_ops(fn)[0] for k, fn in arms.items()}

        # the hip arm stage by stage, each on the input the stage before it left
        v = m_h.VGG_model
        stages, h = {}, x
        steps = [("stem", v.stem_nhwc)] + [(n, getattr(v, n).forward_nhwc) for n in ("layer1", "layer2", "layer3", "layer4")]
        for name, fn in steps:
            inp = h
            h = fn(inp)
            stages[name] = (lambda fn=fn, inp=inp: fn(inp))
        rows = h.view(-1, h.shape[3])
        n_tok = h.shape[1] * h.shape[2]

        def conv_pos():
            t = A.vggface2._Conv1x1Fn.apply(rows, m_h.conv.weight, True)
            return A.heads._AssembleFn.apply(t.view(args.frames, n_tok, m_h.dim), None, m_h.pos_embedding)

        tok = conv_pos()
        stages["conv1x1_pos"] = conv_pos
        stages["transformer_mean"] = lambda: m_h.spatial_transformer(tok, pool='mean')
        stage_ms = {}
        for name, fn in stages.items():
            fn()
            ms, n = kernel_sum_ms(fn)
            stage_ms[name] = {"kernel_sum_ms": ms, "device_ops": n}
    out = {"name": args.name, "frames": args.frames, "size": args.size, "box": box_id(), "clock_before": clock_before,
           "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0), "alternations": args.groups,
           "calls_per_group": args.calls, "warmup_calls": args.warmup,
           "launch": "eager, device events around the calls, inputs already on the device, torch.no_grad()",
           "arms": {"torch": "VGGFormer(backend='torch'): fp32 NCHW torch ops, the only path before",
                    "hip": "VGGFormer(backend='hip', stem='hip', conv_dtype='bf16')"},
           "ms_per_call": runs, "median_ms_per_call": med,
           "spread_ms_max_minus_min": {k: round(max(v) - min(v), 5) for k, v in runs.items()},
           "hip_over_torch": round(med["hip"] / med["torch"], 4), "device_ops_per_call": ops_count,
           "rel_fro_hip_vs_torch": err, "hip_stages": stage_ms}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms_per_call", "hip_over_torch", "device_ops_per_call", "rel_fro_hip_vs_torch", "hip_stages")}))


if __name__ == "__main__":
    main()
