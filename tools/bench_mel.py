"""The audio front-end through both backends of audio.MelFrontEnd on the same box, in one process, alternated.

    python tools/bench_mel.py [--batch 64] [--seconds 10] [--groups 7] [--calls 100] [--warmup 5]

  torch   torch.stft (rocFFT) + ATen ops: the only path before backend="hip" existed, and still the default
  hip     csrc/mel.hip: one memset and two launches

Input: [batch, 1, seconds * 44100] fp32 on the device (two tones plus noise, every clip at its own gain).  A timed window is
`--calls` forward() calls between two device events; the groups alternate torch, hip, torch, hip, ... after `--warmup` calls of
each.  The device operations of ONE call are counted with torch.profiler in a pass of its own, after the timing.  The largest
difference of the two outputs at the timed size is recorded beside the times.  Writes <out-dir>/<name>.json (default
profiles/ab/mel_front_end.json) and prints the medians.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shader_clock():
    """what rocm-smi reports for the clocks of GPU 0 (a read-only query), or "?" """
    try:
        out = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(out).values()))
        return {k: v for k, v in card.items() if "sclk" in k.lower() or "mclk" in k.lower()} or "?"
    except Exception:
        return "?"


def device_ops(fn):
    """-> (count, names) of the device operations (kernels, memsets, copies) one call of fn enqueues, or (None, reason)"""
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name[:96] for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
        return (len(names), names) if names else (None, "the profiler recorded no device event")
    except Exception as e:  # the count is a by-product: the timing stands without it
        return None, f"{type(e).__name__}: {e}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--name", default="mel_front_end")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    if not torch.cuda.is_available():
        raise SystemExit("bench_mel.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    samples = int(args.seconds * 44100)
    g = torch.Generator().manual_seed(123)
    t = torch.arange(samples) / 44100.0
    gains = 10.0 ** torch.linspace(-3.0, 1.0, args.batch)
    x = (0.3 * torch.sin(2 * torch.pi * 440.0 * t) + 0.1 * torch.sin(2 * torch.pi * 3000.0 * t + 1.0))[None] \
        + 0.02 * torch.randn(args.batch, samples, generator=g)
    x = (gains[:, None] * x)[:, None].to(dev)                       # [batch, 1, samples]
    fes = {"torch": A.audio.MelFrontEnd(backend="torch").to(dev), "hip": A.audio.MelFrontEnd(backend="hip").to(dev)}
    clock_before = shader_clock()
    outs = {}
    with torch.no_grad():
        for name, fe in fes.items():
            for _ in range(args.warmup):
                outs[name] = fe(x)
        torch.cuda.synchronize()
        diff = float((outs["torch"] - outs["hip"]).abs().max())
        shape = list(outs["hip"].shape)
        outs.clear()
        runs = {k: [] for k in fes}
        for r in range(args.groups):
            for name, fe in fes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fe(x)
                e1.record()
                e1.synchronize()
                runs[name].append(round(e0.elapsed_time(e1) / args.calls, 5))
            print(f"group {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f} ms" for k, v in runs.items()), flush=True)
        clock_after = shader_clock()
        ops = {name: device_ops(lambda fe=fe: fe(x)) for name, fe in fes.items()}
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"name": args.name, "input": [args.batch, 1, samples], "output": shape, "launch": "eager, device events around the calls",
           "box": box_id(), "clock_before": clock_before, "clock_after": clock_after, "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "ms_per_call": runs,
           "median_ms_per_call": med, "hip_over_torch": round(med["hip"] / med["torch"], 4),
           "device_ops_per_call": {k: v[0] for k, v in ops.items()}, "device_op_names": {k: v[1] for k, v in ops.items()},
           "max_abs_difference_of_the_outputs": diff}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms_per_call", "hip_over_torch", "device_ops_per_call",
                                          "max_abs_difference_of_the_outputs")}))


if __name__ == "__main__":
    main()
