"""Clip AutoAugment (augment.ClipAutoAugment) on the device, and the numpy backend on the same box's CPU.

    python tools/bench_autoaugment.py [--batch 64] [--frames 16] [--size 112] [--channels 3] [--groups 7] [--calls 50] [--warmup 5]
                                      [--numpy-clips 4]

  hip     csrc/augment.hip: one launch, one workgroup per frame.  Timed twice: with the plan already on the device, and with the
          host plan handed to forward() (checked against the frame size and uploaded, 64 bytes per frame)
  numpy   the restatement of the reference's PIL operations, on the host (one core): `--numpy-clips` clips of the batch, scaled
          to the batch.  This is NOT the reference's own time (it runs Pillow); it is what this package's host path costs

Input: uint8 [batch, frames, size, size, channels] on the device (random bytes) and ONE plan drawn with random.Random(123) as
ImageNetPolicy draws it.  A timed window is `--calls` forward() calls between two device events, `--groups` windows of each
variant, alternated, after `--warmup` calls.  The device operations of one call are counted with torch.profiler in a pass of
its own.  The hip output of the timed batch is compared with the numpy backend on the clips the numpy timing covers (it must be
equal), the bytes the transform has to move (every frame read once and written once) give the GB/s, and the share of frames
each operation touches is recorded with the plan.  Writes <out-dir>/<name>.json (default profiles/ab/clip_autoaugment.json) and
prints the medians.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--channels", type=int, default=3, choices=(3, 4))
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--numpy-clips", type=int, default=4)
    ap.add_argument("--name", default="clip_autoaugment")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import device_ops, shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoaugment.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(123)
    shape = (args.batch, args.frames, args.size, args.size, args.channels)
    x_host = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    x = x_host.to(dev)
    plan_host = A.augment.draw_plan(args.batch, args.frames, random.Random(123), size=(args.size, args.size))
    plan_dev = plan_host.to(dev)
    frames = args.batch * args.frames
    codes = plan_host[..., 0].reshape(frames, 2)
    share = {op: round(float(((codes == code).any(dim=1)).sum()) / frames, 4) for op, code in A.augment.OP_CODES.items()}
    share["untouched"] = round(float((codes == 0).all(dim=1).sum()) / frames, 4)
    hip = A.augment.ClipAutoAugment(backend="hip")
    variants = {"hip_plan_on_device": lambda: hip(x, plan_dev), "hip_with_plan_upload": lambda: hip(x, plan_host)}
    clock_before = shader_clock()
    for fn in variants.values():
        for _ in range(args.warmup):
            out = fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in variants}
    for r in range(args.groups):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                fn()
            e1.record()
            e1.synchronize()
            runs[name].append(round(e0.elapsed_time(e1) / args.calls, 5))
        print(f"group {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f} ms" for k, v in runs.items()), flush=True)
    clock_after = shader_clock()
    ops = {name: device_ops(fn) for name, fn in variants.items()}
    k = max(1, min(args.numpy_clips, args.batch))
    ref = A.augment.ClipAutoAugment()
    t0 = time.perf_counter()
    want = ref(x_host[:k], plan_host[:k])
    numpy_s = time.perf_counter() - t0
    same = bool(torch.equal(out[:k].cpu(), want))
    med = {name: statistics.median(v) for name, v in runs.items()}
    moved = 2 * x.numel()
    result = {"name": args.name, "input": list(shape), "plan": "augment.draw_plan(batch, frames, random.Random(123))",
              "share_of_frames_each_operation_touches": share, "launch": "eager, device events around the calls", "box": box_id(),
              "clock_before": clock_before, "clock_after": clock_after, "device": torch.cuda.get_device_name(0),
              "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "ms_per_call": runs,
              "median_ms_per_call": med, "bytes_the_transform_must_move": moved,
              "gb_per_s_of_those_bytes": {name: round(moved / (v * 1e-3) / 1e9, 1) for name, v in med.items()},
              "device_ops_per_call": {name: v[0] for name, v in ops.items()}, "device_op_names": {name: v[1] for name, v in ops.items()},
              "numpy_backend": {"clips_timed": k, "seconds": round(numpy_s, 4), "ms_per_batch_scaled": round(numpy_s / k * args.batch * 1e3, 1),
                                "where": "this box's CPU, one process"},
              "hip_equals_numpy_on_the_timed_clips": same}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({key: result[key] for key in ("median_ms_per_call", "gb_per_s_of_those_bytes", "device_ops_per_call", "numpy_backend",
                                                   "share_of_frames_each_operation_touches", "hip_equals_numpy_on_the_timed_clips")}))


if __name__ == "__main__":
    main()
