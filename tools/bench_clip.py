"""The video clip front-end through both backends of clip.ClipFrontEnd on the same box, in one process, alternated.

    python tools/bench_clip.py [--batch 64] [--frames 16] [--size 112] [--channels 3] [--groups 7] [--calls 100] [--warmup 5]

  torch   ATen ops on the device (cast, divide, subtract, divide, copy): the only path before backend="hip" existed, and still
          the default
  hip     csrc/clip.hip: one launch

Input: uint8 [batch, frames, size, size, channels] on the device (random bytes), half of the clips flagged for the mirror; output
fp32 "cthw".  A timed window is `--calls` forward() calls between two device events; the groups alternate torch, hip, torch, hip,
... after `--warmup` calls of each.  The device operations of ONE call are counted with torch.profiler in a pass of its own,
after the timing.  The largest difference of the two outputs at the timed size is recorded beside the times (it must be 0), and
the bytes the transform has to move (input once, output once) give the hip path's GB/s.  Writes <out-dir>/<name>.json (default
profiles/ab/clip_front_end.json) and prints the medians.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--channels", type=int, default=3, choices=(3, 4))
    ap.add_argument("--no-flip", action="store_true", help="no clip is mirrored (flip=None)")
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--name", default="clip_front_end")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import device_ops, shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(123)
    shape = (args.batch, args.frames, args.size, args.size, args.channels)
    x = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g).to(dev)
    flip = None if args.no_flip else A.clip.draw_flips(args.batch, generator=g).to(dev)
    stats = (A.clip.RGB_MEAN, A.clip.RGB_STD) if args.channels == 3 else (A.clip.RGBM_MEAN, A.clip.RGBM_STD)
    fes = {"torch": A.clip.ClipFrontEnd(*stats, backend="torch").to(dev), "hip": A.clip.ClipFrontEnd(*stats, backend="hip").to(dev)}
    clock_before = shader_clock()
    outs = {}
    with torch.no_grad():
        for name, fe in fes.items():
            for _ in range(args.warmup):
                outs[name] = fe(x, flip)
        torch.cuda.synchronize()
        diff = float((outs["torch"] - outs["hip"]).abs().max())
        same = bool(torch.equal(outs["torch"], outs["hip"]))
        out_shape = list(outs["hip"].shape)
        moved = x.numel() + outs["hip"].numel() * outs["hip"].element_size()
        outs.clear()
        runs = {k: [] for k in fes}
        for r in range(args.groups):
            for name, fe in fes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    fe(x, flip)
                e1.record()
                e1.synchronize()
                runs[name].append(round(e0.elapsed_time(e1) / args.calls, 5))
            print(f"group {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f} ms" for k, v in runs.items()), flush=True)
        clock_after = shader_clock()
        ops = {name: device_ops(lambda fe=fe: fe(x, flip)) for name, fe in fes.items()}
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"name": args.name, "input": list(shape), "output": out_shape, "out_dtype": "float32", "layout": "cthw",
           "flipped_clips": 0 if flip is None else int(flip.sum()), "launch": "eager, device events around the calls",
           "box": box_id(), "clock_before": clock_before, "clock_after": clock_after, "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "ms_per_call": runs,
           "median_ms_per_call": med, "hip_over_torch": round(med["hip"] / med["torch"], 4),
           "bytes_the_transform_must_move": moved,
           "gb_per_s_of_those_bytes": {k: round(moved / (v * 1e-3) / 1e9, 1) for k, v in med.items()},
           "device_ops_per_call": {k: v[0] for k, v in ops.items()}, "device_op_names": {k: v[1] for k, v in ops.items()},
           "max_abs_difference_of_the_outputs": diff, "outputs_equal": same}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms_per_call", "hip_over_torch", "gb_per_s_of_those_bytes", "device_ops_per_call",
                                          "max_abs_difference_of_the_outputs", "outputs_equal")}))


if __name__ == "__main__":
    main()
