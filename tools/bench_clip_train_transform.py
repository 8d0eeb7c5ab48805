"""The training transform (ImageNetPolicy, RandomClipFlip, NumpyToTensor, Normalize) in one launch against the two-launch chain it
replaces, on one box, in one process, the arms alternated.

    python tools/bench_clip_train_transform.py [--batch 64] [--frames 16] [--dilation 3] [--size 112] [--bank-frames 16384]
                                               [--sets 16] [--groups 7] [--calls 50] [--warmup 3]

To fp32 "cthw" planes, index, flip and plan already on the device, the plan drawn as ImageNetPolicy draws it:
  a        the path before: ClipAssembler(hip).augmented (bank -> augmented uint8 clip), then ClipFrontEnd(hip) - two launches with
           the uint8 clip written and read back between them.  The yardstick.
  b        ClipAssembler(hip).augmented_normalized: one launch, no uint8 clip
  c        ClipAssembler(hip).normalized: no augment at all - the floor (what the reads and the plane stores alone cost)
  d_chain  ClipAutoAugment(hip) then ClipFrontEnd(hip) on an already assembled clip on the device
  d_fused  ClipAutoAugment(hip).normalized on that clip: one launch

The bank and the two kinds of index set are those of tools/bench_clip_bank.py (its docstring says what each kind can hold in the
caches): --bank-frames random frames in videos of 1024 frames (16384 frames of 112 x 112 x 3 are 617 MB, above the 256 MiB
Infinity Cache); "scattered" sets name 1024 different frames per batch and --sets of them together read more than the Infinity
Cache holds, "consecutive" sets name 64 + dilation x (frames - 1) different frames, each about nine times.  The d arms work on one
fixed clip: their 38.5 MB of input can stay in the Infinity Cache from call to call.  The 154 MB of planes every arm writes fit
the Infinity Cache too, as does the 38.5 MB uint8 clip between the two launches of a and d_chain - what the chain saves by
fusing is traffic to the caches rather than to HBM, and a launch.

A timed window is --calls eager calls between two device events; the groups alternate over all arms after --warmup calls of
each.  Reported: every window, each arm's median and the spread (max - min) of its windows, the bytes each arm must move, the
device operations of ONE call (torch.profiler), and whether b is below a by more than the spread of a's windows.  Writes
<out-dir>/<name>.json (default profiles/ab/clip_train_transform.json) and prints the medians.
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
    ap.add_argument("--dilation", type=int, default=3)
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--bank-frames", type=int, default=16384)
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--name", default="clip_train_transform")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    import random

    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import device_ops, shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_clip_train_transform.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    B, T, d, S, F = args.batch, args.frames, args.dilation, args.size, args.bank_frames
    if F < 64 * B * 2 or F % 1024 or d * (T - 1) >= 64:
        ap.error("--bank-frames must be a multiple of 1024 and at least 128 x --batch, and a clip must span fewer than 64 frames")
    g = torch.Generator(device=dev).manual_seed(123)
    frames = torch.randint(0, 256, (F, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    bank = A.frames.FrameBank(frames, (torch.arange(F, device=dev) // 1024).to(torch.int32))
    rng = random.Random(5)
    sets = {"scattered": [], "consecutive": []}
    for _ in range(args.sets):
        cells = rng.sample(range(F // 64), B)                                       # one index per cell of 64 frames
        sets["scattered"].append(torch.tensor([64 * c + rng.randrange(d * (T - 1), 64) for c in cells], device=dev))
        start = 1024 * rng.randrange(F // 1024) + rng.randrange(64, 1024 - B)       # inside one video, no black slot
        sets["consecutive"].append(torch.arange(start, start + B, device=dev))
    plan_host, flip_host = A.augment.draw_plan(B, T, random.Random(7), flip_p=0.5, size=(S, S))
    plan, flip = plan_host.to(dev), flip_host.to(dev)
    codes = plan_host[..., 0].reshape(B * T, 2)
    share = {op: round(float(((codes == code).any(dim=1)).sum()) / (B * T), 4) for op, code in A.augment.OP_CODES.items()}
    share["untouched"] = round(float((codes == 0).all(dim=1).sum()) / (B * T), 4)
    fe = A.clip.ClipFrontEnd(backend="hip").to(dev)
    aug = A.augment.ClipAutoAugment(backend="hip")
    asm = A.frames.ClipAssembler(T, d, backend="hip")
    clock_before = shader_clock()
    result = {}
    with torch.no_grad():
        for kind, idx in sets.items():
            clip_dev = asm(bank, idx[0])                                             # the assembled clip of set 0
            turn = {"n": 0}

            def nxt():
                turn["n"] += 1
                return idx[turn["n"] % len(idx)]
            arms = {"a": lambda: fe(asm.augmented(bank, nxt(), plan, aug), flip),
                    "b": lambda: asm.augmented_normalized(bank, nxt(), plan, aug, fe, flip),
                    "c": lambda: asm.normalized(bank, nxt(), fe, flip),
                    "d_chain": lambda: fe(aug(clip_dev, plan), flip),
                    "d_fused": lambda: aug.normalized(clip_dev, plan, fe, flip)}
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            want = fe(aug(clip_dev, plan), flip)
            same = {"a": bool(torch.equal(fe(asm.augmented(bank, idx[0], plan, aug), flip), want)),
                    "b": bool(torch.equal(asm.augmented_normalized(bank, idx[0], plan, aug, fe, flip), want)),
                    "d_fused": bool(torch.equal(aug.normalized(clip_dev, plan, fe, flip), want))}
            out_bytes = want.numel() * want.element_size()
            del want
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
                print(f"{kind} group {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in runs.items()) + " ms", flush=True)
            ops = {name: device_ops(fn) for name, fn in arms.items()}
            med = {k: statistics.median(v) for k, v in runs.items()}
            spread = {k: round(max(v) - min(v), 5) for k, v in runs.items()}
            unique = int(torch.unique(asm.source_table(bank, idx[0]).clamp(min=0)).numel())
            clip_bytes, frame_bytes = clip_dev.numel(), S * S * 3
            result[kind] = {
                "ms_per_call": runs, "median_ms_per_call": med, "spread_ms_max_minus_min": spread,
                "a_minus_b_ms": round(med["a"] - med["b"], 5), "b_over_a": round(med["b"] / med["a"], 4),
                "b_below_a_by_more_than_the_spread_of_a": bool(med["a"] - med["b"] > spread["a"]),
                "b_minus_c_ms": round(med["b"] - med["c"], 5),
                "d_chain_minus_d_fused_ms": round(med["d_chain"] - med["d_fused"], 5),
                "d_fused_below_d_chain_by_more_than_the_spread_of_d_chain": bool(med["d_chain"] - med["d_fused"] > spread["d_chain"]),
                "device_ops_per_call": {k: v[0] for k, v in ops.items()}, "device_op_names": {k: v[1] for k, v in ops.items()},
                "different_frames_in_a_batch": unique,
                "bytes_that_must_move": {
                    "a": {"device_read": 2 * clip_bytes, "device_write": clip_bytes + out_bytes,
                          "of_the_read_from_different_frames": unique * frame_bytes},
                    "b": {"device_read": clip_bytes, "device_write": out_bytes, "of_the_read_from_different_frames": unique * frame_bytes},
                    "c": {"device_read": clip_bytes, "device_write": out_bytes, "of_the_read_from_different_frames": unique * frame_bytes},
                    "d_chain": {"device_read": 2 * clip_bytes, "device_write": clip_bytes + out_bytes},
                    "d_fused": {"device_read": clip_bytes, "device_write": out_bytes}},
                "outputs_equal_to_the_chain_on_set_0": same}
            del clip_dev
    out = {"name": args.name, "clip": [B, T, S, S, 3], "dilation": d, "output": "float32 cthw", "bank_frames": F,
           "bank_bytes": frames.numel(), "index_sets_per_kind": args.sets, "flipped_clips": int(flip.sum()),
           "plan": "augment.draw_plan(batch, frames, random.Random(7), flip_p=0.5)", "share_of_frames_each_operation_touches": share,
           "launch": "eager, device events around the calls; index, flip and plan already on the device",
           "infinity_cache": {"bytes": 256 * 2 ** 20,
                              "fit": ["the 154 MB of planes", "the 38.5 MB uint8 clip between the two launches of a and d_chain",
                                      "the fixed input clip of the d arms", "the 4.1 MB of frames of a consecutive set"],
                              "do_not_fit": ["the bank", "the frames of all scattered sets together"]},
           "box": box_id(), "clock_before": clock_before, "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "index_sets": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for kind, r in result.items():
        print(json.dumps({"index_set": kind, **{k: r[k] for k in (
            "median_ms_per_call", "spread_ms_max_minus_min", "a_minus_b_ms", "b_below_a_by_more_than_the_spread_of_a", "b_minus_c_ms",
            "d_chain_minus_d_fused_ms", "device_ops_per_call", "outputs_equal_to_the_chain_on_set_0")}}))


if __name__ == "__main__":
    main()
