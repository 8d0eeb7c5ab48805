"""Clip assembly from a resident frame bank (frames.ClipAssembler) against the path before it, on one box, in one process, the
arms alternated.

    python tools/bench_clip_bank.py [--batch 64] [--frames 16] [--dilation 3] [--size 112] [--bank-frames 16384] [--sets 16]
                                    [--groups 7] [--calls 50] [--warmup 3]

To fp32 "cthw" planes, without AutoAugment:
  a          the path before the bank: a host-assembled uint8 clip in pinned memory, uploaded, ClipFrontEnd(backend="hip")
  b          the bank on the device, ClipAssembler(backend="torch") (index arithmetic, index_select, where), ClipFrontEnd(backend="hip")
  c          ClipAssembler(backend="hip").normalized: one launch, no uint8 clip
  yardstick  ClipFrontEnd(backend="hip") on an already assembled clip of the same shape on the device (avf_clip_normalize): the
             bytes of c, without the indirection
... and the same four with ClipAutoAugment(backend="hip") in the chain (a_aug, b_aug, c_aug = ClipAssembler(hip).augmented then
the front end, yardstick_aug = augment then front end on the assembled clip).

The bank holds --bank-frames random frames (16384 frames of 112 x 112 x 3 are 617 MB, above the 256 MiB Infinity Cache) in videos
of 1024 frames.  Two kinds of index set, --sets of each, and every call of b / c takes the next set of its kind:
  scattered    64 indices, each with its slots inside a 64-frame cell of its own: the 1024 slots of a batch are 1024 different
               frames (38.5 MB).  The --sets sets together read --sets x 38.5 MB, more than the Infinity Cache holds, so the
               frame reads of a call cannot be hits left over from the call before; within a call no frame is read twice.
  consecutive  64 neighbouring indices: the 1024 slots name 64 + dilation x (frames - 1) different frames (4.1 MB at the
               defaults), each about nine times.  The first read of a frame comes from HBM, the others can hit in L2 / the
               Infinity Cache.
Arm a and the yardsticks work on one fixed clip, as the path before did: their 38.5 MB of input can stay in the Infinity Cache
from call to call, so where c (scattered) is behind its yardstick by more than the yardstick's spread, that difference is the
bank's HBM reads.  A timed window is --calls calls between two device events; the groups alternate over all arms after --warmup
calls of each.  The device operations of ONE call are counted with torch.profiler afterwards.  Writes <out-dir>/<name>.json
(default profiles/ab/clip_bank.json) and prints the medians.
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
    ap.add_argument("--name", default="clip_bank")
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
        raise SystemExit("bench_clip_bank.py measures on the GPU; no device found")
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
    flip = A.clip.draw_flips(B, generator=torch.Generator().manual_seed(1)).to(dev)
    plan = A.augment.draw_plan(B, T, random.Random(7), size=(S, S)).to(dev)
    fe = A.clip.ClipFrontEnd(backend="hip").to(dev)
    aug = A.augment.ClipAutoAugment(backend="hip")
    asm_t, asm_h = A.frames.ClipAssembler(T, d), A.frames.ClipAssembler(T, d, backend="hip")
    clock_before = shader_clock()
    result = {}
    with torch.no_grad():
        for kind, idx in sets.items():
            clip_dev = asm_t(bank, idx[0])                                           # the assembled clip of set 0, on the device ...
            clip_pin = clip_dev.cpu().pin_memory()                                   # ... and as the host's loader would hand it over
            turn = {"n": 0}

            def nxt():
                turn["n"] += 1
                return idx[turn["n"] % len(idx)]
            arms = {"a": lambda: fe(clip_pin.to(dev, non_blocking=True), flip),
                    "b": lambda: asm_t.normalized(bank, nxt(), fe, flip),
                    "c": lambda: asm_h.normalized(bank, nxt(), fe, flip),
                    "yardstick": lambda: fe(clip_dev, flip),
                    "a_aug": lambda: fe(aug(clip_pin.to(dev, non_blocking=True), plan), flip),
                    "b_aug": lambda: fe(asm_t.augmented(bank, nxt(), plan, aug), flip),
                    "c_aug": lambda: fe(asm_h.augmented(bank, nxt(), plan, aug), flip),
                    "yardstick_aug": lambda: fe(aug(clip_dev, plan), flip)}
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            want, want_aug = fe(clip_dev, flip), fe(aug(clip_dev, plan), flip)
            same = {"b": bool(torch.equal(asm_t.normalized(bank, idx[0], fe, flip), want)),
                    "c": bool(torch.equal(asm_h.normalized(bank, idx[0], fe, flip), want)),
                    "b_aug": bool(torch.equal(fe(asm_t.augmented(bank, idx[0], plan, aug), flip), want_aug)),
                    "c_aug": bool(torch.equal(fe(asm_h.augmented(bank, idx[0], plan, aug), flip), want_aug)),
                    "gather": bool(torch.equal(asm_h(bank, idx[0]), clip_dev))}
            out_bytes = want.numel() * want.element_size()
            del want, want_aug
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
            spread = {k: round(max(runs[k]) - min(runs[k]), 5) for k in ("yardstick", "yardstick_aug")}
            unique = int(torch.unique(asm_t.source_table(bank, idx[0]).clamp(min=0)).numel())
            clip_bytes, frame_bytes = clip_dev.numel(), S * S * 3
            result[kind] = {
                "ms_per_call": runs, "median_ms_per_call": med,
                "yardstick_spread_ms_max_minus_min": spread,
                "c_minus_yardstick_ms": round(med["c"] - med["yardstick"], 5),
                "c_aug_minus_yardstick_aug_ms": round(med["c_aug"] - med["yardstick_aug"], 5),
                "device_ops_per_call": {k: v[0] for k, v in ops.items()}, "device_op_names": {k: v[1] for k, v in ops.items()},
                "different_frames_in_a_batch": unique,
                "bytes_that_must_move": {
                    "a": {"host_link": clip_bytes, "device_read": clip_bytes, "device_write": out_bytes},
                    "b": {"host_link": 0, "device_read": 2 * clip_bytes, "device_write": clip_bytes + out_bytes,
                          "of_the_read_from_different_frames": unique * frame_bytes},
                    "c": {"host_link": 0, "device_read": clip_bytes, "device_write": out_bytes,
                          "of_the_read_from_different_frames": unique * frame_bytes},
                    "yardstick": {"host_link": 0, "device_read": clip_bytes, "device_write": out_bytes},
                    "each_aug_arm_adds": {"device_read": clip_bytes, "device_write": clip_bytes}},
                "outputs_equal_to_the_yardsticks_on_set_0": same}
            del clip_dev, clip_pin
    out = {"name": args.name, "clip": [B, T, S, S, 3], "dilation": d, "output": "float32 cthw", "bank_frames": F,
           "bank_bytes": frames.numel(), "index_sets_per_kind": args.sets, "flipped_clips": int(flip.sum()),
           "launch": "eager, device events around the calls; index, flip and plan already on the device",
           "box": box_id(), "clock_before": clock_before, "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "index_sets": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for kind, r in result.items():
        print(json.dumps({"index_set": kind, **{k: r[k] for k in (
            "median_ms_per_call", "yardstick_spread_ms_max_minus_min", "c_minus_yardstick_ms", "c_aug_minus_yardstick_aug_ms",
            "device_ops_per_call", "different_frames_in_a_batch", "outputs_equal_to_the_yardsticks_on_set_0")}}))


if __name__ == "__main__":
    main()
