"""Whole-video inference from a feature bank (FrozenVideoModel.frame_features / forward_bank, frames.FeatureClipAssembler) against
the path before it, on one box, in one process, the arms alternated.

    python tools/bench_feature_bank.py [--batch 64] [--frames 16] [--dilation 3] [--size 112] [--bank-frames 4096] [--sets 16]
                                       [--groups 7] [--calls 50] [--warmup 2]

The video stream of one batch of --batch consecutive labels of a resident bank of [*, size, size, 3] uint8 frames, to the [B, 512]
features of FrozenVideoModel(backend="hip", stem="hip"), bf16 compute:
  a            the direct path: ClipAssembler(hip).normalized then FrozenVideoModel.forward on [B, 3, T, size, size] - the
               S-Former on B x T frames
  b            the steady state of the bank path: the S-Former on the B NEW frames (the labelled ones; every earlier frame's
               features are in the bank already), written into the feature bank, then forward_bank
  c            forward_bank alone: the token launch and the temporal stack
  ... and the split of c's front:
  tokens_hip   FeatureClipAssembler(hip).tokens: one launch of csrc/feature_bank.hip
  tokens_torch FeatureClipAssembler(torch).tokens: the table, index_select, where, cat, add
  yardstick    avf_assemble_tokens on rows gathered beforehand: the bytes of tokens_hip without the indirection
Every call takes the next of --sets label runs (inside one video, no black slot).  A timed window is --calls calls (a, b, c) or
20 x --calls calls (the three token arms) between two device events; the groups alternate over all arms after --warmup calls of
each.  Eager calls of a launch-bound operation measure the host's enqueue as much as the device, so tokens_hip and yardstick are
also timed as 20 launches captured into one graph and replayed (``graph_ms_per_launch``): the device's side of the two.  The
device operations of ONE call are counted with torch.profiler afterwards.  The largest difference between the outputs of a and b
on set 0 is recorded beside the times.  The one pass condition: b is not slower than a (exit status 1 otherwise).  Writes
<out-dir>/<name>.json (default profiles/ab/feature_bank.json) and prints the medians.
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
    ap.add_argument("--bank-frames", type=int, default=4096)
    ap.add_argument("--sets", type=int, default=16)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--name", default="feature_bank")
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
        raise SystemExit("bench_feature_bank.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    B, T, d, S, F = args.batch, args.frames, args.dilation, args.size, args.bank_frames
    span = d * (T - 1)
    if F % 1024 or F < 1024 or span + B >= 1024:
        ap.error("--bank-frames must be a multiple of 1024, and a batch's clips must fit one video of 1024 frames")
    g = torch.Generator(device=dev).manual_seed(123)
    frames = torch.randint(0, 256, (F, S, S, 3), dtype=torch.uint8, device=dev, generator=g)
    bank = A.frames.FrameBank(frames, (torch.arange(F, device=dev) // 1024).to(torch.int32))
    rng = random.Random(5)
    starts = [1024 * rng.randrange(F // 1024) + rng.randrange(span, 1024 - B) for _ in range(args.sets)]
    sets = [torch.arange(s, s + B, device=dev) for s in starts]
    torch.manual_seed(7)
    model = A.FrozenVideoModel(backend="hip", compute_dtype="bf16", stem="hip").eval()
    for m in model.modules():                                                   # BatchNorm statistics that keep the activations of order 1
        if isinstance(m, torch.nn.BatchNorm2d):
            with torch.no_grad():
                m.running_var.uniform_(0.8, 1.6)
                m.weight.uniform_(0.6, 1.0)
    for p in model.parameters():
        p.requires_grad_(False)
    model = model.to(dev)
    fe_clip = A.clip.ClipFrontEnd(backend="hip").to(dev)
    fe_frame = A.clip.ClipFrontEnd(layout="tchw", channels=3, backend="hip").to(dev)
    asm_clip = A.frames.ClipAssembler(T, d, backend="hip")
    asm_hip, asm_torch = A.frames.FeatureClipAssembler(T, d, backend="hip"), A.frames.FeatureClipAssembler(T, d)
    t_former = model.t_former
    lead, pos = t_former.cls_token.detach().reshape(1, -1), t_former.pos_embedding.detach().reshape(T + 1, -1)
    clock_before = shader_clock()
    with torch.no_grad():
        fb = model.frame_features(bank, fe_frame)                               # once per data set split: not part of a batch
        rows0 = asm_torch.tokens(fb, sets[0])                                    # [B, T, 512], gathered beforehand
        turn = {"n": 0}

        def nxt():
            turn["n"] += 1
            return sets[turn["n"] % len(sets)]

        def arm_a(idx=None):
            idx = nxt() if idx is None else idx
            return model(asm_clip.normalized(bank, idx, fe_clip))

        def arm_b(idx=None):
            idx = nxt() if idx is None else idx
            fb.features.index_copy_(0, idx, model.s_former(fe_frame(bank.frames.index_select(0, idx).unsqueeze(1))))
            return model.forward_bank(fb, idx, asm_hip)

        arms = {"a": arm_a, "b": arm_b,
                "c": lambda: model.forward_bank(fb, nxt(), asm_hip),
                "tokens_hip": lambda: asm_hip.tokens(fb, nxt(), lead, pos),
                "tokens_torch": lambda: asm_torch.tokens(fb, nxt(), lead, pos),
                "yardstick": lambda: A.ops.assemble_tokens(rows0, lead, pos)}
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        out_a, out_b = arm_a(sets[0]).float(), arm_b(sets[0]).float()
        tokens_equal = bool(torch.equal(asm_hip.tokens(fb, sets[0], lead, pos), asm_torch.tokens(fb, sets[0], lead, pos))
                            and torch.equal(asm_hip.tokens(fb, sets[0], lead, pos), A.ops.assemble_tokens(rows0, lead, pos)))
        diff = {"max_abs": float((out_a - out_b).abs().max()), "rel_fro": float((out_a - out_b).norm() / out_a.norm()),
                "mean_abs_of_a": float(out_a.abs().mean())}
        per_graph = 20
        graphs, keep = {}, []
        for name in ("tokens_hip", "yardstick"):                                # 20 launches per graph, each on the next label run
            graphs[name] = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graphs[name]):
                keep += [arms[name]() for _ in range(per_graph)]
            graphs[name].replay()
        torch.cuda.synchronize()
        calls = {k: args.calls * (1 if k in ("a", "b", "c") else 20) for k in arms}
        runs, graph_runs = {k: [] for k in arms}, {k: [] for k in graphs}
        for r in range(args.groups):
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls[name]):
                    fn()
                e1.record()
                e1.synchronize()
                runs[name].append(round(e0.elapsed_time(e1) / calls[name], 5))
            for name, graph in graphs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.calls):
                    graph.replay()
                e1.record()
                e1.synchronize()
                graph_runs[name].append(round(e0.elapsed_time(e1) / (args.calls * per_graph), 5))
            print(f"group {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in runs.items()) + " ms;  in a graph: "
                  + "  ".join(f"{k} {v[-1]:.4f}" for k, v in graph_runs.items()) + " ms", flush=True)
        del keep
        ops = {name: device_ops(fn) for name, fn in arms.items()}
    med = {k: statistics.median(v) for k, v in runs.items()}
    spread = {k: round(max(v) - min(v), 5) for k, v in runs.items()}
    ok = med["b"] <= med["a"]
    out = {"name": args.name, "batch": B, "clip": [T, S, S, 3], "dilation": d, "bank_frames": F, "label_runs": args.sets,
           "model": "FrozenVideoModel(backend='hip', stem='hip', compute_dtype='bf16'), fp32 planes from ClipFrontEnd(backend='hip')",
           "launch": "eager, device events around the calls; index already on the device",
           "box": box_id(), "clock_before": clock_before, "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": calls, "warmup_calls": args.warmup,
           "s_former_frames_per_batch": {"a": B * T, "b": B, "c": 0},
           "ms_per_batch": runs, "median_ms_per_batch": med, "spread_ms_max_minus_min": spread,
           "b_over_a": round(med["b"] / med["a"], 4), "pass_b_not_slower_than_a": ok,
           "graph_ms_per_launch": graph_runs, "median_graph_ms_per_launch": {k: statistics.median(v) for k, v in graph_runs.items()},
           "launches_per_graph": per_graph,
           "device_ops_per_call": {k: v[0] for k, v in ops.items()},
           "device_op_names": {k: v[1] for k, v in ops.items() if k in ("tokens_hip", "tokens_torch", "yardstick")},
           "difference_of_the_outputs_a_b_on_set_0": diff, "tokens_hip_torch_yardstick_bit_equal_on_set_0": tokens_equal}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms_per_batch", "spread_ms_max_minus_min", "b_over_a", "pass_b_not_slower_than_a",
                                          "median_graph_ms_per_launch",
                                          "device_ops_per_call", "difference_of_the_outputs_a_b_on_set_0",
                                          "tokens_hip_torch_yardstick_bit_equal_on_set_0")}))
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
