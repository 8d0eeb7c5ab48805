"""The frozen ResNet stages of the S-Former (backbone.FrozenResFormer) on the HIP conv kernels against the two ways PyTorch runs
them, on one box, in one process, the arms alternated.

    python tools/bench_backbone.py [--frames 1024 16] [--size 112] [--groups 7] [--calls 5] [--warmup 2]

  a   FrozenResFormer(backend="torch"): fp32, NCHW, as the reference runs it
  b   the same torch ops on a bf16 channels_last copy of the conv stages: the vendor library's best case (the token section is
      this package's Transformer in every arm; b reaches it through the reference's permutes)
  c   FrozenResFormer(backend="hip")
Per frame count B' (1024 = 64 clips x 16 frames, 16 = batch-1 inference) three sections are timed separately: layer1..3 (from
the stem's output to the stage-3 map / tokens), the layer4 + avgpool tail (from a stage-3 map), and the whole module.  A timed
window is --calls calls between two device events; the groups alternate over all arms after --warmup calls of each; the
result is the median of the groups.  Then every distinct conv shape of the stages runs alone on avf_conv2d_nhwc and its
achieved fraction of the bf16 MFMA peak (2.5 PFLOP/s dense) is reported, and the device operations of arm c from the stage-3
tokens to the pooled features are counted with torch.profiler: next to the token section's own there must be the positional
add, layer4's five conv launches and the pool, and no permute.  Writes <out-dir>/<name>.json (default
profiles/ab/backbone_frozen.json) and prints the medians.

    python tools/bench_backbone.py --stem [--groups 7] [--calls 5] [--warmup 2]

The stem in front of those stages (conv1 7x7 / 2 - bn1 - relu - maxpool 3x3 / 2), on [1024, 3, 112, 112] and [16, 3, 112, 112] video
frames and the [64, 1, 64, 1001] mel maps of the audio stream, fp32 planes in, the NHWC bf16 map of layer1 out:
  a        the torch stem (fp32, NCHW) plus backbone.to_nhwc: the path before csrc/stem.hip
  b        the same ops on a bf16 channels_last copy (the conversion of x included; its output is the NHWC bf16 map already): the
           vendor library's best case
  c        ops.stem_nchw: one launch
  whole    FrozenResFormer(backend="hip") with stem="torch" and with stem="hip" (the video shapes), FrozenAudioModel on both backends
           (the mel shape)
Same windows, alternation and medians.  Per shape the JSON also holds the bytes the stem must move (x in once, out once) and the
rate arm c reaches on them.  Writes <out-dir>/backbone_stem.json.

    python tools/bench_backbone.py --conv-dtype f32 [--frames 1024 16] [--groups 7] [--calls 5] [--warmup 2]

The parity form of the conv stages (conv_dtype="f32", csrc/conv_f32.hip: fp32 maps, three bf16 MFMA products per fp32 product)
against the throughput form (conv_dtype="bf16"), both FrozenResFormer(backend="hip", stem="torch"), in one process, the arms
alternated: the same three sections, then every distinct conv shape of the stages alone on avf_conv2d_nhwc (bf16 in, bf16 out)
and on avf_conv2d_nhwc_f32x3, alternated per shape.  The errors are against arm a (backend="torch").  Writes
<out-dir>/backbone_f32.json.

    python tools/bench_backbone.py --train-tokens [--frames 1024 16] [--groups 7] [--calls 5] [--warmup 2]

Training the token section behind the frozen layer4 (FrozenResFormer(train_tokens=True), csrc/conv_dgrad.hip): forward + backward
of the whole module on the hip backend against backend="torch" (fp32 NCHW autograd through layer4), both with the stem and the
stages frozen, in one process, the arms alternated; the forward with train_tokens=True under no_grad against the default
forward (the same launches: the difference belongs inside the spread of the two); then the five data-gradient launches of
layer4's backward and the pool backward alone, each with the FLOPs of its live taps (2 * N*Ho*Wo * k*k * Cin * Cout) as a share
of the bf16 MFMA peak, the bytes it must move as a share of the HBM rate, and which of the two bounds it.  The launches are
timed with device events around back-to-back calls of one launch, not with a profiler.  Writes
<out-dir>/backbone_token_grad.json."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BF16 = 2.5e15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[1024, 16])
    ap.add_argument("--size", type=int, default=112)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stem", action="store_true", help="time the stem arms instead (profiles/ab/backbone_stem.json)")
    ap.add_argument("--conv-dtype", choices=("bf16", "f32"), default="bf16",
                    help="f32: time the parity form of the conv stages against the bf16 form instead (profiles/ab/backbone_f32.json)")
    ap.add_argument("--train-tokens", action="store_true",
                    help="time forward + backward with train_tokens=True against backend='torch' (profiles/ab/backbone_token_grad.json)")
    ap.add_argument("--name", default=None)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    if args.name is None:
        args.name = "backbone_token_grad" if args.train_tokens else "backbone_stem" if args.stem else "backbone_f32" if args.conv_dtype == "f32" else "backbone_frozen"
    if args.train_tokens:
        return train_tokens_main(args)
    if args.stem:
        return stem_main(args)
    if args.conv_dtype == "f32":
        return conv_dtype_main(args)
    import torch
    from torch.nn import functional as F
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import device_ops, shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_backbone.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m_a = A.FrozenResFormer(backend="torch").to(dev).eval()
    for p in m_a.parameters():
        p.requires_grad_(False)
    m_c = copy.deepcopy(m_a).set_backend("hip")
    m_b = copy.deepcopy(m_a)
    stages_b = torch.nn.ModuleDict({n: getattr(m_b, n) for n in ("conv1", "bn1", "layer1", "layer2", "layer3", "layer4")})
    stages_b.to(dtype=torch.bfloat16, memory_format=torch.channels_last)

    def stem_b(x):
        return m_b.maxpool(F.relu(A.FrozenBasicBlock._bn(m_b.conv1(x), m_b.bn1)))

    def l123(m, h):
        return m.layer3(m.layer2(m.layer1(h)))

    def tail(m, f):
        return torch.flatten(m.avgpool(m.layer4(f)), 1)

    def whole_b(x):
        f = l123(m_b, stem_b(x.to(dtype=torch.bfloat16, memory_format=torch.channels_last)))
        f = A.ResFormerTokens.forward(m_b, f.float()).to(dtype=torch.bfloat16, memory_format=torch.channels_last)
        return tail(m_b, f).float()

    clock_before = shader_clock()
    result = {}
    with torch.no_grad():
        for Bp in args.frames:
            x = torch.randn(Bp, 3, args.size, args.size, device=dev)
            h = m_a.stem(x)                                              # [B', 64, 28, 28]
            f3 = l123(m_a, h)                                            # [B', 256, 7, 7]
            h_b = h.to(dtype=torch.bfloat16, memory_format=torch.channels_last)
            f3_b = f3.to(dtype=torch.bfloat16, memory_format=torch.channels_last)
            tok = f3.permute(0, 2, 3, 1).reshape(Bp, -1, f3.shape[1]).contiguous()   # what the transformer hands to layer4 in arm c
            hw = tuple(f3.shape[2:])
            arms = {"a_l123": lambda: l123(m_a, h), "b_l123": lambda: l123(m_b, h_b), "c_l123": lambda: m_c.stages_to_tokens(h),
                    "a_tail": lambda: tail(m_a, f3), "b_tail": lambda: tail(m_b, f3_b), "c_tail": lambda: m_c.tokens_to_features(tok, hw),
                    "a_whole": lambda: m_a(x), "b_whole": lambda: whole_b(x), "c_whole": lambda: m_c(x)}
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            want = m_a(x)
            err = {k: float((arms[k]().float() - want).norm() / want.norm()) for k in ("b_whole", "c_whole")}
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
                print(f"B'={Bp} group {r + 1}: " + "  ".join(f"{k} {v[-1]:.3f}" for k, v in runs.items()) + " ms", flush=True)
            med = {k: statistics.median(v) for k, v in runs.items()}

            # every distinct conv shape of the stages, alone
            shapes, seen, xs = [], set(), stage_conv_shapes(m_c, Bp, h.shape[2], h.shape[3])
            for (N, H, W, Cin, Cout, k, s) in xs:
                if (N, H, W, Cin, Cout, k, s) in seen:
                    continue
                seen.add((N, H, W, Cin, Cout, k, s))
                xi = torch.randn(N, H, W, Cin, device=dev).bfloat16()
                wp = torch.randn(Cout, k * k * Cin, device=dev).bfloat16()
                sc = torch.ones(Cout, device=dev)
                out = A.ops.conv2d_nhwc(xi, wp, sc, sc, k, s, relu=True)
                n = 20 if Bp <= 64 else 5
                t = []
                for _ in range(5):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(n):
                        A.ops.conv2d_nhwc(xi, wp, sc, sc, k, s, relu=True, out=out)
                    e1.record()
                    e1.synchronize()
                    t.append(e0.elapsed_time(e1) / n)
                ms = statistics.median(t)
                flops = 2.0 * out.numel() * k * k * Cin
                shapes.append({"x": [N, H, W, Cin], "Cout": Cout, "k": k, "stride": s, "M": out.numel() // Cout, "K": k * k * Cin,
                               "tile": A.ops.conv_plan(N, H, W, Cin, Cout, k, s)["tile"], "ms": round(ms, 5),
                               "tflops": round(flops / ms / 1e9, 2), "fraction_of_bf16_peak": round(flops / (ms * 1e-3) / PEAK_BF16, 4)})
            # device operations of arm c from the stage-3 tokens to the pooled features
            st = m_c.spatial_transformer
            t_in = tok + m_c.pos_embedding
            n_mid, names_mid = device_ops(lambda: m_c.tokens_to_features(st(tok + m_c.pos_embedding[:, :tok.shape[1]]), hw))
            n_st, _ = device_ops(lambda: st(t_in))
            permutes = None if n_mid is None else [n for n in names_mid if any(s in n.lower() for s in ("permute", "transpose", "copy"))]
            result[str(Bp)] = {
                "ms_per_call": runs, "median_ms_per_call": med,
                "spread_ms_max_minus_min": {k: round(max(v) - min(v), 5) for k, v in runs.items()},
                "c_over_b": {s: round(med["c_" + s] / med["b_" + s], 3) for s in ("l123", "tail", "whole")},
                "c_over_a": {s: round(med["c_" + s] / med["a_" + s], 3) for s in ("l123", "tail", "whole")},
                "rel_fro_vs_a_whole": err, "conv_shapes": shapes,
                "tokens_to_features_device_ops": {"count": n_mid, "of_the_token_section_alone": n_st, "names": names_mid,
                                                  "expected_next_to_the_token_section": "1 positional add + 5 conv launches + 1 pool = 7",
                                                  "permute_or_copy_kernels": permutes}}
            del x, h, f3, h_b, f3_b, tok
    out = {"name": args.name, "frame_counts": args.frames, "size": args.size, "box": box_id(), "clock_before": clock_before,
           "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0), "alternations": args.groups,
           "calls_per_group": args.calls, "warmup_calls": args.warmup, "bf16_peak_flops_assumed": PEAK_BF16,
           "launch": "eager, device events around the calls, inputs already on the device, torch.no_grad()", "frames": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for Bp, r in result.items():
        print(json.dumps({"frames": Bp, "median_ms_per_call": r["median_ms_per_call"], "c_over_b": r["c_over_b"], "c_over_a": r["c_over_a"],
                          "rel_fro_vs_a_whole": r["rel_fro_vs_a_whole"],
                          "device_ops": {k: r["tokens_to_features_device_ops"][k] for k in ("count", "of_the_token_section_alone", "permute_or_copy_kernels")}}))
        for s in r["conv_shapes"]:
            print(json.dumps(s))


STEM_SHAPES = ((1024, 3, 112, 112), (16, 3, 112, 112), (64, 1, 64, 1001))


def stem_main(args):
    import torch
    from torch.nn import functional as F
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_backbone.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    video = A.FrozenResFormer(backend="hip").to(dev).eval()
    audio = A.FrozenAudioModel(backend="torch").to(dev).eval()
    for m in (video, audio):
        for p in m.parameters():
            p.requires_grad_(False)
    video_fused = copy.deepcopy(video).set_backend("hip", stem="hip")
    audio_hip = copy.deepcopy(audio).set_backend("hip")

    def timed(arms):
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
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
        return runs

    clock_before = shader_clock()
    result = {}
    with torch.no_grad():
        for shape in STEM_SHAPES:
            N, Cin, H, W = shape
            x = torch.randn(*shape, device=dev)
            net = video if Cin == 3 else audio.resnet          # conv1 / bn1 / maxpool of the module the shape belongs to
            net_b = copy.deepcopy(torch.nn.ModuleDict({"conv1": net.conv1, "bn1": net.bn1}))
            net_b.to(dtype=torch.bfloat16, memory_format=torch.channels_last)
            packed = net._stem_pack(dev)
            Hp, Wp = A.ops.stem_out_hw(H, W)
            out_c = torch.empty(N, Hp, Wp, 64, dtype=torch.bfloat16, device=dev)

            def arm_a():
                return A.backbone.to_nhwc(net.stem(x))

            def arm_b():
                xb = x.to(dtype=torch.bfloat16, memory_format=torch.channels_last)
                return net.maxpool(F.relu(A.FrozenBasicBlock._bn(net_b["conv1"](xb), net_b["bn1"])))

            def arm_c():
                return A.ops.stem_nchw(x, *packed, out=out_c)

            arms = {"a_stem": arm_a, "b_stem": arm_b, "c_stem": arm_c}
            if Cin == 3:
                arms.update({"whole_stem_torch": lambda: video(x), "whole_stem_hip": lambda: video_fused(x)})
            else:
                arms.update({"whole_torch": lambda: audio(x), "whole_hip": lambda: audio_hip(x)})
            want = arm_a().float()
            err = {"b_stem": float((arm_b().permute(0, 2, 3, 1).float() - want).norm() / want.norm()),
                   "c_stem": float((arm_c().float() - want).norm() / want.norm())}
            wholes = [k for k in arms if k.startswith("whole")]
            ref = arms[wholes[0]]().float()
            err[wholes[1] + "_vs_" + wholes[0]] = float((arms[wholes[1]]().float() - ref).norm() / ref.norm())
            print(f"shape {shape}", flush=True)
            runs = timed(arms)
            med = {k: statistics.median(v) for k, v in runs.items()}
            spread = {k: round(max(v) - min(v), 5) for k, v in runs.items()}
            must_move = x.numel() * x.element_size() + out_c.numel() * out_c.element_size()
            result["x".join(map(str, shape))] = {
                "ms_per_call": runs, "median_ms_per_call": med, "spread_ms_max_minus_min": spread,
                "c_over_a": round(med["c_stem"] / med["a_stem"], 4), "c_over_b": round(med["c_stem"] / med["b_stem"], 4),
                "a_minus_c_ms": round(med["a_stem"] - med["c_stem"], 5),
                "c_below_a_by_more_than_the_spread_of_a": bool(med["a_stem"] - med["c_stem"] > spread["a_stem"]),
                "c_below_b": bool(med["c_stem"] < med["b_stem"]),
                "whole_ratio_" + wholes[1] + "_over_" + wholes[0]: round(med[wholes[1]] / med[wholes[0]], 4),
                "stem_bytes_x_in_once_out_once": must_move, "c_stem_gb_per_s": round(must_move / (med["c_stem"] * 1e-3) / 1e9, 1),
                "stem_tile": A.ops.stem_plan(*shape), "rel_fro": err}
            del x, out_c
    out = {"name": args.name, "shapes": [list(s) for s in STEM_SHAPES], "box": box_id(), "clock_before": clock_before,
           "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0), "alternations": args.groups,
           "calls_per_group": args.calls, "warmup_calls": args.warmup,
           "launch": "eager, device events around the calls, inputs already on the device, torch.no_grad()", "stem": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for k, r in result.items():
        print(json.dumps({"shape": k, **{n: r[n] for n in r if n != "ms_per_call"}}))


def conv_dtype_main(args):
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_backbone.py measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m_a = A.FrozenResFormer(backend="torch").to(dev).eval()
    for p in m_a.parameters():
        p.requires_grad_(False)
    m16 = copy.deepcopy(m_a).set_backend("hip")
    m32 = copy.deepcopy(m_a).set_backend("hip").set_conv_dtype("f32")

    def median_ms(fn, n):
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            t.append(e0.elapsed_time(e1) / n)
        return statistics.median(t)

    clock_before = shader_clock()
    result = {}
    with torch.no_grad():
        for Bp in args.frames:
            x = torch.randn(Bp, 3, args.size, args.size, device=dev)
            h = m_a.stem(x)                                              # [B', 64, 28, 28]
            f3 = m_a.layer3(m_a.layer2(m_a.layer1(h)))                   # [B', 256, 7, 7]
            tok = f3.permute(0, 2, 3, 1).reshape(Bp, -1, f3.shape[1]).contiguous()
            hw = tuple(f3.shape[2:])
            arms = {"bf16_l123": lambda: m16.stages_to_tokens(h), "f32_l123": lambda: m32.stages_to_tokens(h),
                    "bf16_tail": lambda: m16.tokens_to_features(tok, hw), "f32_tail": lambda: m32.tokens_to_features(tok, hw),
                    "bf16_whole": lambda: m16(x), "f32_whole": lambda: m32(x)}
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            want = {"l123": tok + m_a.pos_embedding[:, :tok.shape[1]], "tail": torch.flatten(m_a.avgpool(m_a.layer4(f3)), 1), "whole": m_a(x)}
            err = {}
            for k, fn in arms.items():
                got = fn()
                got = got[0] if isinstance(got, tuple) else got
                err[k] = float((got.float() - want[k.split("_")[1]]).norm() / want[k.split("_")[1]].norm())
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
                print(f"B'={Bp} group {r + 1}: " + "  ".join(f"{k} {v[-1]:.3f}" for k, v in runs.items()) + " ms", flush=True)
            med = {k: statistics.median(v) for k, v in runs.items()}
            shapes, seen = [], set()
            for shp in stage_conv_shapes(m16, Bp, h.shape[2], h.shape[3]):
                if shp in seen:
                    continue
                seen.add(shp)
                N, H, W, Cin, Cout, k, s = shp
                xi = torch.randn(N, H, W, Cin, device=dev)
                xb = xi.bfloat16()
                w = torch.randn(Cout, k * k * Cin, device=dev)
                wb, wl = w.bfloat16(), (w - w.bfloat16().float()).bfloat16()
                sc = torch.ones(Cout, device=dev)
                o16 = A.ops.conv2d_nhwc(xb, wb, sc, sc, k, s, relu=True)
                o32 = A.ops.conv2d_nhwc_f32(xi, (wb, wl), sc, sc, k, s, relu=True)
                n = 20 if Bp <= 64 else 5
                ms16, ms32 = [], []
                for _ in range(3):                                       # alternated per shape
                    ms16.append(median_ms(lambda: A.ops.conv2d_nhwc(xb, wb, sc, sc, k, s, relu=True, out=o16), n))
                    ms32.append(median_ms(lambda: A.ops.conv2d_nhwc_f32(xi, (wb, wl), sc, sc, k, s, relu=True, out=o32), n))
                ms16, ms32 = statistics.median(ms16), statistics.median(ms32)
                flops = 2.0 * o16.numel() * k * k * Cin
                shapes.append({"x": [N, H, W, Cin], "Cout": Cout, "k": k, "stride": s, "M": o16.numel() // Cout, "K": k * k * Cin,
                               "tile": A.ops.conv_plan(N, H, W, Cin, Cout, k, s)["tile"], "bf16_ms": round(ms16, 5), "f32_ms": round(ms32, 5),
                               "f32_over_bf16": round(ms32 / ms16, 3),
                               "f32_mfma_fraction_of_bf16_peak": round(3 * flops / (ms32 * 1e-3) / PEAK_BF16, 4)})
                del xi, xb, o16, o32
            result[str(Bp)] = {"ms_per_call": runs, "median_ms_per_call": med,
                               "spread_ms_max_minus_min": {k: round(max(v) - min(v), 5) for k, v in runs.items()},
                               "f32_over_bf16": {s: round(med["f32_" + s] / med["bf16_" + s], 3) for s in ("l123", "tail", "whole")},
                               "rel_fro_vs_torch_backend": err, "conv_shapes": shapes}
            del x, h, f3, tok
    out = {"name": args.name, "frame_counts": args.frames, "size": args.size, "box": box_id(), "clock_before": clock_before,
           "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0), "alternations": args.groups,
           "calls_per_group": args.calls, "warmup_calls": args.warmup, "bf16_peak_flops_assumed": PEAK_BF16,
           "launch": "eager, device events around the calls, inputs already on the device, torch.no_grad()", "frames": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for Bp, r in result.items():
        print(json.dumps({"frames": Bp, "median_ms_per_call": r["median_ms_per_call"], "f32_over_bf16": r["f32_over_bf16"],
                          "rel_fro_vs_torch_backend": r["rel_fro_vs_torch_backend"]}))
        for s in r["conv_shapes"]:
            print(json.dumps(s))


PEAK_HBM = 8.0e12  # bytes / s


def train_tokens_main(args):
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import shader_clock
    if not torch.cuda.is_available():
        raise SystemExit("bench_backbone.py measures on the GPU; no device found")
    dev, ops = torch.device("cuda:0"), A.ops
    torch.manual_seed(0)
    m_t = A.FrozenResFormer(backend="torch", train_tokens=True).to(dev).eval()
    m_h = copy.deepcopy(m_t).set_backend("hip")
    m_d = copy.deepcopy(m_t).set_backend("hip").set_train_tokens(False)  # the forward-only module (everything frozen above stays so)

    def step(m, x, w):
        for p in m.parameters():
            p.grad = None
        (m(x) * w).sum().backward()

    def window(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def alternate(arms, calls):
        for fn in arms.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        runs = {k: [] for k in arms}
        for _ in range(args.groups):
            for k, fn in arms.items():
                runs[k].append(round(window(fn, calls), 5))
        return runs

    def no_grad(m, x):
        with torch.no_grad():
            return m(x)

    clock_before = shader_clock()
    result = {}
    for Bp in args.frames:
        x = torch.randn(Bp, 3, args.size, args.size, device=dev)
        w = torch.randn(Bp, 512, device=dev)
        runs = alternate({"hip_fwd_bwd": lambda: step(m_h, x, w), "torch_fwd_bwd": lambda: step(m_t, x, w)}, args.calls)
        step(m_h, x, w)
        g_h = torch.cat([p.grad.flatten() for p in m_h.parameters() if p.grad is not None])
        step(m_t, x, w)
        g_t = torch.cat([p.grad.flatten() for p in m_t.parameters() if p.grad is not None])
        runs.update(alternate({"fwd_no_grad_train_tokens": lambda: no_grad(m_h, x), "fwd_no_grad_default": lambda: no_grad(m_d, x),
                               "fwd_no_grad_default_again": lambda: no_grad(m_d, x)}, args.calls))
        med = {k: statistics.median(v) for k, v in runs.items()}
        # layer4's backward, launch by launch, in the order it runs: the maps bf16, the last launch's output fp32
        hh = (args.size // 16, args.size // 16)
        ho = ((hh[0] - 1) // 2 + 1, (hh[1] - 1) // 2 + 1)
        launches = [("block2.conv2", ho, 512, 512, 3, 1, False, True, torch.bfloat16), ("block2.conv1", ho, 512, 512, 3, 1, True, True, torch.bfloat16),
                    ("block1.conv2", ho, 512, 512, 3, 1, False, True, torch.bfloat16), ("block1.downsample", hh, 256, 512, 1, 2, False, False, torch.float32),
                    ("block1.conv1", hh, 256, 512, 3, 2, True, False, torch.float32)]
        per, n = [], 20 if Bp <= 64 else 5
        dout = torch.randn(Bp, 512, device=dev)
        gate = torch.randn(Bp, ho[0] * ho[1], 512, device=dev).clamp_min(0).bfloat16()
        out = ops.avgpool_nhwc_bwd(dout, ho[0] * ho[1], gate=gate)
        ms = statistics.median(window(lambda: ops.avgpool_nhwc_bwd(dout, ho[0] * ho[1], gate=gate, out=out), n) for _ in range(5))
        nbytes = dout.numel() * 4 + gate.numel() * 2 + out.numel() * 2
        per.append({"launch": "avgpool_bwd", "ms": round(ms, 5), "bytes": nbytes, "hbm_fraction": round(nbytes / (ms * 1e-3) / PEAK_HBM, 4),
                    "bound": "memory (no arithmetic to speak of)"})
        for name, (H, W), Cin, Cout, k, s, add, gated, odt in launches:
            oh, ow = ops.conv_out_hw(H, W, k, s)
            gy = torch.randn(Bp, oh, ow, Cout, device=dev).bfloat16()
            wt = torch.randn(Cin, k * k * Cout, device=dev).bfloat16()
            a = torch.randn(Bp, H, W, Cin, device=dev).to(odt) if add else None
            g = torch.randn(Bp, H, W, Cin, device=dev).clamp_min(0).to(odt) if gated else None
            o = ops.conv2d_nhwc_dgrad(gy, wt, (H, W), k, s, addend=a, gate=g, out_dtype=odt)
            ms = statistics.median(window(lambda: ops.conv2d_nhwc_dgrad(gy, wt, (H, W), k, s, addend=a, gate=g, out=o), n) for _ in range(5))
            flops = 2.0 * Bp * oh * ow * k * k * Cin * Cout
            nbytes = sum(t.numel() * t.element_size() for t in (gy, wt, a, g, o) if t is not None)
            t_mfma, t_hbm = flops / PEAK_BF16 * 1e3, nbytes / PEAK_HBM * 1e3
            per.append({"launch": name, "gy": [Bp, oh, ow, Cout], "out": [Bp, H, W, Cin], "k": k, "stride": s, "addend": add, "gate": gated,
                        "tile": ops.conv_dgrad_plan(Bp, H, W, Cin, Cout, k, s)["tile"], "ms": round(ms, 5), "live_tap_flops": flops,
                        "issued_flops": 2.0 * Bp * H * W * k * k * Cin * Cout, "bytes": nbytes,
                        "mfma_fraction_of_bf16_peak": round(flops / (ms * 1e-3) / PEAK_BF16, 4),
                        "hbm_fraction": round(nbytes / (ms * 1e-3) / PEAK_HBM, 4),
                        "bound": ("launch latency" if ms < 0.02 and max(t_mfma, t_hbm) < 0.25 * ms else "mfma" if t_mfma >= t_hbm else "memory")})
            del gy, wt, a, g, o
        result[str(Bp)] = {"ms_per_call": runs, "median_ms_per_call": med,
                           "spread_ms_max_minus_min": {k: round(max(v) - min(v), 5) for k, v in runs.items()},
                           "torch_over_hip_fwd_bwd": round(med["torch_fwd_bwd"] / med["hip_fwd_bwd"], 3),
                           "fwd_no_grad_train_tokens_minus_default_ms": round(med["fwd_no_grad_train_tokens"] - med["fwd_no_grad_default"], 5),
                           "fwd_no_grad_default_a_a_ms": round(abs(med["fwd_no_grad_default_again"] - med["fwd_no_grad_default"]), 5),
                           "grad_rel_fro_hip_vs_torch": float((g_h - g_t).norm() / g_t.norm()), "backward_launches": per}
        del x, w
    out = {"name": args.name, "frame_counts": args.frames, "size": args.size, "box": box_id(), "clock_before": clock_before,
           "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0), "alternations": args.groups,
           "calls_per_group": args.calls, "warmup_calls": args.warmup, "bf16_peak_flops_assumed": PEAK_BF16, "hbm_bytes_per_s_assumed": PEAK_HBM,
           "launch": "eager, device events around the calls, inputs already on the device; per-launch times: device events around "
                     "back-to-back calls of one launch (no profiler pass)", "frames": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for Bp, r in result.items():
        print(json.dumps({"frames": Bp, "median_ms_per_call": r["median_ms_per_call"], "torch_over_hip_fwd_bwd": r["torch_over_hip_fwd_bwd"],
                          "grad_rel_fro_hip_vs_torch": r["grad_rel_fro_hip_vs_torch"]}))
        for s in r["backward_launches"]:
            print(json.dumps(s))


def stage_conv_shapes(model, Bp, H, W):
    """(N, H, W, Cin, Cout, k, stride) of every conv launch of layer1 .. layer4, in order"""
    out = []
    for stage in (model.layer1, model.layer2, model.layer3, model.layer4):
        for blk in stage:
            s = blk.stride
            out.append((Bp, H, W, blk.inplanes, blk.planes, 3, s))
            if blk.downsample is not None:
                out.append((Bp, H, W, blk.inplanes, blk.planes, 1, s))
            H, W = (H - 1) // s + 1, (W - 1) // s + 1
            out.append((Bp, H, W, blk.planes, blk.planes, 3, 1))
    return out


if __name__ == "__main__":
    main()
