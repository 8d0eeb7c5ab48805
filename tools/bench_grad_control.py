"""What gradient clipping costs on the bench step: three optimizers on the same model, batch and box, alternated.

    python tools/bench_grad_control.py [--config c2] [--dtype bf16] [--rounds 5] [--steps 200]

  default     FusedAdam(model)                                   the unclipped step
  fused_clip  FusedAdam(model, max_grad_norm=...)                norm + multiplier on the device (csrc/grad_control.hip)
  torch_clip  clip_grad_norm_(model.parameters(), ...) in front of FusedAdam.step()

Every variant is the step of bench.py (zero_grad, forward, AU loss, backward, optimizer) captured by GraphedTrainStep and
replayed; a timed window is `--steps` replays between two device events.  max_grad_norm is a quarter of the first step's norm,
so the clip is active.  Writes <out-dir>/<name>.json (default profiles/ab/) and prints the medians.
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
    ap.add_argument("--config", default="c2")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--name", default="grad_control_clip_cost")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    args = ap.parse_args()
    import torch
    import avformer_amd as A
    from bench import CONFIGS
    from tools.ab_bench import box_id
    c = CONFIGS[args.config]
    dev = torch.device("cuda:0")
    B, Tv, Ta = c["batch"], c["t_video"], c["t_audio"]
    g = torch.Generator().manual_seed(123)
    labels = (torch.rand(B, 12, generator=g) > 0.5).float()
    labels[::16] = -1
    batch = {"clip": torch.randn(B, Tv, c["dim"], generator=g).to(dev), "audio_features": torch.randn(B, Ta, c["dim"], generator=g).to(dev),
             "labels": labels.to(dev)}

    def model():
        torch.manual_seed(123)
        return A.SyntheticAVFormer(c["dim"], c["depth"], c["heads"], c["dim_head"], c["mlp_dim"], Tv, Ta, task="AU",
                                   compute_dtype=args.dtype, residual_dtype=args.dtype).to(dev)

    def loss_fn(m, b):
        return m.get_au_loss(m({"clip": b["clip"], "audio_features": b["audio_features"]}), b["labels"])

    probe = model()
    loss_fn(probe, batch).backward()
    max_norm = 0.25 * float(torch.sqrt(sum(p.grad.double().pow(2).sum() for p in probe.parameters() if p.grad is not None)))
    del probe

    class ClipThenStep:
        """clip_grad_norm_ in front of FusedAdam.step(), behind the two methods GraphedTrainStep calls"""
        def __init__(self, m):
            self.m, self.opt = m, A.optim.FusedAdam(m, lr=5e-4, weight_decay=5e-5)

        def zero_grad(self, set_to_none=True):
            self.opt.zero_grad(set_to_none=set_to_none)

        def step(self):
            torch.nn.utils.clip_grad_norm_(self.m.parameters(), max_norm)
            self.opt.step()

    steps = {}
    for name in ("default", "fused_clip", "torch_clip"):
        m = model()
        opt = (A.optim.FusedAdam(m, lr=5e-4, weight_decay=5e-5) if name == "default" else
               A.optim.FusedAdam(m, lr=5e-4, weight_decay=5e-5, max_grad_norm=max_norm) if name == "fused_clip" else ClipThenStep(m))
        steps[name] = A.graphs.GraphedTrainStep(m, opt, loss_fn, batch)
        for _ in range(20):
            steps[name].graph.replay()
    torch.cuda.synchronize()
    runs = {k: [] for k in steps}
    for r in range(args.rounds):
        for name, s in steps.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.steps):
                s.graph.replay()
            e1.record()
            e1.synchronize()
            runs[name].append(round(e0.elapsed_time(e1) / args.steps, 5))
        print(f"round {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f} ms" for k, v in runs.items()), flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    out = {"name": args.name, "config": args.config, "dtype": args.dtype, "launch": "hipGraph replay", "box": box_id(),
           "alternations": args.rounds, "steps": args.steps, "max_grad_norm": max_norm, "ms_per_step": runs, "median_ms_per_step": med,
           "fused_clip_minus_default_us": round(1e3 * (med["fused_clip"] - med["default"]), 2),
           "torch_clip_minus_default_us": round(1e3 * (med["torch_clip"] - med["default"]), 2)}
    d = args.out_dir
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms_per_step", "fused_clip_minus_default_us", "torch_clip_minus_default_us")}))


if __name__ == "__main__":
    main()
