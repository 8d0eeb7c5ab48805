#!/usr/bin/env python3
"""Idle time at the kernel boundaries of the replayed bench step, from a rocprofv3 kernel trace.

  rocprofv3 --kernel-trace --output-format csv -d <dir> -o t -- python bench.py --steps 20 --warmup 5
  python tools/boundary_gaps.py <dir>/.../t_kernel_trace.csv <out.csv> [--steps 20]

(kernel trace only, in a run of its own, the program directly after "--".)  The captured step is a fixed sequence of launches, so
the replays show in the trace as the longest run of dispatches whose kernel names repeat with one period P; the LAST --steps
periods of that run are the timed steps (what runs in front of them - eager warm-up, capture, settling replays - has the same
names, so only the position tells them apart).  The period is cut where its mean gap is largest: that gap is the host's graph
launch, not a kernel boundary, and is reported on a row of its own and kept out of the sums.

For every consecutive pair of one step, in start order: gap = start(next) - end(prev).  The table has
  kind=pair   one row per position of the step: the two kernels, the gap over the steps (mean / median / min / max), prev's duration
  kind=prev   the gaps grouped by the predecessor's kernel name: launches per step, mean gap, gap sum and duration sum per step
  kind=class  the same grouped by kernel class (the classes of DESIGN section 10)
  kind=launch the gap between two replays
  kind=total  per step: gap sum, duration sum, first start to last end
all times in microseconds.  A negative gap is two kernels of parallel graph branches overlapping; it is summed as it is."""
import argparse
import collections
import csv
import re
import statistics
import sys

import numpy as np

CLASSES = (("gemm_bf16_nt_ws", "persistent K=512 GEMM"), ("gemm_bf16_nt", "tiled NT GEMM"), ("attn_", "attention fwd + bwd"),
           ("gemm_bf16_tn_group", "grouped dW + folds"), ("fold_", "grouped dW + folds"), ("ln_", "LayerNorm"), ("adam_", "Adam"))


def short(n):
    n = re.sub(r"\(anonymous namespace\)::", "", n)
    n = re.sub(r"^void ", "", n).replace("avf::", "")
    depth, out = 0, []
    for ch in n:  # the name with its template arguments, without the parameter list
        if ch == "<":
            depth += 1
        elif ch == ">":
            depth -= 1
        elif ch == "(" and depth == 0:
            break
        out.append(ch)
    return "".join(out).strip()


def klass(name):
    for prefix, c in CLASSES:
        if name.startswith(prefix):
            return c
    return "other"


def read_trace(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short(r["Kernel_Name"])))
    rows.sort()
    return rows


def find_replays(names, min_period=8, max_period=2000):
    """(start index, period) of the longest run with names[i] == names[i - P], smallest such P.  The run returned starts at the
    first dispatch of its first whole period."""
    ids = {}
    seq = np.array([ids.setdefault(n, len(ids)) for n in names])
    n = len(seq)
    best = (0, 0, 0)  # (run length, period, index behind the run); a multiple of the true period gives a shorter run
    for P in range(min_period, min(max_period, n // 3) + 1):
        eq = np.concatenate(([0], (seq[P:] == seq[:-P]).astype(np.int8), [0]))
        edge = np.flatnonzero(np.diff(eq))  # rises and falls alternate
        if len(edge) == 0:
            continue
        runs = edge[1::2] - edge[0::2]
        k = int(np.argmax(runs))
        if runs[k] >= 2 * P and runs[k] > best[0]:
            best = (int(runs[k]), P, int(edge[2 * k + 1]) + P)
    if best[0] == 0:
        sys.exit("no periodic run of launches found: is this the trace of a graph-replayed bench run?")
    run, P, end = best
    return end - run - P, P, end


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("out")
    ap.add_argument("--steps", type=int, default=20, help="the timed steps of the traced run: the last ones of the periodic run")
    args = ap.parse_args()
    rows = read_trace(args.trace)
    lo, P, hi = find_replays([r[2] for r in rows])
    whole = (hi - lo) // P
    # phase: cut the period at its largest mean gap (the graph launch)
    steps = min(args.steps, whole - 1)
    if steps < 1:
        sys.exit(f"periodic run of {whole} periods of {P} launches: too short")
    tail = rows[hi - (steps + 1) * P:hi]
    gap_at = [statistics.mean((tail[s * P + k + 1][0] - tail[s * P + k][1]) for s in range(steps)) for k in range(P)]
    cut = max(range(P), key=lambda k: gap_at[k]) + 1  # the step starts behind that gap
    base = hi - (steps + 1) * P + cut
    step_rows = [rows[base + s * P:base + (s + 1) * P] for s in range(steps)]
    us = 1e-3
    pairs = []  # per position k (0 .. P-2): gaps over the steps
    for k in range(P - 1):
        g = [(st[k + 1][0] - st[k][1]) * us for st in step_rows]
        d = [(st[k][1] - st[k][0]) * us for st in step_rows]
        pairs.append((k, step_rows[0][k][2], step_rows[0][k + 1][2], g, d))
    last_d = [(st[P - 1][1] - st[P - 1][0]) * us for st in step_rows]
    launch = [(step_rows[s + 1][0][0] - step_rows[s][P - 1][1]) * us for s in range(steps - 1)]
    out = [("kind", "key", "next", "launches_per_step", "gap_mean_us", "gap_median_us", "gap_min_us", "gap_max_us",
            "gap_sum_per_step_us", "dur_mean_us", "dur_sum_per_step_us")]
    f3 = lambda x: f"{x:.3f}"
    for k, a, b, g, d in pairs:
        out.append(("pair", f"{k:03d} {a}", b, 1, f3(statistics.mean(g)), f3(statistics.median(g)), f3(min(g)), f3(max(g)),
                    f3(statistics.mean(g)), f3(statistics.mean(d)), f3(statistics.mean(d))))
    for kind, keyf in (("prev", lambda a: a), ("class", klass)):
        grp = collections.OrderedDict()
        for k, a, b, g, d in pairs:
            e = grp.setdefault(keyf(a), [0, [], 0.0, 0.0])
            e[0] += 1
            e[1] += g
            e[2] += statistics.mean(g)
            e[3] += statistics.mean(d)
        e = grp.setdefault(keyf(step_rows[0][P - 1][2]), [0, [], 0.0, 0.0])  # the step's last kernel: a launch with no gap behind it
        e[0] += 1
        e[3] += statistics.mean(last_d)
        for key, (cnt, g, gsum, dsum) in sorted(grp.items(), key=lambda kv: -kv[1][2]):
            gs = (f3(statistics.mean(g)), f3(statistics.median(g)), f3(min(g)), f3(max(g))) if g else ("", "", "", "")
            out.append((kind, key, "", cnt) + gs + (f3(gsum), f3(dsum / cnt), f3(dsum)))
    if launch:
        out.append(("launch", "replay to replay", "", 1, f3(statistics.mean(launch)), f3(statistics.median(launch)), f3(min(launch)),
                    f3(max(launch)), "", "", ""))
    gap_sum = sum(statistics.mean(g) for _, _, _, g, _ in pairs)
    dur_sum = sum(statistics.mean(d) for _, _, _, _, d in pairs) + statistics.mean(last_d)
    span = statistics.mean((st[P - 1][1] - st[0][0]) * us for st in step_rows)
    out.append(("total", f"{steps} steps of {P} launches", "", P, f3(gap_sum / (P - 1)), "", "", "", f3(gap_sum), f3(dur_sum / P), f3(dur_sum)))
    out.append(("total", "first start to last end", "", "", "", "", "", "", "", "", f3(span)))
    with open(args.out, "w", newline="") as f:
        csv.writer(f).writerows(out)
    print(f"{steps} steps of {P} launches: gaps {gap_sum:.1f} us, kernels {dur_sum:.1f} us, span {span:.1f} us per step -> {args.out}")
    for r in out:
        if r[0] == "class":
            print(f"  {r[1]:<24} {r[3]:>3} launches  mean gap {r[4] or '-':>7}  gap sum {r[8]:>8}  kernel sum {r[10]:>9}")


if __name__ == "__main__":
    main()
