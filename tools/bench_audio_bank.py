"""Audio windows from a resident waveform bank (audio_bank.AudioAssembler) against the path before it, on one box, in one process,
the arms alternated.

    python tools/bench_audio_bank.py [--batch 64] [--wavs 5] [--wav-seconds 60] [--sets 8] [--groups 7] [--calls 50] [--warmup 3]
    python tools/bench_audio_bank.py --dense-ab <pkg>/lib/ab_base.so [--groups 9] [--calls 100]

To the normalised log-mel tensor [batch, 1, 64, 1001], full-length (ten-second) windows:
  a          the path before the bank: a host-assembled fp32 [batch, 1, 441000] in pinned memory, uploaded, MelFrontEnd(backend="hip")
  b          the bank on the device, AudioAssembler(backend="torch").features with MelFrontEnd(backend="torch"): the table is read on
             the host (one synchronisation), torch.stft per distinct length
  c          AudioAssembler(backend="hip").features on the fp32 bank: one memset and two launches, index read on the device
  c_i16      the same on the int16 bank
  yardstick  MelFrontEnd(backend="hip") on an already assembled [batch, 1, 441000] on the device: the arithmetic of c without the
             indirection
  audio      AudioAssembler(backend="hip").forward, the gather to fp32 [batch, 1, 441000] (no yardstick: it is a copy of 113 MB)

The bank holds --wavs wavs of --wav-seconds seconds (5 x 60 s: 13.2 M samples, 53 MB as fp32, 26 MB as int16), with a sample
every 1/30 s wherever the ten-second window is whole.  Where the bytes sit: the bank is smaller than the 256 MiB Infinity Cache
and larger than the 4 MiB L2, and so is the 113 MB dense input of arm a and the yardstick; after the warm-up calls all of them
can be served from the Infinity Cache, none from L2.  Within a call every sample of a window is read by the two or three frames
that cover it (1024 / 441); those repeats can hit in L2 in every arm alike.  Two kinds of index set, --sets of each, and every
call of b / c / audio takes the next set of its kind:
  scattered    batch random samples of the data set: 64 windows of 10 s out of 300 s overlap, the different samples of a batch are
               counted and reported
  consecutive  batch neighbouring samples: the windows name 10 s + 63 / 30 s of one wav (2.1 MB as fp32), each sample about 53
               times; all but the first read of it can hit in L2
A timed window is --calls calls between two device events; the groups alternate over all arms after --warmup calls of each.  The
device operations of ONE call are counted with torch.profiler afterwards.  Writes <out-dir>/<name>.json (default
profiles/ab/audio_bank.json) and prints the medians.

--dense-ab: the gate on the existing path.  tools/ab_bench.py alternates two builds of the library on bench.py's step, which has
no audio stage; this mode follows its scheme for the dense call instead: avf_mel_power + avf_mel_db_norm at [batch, 441000]
through the library given (the parent commit's build, arms A1 and A2 - two A/A runs -) and through this build (arm B), both
loaded in this process, the arms alternated group by group.  B passes where its median lies inside [min, max] of the A groups.
Writes <out-dir>/audio_bank_dense_ab.json.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    e1.synchronize()
    return round(e0.elapsed_time(e1) / calls, 5)


def test_batch(batch, samples, dev):
    """[batch, 1, samples] fp32: two tones plus noise, every clip at its own gain (the input of tools/bench_mel.py)"""
    import torch
    g = torch.Generator().manual_seed(123)
    t = torch.arange(samples) / 44100.0
    gains = 10.0 ** torch.linspace(-3.0, 1.0, batch)
    x = (0.3 * torch.sin(2 * torch.pi * 440.0 * t) + 0.1 * torch.sin(2 * torch.pi * 3000.0 * t + 1.0))[None] \
        + 0.02 * torch.randn(batch, samples, generator=g)
    return (gains[:, None] * x)[:, None].to(dev)


def dense_ab(args):
    import torch
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import shader_clock
    dev = torch.device("cuda:0")
    libs = {"A": ctypes.CDLL(os.path.abspath(args.dense_ab)), "B": A._lib.load()}
    for name in ("avf_mel_power", "avf_mel_db_norm", "avf_last_error"):
        fn = getattr(libs["A"], name)
        fn.restype, fn.argtypes = A._lib.SIGNATURES[name]
    fe = A.audio.MelFrontEnd(backend="hip").to(dev)
    x = test_batch(args.batch, 441000, dev).reshape(args.batch, 441000).contiguous()
    p, vp = (lambda t: ctypes.c_void_p(t.data_ptr())), ctypes.c_void_p
    outs = {k: (torch.empty(args.batch, fe.n_mels, fe.full_frames, device=dev), torch.empty(args.batch, dtype=torch.int32, device=dev))
            for k in libs}

    def call(k):
        lib, (mel, peak) = libs[k], outs[k]
        s = vp(torch.cuda.current_stream().cuda_stream)
        rc = lib.avf_mel_power(p(x), args.batch, 441000, p(fe.window), fe.win_length, fe.n_fft, fe.hop_length, p(fe.fb), p(fe.bin_lo),
                               p(fe.bin_hi), fe.n_mels, fe.full_frames, 1, p(mel), p(peak), s)
        rc = rc or lib.avf_mel_db_norm(p(mel), p(peak), args.batch, fe.n_mels, fe.full_frames, 1, fe.top_db, fe.mean, fe.std, s)
        if rc:
            raise RuntimeError(lib.avf_last_error().decode())
    arms = {"A1": lambda: call("A"), "A2": lambda: call("A"), "B": lambda: call("B")}
    clock_before = shader_clock()
    for fn in arms.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(outs["A"][0], outs["B"][0]))
    runs = {k: [] for k in arms}
    for r in range(args.groups):
        for name, fn in arms.items():
            runs[name].append(timed(fn, args.calls))
        print(f"group {r + 1}: " + "  ".join(f"{k} {v[-1]:.5f}" for k, v in runs.items()) + " ms", flush=True)
    med = {k: statistics.median(v) for k, v in runs.items()}
    a_all = runs["A1"] + runs["A2"]
    out = {"name": "audio_bank_dense_ab", "workload": f"avf_mel_power + avf_mel_db_norm, audio [{args.batch}, 441000], one clip per row",
           "arm_A": "the parent commit's build of the library (A1 and A2: the same library in two slots of the alternation)",
           "arm_B": "this build: mel_power_kernel<MelDenseSource> from mel_kernels.hpp",
           "launch": "eager, device events around the calls, both libraries loaded in one process",
           "box": box_id(), "clock_before": clock_before, "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "ms_per_call": runs,
           "median_ms_per_call": med, "A1_minus_A2_median_ms": round(med["A1"] - med["A2"], 5),
           "A_groups_min_max_ms": [min(a_all), max(a_all)], "B_over_A": round(med["B"] / statistics.median(a_all), 4),
           "B_median_inside_the_A_spread": bool(min(a_all) <= med["B"] <= max(a_all)) or bool(med["B"] <= min(a_all)),
           "outputs_bit_equal": same}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "audio_bank_dense_ab.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: out[k] for k in ("median_ms_per_call", "A_groups_min_max_ms", "B_over_A", "B_median_inside_the_A_spread",
                                          "outputs_bit_equal")}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--wavs", type=int, default=5)
    ap.add_argument("--wav-seconds", type=int, default=60)
    ap.add_argument("--sets", type=int, default=8)
    ap.add_argument("--groups", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--name", default="audio_bank")
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "ab"))
    ap.add_argument("--dense-ab", default=None, metavar="LIB", help="the parent commit's build of the library: run the gate only")
    args = ap.parse_args()
    if args.groups < 5:
        ap.error("--groups must be at least 5 (the result is a median)")
    import random

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_audio_bank.py measures on the GPU; no device found")
    if args.dense_ab:
        return dense_ab(args)
    import avformer_amd as A
    from tools.ab_bench import box_id
    from tools.bench_mel import device_ops, shader_clock
    dev = torch.device("cuda:0")
    B, SR, N = args.batch, 44100, 441000
    if args.wav_seconds < 20:
        ap.error("--wav-seconds must be at least 20: a whole window needs 10 s before the time stamp and 5 s behind it")
    waves = [test_batch(1, args.wav_seconds * SR, "cpu")[0, 0] * (0.5 + 0.1 * v) for v in range(args.wavs)]
    per_wav = (args.wav_seconds - 15) * 30                                          # time stamps 10 s .. wav_seconds - 5 s
    if per_wav < 2 * B:
        ap.error("--wav-seconds is too small for --batch consecutive samples")
    ts = np.tile(10000.0 + np.arange(per_wav) * (1000.0 / 30), args.wavs)
    wav_of = np.repeat(np.arange(args.wavs), per_wav)
    bank = A.audio_bank.AudioBank.from_waves(waves, wav_of, ts, SR).to(dev)
    q = [torch.round(w * 32768.0 / float(w.abs().max() * 1.01)).to(torch.int16) for w in waves]
    bank16 = A.audio_bank.AudioBank.from_waves(q, wav_of, ts, SR).to(dev)
    F = len(bank)
    rng = random.Random(5)
    sets = {"scattered": [], "consecutive": []}
    for _ in range(args.sets):
        sets["scattered"].append(torch.tensor(rng.sample(range(F), B), device=dev))
        start = per_wav * rng.randrange(args.wavs) + rng.randrange(per_wav - B)
        sets["consecutive"].append(torch.arange(start, start + B, device=dev))
    fe, fe_t = A.audio.MelFrontEnd(backend="hip").to(dev), A.audio.MelFrontEnd(backend="torch").to(dev)
    asm_t, asm_h = A.audio_bank.AudioAssembler(), A.audio_bank.AudioAssembler(backend="hip")
    clock_before = shader_clock()
    result = {}
    with torch.no_grad():
        for kind, idx in sets.items():
            for i in idx:
                assert bool((asm_t.window_table(bank, i, fe)[:, 1] == N).all()), "every timed window is a whole one"
            x_dev = asm_t(bank, idx[0], fe)                                          # the assembled batch of set 0, on the device ...
            x_pin = x_dev.cpu().pin_memory()                                         # ... and as the host's loader would hand it over
            turn = {"n": 0}

            def nxt():
                turn["n"] += 1
                return idx[turn["n"] % len(idx)]
            arms = {"a": lambda: fe(x_pin.to(dev, non_blocking=True)),
                    "b": lambda: asm_t.features(bank, nxt(), fe_t),
                    "c": lambda: asm_h.features(bank, nxt(), fe),
                    "c_i16": lambda: asm_h.features(bank16, nxt(), fe),
                    "yardstick": lambda: fe(x_dev),
                    "audio": lambda: asm_h(bank, nxt(), fe)}
            for fn in arms.values():
                for _ in range(args.warmup):
                    fn()
            torch.cuda.synchronize()
            want = fe(x_dev)
            same = {"c": bool(torch.equal(asm_h.features(bank, idx[0], fe), want)),
                    "audio": bool(torch.equal(asm_h(bank, idx[0], fe), x_dev)),
                    "b_max_abs_difference": float((asm_t.features(bank, idx[0], fe_t) - want).abs().max()),
                    "c_i16": bool(torch.equal(asm_h.features(bank16, idx[0], fe), fe(asm_t(bank16, idx[0], fe))))}
            out_bytes = want.numel() * want.element_size()
            del want
            runs = {k: [] for k in arms}
            for r in range(args.groups):
                for name, fn in arms.items():
                    runs[name].append(timed(fn, args.calls))
                print(f"{kind} group {r + 1}: " + "  ".join(f"{k} {v[-1]:.4f}" for k, v in runs.items()) + " ms", flush=True)
            ops = {name: device_ops(fn) for name, fn in arms.items()}
            med = {k: statistics.median(v) for k, v in runs.items()}
            first = asm_t.window_table(bank, idx[0], fe)[:, 0].cpu().numpy()
            covered = np.zeros(bank.wave.numel(), dtype=bool)
            for f0 in first:
                covered[f0:f0 + N] = True
            unique, batch_bytes = int(covered.sum()), B * N * 4
            result[kind] = {
                "ms_per_call": runs, "median_ms_per_call": med,
                "yardstick_spread_ms_max_minus_min": round(max(runs["yardstick"]) - min(runs["yardstick"]), 5),
                "c_minus_yardstick_ms": round(med["c"] - med["yardstick"], 5),
                "c_i16_minus_yardstick_ms": round(med["c_i16"] - med["yardstick"], 5),
                "device_ops_per_call": {k: v[0] for k, v in ops.items()}, "device_op_names": {k: v[1] for k, v in ops.items()},
                "different_samples_in_a_batch_of_set_0": unique,
                "bytes_that_must_move": {
                    "a": {"host_link": batch_bytes, "device_read": batch_bytes, "device_write": out_bytes},
                    "b": {"host_link": 8 * B, "device_read": 2 * batch_bytes, "device_write": batch_bytes + out_bytes,
                          "of_the_read_from_different_samples": unique * 4},
                    "c": {"host_link": 0, "device_read": batch_bytes, "device_write": out_bytes, "of_the_read_from_different_samples": unique * 4},
                    "c_i16": {"host_link": 0, "device_read": batch_bytes // 2, "device_write": out_bytes,
                              "of_the_read_from_different_samples": unique * 2},
                    "yardstick": {"host_link": 0, "device_read": batch_bytes, "device_write": out_bytes},
                    "audio": {"host_link": 0, "device_read": batch_bytes, "device_write": batch_bytes},
                    "note": "every arm also reads its mel power back once in the dB launch and reads a sample once per frame that "
                            "covers it (1024 / 441 times); only the first read of a sample is counted"},
                "outputs_on_set_0": same}
            del x_dev, x_pin
    out = {"name": args.name, "batch": B, "window": [1, N], "output": [B, 1, fe.n_mels, fe.full_frames], "wavs": args.wavs,
           "wav_seconds": args.wav_seconds, "samples_of_the_data_set": F, "bank_bytes": {"fp32": bank.wave.numel() * 4, "int16": bank16.wave.numel() * 2},
           "index_sets_per_kind": args.sets, "launch": "eager, device events around the calls; index already on the device",
           "box": box_id(), "clock_before": clock_before, "clock_after": shader_clock(), "device": torch.cuda.get_device_name(0),
           "alternations": args.groups, "calls_per_group": args.calls, "warmup_calls": args.warmup, "index_sets": result}
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, args.name + ".json"), "w") as f:
        json.dump(out, f, indent=1)
    for kind, r in result.items():
        print(json.dumps({"index_set": kind, **{k: r[k] for k in (
            "median_ms_per_call", "yardstick_spread_ms_max_minus_min", "c_minus_yardstick_ms", "c_i16_minus_yardstick_ms",
            "device_ops_per_call", "different_samples_in_a_batch_of_set_0", "outputs_on_set_0")}}))


if __name__ == "__main__":
    main()
