"""-m gpu: the training transform in ONE launch - ``avf_clip_autoaugment_normalize`` / ``avf_clip_gather_autoaugment_normalize``
(the AutoAugment kernel of csrc/augment_kernels.hpp with the planes as its sink) behind ``ClipAutoAugment(hip).normalized`` and
``ClipAssembler(hip).augmented_normalized``.  Every comparison is bitwise (clip_util.same_bits) against two yardsticks: the
two-launch hip chain ``ClipFrontEnd(hip)(ClipAutoAugment(hip)(clip, plan), flip)`` and the numpy chain of train_transform_util.py.
No tolerance is involved: every output is a table entry.  Frames of 5 x 7 and 37 x 53 put planes off a 16-byte boundary and end
rows inside a vector; a frame of 1 x 1 and the 5 x 7 ones are too small to hold the table in the idle frame buffer."""
import ctypes
import functools
import random

import pytest
import torch

import avformer_amd as A
from clip_util import same_bits
from frames_util import F_SMALL, VIDEOS, boundary_indices, holes, random_frames, reference_clips, video_numbers
from train_transform_util import augmented_clips, front_end, reference_chain

pytestmark = pytest.mark.gpu

FR, AUG = A.frames, A.augment
MISSING = (3, 7, 8, 20, 27, 39)
F32, BF16 = torch.float32, torch.bfloat16
SIGNED = set(AUG.SIGNED_OPS)
# the ten operations, both signs where signed, alone in slot 1 and alone in slot 2: 30 frames (+ 2 untouched) = two clips of [4, 4]
ONE_OP = [(op, 8, s) for op in AUG.OPS for s in ((1, -1) if op in SIGNED else (1,))]
ONE_OP_SLOTS = [(o, None) for o in ONE_OP] + [(None, o) for o in ONE_OP] + [(None, None)] * 2


def _noise(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)


def _grid(slots, size):
    """plans [n, 4, 4, 2, 8]: the slots, 16 frames per clip tensor of B = 4, T = 4"""
    assert len(slots) % 16 == 0
    return [AUG.make_plan([slots[i + 4 * b:i + 4 * b + 4] for b in range(4)], size=size) for i in range(0, len(slots), 16)]


def _check_clip(clip, plan, flip, C, k, layout, dtype, augmented=None):
    """the fused launch on an assembled clip against both yardsticks"""
    fe = front_end(C, k, layout, dtype, backend="hip").cuda()
    aug = AUG.ClipAutoAugment(backend="hip")
    dev, plan_dev, flip_dev = clip.cuda(), plan.cuda(), None if flip is None else flip.cuda()
    got = aug.normalized(dev, plan_dev, fe, flip_dev)
    assert got.is_cuda and got.dtype == dtype and got.is_contiguous()
    assert same_bits(got, fe(aug(dev, plan_dev), flip_dev)), ("two launches", C, k, layout, dtype)
    want = reference_chain(clip.numpy(), plan, flip, k, layout, dtype, augmented=augmented)
    assert same_bits(got, want), ("numpy", C, k, layout, dtype)
    assert torch.equal(dev.cpu(), clip)                                           # the source is left alone
    return got


@functools.lru_cache(maxsize=None)
def _one_op_case(H, W, C):
    clips = [_noise((4, 4, H, W, C), 10 * H + C + i) for i in range(2)]
    plans = _grid(ONE_OP_SLOTS, (H, W))
    return clips, plans, [augmented_clips(c.numpy(), p) for c, p in zip(clips, plans)]


@pytest.mark.parametrize("C,k", [(3, 3), (3, 1), (4, 4), (4, 1), (4, 3)])
@pytest.mark.parametrize("size", [(5, 7), (37, 53)])
def test_each_operation_in_each_slot(size, C, k):
    H, W = size
    clips, plans, augmented = _one_op_case(H, W, C)
    flip = torch.tensor([True, False, False, True])
    for layout in ("cthw", "tchw"):
        for dtype in (F32, BF16):
            for clip, plan, aug in zip(clips, plans, augmented):
                _check_clip(clip, plan, flip, C, k, layout, dtype, augmented=aug)
    _check_clip(clips[0], plans[0], None, C, k, "cthw", F32, augmented=augmented[0])   # no flags at all


@pytest.mark.parametrize("size", [(1, 1), (16, 16)])
def test_all_sub_policies_with_both_slots_on(size):
    def slot(op, idx, sign):
        return (op, idx, sign if op in SIGNED else 1)
    slots = [(slot(op1, i1, 1), slot(op2, i2, -1)) for _, op1, i1, _, op2, i2 in AUG.IMAGENET_POLICY] + [(None, None)] * 7
    assert len(AUG.IMAGENET_POLICY) == 25
    flip = torch.tensor([False, True, True, False])
    for i, plan in enumerate(_grid(slots, size)):
        clip = _noise((4, 4) + size + (3,), 50 + i)
        _check_clip(clip, plan, flip, 3, 3, "cthw", F32)
        _check_clip(clip, plan, flip, 3, 3, "tchw", BF16)


def _banks(shape, seed, present=True):
    frames, nr = random_frames(F_SMALL, *shape, seed=seed), torch.from_numpy(video_numbers(VIDEOS))
    cpu = FR.FrameBank(frames, nr, torch.from_numpy(holes(F_SMALL, MISSING)) if present else None)
    return cpu, cpu.to("cuda")


def _check_bank(cpu, dev, index, plan, flip, T, d, C, k, layout, dtype):
    """the fused launch from the bank against both yardsticks"""
    fe = front_end(C, k, layout, dtype, backend="hip").cuda()
    aug = AUG.ClipAutoAugment(backend="hip")
    hip = FR.ClipAssembler(T, d, backend="hip")
    idx_dev, plan_dev, flip_dev = index.cuda(), plan.cuda(), None if flip is None else flip.cuda()
    got = hip.augmented_normalized(dev, idx_dev, plan_dev, aug, fe, flip_dev)
    assert got.is_cuda and got.dtype == dtype and got.is_contiguous()
    assert same_bits(got, fe(hip.augmented(dev, idx_dev, plan_dev, aug), flip_dev)), ("two launches", T, d, k, layout, dtype)
    present = None if cpu.present is None else cpu.present.numpy()
    clips = reference_clips(cpu.frames.numpy(), cpu.video_db_nr.numpy(), present, index.numpy(), T, d)
    assert same_bits(got, reference_chain(clips, plan, flip, k, layout, dtype)), ("numpy", T, d, k, layout, dtype)
    return got, clips


@pytest.mark.parametrize("T", [4, 16])
@pytest.mark.parametrize("d", [1, 6])
def test_from_the_bank_at_every_boundary(d, T):
    H, W = 5, 7
    index = torch.tensor(boundary_indices())                                      # -1 and F among them: all-black clips
    B = len(index)
    flip = torch.arange(B) % 2 == 0
    plan = AUG.draw_plan(B, T, random.Random(T + d), size=(H, W))
    for C, k, layout, dtype in ((3, 3, "cthw", F32), (4, 1, "tchw", BF16), (4, 4, "cthw", BF16), (3, 1, "tchw", F32)):
        cpu, dev = _banks((H, W, C), seed=T + d + C)
        _, clips = _check_bank(cpu, dev, index, plan, flip, T, d, C, k, layout, dtype)
        black = (clips == 0).all(axis=(2, 3, 4))
        assert bool(black.any()) and bool((~black).any())
    cpu, dev = _banks((H, W, 3), seed=d, present=False)                           # no presence table
    _check_bank(cpu, dev, index, plan, None, T, d, 3, 3, "cthw", F32)
    assert torch.equal(FR.ClipAssembler(T, d, backend="hip").augmented_normalized(            # a plan on the CPU is uploaded
        dev, index.cuda(), plan, AUG.ClipAutoAugment(backend="hip"), front_end(3, 3, backend="hip").cuda()),
        FR.ClipAssembler(T, d, backend="hip").augmented_normalized(
        dev, index.cuda(), plan.cuda(), AUG.ClipAutoAugment(backend="hip"), front_end(3, 3, backend="hip").cuda()))


@pytest.mark.parametrize("size", [(5, 7), (37, 53)])
def test_a_black_slot_is_augmented_and_then_normalised(size):
    H, W = size
    T, d, C = 4, 2, 3
    cpu, dev = _banks((H, W, C), seed=H)
    index = torch.tensor([2, 11, F_SMALL, 30])                                    # black black real real, twice; all black; all real
    inv, sol = (("invert",), None), (None, ("solarize", 4))
    plan = AUG.make_plan([[inv, sol, inv, sol], [sol, inv, sol, inv], [inv, inv, sol, (("invert",), ("invert",))],
                          [inv, sol, inv, sol]], size=size)
    for k, layout, dtype in ((3, "cthw", F32), (1, "tchw", BF16)):
        got, clips = _check_bank(cpu, dev, index, plan, torch.tensor([True, False, True, False]), T, d, C, k, layout, dtype)
    assert (clips[0, 0] == 0).all() and (clips[2] == 0).all()
    fe = front_end(C, C, backend="hip").cuda()
    planes = FR.ClipAssembler(T, d, backend="hip").augmented_normalized(dev, index.cuda(), plan.cuda(), AUG.ClipAutoAugment(backend="hip"),
                                                                        fe).cpu()
    lut = fe.lut.cpu()
    for c in range(C):
        assert bool((planes[0, c, 0] == lut[c, 255]).all()) and lut[c, 255] != lut[c, 0]   # inverted black: the entry of 255
        assert bool((planes[1, c, 0] == lut[c, 0]).all())                                   # solarised black (0 < threshold) stays 0
        assert bool((planes[2, c, 3] == lut[c, 0]).all())                                   # inverted twice


def test_an_empty_plan_is_the_plain_normalise_launch():
    T, d = 4, 2
    index = torch.tensor(boundary_indices()).cuda()
    B = len(index)
    flip = (torch.arange(B) % 3 == 0).cuda()
    aug = AUG.ClipAutoAugment(backend="hip")
    for shape, k, layout, dtype in (((5, 7, 3), 3, "cthw", F32), ((37, 53, 4), 1, "tchw", BF16), ((16, 16, 4), 4, "cthw", BF16)):
        _, dev = _banks(shape, seed=9)
        hip = FR.ClipAssembler(T, d, backend="hip")
        fe = front_end(shape[-1], k, layout, dtype, backend="hip").cuda()
        plan = torch.zeros(B, T, 2, 8, dtype=torch.int32, device="cuda")
        assert same_bits(hip.augmented_normalized(dev, index, plan, aug, fe, flip), hip.normalized(dev, index, fe, flip))
        plan[..., 0] = 11                                                           # codes outside the table do nothing either
        assert same_bits(hip.augmented_normalized(dev, index, plan, aug, fe, flip), hip.normalized(dev, index, fe, flip))


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _sentinel(n, dtype):
    """n elements whose bits no table entry has: a NaN with a payload (fp32), 0x7fc1 (bf16)"""
    if dtype == F32:
        return torch.full((n,), 0x7FC00A5A, dtype=torch.int32, device="cuda").view(torch.float32)
    return torch.full((n,), 0x7FC1, dtype=torch.int16, device="cuda").view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def test_c_abi_sentinels_null_flip_and_refusals():
    lib = A._lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W, C, T, d, k = 5, 7, 3, 4, 2, 2
    cpu, dev = _banks((H, W, C), seed=3, present=False)
    index = torch.tensor(boundary_indices())
    idx_dev = index.cuda()
    B, F = len(index), F_SMALL
    plan = AUG.draw_plan(B, T, random.Random(2), size=(H, W))
    plan_dev = plan.cuda()
    clips = reference_clips(cpu.frames.numpy(), cpu.video_db_nr.numpy(), None, index.numpy(), T, d)
    clip_dev = torch.from_numpy(clips).cuda()
    flip = (torch.arange(B) % 2 == 1)
    zeros = torch.zeros(B, dtype=torch.uint8, device="cuda")
    n = B * k * T * H * W
    augmented = augmented_clips(clips, plan)
    for dtype, code in ((F32, A._lib.F32), (BF16, A._lib.BF16)):
        lut = front_end(C, k).lut.cuda()
        for off in (0, 1, 3):                                                       # dst sits at any element of a larger buffer
            for fl in (flip.cuda(), None, zeros):
                want = reference_chain(clips, plan, None if fl is None or fl is zeros else flip, k, "cthw", dtype, augmented=augmented)
                fill = _sentinel(n + 16, dtype)
                for call in ("bank", "clip"):
                    buf = fill.clone()
                    dst = buf[off:off + n]
                    if call == "bank":
                        rc = lib.avf_clip_gather_autoaugment_normalize(_p(dev.frames), _p(dev.video_db_nr), None, _p(idx_dev), F, B, T, d, H,
                                                                       W, C, _p(plan_dev), k, _p(lut), _p(fl), _p(dst), code,
                                                                       A._lib.CLIP_CTHW, stream)
                    else:
                        rc = lib.avf_clip_autoaugment_normalize(_p(clip_dev), B, T, H, W, C, _p(plan_dev), k, _p(lut), _p(fl), _p(dst),
                                                                code, A._lib.CLIP_CTHW, stream)
                    assert rc == 0, lib.avf_last_error()
                    host = buf.cpu()
                    assert same_bits(host[off:off + n].view(want.shape), want), (call, dtype, off)   # every element overwritten
                    assert torch.equal(_bits(host[:off]), _bits(fill.cpu()[:off])), (call, dtype, off)
                    assert torch.equal(_bits(host[off + n:]), _bits(fill.cpu()[off + n:])), (call, dtype, off)

    # bad arguments are refused before anything is enqueued; the message names them
    lut = front_end(C, k).lut.cuda()
    fill = _sentinel(n + 16, F32)
    buf = fill.clone()
    inside = dev.frames.view(-1)[16:].view(torch.float32)                            # a dst inside the bank / the clip
    inside_clip = clip_dev.view(-1)[16:].view(torch.float32)

    def calls(which, bank=dev.frames, src=clip_dev, T_=T, d_=d, C_=C, k_=k, lut_=lut, plan_=plan_dev, dst=buf, dst_clip=None,
              code=A._lib.F32, layout=A._lib.CLIP_CTHW, lut_off=0, dst_off=0):
        lp = None if lut_ is None else ctypes.c_void_p(lut_.data_ptr() + lut_off)
        dp = None if dst is None else ctypes.c_void_p(dst.data_ptr() + dst_off)
        if "bank" in which:
            yield lib.avf_clip_gather_autoaugment_normalize(_p(bank), _p(dev.video_db_nr), None, _p(idx_dev), F, B, T_, d_, H, W, C_,
                                                            _p(plan_), k_, lp, None, dp, code, layout, stream)
        if "clip" in which:
            yield lib.avf_clip_autoaugment_normalize(_p(src), B, T_, H, W, C_, _p(plan_), k_, lp, None, dp if dst_clip is None else _p(dst_clip),
                                                     code, layout, stream)
    both = ("bank", "clip")
    cases = ((both, {"C_": 5}, b"C is 5"), (both, {"C_": 2}, b"C is 2"), (both, {"T_": 0}, b"T is 0"), (("bank",), {"d_": 0}, b"d is 0"),
             (("bank",), {"bank": None}, b"bank is null"), (("clip",), {"src": None}, b"src is null"), (both, {"k_": 0}, b"k is 0"),
             (both, {"k_": C + 1}, b"k is 4"), (both, {"lut_": None}, b"lut is null"), (both, {"dst": None}, b"dst is null"),
             (both, {"plan_": None}, b"plan is null"), (both, {"lut_off": 2}, b"lut is not aligned"),
             (both, {"dst_off": 2}, b"dst is not aligned"), (both, {"code": 7}, b"out_dtype is 7"), (both, {"layout": 2}, b"layout is 2"),
             (both, {"dst": inside, "dst_clip": inside_clip}, b"overlaps"))
    for which, kw, word in cases:
        rcs = list(calls(which, **kw))
        assert len(rcs) == len(which)
        for rc in rcs:
            assert rc != 0 and word in lib.avf_last_error(), (kw, lib.avf_last_error())
    P = A.ops.clip_autoaugment_max_pixels()
    rc = lib.avf_clip_autoaugment_normalize(_p(clip_dev), 1, 1, P + 1, 1, 3, _p(plan_dev), 3, _p(lut), None, _p(buf), A._lib.F32,
                                            A._lib.CLIP_CTHW, stream)
    assert rc != 0 and f"limit of {P} pixels".encode() in lib.avf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(buf.cpu()), _bits(fill.cpu()))                          # nothing was written
    assert torch.equal(dev.frames.cpu(), cpu.frames) and torch.equal(clip_dev.cpu(), torch.from_numpy(clips))


def test_real_size_from_a_bank_and_from_a_clip():
    H = W = 112
    T, d = 16, 1
    lengths = VIDEOS + (24,)                                                       # F = 64
    frames, nr = random_frames(64, H, W, 3, seed=64), torch.from_numpy(video_numbers(lengths))
    cpu = FR.FrameBank(frames, nr, torch.from_numpy(holes(64, MISSING)))
    dev = cpu.to("cuda")
    index = torch.tensor([63, 25])
    plan, flip = AUG.draw_plan(2, T, random.Random(0), flip_p=0.5, size=(H, W))
    assert int((plan[..., 0] != 0).sum()) >= 8
    got, clips = _check_bank(cpu, dev, index, plan, flip, T, d, 3, 3, "cthw", F32)
    from_clip = _check_clip(torch.from_numpy(clips), plan, flip, 3, 3, "cthw", F32)
    assert same_bits(got, from_clip)


def test_largest_frames():
    """both frame buffers at the LDS limit, the table in the idle one: the longest frame the entry points take, and 160 x 160"""
    P = A.ops.clip_autoaugment_max_pixels()
    assert 160 * 160 <= P
    both = (("sharpness", 7, -1), ("rotate", 8, 1))
    for (H, W), C in (((160, 160), 3), ((P // 163, 163), 3), ((1, P), 3), ((P * 3 // 4, 1), 4), ((P * 3 // 4 // 141, 141), 4)):
        clip = _noise((1, 1, H, W, C), H)
        plan = AUG.make_plan([[both]], size=(H, W))
        _check_clip(clip, plan, torch.tensor([True]), C, C, "cthw", F32)
    fe = front_end(3, 3, backend="hip").cuda()
    with pytest.raises(RuntimeError, match=f"limit of {P} pixels"):
        AUG.ClipAutoAugment(backend="hip").normalized(torch.zeros(1, 1, P + 1, 1, 3, dtype=torch.uint8, device="cuda"),
                                                      torch.zeros(1, 1, 2, 8, dtype=torch.int32, device="cuda"), fe)


def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_one_launch_per_call():
    _, dev = _banks((5, 7, 3), seed=4)
    hip = FR.ClipAssembler(4, 2, backend="hip")
    index = torch.tensor(boundary_indices(), device="cuda")
    B = index.numel()
    fe = front_end(3, 3, backend="hip").cuda()
    flip = (torch.arange(B, device="cuda") % 2 == 0)
    aug = AUG.ClipAutoAugment(backend="hip")
    plan = AUG.make_plan([[(("equalize",), ("rotate", 8, 1))] * 4] * B, size=(5, 7)).cuda()
    clip = hip(dev, index)
    fns = {"bank": lambda: hip.augmented_normalized(dev, index, plan, aug, fe, flip), "clip": lambda: aug.normalized(clip, plan, fe, flip)}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    events = {name: _device_events(fn) for name, fn in fns.items()}
    print(events)
    if not any(events.values()):
        pytest.skip("kineto recorded no device activity here: the launch count cannot be read")
    for name, ev in events.items():
        assert len(ev) == 1 and "clip_autoaugment_kernel" in ev[0] and "AugPlanesSink" in ev[0], (name, ev)   # no memset, copy or second pass


def test_capture_and_replay_reads_index_flags_and_plan_at_run_time():
    H, W, T, d = 5, 7, 4, 2
    cpu, dev = _banks((H, W, 3), seed=5)
    hip, aug = FR.ClipAssembler(T, d, backend="hip"), AUG.ClipAutoAugment(backend="hip")
    fe = front_end(3, 3, backend="hip").cuda()
    i0, i1 = torch.tensor([2, 30, 39]), torch.tensor([40, 11, 26])
    f0, f1 = torch.tensor([1, 0, 0], dtype=torch.bool), torch.tensor([0, 1, 1], dtype=torch.bool)
    p0 = AUG.make_plan([[(("equalize",), ("rotate", 9, 1))] * T] * 3, size=(H, W))
    p1 = AUG.make_plan([[(("shearX", 5, -1), ("solarize", 5))] * T] * 3, size=(H, W))
    index, flags, plan = i0.cuda(), f0.cuda(), p0.cuda()
    hip.augmented_normalized(dev, index, plan, aug, fe, flags)                    # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.augmented_normalized(dev, index, plan, aug, fe, flags)
    index.copy_(i1.cuda())
    flags.copy_(f1.cuda())
    plan.copy_(p1.cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone().cpu()

    def want(i, f, p):
        clips = reference_clips(cpu.frames.numpy(), cpu.video_db_nr.numpy(), cpu.present.numpy(), i.numpy(), T, d)
        return reference_chain(clips, p, f)
    assert same_bits(got, want(i1, f1, p1))
    assert not same_bits(got, want(i0, f1, p1)) and not same_bits(got, want(i1, f0, p1)) and not same_bits(got, want(i1, f1, p0))
