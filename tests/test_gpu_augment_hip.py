"""-m gpu: ``augment.ClipAutoAugment(backend="hip")`` - the kernel of csrc/augment.hip - against the numpy backend, which
test_augment_cpu.py holds byte for byte to the reference on Pillow.  Every comparison is torch.equal on forced plans (one drawn
plan at the real size).  A case batches its (magnitude, sign) combinations as the frames of one clip: one launch per clip."""
import random

import pytest
import torch

import avformer_amd as A

pytestmark = pytest.mark.gpu

AUG = A.augment
SIZES = ((1, 1), (5, 7), (16, 16), (37, 53))


def _noise(shape, seed, lo=0, hi=256):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi, shape, dtype=torch.uint8, generator=g)


def _both(clip, plan, **kw):
    """-> (hip result on the CPU, numpy result)"""
    got = AUG.ClipAutoAugment(backend="hip", **kw)(clip.cuda(), plan.cuda())
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == clip.shape and got.is_contiguous()
    return got.cpu(), AUG.ClipAutoAugment()(clip, plan)


def _combos(op):
    """every (magnitude index, sign) under which the 25 rows can reach this operation"""
    idxs = sorted({r[2] for r in AUG.IMAGENET_POLICY if r[1] == op} | {r[5] for r in AUG.IMAGENET_POLICY if r[4] == op})
    return [(i, s) for i in idxs for s in ((-1, 1) if op in AUG.SIGNED_OPS else (1,))]


@pytest.mark.parametrize("op", AUG.OPS)
def test_each_operation_alone(op):
    combos = _combos(op)
    assert combos
    for H, W in SIZES:          # (1,1), (5,7): equalize's step == 0 and no interior for sharpness; (37,53): unaligned rows, odd byte count
        for C in (3, 4):
            clip = _noise((2, len(combos), H, W, C), seed=1000 * H + 10 * W + C)
            plan = AUG.make_plan([[((op, i, s), None) for i, s in combos], [(None, (op, i, s)) for i, s in combos]], size=(H, W))
            got, want = _both(clip, plan)
            assert torch.equal(got, want), (op, H, W, C, [t for t in range(len(combos)) if not torch.equal(got[:, t], want[:, t])])
            if C == 4:
                assert torch.equal(got[..., 3], clip[..., 3])


def test_degenerate_inputs():
    H, W = 9, 13
    flat = torch.full((H, W, 3), 91, dtype=torch.uint8)
    flat1 = _noise((H, W, 3), 1)
    flat1[..., 1] = 200                                                            # every lane of a wave on one histogram bin
    two = _noise((H, W, 3), 2, 40, 42)                                             # two bins
    frames = torch.stack([flat, flat1, two])
    choices = []
    for op in ("autocontrast", "equalize", "contrast", "color", "sharpness", "invert"):
        choices.append([((op, 8, -1), None)] * 3)
        choices.append([((op, 8, 1), ("equalize",))] * 3)
    clip = frames[None].repeat(len(choices), 1, 1, 1, 1)
    got, want = _both(clip, AUG.make_plan(choices, size=(H, W)))
    assert torch.equal(got, want)
    assert torch.equal(got[0, 0], flat) and torch.equal(got[0, 1, ..., 1], flat1[..., 1])   # the identity branches of autocontrast
    assert torch.equal(got[2, 0], flat)                                            # ... and of equalize

    v = torch.arange(256).view(16, 16, 1)
    allv = ((v + torch.tensor([0, 37, 101])) % 256).to(torch.uint8)                # 16 x 16 with all 256 values in every channel
    every = [(op, i, s) for op in AUG.OPS for i, s in _combos(op)]
    clip = allv[None, None].repeat(1, len(every), 1, 1, 1)
    got, want = _both(clip, AUG.make_plan([[(e, None) for e in every]], size=(16, 16)))
    assert torch.equal(got, want)

    clip = _noise((1, 6, 11, 10, 3), 3)
    forced = [("color", 0, 1), ("color", 0, -1),                                   # the factor is exactly 1: the copy branch
              ("contrast", 8, 1), ("contrast", 8, -1),                             # 1.8 clips, 0.2 does not
              ("solarize", 0, 1), ("solarize", 9, 1)]                              # thresholds 256 (nothing turns) and 0 (all do)
    got, want = _both(clip, AUG.make_plan([[(f, None) for f in forced]], size=(11, 10)))
    assert torch.equal(got, want)
    assert torch.equal(got[0, 0], clip[0, 0]) and torch.equal(got[0, 1], clip[0, 1]) and torch.equal(got[0, 4], clip[0, 4])
    assert torch.equal(got[0, 5], 255 - clip[0, 5]) and not torch.equal(got[0, 2], got[0, 3])


def test_all_sub_policies_with_both_slots_on():
    H, W = 37, 53
    clip = _noise((25, 2, H, W, 3), 25)
    choices = [[((r[1], r[2], s), (r[4], r[5], s)) for s in (1, -1)] for r in AUG.IMAGENET_POLICY]
    plan = AUG.make_plan(choices, size=(H, W))
    got, want = _both(clip, plan)
    assert torch.equal(got, want), [b for b in range(25) if not torch.equal(got[b], want[b])]
    first = plan.clone()
    first[:, :, 1] = 0                                                             # slot 2 works on slot 1's output
    only1 = AUG.ClipAutoAugment()(clip, first)
    second = torch.zeros_like(plan)
    second[:, :, 0] = plan[:, :, 1]
    assert torch.equal(AUG.ClipAutoAugment(backend="hip")(only1.cuda(), second.cuda()).cpu(), want)


def test_real_size_drawn_plan_into_the_front_end_and_in_place():
    B, T, H, W = 2, 16, 112, 112
    clip = _noise((B, T, H, W, 3), 112)
    plan, flips = AUG.draw_plan(B, T, random.Random(31), flip_p=0.5, size=(H, W))
    assert int((plan[..., 0] != 0).sum()) >= 8
    dev = clip.cuda()
    hip = AUG.ClipAutoAugment(backend="hip")
    got = hip(dev, plan)                                                           # a host plan: checked, uploaded
    want = AUG.ClipAutoAugment()(clip, plan)
    assert torch.equal(got.cpu(), want) and torch.equal(dev.cpu(), clip)
    mean, std = A.clip.RGB_MEAN, A.clip.RGB_STD
    planes = A.clip.ClipFrontEnd(mean, std, backend="hip").cuda()(got, flips.cuda())
    assert torch.equal(planes.cpu(), A.clip.ClipFrontEnd(mean, std, backend="torch")(want, flips))
    same = AUG.ClipAutoAugment(backend="hip", inplace=True)(dev, plan.cuda())      # dst == src
    assert same.data_ptr() == dev.data_ptr() and torch.equal(dev.cpu(), want)


def test_largest_frames():
    """both frame buffers at the LDS limit: the longest frame the entry point takes, and 160 x 160"""
    P = A.ops.clip_autoaugment_max_pixels()
    assert 160 * 160 <= P < 64 * 1024
    clip = _noise((1, 2, P, 1, 3), 7)
    plan = AUG.make_plan([[(("equalize",), ("contrast", 8, 1)), (("color", 4, -1), ("autocontrast",))]], size=(P, 1))
    got, want = _both(clip, plan)
    assert torch.equal(got, want)
    P4 = P * 3 // 4
    clip = _noise((1, 1, 1, P4, 4), 8)
    got, want = _both(clip, AUG.make_plan([[(("shearX", 5, 1), ("equalize",))]], size=(1, P4)))
    assert torch.equal(got, want)
    clip = _noise((1, 4, 160, 160, 3), 9)
    choices = [[(("rotate", 9, 1), ("sharpness", 7, -1)), (("shearX", 5, -1), ("equalize",)), (("sharpness", 7, 1), ("rotate", 8, -1)),
                (("equalize",), ("shearX", 5, 1))]]
    got, want = _both(clip, AUG.make_plan(choices, size=(160, 160)))
    assert torch.equal(got, want)


def test_empty_slots_views_and_unknown_codes():
    H, W = 5, 7
    clip = _noise((3, 2, H, W, 3), 4)
    dev = clip.cuda()
    hip = AUG.ClipAutoAugment(backend="hip")
    empty = AUG.make_plan([[(None, None)] * 2] * 3, size=(H, W))
    out = hip(dev, empty.cuda())
    assert out.data_ptr() != dev.data_ptr() and torch.equal(out.cpu(), clip)       # copied, unchanged
    odd = empty.clone()
    odd[..., 0] = torch.tensor([11, -3])                                           # codes outside the table do nothing
    odd[..., 1:] = 0x7FFFFFFF
    assert torch.equal(hip(dev, odd.cuda()).cpu(), clip)
    mixed = AUG.make_plan([[(None, None), (("invert",), None)], [(("rotate", 8, 1), None), (None, None)],
                           [(None, ("shearX", 5, 1)), (None, None)]], size=(H, W))
    want = AUG.ClipAutoAugment()(clip, mixed)
    assert torch.equal(hip(dev, mixed.cuda()).cpu(), want)
    assert torch.equal(want[0, 0], clip[0, 0]) and torch.equal(want[1, 1], clip[1, 1])
    inplace = dev.clone()
    AUG.ClipAutoAugment(backend="hip", inplace=True)(inplace, mixed.cuda())
    assert torch.equal(inplace.cpu(), want)
    off = dev[1:]                                       # contiguous; its first byte sits elsewhere in its 16-byte chunk than the output's
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    assert torch.equal(hip(off, mixed[1:].cuda()).cpu(), want[1:])
    AUG.ClipAutoAugment(backend="hip", inplace=True)(off, mixed[1:].cuda())        # ... and in place: the same place
    assert torch.equal(dev.cpu()[1:], want[1:]) and torch.equal(dev.cpu()[0], clip[0])
    dev = clip.cuda()
    crop = dev[:, :, 1:4, 2:6]                                                      # non-contiguous in H and W
    cplan = AUG.make_plan([[(("rotate", 8, 1), ("equalize",))] * 2] * 3, size=(3, 4))
    assert torch.equal(hip(crop, cplan.cuda()).cpu(), AUG.ClipAutoAugment()(clip[:, :, 1:4, 2:6], cplan))
    one = hip(dev[2], mixed[2].cuda())                                             # a 4-D clip, a [T, 2, 8] plan
    assert one.shape == (2, H, W, 3) and torch.equal(one.cpu(), want[2])


def test_errors_before_any_launch():
    P = A.ops.clip_autoaugment_max_pixels()
    plan = AUG.make_plan([[(("invert",), None)]]).cuda()
    with pytest.raises(RuntimeError, match=f"limit of {P} pixels"):
        A.ops.clip_autoaugment(torch.zeros(1, 1, P + 1, 1, 3, dtype=torch.uint8, device="cuda"), plan)
    with pytest.raises(RuntimeError, match=f"limit of {P * 3 // 4} pixels"):
        A.ops.clip_autoaugment(torch.zeros(1, 1, 1, P * 3 // 4 + 1, 4, dtype=torch.uint8, device="cuda"), plan)
    with pytest.raises(RuntimeError, match="C is 2"):
        A.ops.clip_autoaugment(torch.zeros(1, 1, 4, 4, 2, dtype=torch.uint8, device="cuda"), plan)
    x = torch.zeros(2, 1, 4, 4, 3, dtype=torch.uint8, device="cuda")
    plan2 = torch.zeros(2, 1, 2, 8, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="overlaps"):
        A.ops.clip_autoaugment(x[:1], plan2[:1], out=x.view(-1)[16:16 + 48].view(1, 1, 4, 4, 3))
    hip = AUG.ClipAutoAugment(backend="hip")
    with pytest.raises(ValueError, match="channels"):
        hip(torch.zeros(1, 1, 4, 4, 2, dtype=torch.uint8, device="cuda"), plan)
    with pytest.raises(ValueError, match="frame size"):
        hip(x, AUG.make_plan([[(("rotate", 3, 1), None)]] * 2, size=(5, 4)))         # a host plan is checked against the clip
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip(x.cpu(), plan2.cpu())
    torch.cuda.synchronize()


def test_capture_and_replay_reads_the_plan_at_run_time():
    H, W = 9, 13
    a, b = _noise((2, 2, H, W, 3), 5), _noise((2, 2, H, W, 3), 6)
    p1 = AUG.make_plan([[(("equalize",), ("rotate", 9, 1))] * 2] * 2, size=(H, W))
    p2 = AUG.make_plan([[(("shearX", 5, -1), ("solarize", 5))] * 2] * 2, size=(H, W))
    hip = AUG.ClipAutoAugment(backend="hip")
    static, plan = a.cuda(), p1.cuda()
    hip(static, plan)                                                              # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip(static, plan)
    static.copy_(b.cuda())
    plan.copy_(p2.cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), AUG.ClipAutoAugment()(b, p2))


def test_one_launch_per_call():
    from torch.profiler import ProfilerActivity, profile
    hip = AUG.ClipAutoAugment(backend="hip")
    clip = _noise((4, 2, 9, 13, 3), 7).cuda()
    plan = AUG.draw_plan(4, 2, random.Random(3), size=(9, 13)).cuda()
    hip(clip, plan)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        hip(clip, plan)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print(names)
    if not names:
        pytest.skip("kineto recorded no device activity here: the launch count cannot be read")
    assert len(names) == 1 and "clip_autoaugment_kernel" in names[0], names       # no memset, no copy, no second pass
