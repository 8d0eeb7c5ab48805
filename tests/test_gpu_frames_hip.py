"""-m gpu: ``frames.ClipAssembler(backend="hip")`` - the kernels of csrc/clip_bank.hip - against the torch backend on the CPU, which
test_frames_cpu.py holds bytewise to the numpy restatement of the reference's clip assembly.  Every comparison is torch.equal.
The banks: 75-byte frames (every second one off a 16-byte boundary), 256-byte frames (aligned; RGB + mask), one row longer than
a tile, and 64 frames of the real size.  Videos of 7, 1, 20 and 12 frames; the indices take both sides of every boundary, -1 and
F; ``present`` has holes, the labelled frame itself among them.  The largest tensor of any case is 2.4 MB."""
import ctypes

import pytest
import torch

import avformer_amd as A
from clip_util import STATS, same_bits
from frames_util import F_SMALL, VIDEOS, boundary_indices, holes, random_frames, reference_clips, video_numbers

pytestmark = pytest.mark.gpu

FR = A.frames
MISSING = (3, 7, 8, 20, 27, 39)
SHAPES = ((5, 5, 3), (8, 8, 4), (1, 2100, 1))
INDEX = boundary_indices() + [13, 14, 30]
BIG_VIDEOS = VIDEOS + (24,)                                                     # F = 64


def _banks(shape, seed, lengths=VIDEOS, present=True):
    F = sum(lengths)
    frames, nr = random_frames(F, *shape, seed=seed), torch.from_numpy(video_numbers(lengths))
    p = torch.from_numpy(holes(F, MISSING)) if present else None
    cpu = FR.FrameBank(frames, nr, p)
    return cpu, cpu.to("cuda")


def _pair(T, d):
    return FR.ClipAssembler(T, d), FR.ClipAssembler(T, d, backend="hip")


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("T", [4, 16])
@pytest.mark.parametrize("d", [1, 2, 6])
def test_forward_sweep(d, T, shape):
    index = torch.tensor(INDEX)
    ref, hip = _pair(T, d)
    for present in (True, False):
        cpu, dev = _banks(shape, seed=T + d, present=present)
        want = ref(cpu, index)
        got = hip(dev, index.cuda())
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == want.shape and got.is_contiguous()
        assert torch.equal(got.cpu(), want), (shape, T, d, present)
        assert bool((want == 0).all(dim=(2, 3, 4)).any()) and bool((want != 0).any())   # black slots and real ones
    one = hip(dev, index.cuda()[5:6])                                          # B = 1; index is a view into a larger tensor
    assert torch.equal(one.cpu(), want[5:6])


@pytest.mark.parametrize("shape,k", [((5, 5, 3), 3), ((5, 5, 3), 1), ((8, 8, 4), 4), ((8, 8, 4), 1), ((1, 2100, 1), 1)])
def test_normalized_sweep(shape, k):
    C = shape[-1]
    mean, std = STATS[C]
    cpu, dev = _banks(shape, seed=k)
    index = torch.tensor(INDEX)
    flip = (torch.arange(len(INDEX)) % 3 == 0)                                  # mixed
    for T, d in ((4, 2), (16, 1), (4, 6)):
        ref, hip = _pair(T, d)
        for layout in ("cthw", "tchw"):
            for dtype in (torch.float32, torch.bfloat16):
                fe = A.clip.ClipFrontEnd(mean, std, channels=k, layout=layout, out_dtype=dtype)
                fe_dev = A.clip.ClipFrontEnd(mean, std, channels=k, layout=layout, out_dtype=dtype, backend="hip").cuda()
                for fl in (None, flip):
                    want = ref.normalized(cpu, index, fe, fl)
                    got = hip.normalized(dev, index.cuda(), fe_dev, None if fl is None else fl.cuda())
                    assert got.is_cuda and got.dtype == dtype and got.is_contiguous()
                    assert same_bits(got, want), (shape, k, T, d, layout, dtype, fl is not None)
    # black is a byte value: every pixel of an all-black clip (index F) is lut[c, 0]
    fe_dev = A.clip.ClipFrontEnd(mean, std, channels=k, backend="hip").cuda()
    black = hip.normalized(dev, torch.tensor([F_SMALL], device="cuda"), fe_dev)[0].cpu()
    for ci in range(k):
        assert bool((black[ci] == fe_dev.lut[C - k + ci, 0].cpu()).all()) and float(fe_dev.lut[C - k + ci, 0]) != 0.0


NEIGHBOUR_OPS = (("sharpness", 8, 1), ("rotate", 8, -1), ("shearX", 4, 1), ("equalize",))


@pytest.mark.parametrize("shape", [(5, 5, 3), (8, 8, 4), (37, 53, 3)])
def test_augmented_is_the_numpy_policy_on_the_restated_clip(shape):
    H, W, C = shape
    T, d = 4, 2
    cpu, dev = _banks(shape, seed=H)
    # index 2: slots -4 -2 0 2, black black real real;  index 11: slots 5 7 9 11 of another video / absent 8.. -> black black real real
    index = torch.tensor([2, 11, 2, 11, 30, 7])
    clips = reference_clips(cpu.frames.numpy(), cpu.video_db_nr.numpy(), cpu.present.numpy(), index.numpy(), T, d)
    black = (clips == 0).all(axis=(2, 3, 4))
    assert black[0].tolist() == [True, True, False, False] and black[1].tolist() == [True, True, False, False]
    a, b, c, e = NEIGHBOUR_OPS
    choices = [[(a, None), (b, None), (a, None), (b, None)],                   # each of the four on a black slot and on a real one
               [(c, None), (e, None), (c, None), (e, None)],
               [(None, b), (None, a), (None, b), (None, a)],
               [(e, c), (c, e), (e, c), (c, e)],
               [(("color", 8, -1), ("contrast", 8, 1)), (("autocontrast",), ("posterize", 8)), (None, None), (("solarize", 4), ("invert",))],
               [(a, e), (b, c), (e, a), (("invert",), None)]]                   # the one-frame video, absent: an all-black clip
    plan = A.augment.make_plan(choices, size=(H, W))
    want = A.augment.ClipAutoAugment(backend="numpy")(torch.from_numpy(clips), plan)
    hip = FR.ClipAssembler(T, d, backend="hip")
    aug = A.augment.ClipAutoAugment(backend="hip")
    got = hip.augmented(dev, index.cuda(), plan.cuda(), aug)
    assert got.is_cuda and got.dtype == torch.uint8 and got.is_contiguous()
    assert torch.equal(got.cpu(), want), [(b_, t) for b_ in range(6) for t in range(T) if not torch.equal(got[b_, t].cpu(), want[b_, t])]
    assert torch.equal(hip.augmented(dev, index.cuda(), plan, aug).cpu(), want)           # a plan on the CPU is uploaded
    assert torch.equal(FR.ClipAssembler(T, d).augmented(dev, index.cuda(), plan.cuda(), aug).cpu(), want)   # torch gather + hip policy


def test_real_size():
    import random
    shape = (112, 112, 3)
    cpu, dev = _banks(shape, seed=64, lengths=BIG_VIDEOS)
    assert len(cpu) == 64
    index = torch.tensor([0, 63, 39, 40, 41, 7, 64, 25])
    ref, hip = _pair(16, 1)
    want = ref(cpu, index)
    assert torch.equal(hip(dev, index.cuda()).cpu(), want)
    flip = torch.tensor([1, 0, 1, 0, 0, 1, 1, 0], dtype=torch.bool)
    for kw in ({}, {"layout": "tchw", "out_dtype": torch.bfloat16}):
        fe, fe_dev = A.clip.ClipFrontEnd(**kw), A.clip.ClipFrontEnd(backend="hip", **kw).cuda()
        assert same_bits(hip.normalized(dev, index.cuda(), fe_dev, flip.cuda()), fe(want, flip))
    ref4, hip4 = _pair(4, 6)
    idx4 = index[:3]
    plan = A.augment.draw_plan(3, 4, random.Random(7))
    want4 = A.augment.ClipAutoAugment()(ref4(cpu, idx4), plan)
    assert torch.equal(hip4.augmented(dev, idx4.cuda(), plan.cuda(), A.augment.ClipAutoAugment(backend="hip")).cpu(), want4)


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_c_abi_sentinels_null_present_and_refusals():
    lib = A._lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, W, C, T, d = 5, 5, 3, 4, 2
    cpu, dev = _banks((H, W, C), seed=3, present=False)
    index = torch.tensor(INDEX)
    idx_dev = index.cuda()
    B, F = len(INDEX), F_SMALL
    want = FR.ClipAssembler(T, d)(cpu, index)
    n = want.numel()
    for off in (0, 1, 16, 21):                                                  # the destination sits at any byte
        buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        dst = buf[off:off + n]
        rc = lib.avf_clip_gather(_p(dev.frames), _p(dev.video_db_nr), None, _p(idx_dev), F, B, T, d, H, W, C, _p(dst), stream)
        assert rc == 0, lib.avf_last_error()
        host = buf.cpu()
        assert torch.equal(host[off:off + n].view(want.shape), want), off
        assert bool((host[:off] == 0xA5).all()) and bool((host[off + n:] == 0xA5).all()), off
    # the fused entry points: the planes / the augmented clip inside sentinels
    fe = A.clip.ClipFrontEnd(channels=2)
    planes = fe(want)
    lut = fe.lut.cuda()
    fbuf = torch.full((planes.numel() + 8,), -7.0, device="cuda")
    rc = lib.avf_clip_gather_normalize(_p(dev.frames), _p(dev.video_db_nr), None, _p(idx_dev), F, B, T, d, H, W, C, 2, _p(lut), None,
                                       _p(fbuf[3:]), A._lib.F32, A._lib.CLIP_CTHW, stream)
    assert rc == 0, lib.avf_last_error()
    host = fbuf.cpu()
    assert torch.equal(host[3:3 + planes.numel()].view(planes.shape), planes)
    assert bool((host[:3] == -7.0).all()) and bool((host[3 + planes.numel():] == -7.0).all())
    plan = A.augment.make_plan([[(("rotate", 8, 1), ("equalize",))] * T] * B, size=(H, W))
    aug_want = A.augment.ClipAutoAugment()(want, plan)
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = lib.avf_clip_gather_autoaugment(_p(dev.frames), _p(dev.video_db_nr), None, _p(idx_dev), F, B, T, d, H, W, C, _p(plan.cuda()),
                                         _p(buf[21:]), stream)
    assert rc == 0, lib.avf_last_error()
    host = buf.cpu()
    assert torch.equal(host[21:21 + n].view(want.shape), aug_want)
    assert bool((host[:21] == 0xA5).all()) and bool((host[21 + n:] == 0xA5).all())

    # bad arguments are refused before anything is enqueued; the message names them
    buf = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    dst, plan_dev = buf[:n], plan.cuda()

    def calls(bank=dev.frames, T_=T, d_=d, C_=C):
        args = (_p(bank), _p(dev.video_db_nr), None, _p(idx_dev), F, B, T_, d_, H, W, C_)
        yield lib.avf_clip_gather(*args, _p(dst), stream)
        yield lib.avf_clip_gather_normalize(*args, 1, _p(lut), None, _p(fbuf), A._lib.F32, A._lib.CLIP_CTHW, stream)
        yield lib.avf_clip_gather_autoaugment(*args, _p(plan_dev), _p(dst), stream)
    for kw, word in (({"C_": 5}, b"C is 5"), ({"T_": 0}, b"T is 0"), ({"d_": 0}, b"d is 0"), ({"bank": None}, b"bank is null")):
        for rc in calls(**kw):
            assert rc != 0 and word in lib.avf_last_error(), (kw, lib.avf_last_error())
    torch.cuda.synchronize()
    assert bool((buf == 0xA5).all())


def _device_events(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_one_launch_per_call():
    _, dev = _banks((5, 5, 3), seed=4)
    hip = FR.ClipAssembler(4, 2, backend="hip")
    index = torch.tensor(INDEX, device="cuda")
    fe = A.clip.ClipFrontEnd(backend="hip").cuda()
    flip = (torch.arange(len(INDEX), device="cuda") % 2 == 0)
    aug = A.augment.ClipAutoAugment(backend="hip")
    plan = A.augment.make_plan([[(("equalize",), ("rotate", 8, 1))] * 4] * len(INDEX), size=(5, 5)).cuda()
    fns = {"clip_gather_kernel": lambda: hip(dev, index), "clip_normalize_kernel": lambda: hip.normalized(dev, index, fe, flip),
           "clip_autoaugment_kernel": lambda: hip.augmented(dev, index, plan, aug)}
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    events = {name: _device_events(fn) for name, fn in fns.items()}
    print(events)
    if not any(events.values()):
        pytest.skip("kineto recorded no device activity here: the launch count cannot be read")
    for name, ev in events.items():
        assert len(ev) == 1 and name in ev[0], (name, ev)                       # no memset, no copy, no second pass


def test_capture_and_replay_reads_index_and_flags_at_run_time():
    cpu, dev = _banks((5, 5, 3), seed=5)
    ref, hip = _pair(4, 2)
    fe, fe_dev = A.clip.ClipFrontEnd(), A.clip.ClipFrontEnd(backend="hip").cuda()
    i0, i1 = torch.tensor([2, 30, 39]), torch.tensor([40, 11, 26])
    f0, f1 = torch.tensor([1, 0, 0], dtype=torch.bool), torch.tensor([0, 1, 1], dtype=torch.bool)
    index, flags = i0.cuda(), f0.cuda()
    hip.normalized(dev, index, fe_dev, flags)                                   # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip.normalized(dev, index, fe_dev, flags)
    index.copy_(i1.cuda())
    flags.copy_(f1.cuda())
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone().cpu()
    assert torch.equal(got, ref.normalized(cpu, i1, fe, f1))
    assert not torch.equal(got, ref.normalized(cpu, i0, fe, f1)) and not torch.equal(got, ref.normalized(cpu, i1, fe, f0))
