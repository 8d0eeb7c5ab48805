"""-m gpu: ``clip.ClipFrontEnd(backend="hip")`` - the kernels of csrc/clip.hip - against the torch backend on the CPU, which
test_clip_cpu.py holds bitwise to the numpy restatement of the reference's clip transform.  Every comparison is torch.equal.
The sweep's widths give rows shorter than a vector, exact vectors, tails, and (C = 3) rows that start unaligned; the largest
tensor of any case is 2.4 MB."""
import pytest
import torch

import avformer_amd as A
from clip_util import STATS, all_values_clip, ramp_noise_clip, random_clip

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 4, 5, 8, 13, 16, 37)
LAYOUTS = ("cthw", "tchw")
DTYPES = (torch.float32, torch.bfloat16)
FLIPS = (None, [0, 1], [1, 1])


def _pair(C, **kw):
    mean, std = STATS[C]
    return A.clip.ClipFrontEnd(mean, std, backend="torch", **kw), A.clip.ClipFrontEnd(mean, std, backend="hip", **kw).cuda()


def _flags(flip, device):
    return None if flip is None else torch.tensor(flip, dtype=torch.bool, device=device)


@pytest.mark.parametrize("C", [1, 3, 4])
@pytest.mark.parametrize("W", WIDTHS)
def test_forward_sweep(W, C):
    clips = [random_clip(2, 2, 3, W, C, seed=100 * W + C)]
    if W == 16:
        clips.append(all_values_clip(C, T=2).reshape(2, 1, 16, 16, C))     # all 256 values in every channel
    for clip in clips:
        dev = clip.cuda()
        for k in sorted({1, C}):
            for layout in LAYOUTS:
                for dtype in DTYPES:
                    ref, hip = _pair(C, channels=k, layout=layout, out_dtype=dtype)
                    for flip in FLIPS:
                        want = ref(clip, _flags(flip, "cpu"))
                        got = hip(dev, _flags(flip, "cuda"))
                        assert got.is_cuda and got.dtype == dtype and got.shape == want.shape and got.is_contiguous()
                        assert torch.equal(got.cpu(), want), (tuple(clip.shape), k, layout, dtype, flip)


@pytest.mark.parametrize("shape,k", [((2, 16, 112, 112, 3), 3), ((1, 8, 112, 112, 4), 4), ((1, 8, 112, 112, 4), 1)])
def test_forward_real_size(shape, k):
    C = shape[-1]
    clip = random_clip(*shape, seed=k)
    ref, hip = _pair(C, channels=k)
    flip = [1, 0][:shape[0]]
    want = ref(clip, _flags(flip, "cpu"))
    got = hip(clip.cuda(), _flags(flip, "cuda"))
    assert torch.equal(got.cpu(), want)
    ref16, hip16 = _pair(C, channels=k, layout="tchw", out_dtype=torch.bfloat16)
    assert torch.equal(hip16(clip.cuda()).cpu(), ref16(clip))


@pytest.mark.parametrize("W", [13, 16])
def test_a_flip_mirrors_w_only(W):
    clip = ramp_noise_clip(2, 3, 5, W, 3, seed=W)
    for layout in LAYOUTS:
        _, hip = _pair(3, layout=layout)
        plain = hip(clip.cuda()).cpu()
        assert not torch.equal(plain, plain.flip(-1)) and not torch.equal(plain[0], plain[1])
        both = hip(clip.cuda(), _flags([1, 1], "cuda")).cpu()
        assert torch.equal(both, plain.flip(-1))                            # W reversed; T, H and channels where they were
        first = hip(clip.cuda(), _flags([1, 0], "cuda")).cpu()
        assert torch.equal(first[0], plain[0].flip(-1)) and torch.equal(first[1], plain[1])
        u8 = hip(clip.cuda(), torch.tensor([1, 0], dtype=torch.uint8, device="cuda")).cpu()
        assert torch.equal(u8, first)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES)
def test_invert_equals_the_torch_backend(dtype, layout):
    for C, W in ((1, 5), (3, 13), (4, 16), (3, 37)):
        ref, hip = _pair(C, layout=layout, out_dtype=dtype)
        clip = random_clip(2, 2, 3, W, C, seed=C + W)
        x = ref(clip)                                                       # in range ...
        flat = x.view(-1)
        g = torch.Generator().manual_seed(W)
        idx = torch.randperm(flat.numel(), generator=g)[:8]
        flat[idx] = torch.tensor([float("nan"), float("inf"), float("-inf"), -1e9, 1e9, -3.0, 3.5, 1e-3], dtype=dtype)
        want = ref.invert(x)
        got = hip.invert(x.cuda())
        assert got.is_cuda and got.dtype == torch.uint8 and got.shape == clip.shape
        assert torch.equal(got.cpu(), want), (C, W)
        assert torch.equal(hip.invert(x[0].cuda()).cpu(), want[0])
    ref, hip = _pair(3, layout=layout, out_dtype=dtype)                     # more than one tile per frame
    x = ref(random_clip(1, 2, 112, 112, 3, seed=9))
    assert torch.equal(hip.invert(x.cuda()).cpu(), ref.invert(x))


def test_device_behaviour():
    ref, hip = _pair(3)
    clip = random_clip(4, 2, 6, 13, 3, seed=3)
    dev = clip.cuda()
    y = hip(dev)
    assert y.is_cuda and not y.requires_grad and y.shape == (4, 3, 2, 6, 13)
    one = hip(dev[1])
    assert one.shape == (3, 2, 6, 13) and torch.equal(one, y[1])
    view = dev[::2]                                                         # a sliced batch
    assert not view.is_contiguous()
    assert torch.equal(hip(view), hip(view.contiguous())) and torch.equal(hip(view).cpu(), ref(clip[::2]))
    off = dev[1:]                                                           # contiguous, but its first byte is not 16-byte aligned
    assert off.is_contiguous() and off.data_ptr() % 16 != 0
    assert torch.equal(hip(off).cpu(), ref(clip[1:]))
    crop = dev[:, :, 1:5, 2:9]                                              # non-contiguous in H and W
    assert torch.equal(hip(crop).cpu(), ref(clip[:, :, 1:5, 2:9]))


def test_capture_and_replay_reads_the_flags_at_run_time():
    ref, hip = _pair(3)
    a, b = random_clip(2, 2, 5, 13, 3, seed=1), random_clip(2, 2, 5, 13, 3, seed=2)
    static, flags = a.cuda(), _flags([1, 0], "cuda")
    hip(static, flags)                                                      # (the library is loaded before the capture)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = hip(static, flags)
    static.copy_(b.cuda())
    flags.copy_(_flags([0, 1], "cuda"))
    graph.replay()
    torch.cuda.synchronize()
    got = out.clone().cpu()
    assert torch.equal(got, ref(b, _flags([0, 1], "cpu")))
    assert not torch.equal(got, ref(b, _flags([1, 0], "cpu"))) and not torch.equal(got, ref(a, _flags([0, 1], "cpu")))


def test_one_launch_per_call():
    from torch.profiler import ProfilerActivity, profile
    _, hip = _pair(3)
    clip, flags = random_clip(2, 2, 5, 13, 3, seed=4).cuda(), _flags([1, 0], "cuda")
    x = hip(clip, flags)
    hip.invert(x)
    torch.cuda.synchronize()

    def device_events(fn):
        with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
            fn()
            torch.cuda.synchronize()
        return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    fwd = device_events(lambda: hip(clip, flags))
    inv = device_events(lambda: hip.invert(x))
    print(fwd, inv)
    if not fwd and not inv:
        pytest.skip("kineto recorded no device activity here: the launch count cannot be read")
    assert len(fwd) == 1 and "clip_normalize_kernel" in fwd[0], fwd          # no memset, no copy, no second pass
    assert len(inv) == 1 and "clip_denormalize_kernel" in inv[0], inv
