"""Shared by the clip front-end tests: an independent numpy restatement of the reference's clip transform and the test clips.

The reference's dataloader/clip_transforms.py cannot be imported here (it needs cv2 and torchaudio), so the front-end's parity is
unpinned by a reference fixture; it is held bitwise to this restatement of the cited lines instead:

  RandomClipFlip   (clip_transforms.py:111-128)   cv2.flip(frame, 1) on every frame of a flagged clip = [..., ::-1, :] on W
  NumpyToTensor    (clip_transforms.py:31-45)     clip.astype(np.float32) / 255, then permute(3, 0, 1, 2)
  Normalize        (clip_transforms.py:59-93)     in place sub_(mean_t).div_(std_t), fp32, per channel
  the model        (models/sformer.py:365-373)    clip[:, -num_channels:], permute(0, 2, 1, 3, 4)

Only numpy arithmetic is used up to the final dtype; bf16 is fp32 rounded to nearest even on the bit pattern."""
import numpy as np
import torch

RGB = ((0.43216, 0.394666, 0.37645), (0.22803, 0.22145, 0.216989))
RGBM = ((0.43216, 0.394666, 0.37645, 0.5), (0.22803, 0.22145, 0.216989, 0.225))
GREY = ((0.45,), (0.225,))
STATS = {1: GREY, 3: RGB, 4: RGBM}


def bf16_round(x: np.ndarray) -> torch.Tensor:
    """fp32 array (no NaN) -> torch.bfloat16, round to nearest even, on the bits"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    bits = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return torch.from_numpy(bits.view(np.int16).copy()).view(torch.bfloat16)


def reference_transform(clip_u8: np.ndarray, mean, std, flip=None, k=None, layout="cthw", bf16=False) -> torch.Tensor:
    """clip_u8 uint8 [B, T, H, W, C] -> [B, k, T, H, W] / [B, T, k, H, W], clip by clip as the data loader does"""
    B, C = clip_u8.shape[0], clip_u8.shape[-1]
    k = C if k is None else k
    mean_t = np.asarray(mean, dtype=np.float32)[:, None, None, None]
    std_t = np.asarray(std, dtype=np.float32)[:, None, None, None]
    out = []
    for b in range(B):
        clip = clip_u8[b].copy()                                   # [T, H, W, C]
        if flip is not None and bool(flip[b]):
            clip = clip[..., ::-1, :]
        x = clip.astype(np.float32) / 255
        x = np.ascontiguousarray(np.transpose(x, (3, 0, 1, 2)))    # [C, T, H, W]
        x -= mean_t
        x /= std_t
        out.append(x)
    x = np.stack(out)[:, C - k:]
    if layout == "tchw":
        x = np.transpose(x, (0, 2, 1, 3, 4))
    x = np.ascontiguousarray(x)
    assert x.dtype == np.float32
    return bf16_round(x) if bf16 else torch.from_numpy(x)


def random_clip(B, T, H, W, C, seed) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, T, H, W, C), dtype=torch.uint8, generator=g)


def all_values_clip(C, T=1) -> torch.Tensor:
    """uint8 [1, T, 16, 16, C]: every byte value in every channel of every frame, at another place in each"""
    v = torch.arange(256).view(1, 1, 256, 1)
    shift = 37 * torch.arange(C).view(1, 1, 1, C) + 101 * torch.arange(T).view(1, T, 1, 1)
    return ((v + shift) % 256).to(torch.uint8).reshape(1, T, 16, 16, C)


def ramp_noise_clip(B, T, H, W, C, seed) -> torch.Tensor:
    """a ramp over (t, h, w, c) plus noise: no symmetry along any axis that a wrong mirror could hide behind"""
    g = torch.Generator().manual_seed(seed)
    t, h, w, c = torch.meshgrid(torch.arange(T), torch.arange(H), torch.arange(W), torch.arange(C), indexing="ij")
    ramp = (w * 200) // max(W - 1, 1) + 7 * h + 29 * t + 13 * c
    noise = torch.randint(0, 16, (B, T, H, W, C), generator=g) + 3 * torch.arange(B).view(B, 1, 1, 1, 1)
    return ((ramp[None] + noise) % 256).to(torch.uint8)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """torch.equal on the bit patterns (it would call -0.0 and 0.0 equal, and no NaN equal to itself)"""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {torch.float32: torch.int32, torch.bfloat16: torch.int16}.get(a.dtype)
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    return torch.equal(a.view(view), b.view(view)) if view is not None else torch.equal(a, b)
