"""Video front-end wire format: uint8 clip [B, T, H, W, C] -> the normalised planes the visual stream
consumes, [B, k, T, H, W] (the reference's wire format) or [B, T, k, H, W] (what ResFormer.forward views as [B*T, k, H, W]).

The reference's data loader builds every clip as uint8 [T, H, W, C] and transforms it on the host
(dataloader/aff2compdataset.py:69-77, 122-168; dataloader/clip_transforms.py):

  * RandomClipFlip: ``cv2.flip(frame, 1)`` on every frame of a clip - a mirror along W                    (111-128)
  * NumpyToTensor: ``astype(float32) / 255``, then ``permute(3, 0, 1, 2)``                                 (31-45)
  * Normalize: in place ``sub_(mean).div_(std)`` per channel, fp32                                         (59-93)
  * the model keeps ``clip[:, -num_channels:]`` and permutes to [B, T, k, H, W]                  (models/sformer.py:365-373)

Here the clip stays uint8 through the loader and the host link (a quarter of the bytes) and is transformed on the device.
``backend="torch"`` (default) runs that op sequence with ATen ops on any device; ``backend="hip"`` is one launch of
csrc/clip.hip that indexes a 256-entry table per channel - the table is built once, on the CPU, with the same op sequence, so the
two backends agree bit for bit.  ``invert`` is the inverse direction of the reference's ``ComposeWithInvert``.

Parity: unpinned by a reference fixture (clip_transforms.py needs cv2 and torchaudio, which are not importable here); checked
bitwise against an independent numpy restatement of the cited lines (tests/clip_util.py).
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from . import ops

BACKENDS = ("torch", "hip")
LAYOUTS = ("cthw", "tchw")
OUT_DTYPES = (torch.float32, torch.bfloat16)
RGB_MEAN, RGB_STD = (0.43216, 0.394666, 0.37645), (0.22803, 0.22145, 0.216989)            # aff2compdataset.py:70-71
RGBM_MEAN, RGBM_STD = RGB_MEAN + (0.5,), RGB_STD + (0.225,)                                # RGB + mask: aff2compdataset.py:76-77
MAX_CHANNELS = 4


def draw_flips(B: int, p: float = 0.5, device=None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """bool [B]: which clips of a batch RandomClipFlip(p) mirrors (``torch.rand(B) < p``), drawn on ``device``."""
    return torch.rand(B, device=device, generator=generator) < p


def build_lut(mean: torch.Tensor, std: torch.Tensor) -> torch.Tensor:
    """fp32 [C, 256]: the reference's op sequence on the 256 byte values - astype(float32) / 255, sub_(mean), div_(std)."""
    v = torch.arange(256, dtype=torch.uint8).to(torch.float32) / torch.tensor(255.0)
    lut = v.repeat(mean.numel(), 1)
    return lut.sub_(mean[:, None]).div_(std[:, None])


class ClipFrontEnd(nn.Module):
    """``forward(clip_u8 [B, T, H, W, C] or [T, H, W, C], flip=None)`` -> [B, k, T, H, W] (``layout="cthw"``) or [B, T, k, H, W]
    (``"tchw"``) in ``out_dtype`` (fp32 / bf16, round to nearest even), without the batch axis for a 4-D clip.  ``channels=k``
    keeps the LAST k of the C channels (k = 1 of an RGB+mask clip is the mask alone).  ``flip``: None, or bool / uint8 [B] on the
    clip's device (``draw_flips``); a flagged clip is mirrored along W.  The flags are read on the device.

    ``backend="torch"`` (default): ATen ops on any device.  ``backend="hip"``: one launch of csrc/clip.hip, the clip must be on
    the GPU (no CPU fallback), under ``no_grad``.  Both give the same bits: ``lut[c, byte]``.

    ``invert(x)``: x in the module's layout with all C channels -> uint8 [B, T, H, W, C] (or [T, H, W, C]),
    ``trunc(clamp(((x * std) + mean) * 255, 0, 255))`` with each operation rounded to fp32, NaN -> 0.  The clamp is this
    project's definition: the reference casts ``mul(255)`` to uint8 directly, which is undefined outside 0..255.  A flip is not
    undone (RandomClipFlip does nothing on invert)."""

    def __init__(self, mean: Sequence[float] = RGB_MEAN, std: Sequence[float] = RGB_STD, channels: Optional[int] = None,
                 layout: str = "cthw", out_dtype: torch.dtype = torch.float32, backend: str = "torch"):
        super().__init__()
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        if layout not in LAYOUTS:
            raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
        if out_dtype not in OUT_DTYPES:
            raise ValueError(f"out_dtype must be one of {OUT_DTYPES}, got {out_dtype!r}")
        mean, std = tuple(float(m) for m in mean), tuple(float(s) for s in std)
        if len(mean) != len(std):
            raise ValueError(f"mean has {len(mean)} entries and std {len(std)}")
        if not 1 <= len(mean) <= MAX_CHANNELS:
            raise ValueError(f"a clip has 1..{MAX_CHANNELS} channels, mean / std have {len(mean)}")
        C = len(mean)
        k = C if channels is None else int(channels)
        if not 1 <= k <= C:
            raise ValueError(f"channels must be in 1..{C}, got {channels!r}")
        self.backend, self.layout, self.out_dtype = backend, layout, out_dtype
        self.in_channels, self.channels = C, k
        self.mean, self.std = mean, std
        mean_t, std_t = torch.tensor(mean, dtype=torch.float32), torch.tensor(std, dtype=torch.float32)
        self.register_buffer("lut", build_lut(mean_t, std_t), persistent=False)
        self.register_buffer("mean_t", mean_t, persistent=False)
        self.register_buffer("std_t", std_t, persistent=False)
        # x / 255 with a TENSOR divisor: a Python scalar becomes a multiplication by the reciprocal on the GPU (one ulp off)
        self.register_buffer("c255", torch.tensor(255.0), persistent=False)

    def _batched(self, t: torch.Tensor, what: str):
        if t.dim() not in (4, 5):
            raise ValueError(f"{what}: expected 4 or 5 dimensions, got {tuple(t.shape)}")
        return (t[None], True) if t.dim() == 4 else (t, False)

    def _flags(self, flip, B: int, device) -> Optional[torch.Tensor]:
        if flip is None:
            return None
        if not torch.is_tensor(flip) or flip.dtype not in (torch.bool, torch.uint8) or tuple(flip.shape) != (B,):
            raise ValueError(f"flip must be None or a bool / uint8 tensor [{B}]")
        if flip.device != device:
            raise ValueError(f"flip is on {flip.device}, the clip on {device}")
        return flip.contiguous()

    def forward(self, clip_u8: torch.Tensor, flip: Optional[torch.Tensor] = None) -> torch.Tensor:
        if clip_u8.dtype != torch.uint8:
            raise ValueError(f"the clip must be uint8, got {clip_u8.dtype}")
        clip, squeeze = self._batched(clip_u8, "clip")
        C, k = self.in_channels, self.channels
        if clip.shape[-1] != C:
            raise ValueError(f"the clip has {clip.shape[-1]} channels, mean / std have {C}")
        if self.backend == "hip" and not clip.is_cuda:
            raise RuntimeError("ClipFrontEnd (HIP) needs its input on the MI355X; there is no CPU fallback - "
                               "use backend='torch' on the host")
        flip = self._flags(flip, clip.shape[0], clip.device)
        if self.backend == "hip":
            with torch.no_grad():
                out = ops.clip_normalize(clip.contiguous(), self.lut, k, flip, self.layout, self.out_dtype)
        else:
            x = clip[..., C - k:]
            if flip is not None:                                       # cv2.flip(frame, 1) on the bytes of the flagged clips
                x = torch.where(flip.to(torch.bool).view(-1, 1, 1, 1, 1), x.flip(3), x)
            x = (x.to(torch.float32) / self.c255).permute(0, 4, 1, 2, 3)   # astype(float32) / 255; [B, k, T, H, W]
            x.sub_(self.mean_t[C - k:].view(1, k, 1, 1, 1)).div_(self.std_t[C - k:].view(1, k, 1, 1, 1))
            if self.layout == "tchw":
                x = x.permute(0, 2, 1, 3, 4)
            out = x.to(self.out_dtype).contiguous()
        return out[0] if squeeze else out

    def invert(self, x: torch.Tensor) -> torch.Tensor:
        C = self.in_channels
        if self.channels != C:
            raise ValueError(f"invert needs all {C} channels (channels=None), this front-end keeps {self.channels}")
        if x.dtype not in OUT_DTYPES:
            raise ValueError(f"x must be one of {OUT_DTYPES}, got {x.dtype}")
        x, squeeze = self._batched(x, "x")
        c_axis = 1 if self.layout == "cthw" else 2
        if x.shape[c_axis] != C:
            raise ValueError(f"x has {x.shape[c_axis]} channels on axis {c_axis}, mean / std have {C}")
        if self.backend == "hip":
            if not x.is_cuda:
                raise RuntimeError("ClipFrontEnd (HIP) needs its input on the MI355X; there is no CPU fallback - "
                                   "use backend='torch' on the host")
            with torch.no_grad():
                out = ops.clip_denormalize(x.contiguous(), self.mean_t, self.std_t, self.layout)
        else:
            shape = [1] * 5
            shape[c_axis] = C
            y = x.detach().to(torch.float32).mul(self.std_t.view(shape)).add_(self.mean_t.view(shape)).mul_(255)
            y = torch.nan_to_num(torch.clamp(y, 0.0, 255.0), nan=0.0).to(torch.uint8)
            out = (y.permute(0, 2, 3, 4, 1) if self.layout == "cthw" else y.permute(0, 1, 3, 4, 2)).contiguous()
        return out[0] if squeeze else out
