"""Clips assembled from a resident frame bank: the last host stage of the video stream, on the device.

The reference's data set builds the clip of a sample on the host (dataloader/aff2compdataset.py:122-156; testset.py:84-113 repeats
the loop).  With clip length ``T`` (``n_frames``, opts.py:35, default 16) and dilation ``d`` (opts.py:36, default 3):

  * the clip starts black: ``np.zeros((clip_len, H, W, C), uint8)``                                             (122-125)
  * slot ``t`` of sample ``index`` is frame ``a = index - d * (T - 1 - t)``:
    ``range(index - T * d + d, index - T * d + d * (T + 1), d)``, whose last entry is ``index`` itself         (45, 126-127)
  * the slot stays black where ``a < 0``, ``a >= len(self)`` or ``video_db_nr[a] != video_db_nr[index]``        (129-132)
  * ... and where loading the frame fails: ``try: clip[clip_i, ...] = img / except: pass``                      (142-155)
  * otherwise it is the frame's bytes

Neighbouring samples share T - 1 of their T frames, so a host-assembled batch carries every frame about T times over the host
link.  Here the cropped frames stay on the device as one uint8 tensor - the bank - and only ``index [B]`` travels per step.

Black is a byte value, not an output value: normalised, a black pixel is ``lut[c, 0]``, and a black frame goes through its
AutoAugment slots like any other (autoaugment.py:104-112 loops over every frame).  An ``index`` outside ``[0, F)`` gives an
all-black clip - this project's definition: the reference would raise, nothing on the device can.

``backend="torch"`` (default) is ATen ops on any device: the table of source frames, ``index_select``, ``where``, then the
existing modules.  ``backend="hip"`` is one launch of csrc/clip_bank.hip per method.  Both give the same bytes and bits.

What holds for bytes over the host link holds for S-Former FLOPs.  The video stream applies ``s_former`` per frame
(vformer.py:232-268 flattens [b, t] into the batch) and, frozen, in eval mode: a frame's 512 features do not depend on the clip it
sits in.  ``FeatureBank`` keeps them once per frame (2 KB against 37.6 KB of pixels), with the features of a black frame beside
them, and ``FeatureClipAssembler`` builds the [B, T + 1, 512] token tensor that ``t_former``'s stack consumes (vformer.py:279-287)
by the same rule, applied to feature rows: one launch of csrc/feature_bank.hip with ``backend="hip"``.

Parity: unpinned by a reference fixture (the data set class needs lmdb and cv2, which are not importable here); checked bytewise
against an independent numpy restatement of the cited lines (tests/frames_util.py).
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from . import ops
from .augment import ClipAutoAugment, _check_rotate_size
from .clip import MAX_CHANNELS, ClipFrontEnd

BACKENDS = ("torch", "hip")


class FrameBank:
    """The frames of a data set split on one device: ``frames_u8`` uint8 [F, H, W, C] (C in 1..4), ``video_db_nr`` int32 [F] (the
    video every frame belongs to; equal numbers need not be neighbours) and ``present`` bool / uint8 [F] or None (0: the frame
    could not be decoded and is black).  All contiguous, all on the device of ``frames_u8``."""

    def __init__(self, frames_u8: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor] = None):
        if not torch.is_tensor(frames_u8) or frames_u8.dtype != torch.uint8 or frames_u8.dim() != 4:
            raise ValueError("frames_u8 must be a uint8 tensor [F, H, W, C]")
        F, H, W, C = frames_u8.shape
        if F < 1 or H < 1 or W < 1:
            raise ValueError(f"the bank needs at least one frame of at least one pixel, got {tuple(frames_u8.shape)}")
        if not 1 <= C <= MAX_CHANNELS:
            raise ValueError(f"a frame has 1..{MAX_CHANNELS} channels, got {C}")
        if not torch.is_tensor(video_db_nr) or video_db_nr.dtype != torch.int32 or tuple(video_db_nr.shape) != (F,):
            raise ValueError(f"video_db_nr must be an int32 tensor [{F}]")
        if present is not None and (not torch.is_tensor(present) or present.dtype not in (torch.bool, torch.uint8)
                                    or tuple(present.shape) != (F,)):
            raise ValueError(f"present must be None or a bool / uint8 tensor [{F}]")
        for name, t in (("video_db_nr", video_db_nr), ("present", present)):
            if t is not None and t.device != frames_u8.device:
                raise ValueError(f"{name} is on {t.device}, the frames on {frames_u8.device}")
        for name, t in (("frames_u8", frames_u8), ("video_db_nr", video_db_nr), ("present", present)):
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        self.frames, self.video_db_nr, self.present = frames_u8, video_db_nr, present

    def __len__(self) -> int:
        return self.frames.shape[0]

    @property
    def device(self) -> torch.device:
        return self.frames.device

    @property
    def frame_shape(self):
        return tuple(self.frames.shape[1:])

    def to(self, device) -> "FrameBank":
        return FrameBank(self.frames.to(device), self.video_db_nr.to(device), None if self.present is None else self.present.to(device))


def _source_table(video_db_nr: torch.Tensor, present: Optional[torch.Tensor], index: torch.Tensor, T: int, d: int) -> torch.Tensor:
    """int64 [B, T]: the bank entry of every slot of the clips of ``index``, -1 for a black one - the rule of the module docstring,
    the one copy of it in torch ops (``ClipAssembler`` applies it to frames, ``FeatureClipAssembler`` to feature rows)."""
    F = video_db_nr.shape[0]
    label_ok = (index >= 0) & (index < F)
    a = index[:, None] - d * (T - 1 - torch.arange(T, device=index.device))[None, :]          # aff2compdataset.py:126-127
    inside = (a >= 0) & (a < F) & label_ok[:, None]
    a_safe, label_safe = torch.where(inside, a, torch.zeros_like(a)), torch.where(label_ok, index, torch.zeros_like(index))
    ok = inside & (video_db_nr[a_safe] == video_db_nr[label_safe][:, None])                    # :129
    if present is not None:
        ok = ok & (present[a_safe] != 0)                                                       # :142-155
    return torch.where(ok, a, torch.full_like(a, -1))


class ClipAssembler(nn.Module):
    """The clips of ``index`` int64 [B] out of a ``FrameBank``, ``clip_len`` frames each, ``dilation`` frames apart, ending at the
    labelled frame ``index[b]`` (the module docstring states the rule).

    ``source_table(bank, index)`` -> int64 [B, T]: the bank frame of every slot, -1 for a black one.  Plain torch, any device.
    ``forward(bank, index)`` -> uint8 [B, T, H, W, C], what ``ClipAutoAugment`` and ``ClipFrontEnd`` take.
    ``normalized(bank, index, front_end, flip=None)`` -> ``front_end(forward(bank, index), flip)``: the planes in the front end's
    layout, dtype and channel slice.
    ``augmented(bank, index, plan, augment)`` -> ``augment(forward(bank, index), plan)``: the augmented uint8 clip.
    ``augmented_normalized(bank, index, plan, augment, front_end, flip=None)`` ->
    ``front_end(augment(forward(bank, index), plan), flip)``: the reference's training transform (aff2compdataset.py:72-74) from
    the bank, in the front end's layout, dtype and channel slice.

    ``backend="torch"`` (default): ATen ops on any device, then the modules that were passed in.  ``backend="hip"``: one launch of
    csrc/clip_bank.hip per method - no uint8 clip is written by ``normalized`` and ``augmented_normalized``, no plain one by
    ``augmented`` -, the bank must be on the GPU (no CPU fallback), under ``no_grad``; ``index``, ``flip`` and ``plan`` are read on
    the device.  Both give the same bytes."""

    def __init__(self, clip_len: int = 16, dilation: int = 3, backend: str = "torch"):
        super().__init__()
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        for name, v in (("clip_len", clip_len), ("dilation", dilation)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an integer of at least 1, got {v!r}")
        self.clip_len, self.dilation, self.backend = clip_len, dilation, backend

    def _check(self, bank: FrameBank, index: torch.Tensor, table_only: bool = False) -> None:
        if not isinstance(bank, FrameBank):
            raise ValueError(f"bank must be a FrameBank, got {type(bank).__name__}")
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
            raise ValueError("index must be an int64 tensor [B] with B >= 1")
        if index.device != bank.device:
            raise ValueError(f"index is on {index.device}, the bank on {bank.device}")
        if self.backend == "hip" and not table_only and not bank.frames.is_cuda:
            raise RuntimeError("ClipAssembler (HIP) needs its bank on the MI355X; there is no CPU fallback - "
                               "use backend='torch' on the host")

    def source_table(self, bank: FrameBank, index: torch.Tensor) -> torch.Tensor:
        self._check(bank, index, table_only=True)
        return _source_table(bank.video_db_nr, bank.present, index, self.clip_len, self.dilation)

    def _gather(self, bank: FrameBank, index: torch.Tensor) -> torch.Tensor:
        table = self.source_table(bank, index)
        B, T = table.shape
        black = (table < 0).view(B, T, 1, 1, 1)
        clip = bank.frames.index_select(0, table.clamp(min=0).view(-1)).view(B, T, *bank.frame_shape)
        return torch.where(black, torch.zeros((), dtype=torch.uint8, device=clip.device), clip)

    def forward(self, bank: FrameBank, index: torch.Tensor) -> torch.Tensor:
        self._check(bank, index)
        if self.backend == "hip":
            with torch.no_grad():
                return ops.clip_gather(bank.frames, bank.video_db_nr, bank.present, index.contiguous(), self.clip_len, self.dilation)
        return self._gather(bank, index)

    def normalized(self, bank: FrameBank, index: torch.Tensor, front_end: ClipFrontEnd,
                   flip: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check(bank, index)
        if not isinstance(front_end, ClipFrontEnd):
            raise ValueError(f"front_end must be a ClipFrontEnd, got {type(front_end).__name__}")
        if self.backend != "hip":
            return front_end(self._gather(bank, index), flip)
        C = bank.frame_shape[-1]
        if C != front_end.in_channels:
            raise ValueError(f"the bank has {C} channels, mean / std have {front_end.in_channels}")
        flip = front_end._flags(flip, index.numel(), bank.device)
        if front_end.lut.device != bank.device:
            raise ValueError(f"the front end is on {front_end.lut.device}, the bank on {bank.device}")
        with torch.no_grad():
            return ops.clip_gather_normalize(bank.frames, bank.video_db_nr, bank.present, index.contiguous(), self.clip_len,
                                             self.dilation, front_end.lut, front_end.channels, flip, front_end.layout,
                                             front_end.out_dtype)

    def augmented(self, bank: FrameBank, index: torch.Tensor, plan: torch.Tensor, augment: ClipAutoAugment) -> torch.Tensor:
        self._check(bank, index)
        if not isinstance(augment, ClipAutoAugment):
            raise ValueError(f"augment must be a ClipAutoAugment, got {type(augment).__name__}")
        if self.backend != "hip":
            return augment(self._gather(bank, index), plan)
        if augment.backend != "hip":
            raise ValueError("ClipAssembler (HIP) runs the policy in its own launch: augment must be ClipAutoAugment(backend='hip')")
        B, T = index.numel(), self.clip_len
        H, W, C = bank.frame_shape
        if C not in (3, 4):
            raise ValueError(f"the bank has {C} channels; the policy transforms RGB (C = 3) or RGB + mask (C = 4)")
        if not torch.is_tensor(plan) or plan.dtype != torch.int32:
            raise ValueError("plan must be an int32 tensor (draw_plan / make_plan)")
        if tuple(plan.shape) != (B, T, 2, 8):
            raise ValueError(f"plan must be [{B}, {T}, 2, 8] for these clips, got {tuple(plan.shape)}")
        if not plan.is_cuda:
            _check_rotate_size(plan, H, W)
            plan = plan.to(bank.device, non_blocking=True)
        elif plan.device != bank.device:
            raise ValueError(f"plan is on {plan.device}, the bank on {bank.device}")
        with torch.no_grad():
            return ops.clip_gather_autoaugment(bank.frames, bank.video_db_nr, bank.present, index.contiguous(), self.clip_len,
                                               self.dilation, plan.contiguous())

    def augmented_normalized(self, bank: FrameBank, index: torch.Tensor, plan: torch.Tensor, augment: ClipAutoAugment,
                             front_end: ClipFrontEnd, flip: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check(bank, index)
        if not isinstance(augment, ClipAutoAugment):
            raise ValueError(f"augment must be a ClipAutoAugment, got {type(augment).__name__}")
        if not isinstance(front_end, ClipFrontEnd):
            raise ValueError(f"front_end must be a ClipFrontEnd, got {type(front_end).__name__}")
        B, T = index.numel(), self.clip_len
        H, W, C = bank.frame_shape
        if C not in (3, 4):
            raise ValueError(f"the bank has {C} channels; the policy transforms RGB (C = 3) or RGB + mask (C = 4)")
        if C != front_end.in_channels:
            raise ValueError(f"front_end: the bank has {C} channels, mean / std have {front_end.in_channels}")
        if not torch.is_tensor(plan) or plan.dtype != torch.int32:
            raise ValueError("plan must be an int32 tensor (draw_plan / make_plan)")
        if tuple(plan.shape) != (B, T, 2, 8):
            raise ValueError(f"plan must be [{B}, {T}, 2, 8] for these clips, got {tuple(plan.shape)}")
        flip = front_end._flags(flip, B, bank.device)
        if self.backend != "hip":
            return front_end(augment(self._gather(bank, index), plan), flip)
        if augment.backend != "hip":
            raise ValueError("ClipAssembler (HIP) runs the policy in its own launch: augment must be ClipAutoAugment(backend='hip')")
        if front_end.lut.device != bank.device:
            raise ValueError(f"front_end is on {front_end.lut.device}, the bank on {bank.device}")
        if not plan.is_cuda:
            _check_rotate_size(plan, H, W)
            plan = plan.to(bank.device, non_blocking=True)
        elif plan.device != bank.device:
            raise ValueError(f"plan is on {plan.device}, the bank on {bank.device}")
        with torch.no_grad():
            return ops.clip_gather_autoaugment_normalize(bank.frames, bank.video_db_nr, bank.present, index.contiguous(), self.clip_len,
                                                         self.dilation, plan.contiguous(), front_end.lut, front_end.channels, flip,
                                                         front_end.layout, front_end.out_dtype)


class FeatureBank:
    """The per-frame features of a data set split on one device: ``features`` fp32 [F, D] (D a multiple of 4), ``black`` fp32 [D]
    (the features of a black frame: black is a byte value, normalised and run through the S-Former like any other frame),
    ``video_db_nr`` int32 [F] and ``present`` bool / uint8 [F] or None as ``FrameBank`` takes them.  All contiguous, all on the
    device of ``features``.  The row of a frame with ``present == 0`` may hold anything: the rule never reads it."""

    def __init__(self, features: torch.Tensor, black: torch.Tensor, video_db_nr: torch.Tensor, present: Optional[torch.Tensor] = None):
        if not torch.is_tensor(features) or features.dtype != torch.float32 or features.dim() != 2:
            raise ValueError("features must be a float32 tensor [F, D]")
        F, D = features.shape
        if F < 1 or D < 4 or D % 4:
            raise ValueError(f"the bank needs at least one frame and a width that is a positive multiple of 4, got {tuple(features.shape)}")
        if not torch.is_tensor(black) or black.dtype != torch.float32 or tuple(black.shape) != (D,):
            raise ValueError(f"black must be a float32 tensor [{D}]")
        if not torch.is_tensor(video_db_nr) or video_db_nr.dtype != torch.int32 or tuple(video_db_nr.shape) != (F,):
            raise ValueError(f"video_db_nr must be an int32 tensor [{F}]")
        if present is not None and (not torch.is_tensor(present) or present.dtype not in (torch.bool, torch.uint8)
                                    or tuple(present.shape) != (F,)):
            raise ValueError(f"present must be None or a bool / uint8 tensor [{F}]")
        for name, t in (("black", black), ("video_db_nr", video_db_nr), ("present", present)):
            if t is not None and t.device != features.device:
                raise ValueError(f"{name} is on {t.device}, the features on {features.device}")
        for name, t in (("features", features), ("black", black), ("video_db_nr", video_db_nr), ("present", present)):
            if t is not None and not t.is_contiguous():
                raise ValueError(f"{name} must be contiguous")
        self.features, self.black, self.video_db_nr, self.present = features, black, video_db_nr, present

    def __len__(self) -> int:
        return self.features.shape[0]

    @property
    def device(self) -> torch.device:
        return self.features.device

    @property
    def dim(self) -> int:
        return self.features.shape[1]

    def to(self, device) -> "FeatureBank":
        return FeatureBank(self.features.to(device), self.black.to(device), self.video_db_nr.to(device),
                           None if self.present is None else self.present.to(device))


class FeatureClipAssembler(nn.Module):
    """The token tensor of ``index`` int64 [B] out of a ``FeatureBank``: ``clip_len`` feature rows per sample, ``dilation`` frames
    apart, ending at the labelled frame ``index[b]`` (the module docstring states the rule; a black slot is ``bank.black``).

    ``source_table(bank, index)`` -> int64 [B, T]: the bank row of every slot, -1 for a black one.  Plain torch, any device.
    ``tokens(bank, index, lead=None, pos=None)`` -> fp32 [B, n_lead + T, D]: ``cat(lead, rows) + pos[:n_lead + T]``, what
    ``TFormer.forward`` builds in front of its stack (vformer.py:279-287).  ``lead`` is [n_lead, D] or the parameter shape
    [1, n_lead, D] (TFormer's ``cls_token`` [1, 1, D]), ``pos`` is [P, D] or [1, P, D] with P >= n_lead + T; None leaves the
    part out.  Each element is at most one fp32 add.

    ``backend="torch"`` (default) is the definition, on any device: the table of source rows, ``index_select``, ``where`` against
    ``black``, ``cat`` with ``lead``, ``+ pos``.  ``backend="hip"``: one launch of csrc/feature_bank.hip, the bank must be on the
    GPU (no CPU fallback), under ``no_grad``; ``index`` is read on the device.  Both give the same bits."""

    def __init__(self, clip_len: int = 16, dilation: int = 3, backend: str = "torch"):
        super().__init__()
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        for name, v in (("clip_len", clip_len), ("dilation", dilation)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an integer of at least 1, got {v!r}")
        self.clip_len, self.dilation, self.backend = clip_len, dilation, backend

    def _check(self, bank: FeatureBank, index: torch.Tensor, table_only: bool = False) -> None:
        if not isinstance(bank, FeatureBank):
            raise ValueError(f"bank must be a FeatureBank, got {type(bank).__name__}")
        if not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1 or index.numel() < 1:
            raise ValueError("index must be an int64 tensor [B] with B >= 1")
        if index.device != bank.device:
            raise ValueError(f"index is on {index.device}, the bank on {bank.device}")
        if self.backend == "hip" and not table_only and not bank.features.is_cuda:
            raise RuntimeError("FeatureClipAssembler (HIP) needs its bank on the MI355X; there is no CPU fallback - "
                               "use backend='torch' on the host")

    def source_table(self, bank: FeatureBank, index: torch.Tensor) -> torch.Tensor:
        self._check(bank, index, table_only=True)
        return _source_table(bank.video_db_nr, bank.present, index, self.clip_len, self.dilation)

    def _rows2d(self, name: str, t: Optional[torch.Tensor], bank: FeatureBank, at_least: int) -> Optional[torch.Tensor]:
        """``lead`` / ``pos`` as [rows, D]: [rows, D] itself or the parameter shape [1, rows, D]"""
        if t is None:
            return None
        D = bank.dim
        if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() not in (2, 3) or t.shape[-1] != D or \
                (t.dim() == 3 and t.shape[0] != 1):
            raise ValueError(f"{name} must be a float32 tensor [rows, {D}] or [1, rows, {D}]")
        if t.device != bank.device:
            raise ValueError(f"{name} is on {t.device}, the bank on {bank.device}")
        t = t.detach().reshape(-1, D)
        if t.shape[0] < at_least:
            raise ValueError(f"{name} has {t.shape[0]} rows, the tokens need {at_least}")
        return t

    def tokens(self, bank: FeatureBank, index: torch.Tensor, lead: Optional[torch.Tensor] = None,
               pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        self._check(bank, index)
        T = self.clip_len
        lead = self._rows2d("lead", lead, bank, 1)
        n_lead = 0 if lead is None else lead.shape[0]
        pos = self._rows2d("pos", pos, bank, n_lead + T)
        if pos is not None:
            pos = pos[:n_lead + T]
        if self.backend == "hip":
            with torch.no_grad():
                return ops.feature_clip_tokens(bank.features, bank.black, bank.video_db_nr, bank.present, index.contiguous(), T,
                                               self.dilation, None if lead is None else lead.contiguous(),
                                               None if pos is None else pos.contiguous())
        table = _source_table(bank.video_db_nr, bank.present, index, T, self.dilation)
        B = table.shape[0]
        rows = bank.features.index_select(0, table.clamp(min=0).view(-1)).view(B, T, bank.dim)
        x = torch.where((table < 0).view(B, T, 1), bank.black, rows)
        if lead is not None:
            x = torch.cat([lead.expand(B, n_lead, bank.dim), x], dim=1)
        return x + pos if pos is not None else x
