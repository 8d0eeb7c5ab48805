"""Clip AutoAugment: the reference's ``ImageNetPolicy`` on uint8 clips [B, T, H, W, C], bit for bit.

The reference's training transform (dataloader/aff2compdataset.py:72-74) starts with ``ImageNetPolicy()``
(dataloader/autoaugment.py, dataloader/ops.py): per clip one of 25 sub-policies ``(p1, op1, idx1, p2, op2, idx2)`` is drawn,
and every frame is turned into a PIL image to which op1 is applied with probability p1 and then op2 with probability p2
(autoaugment.py:104-112).  Here the random draws and everything that needs Python double arithmetic are resolved on the host
into a small integer *plan*, and the pixels are transformed by a backend that needs nothing but that plan:

  * ``draw_plan`` replays ``random`` draws in the reference's order; ``make_plan`` builds a plan from explicit choices.
  * ``ClipAutoAugment(backend="numpy")`` (default) is a numpy restatement of the ten PIL operations the 25 rows name, equal
    byte for byte to Pillow (tests/golden/g19_autoaugment.npz is generated from the reference itself).
  * ``ClipAutoAugment(backend="hip")`` is ONE launch of csrc/augment.hip, one workgroup per frame, equal byte for byte to the
    numpy backend.

shearY, translateX / translateY and brightness are in the reference's tables, but no sub-policy reaches them: not built.

A plan is int32 [B, T, 2, 8]: per frame two slots ``[op_code, p0 .. p6]``, applied in order, slot 2 to the result of slot 1.

  op_code 0  nothing
   1 posterize     p0 = the byte mask ~(2**(8 - bits) - 1)
   2 solarize      p0 = ceil(threshold), 0..256 (``v < threshold`` for an integer v)
   3 invert        4 autocontrast        5 equalize
   6 color         7 contrast            8 sharpness      p0 = the bit pattern of float32(1 + magnitude * sign)
   9 rotate        p0..p5 = the 16.16 fixed-point coefficients a0..a5 of Pillow's nearest-neighbour affine loop for THIS frame
                   size, p6 = H << 16 | W (a plan is made for one frame size; the numpy backend and a host-side plan given to
                   the hip backend are checked against the clip)
  10 shearX        p0, p1 = the low and high word of the fp64 bit pattern of magnitude * sign
"""
from __future__ import annotations

import math
import random
import struct
from typing import Optional, Sequence, Tuple

import numpy as np
import torch
from torch import nn

from . import ops
from .clip import ClipFrontEnd

BACKENDS = ("numpy", "hip")
OPS = ("posterize", "solarize", "invert", "autocontrast", "equalize", "color", "contrast", "sharpness", "rotate", "shearX")
OP_CODES = {name: i + 1 for i, name in enumerate(OPS)}
SIGNED_OPS = ("rotate", "shearX", "color", "contrast", "sharpness")      # ops.py: the ones that call random.choice([-1, 1])
SLOT_WORDS = 8
FILL = 128                                                               # fillcolor=(128, 128, 128), autoaugment.py:18
MAX_SIDE = 32767                                                         # H and W of a rotate slot share one word

# autoaugment.py:19-49
IMAGENET_POLICY = (
    (0.4, "posterize", 8, 0.6, "rotate", 9), (0.6, "solarize", 5, 0.6, "autocontrast", 5),
    (0.8, "equalize", 8, 0.6, "equalize", 3), (0.6, "posterize", 7, 0.6, "posterize", 6),
    (0.4, "equalize", 7, 0.2, "solarize", 4),
    (0.4, "equalize", 4, 0.8, "rotate", 8), (0.6, "solarize", 3, 0.6, "equalize", 7),
    (0.8, "posterize", 5, 1.0, "equalize", 2), (0.2, "rotate", 3, 0.6, "solarize", 8),
    (0.6, "equalize", 8, 0.4, "posterize", 6),
    (0.8, "rotate", 8, 0.4, "color", 0), (0.4, "rotate", 9, 0.6, "equalize", 2),
    (0.0, "equalize", 7, 0.8, "equalize", 8), (0.6, "invert", 4, 1.0, "equalize", 8),
    (0.6, "color", 4, 1.0, "contrast", 8),
    (0.8, "rotate", 8, 1.0, "color", 2), (0.8, "color", 8, 0.8, "solarize", 7),
    (0.4, "sharpness", 7, 0.6, "invert", 8), (0.6, "shearX", 5, 1.0, "equalize", 9),
    (0.4, "color", 0, 0.6, "equalize", 3),
    (0.4, "equalize", 7, 0.2, "solarize", 4), (0.6, "solarize", 5, 0.6, "autocontrast", 5),
    (0.6, "invert", 4, 1.0, "equalize", 8), (0.6, "color", 4, 1.0, "contrast", 8),
    (0.8, "equalize", 8, 0.6, "equalize", 3),
)

# autoaugment.py:63-78 (np.int is gone from numpy: astype(int))
RANGES = {
    "shearX": np.linspace(0, 0.3, 10),
    "rotate": np.linspace(0, 30, 10),
    "color": np.linspace(0.0, 0.9, 10),
    "posterize": np.round(np.linspace(8, 4, 10), 0).astype(int),
    "solarize": np.linspace(256, 0, 10),
    "contrast": np.linspace(0.0, 0.9, 10),
    "sharpness": np.linspace(0.0, 0.9, 10),
    "autocontrast": [0] * 10,
    "equalize": [0] * 10,
    "invert": [0] * 10,
}


def _i32(u: int) -> int:
    """the 32-bit word u as a signed int32 value"""
    u &= 0xFFFFFFFF
    return u - (1 << 32) if u >= (1 << 31) else u


def _fix(v: float) -> int:
    return math.floor(v * 65536.0 + 0.5)


def rotate_coefficients(angle: float, H: int, W: int) -> Tuple[int, ...]:
    """a0..a5 of Pillow's Image.rotate(angle) (nearest, about the centre, no expand) in its 16.16 fixed-point form: source
    column (a2 + a1 * y + a0 * x) >> 16, source row (a5 + a4 * y + a3 * x) >> 16"""
    a = -math.radians(angle % 360.0)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]), _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def encode_slot(op: Optional[str], magnitude_index: int = 0, sign: int = 1, size: Tuple[int, int] = (112, 112)) -> list:
    """one slot ``[op_code, p0 .. p6]``; ``op`` None is the empty slot"""
    slot = [0] * SLOT_WORDS
    if op is None:
        return slot
    if op not in OP_CODES:
        raise ValueError(f"unknown operation {op!r}; the policy's operations are {OPS}")
    if isinstance(magnitude_index, bool) or not isinstance(magnitude_index, (int, np.integer)) or not 0 <= magnitude_index <= 9:
        raise ValueError(f"{op}: the magnitude index must be an integer in 0..9, got {magnitude_index!r}")
    if sign not in (-1, 1):
        raise ValueError(f"{op}: the sign must be -1 or 1, got {sign!r}")
    H, W = (int(s) for s in size)
    if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"size must be (H, W) with both in 1..{MAX_SIDE}, got {size!r}")
    mag = RANGES[op][magnitude_index]
    slot[0] = OP_CODES[op]
    if op == "posterize":
        slot[1] = ~(2 ** (8 - int(mag)) - 1) & 0xFF
    elif op == "solarize":
        slot[1] = int(math.ceil(float(mag)))
    elif op in ("color", "contrast", "sharpness"):
        slot[1] = _i32(struct.unpack("<I", struct.pack("<f", 1 + mag * sign))[0])
    elif op == "rotate":
        slot[1:7] = [_i32(v) for v in rotate_coefficients(mag * sign, H, W)]
        slot[7] = H << 16 | W
    elif op == "shearX":
        bits = struct.unpack("<Q", struct.pack("<d", mag * sign))[0]
        slot[1], slot[2] = _i32(bits), _i32(bits >> 32)
    return slot


def draw_plan(B: int, T: int, rng: random.Random, flip_p: Optional[float] = None, size: Tuple[int, int] = (112, 112)):
    """The plan of B clips of T frames of ``size`` (H, W) under ImageNetPolicy, int32 [B, T, 2, 8] on the CPU, consuming ``rng``
    exactly as the reference consumes ``random``: per clip ``randint(0, 24)``; per frame ``random() < p1``, the sign of op1
    where it fires and is signed, ``random() < p2`` and its sign.  With ``flip_p`` also bool [B], one ``random() < flip_p`` after
    each clip's frames - where RandomClipFlip sits behind the policy in aug_clip_transform (aff2compdataset.py:72-74)."""
    if B < 1 or T < 1:
        raise ValueError(f"B and T must be at least 1, got {B} and {T}")
    plan = np.zeros((B, T, 2, SLOT_WORDS), dtype=np.int64)
    flips = np.zeros(B, dtype=bool)
    for b in range(B):
        p1, op1, i1, p2, op2, i2 = IMAGENET_POLICY[rng.randint(0, len(IMAGENET_POLICY) - 1)]
        for t in range(T):
            for s, (p, op, idx) in enumerate(((p1, op1, i1), (p2, op2, i2))):
                if rng.random() < p:
                    sign = rng.choice([-1, 1]) if op in SIGNED_OPS else 1
                    plan[b, t, s] = encode_slot(op, idx, sign, size)
        if flip_p is not None:
            flips[b] = rng.random() < flip_p
    plan = torch.from_numpy(plan.astype(np.int32))
    return plan if flip_p is None else (plan, torch.from_numpy(flips))


def make_plan(choices: Sequence, size: Tuple[int, int] = (112, 112)) -> torch.Tensor:
    """A plan from explicit choices: ``choices[b][t]`` is a pair of slots, each None or ``(op, magnitude_index, sign)`` (``(op,)``
    and ``(op, magnitude_index)`` default to index 0 and sign 1).  int32 [B, T, 2, 8] on the CPU."""
    B = len(choices)
    if B < 1 or any(len(c) != len(choices[0]) or len(c) < 1 for c in choices):
        raise ValueError("choices must be a non-empty [B][T] nesting with the same T for every clip")
    plan = np.zeros((B, len(choices[0]), 2, SLOT_WORDS), dtype=np.int64)
    for b, clip in enumerate(choices):
        for t, slots in enumerate(clip):
            if len(slots) != 2:
                raise ValueError(f"choices[{b}][{t}] must hold two slots, got {slots!r}")
            for s, slot in enumerate(slots):
                plan[b, t, s] = encode_slot(None) if slot is None else encode_slot(*slot, size=size)
    return torch.from_numpy(plan.astype(np.int32))


# ---- the numpy backend: frame uint8 [H, W, 3] -> uint8 [H, W, 3] --------------------------------------------------------------

def _apply_luts(img: np.ndarray, luts) -> np.ndarray:
    return np.stack([np.asarray(luts[c], dtype=np.uint8)[img[..., c]] for c in range(3)], axis=-1)


def _autocontrast_lut(h: np.ndarray) -> np.ndarray:
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.clip(np.trunc(np.arange(256, dtype=np.float64) * scale + off), 0, 255).astype(np.int64)


def _equalize_lut(h: np.ndarray) -> np.ndarray:
    nz = h[h != 0]
    if len(nz) <= 1:
        return np.arange(256)
    step = (int(h.sum()) - int(nz[-1])) // 255
    if step == 0:
        return np.arange(256)
    n = step // 2 + np.concatenate(([0], np.cumsum(h[:-1])))
    return np.minimum(255, n // step)


def _grey(img: np.ndarray) -> np.ndarray:
    v = img.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def _blend(deg: np.ndarray, img: np.ndarray, alpha: np.float32) -> np.ndarray:
    """Image.blend(deg, img, alpha) on bytes: fp32, the product and the sum rounded one after the other"""
    deg = np.broadcast_to(deg, img.shape)
    if alpha == 0:
        return deg.copy()
    if alpha == 1:
        return img.copy()
    t = deg.astype(np.float32) + alpha * (img.astype(np.int32) - deg.astype(np.int32)).astype(np.float32)
    assert t.dtype == np.float32
    if 0 <= alpha <= 1:
        return np.trunc(t).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def _smooth(img: np.ndarray) -> np.ndarray:
    """ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13 on the interior, the border copied"""
    out = img.copy()
    H, W = img.shape[:2]
    if H < 3 or W < 3:
        return out
    v = img.astype(np.int64)
    S = 4 * v[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            S = S + v[dy:H - 2 + dy, dx:W - 2 + dx]
    out[1:-1, 1:-1] = ((2 * S + 13) // 26).astype(np.uint8)
    return out


def _rotate(img: np.ndarray, a) -> np.ndarray:
    H, W = img.shape[:2]
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    # Pillow steps C ints: 32-bit wrap-around, arithmetic shift
    xs = (a[2] + a[1] * y + a[0] * x).astype(np.int32) >> 16
    ys = (a[5] + a[4] * y + a[3] * x).astype(np.int32) >> 16
    ok = (xs >= 0) & (xs < W) & (ys >= 0) & (ys < H)
    out = np.full_like(img, FILL)
    out[ok] = img[ys[ok], xs[ok]]
    return out


def _shear_x(img: np.ndarray, m: np.float64) -> np.ndarray:
    H, W = img.shape[:2]
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xin = (x + 0.5) + m * (y + 0.5)
    inside = ~((xin < 0.0) | (xin >= W))
    xin = xin - 0.5
    xf = np.floor(xin)
    d = (xin - xf)[..., None]
    xi = xf.astype(np.int64)
    rows = np.arange(H)[:, None]
    v1, v2, v3, v4 = (img[rows, np.clip(xi - 1 + k, 0, W - 1)].astype(np.float64) for k in range(4))
    p1, p2, p3, p4 = v2, -v1 + v3, 2 * (v1 - v2) + v3 - v4, -v1 + v2 - v3 + v4
    v = p1 + d * (p2 + d * (p3 + d * p4))
    v = np.where(v <= 0.0, 0, np.where(v >= 255.0, 255, np.trunc(v))).astype(np.uint8)
    return np.where(inside[..., None], v, np.uint8(FILL)).astype(np.uint8)


def _f32_of(word: int) -> np.float32:
    return np.frombuffer(struct.pack("<I", int(word) & 0xFFFFFFFF), dtype=np.float32)[0]


def apply_slot(img: np.ndarray, slot) -> np.ndarray:
    """one slot of a plan on one frame, uint8 [H, W, 3]; an op code outside 1..10 does nothing"""
    op, p = int(slot[0]), [int(v) for v in slot[1:]]
    H, W = img.shape[:2]
    if op == 1:
        return img & np.uint8(p[0] & 0xFF)
    if op == 2:
        return np.where(img.astype(np.int64) < p[0], img, 255 - img).astype(np.uint8)
    if op == 3:
        return 255 - img
    if op in (4, 5):
        make = _autocontrast_lut if op == 4 else _equalize_lut
        return _apply_luts(img, [make(np.bincount(img[..., c].ravel(), minlength=256)) for c in range(3)])
    if op == 6:
        return _blend(_grey(img)[..., None], img, _f32_of(p[0]))
    if op == 7:
        L = _grey(img).astype(np.int64)
        mean = int(float(L.sum()) / L.size + 0.5)
        return _blend(np.uint8(mean), img, _f32_of(p[0]))
    if op == 8:
        return _blend(_smooth(img), img, _f32_of(p[0]))
    if op == 9:
        if p[6] != (H << 16 | W):
            raise ValueError(f"the plan's rotate slot was made for frames of {p[6] >> 16} x {p[6] & 0xFFFF}, the clip's are {H} x {W}")
        return _rotate(img, p[:6])
    if op == 10:
        m = np.frombuffer(struct.pack("<II", p[0] & 0xFFFFFFFF, p[1] & 0xFFFFFFFF), dtype=np.float64)[0]
        return _shear_x(img, m)
    return img


def _check_rotate_size(plan: torch.Tensor, H: int, W: int) -> None:
    rot = plan[..., 0] == OP_CODES["rotate"]
    if bool((rot & (plan[..., 7] != (H << 16 | W))).any()):
        raise ValueError(f"the plan holds a rotate slot made for another frame size than the clip's {H} x {W}")


class ClipAutoAugment(nn.Module):
    """``forward(clip_u8 [B, T, H, W, C] or [T, H, W, C], plan int32 [B, T, 2, 8] or [T, 2, 8])`` -> uint8 of the clip's shape:
    each frame through the two slots of its plan (``draw_plan`` / ``make_plan``).  C is 3 or 4; channels 0..2 are transformed,
    channel 3 passes through (``clip[t, :, :, 0:3]``, autoaugment.py:106-111).  The output feeds ``ClipFrontEnd`` unchanged.
    ``normalized(clip_u8, plan, front_end, flip=None)`` -> ``front_end(forward(clip_u8, plan), flip)``: the reference's training
    transform (policy, mirror, NumpyToTensor, Normalize; aff2compdataset.py:72-74) in the front end's layout, dtype and channel
    slice.

    ``backend="numpy"`` (default): the numpy restatement, clip and plan on the CPU.  ``backend="hip"``: one launch of
    csrc/augment.hip; the clip must be on the GPU (no CPU fallback), under ``no_grad``; the plan is on the clip's device, or on
    the CPU - then it is checked against the frame size and uploaded.  ``inplace=True`` (hip) writes into the clip.  Frames
    above ``ops.clip_autoaugment_max_pixels()`` pixels are an error.  ``normalized`` is one launch too (no augmented uint8 clip
    is written; ``inplace`` does not apply to it) and takes the front end's table, whatever the front end's own backend."""

    def __init__(self, backend: str = "numpy", inplace: bool = False):
        super().__init__()
        if backend not in BACKENDS:
            raise ValueError(f"backend must be one of {BACKENDS}, got {backend!r}")
        self.backend, self.inplace = backend, bool(inplace)

    def _checked(self, clip_u8: torch.Tensor, plan: torch.Tensor):
        """the argument checks of ``forward`` and ``normalized``: the batched clip, its plan (hip: on the clip's device) and whether
        the batch axis was added"""
        if clip_u8.dtype != torch.uint8:
            raise ValueError(f"the clip must be uint8, got {clip_u8.dtype}")
        if clip_u8.dim() not in (4, 5):
            raise ValueError(f"clip: expected 4 or 5 dimensions, got {tuple(clip_u8.shape)}")
        squeeze = clip_u8.dim() == 4
        clip = clip_u8[None] if squeeze else clip_u8
        B, T, H, W, C = clip.shape
        if C not in (3, 4):
            raise ValueError(f"the clip has {C} channels; the policy transforms RGB (C = 3) or RGB + mask (C = 4)")
        if not torch.is_tensor(plan) or plan.dtype != torch.int32:
            raise ValueError("plan must be an int32 tensor (draw_plan / make_plan)")
        if squeeze and plan.dim() == 3:
            plan = plan[None]
        if tuple(plan.shape) != (B, T, 2, SLOT_WORDS):
            raise ValueError(f"plan must be [{B}, {T}, 2, {SLOT_WORDS}] for this clip, got {tuple(plan.shape)}")
        if self.backend == "hip":
            if not clip.is_cuda:
                raise RuntimeError("ClipAutoAugment (HIP) needs its input on the MI355X; there is no CPU fallback - "
                                   "use backend='numpy' on the host")
            if not plan.is_cuda:
                _check_rotate_size(plan, H, W)
                plan = plan.to(clip.device, non_blocking=True)
            elif plan.device != clip.device:
                raise ValueError(f"plan is on {plan.device}, the clip on {clip.device}")
        return clip, plan, squeeze

    def forward(self, clip_u8: torch.Tensor, plan: torch.Tensor) -> torch.Tensor:
        clip, plan, squeeze = self._checked(clip_u8, plan)
        B, T, H, W, C = clip.shape
        if self.backend == "hip":
            with torch.no_grad():
                src = clip.contiguous()
                if self.inplace and src.data_ptr() != clip.data_ptr():
                    raise ValueError("inplace=True needs a contiguous clip")
                out = ops.clip_autoaugment(src, plan.contiguous(), out=src if self.inplace else None)
        else:
            if clip.is_cuda or plan.is_cuda:
                raise ValueError("backend='numpy' runs on the host: clip and plan must be CPU tensors")
            _check_rotate_size(plan, H, W)
            x, pl = clip.numpy().copy(), plan.numpy()
            for b in range(B):
                for t in range(T):
                    img = x[b, t, :, :, 0:3]
                    for s in range(2):
                        img = apply_slot(img, pl[b, t, s])
                    x[b, t, :, :, 0:3] = img
            out = torch.from_numpy(x)
        return out[0] if squeeze else out

    def normalized(self, clip_u8: torch.Tensor, plan: torch.Tensor, front_end: ClipFrontEnd,
                   flip: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not isinstance(front_end, ClipFrontEnd):
            raise ValueError(f"front_end must be a ClipFrontEnd, got {type(front_end).__name__}")
        clip, plan, squeeze = self._checked(clip_u8, plan)
        C = clip.shape[-1]
        if C != front_end.in_channels:
            raise ValueError(f"front_end: the clip has {C} channels, mean / std have {front_end.in_channels}")
        flip = front_end._flags(flip, clip.shape[0], clip.device)
        if self.backend != "hip":
            return front_end(self(clip_u8, plan), flip)
        if front_end.lut.device != clip.device:
            raise ValueError(f"front_end is on {front_end.lut.device}, the clip on {clip.device}")
        with torch.no_grad():
            out = ops.clip_autoaugment_normalize(clip.contiguous(), plan.contiguous(), front_end.lut, front_end.channels, flip,
                                                 front_end.layout, front_end.out_dtype)
        return out[0] if squeeze else out
