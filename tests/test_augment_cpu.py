"""CPU (no GPU needed): augment.py - the plan (draw order, encoding, argument errors) and the numpy backend of ClipAutoAugment,
held byte for byte to tests/golden/g19_autoaugment.npz (the reference's own ops.py / autoaugment.py on Pillow, see
tests/golden/make_golden_autoaugment.py) and, where Pillow is installed, to Pillow's public calls in a live sweep."""
import math
import os
import random
import struct

import numpy as np
import pytest
import torch

import avformer_amd as A
from conftest import GOLDEN

AUG = A.augment
SIZES = ((1, 1), (2, 3), (3, 3), (5, 7), (16, 16), (3, 40), (40, 3), (37, 53), (40, 56), (112, 112), (160, 160))


@pytest.fixture(scope="module")
def g19():
    return np.load(os.path.join(GOLDEN, "g19_autoaugment.npz"))


def _run(frames: np.ndarray, plan: torch.Tensor) -> np.ndarray:
    return AUG.ClipAutoAugment()(torch.from_numpy(frames), plan).numpy()


def test_fixture_is_small_and_complete(g19):
    assert os.path.getsize(os.path.join(GOLDEN, "g19_autoaugment.npz")) < 400 * 1024
    produced = set()
    for p1, o1, i1, p2, o2, i2 in AUG.IMAGENET_POLICY:
        for op, idx in ((o1, i1), (o2, i2)):
            produced |= {(op, idx, s) for s in ((-1, 1) if op in AUG.SIGNED_OPS else (1,))}
    stored = set(zip(g19["op_name"].tolist(), g19["op_index"].tolist(), g19["op_sign"].tolist()))
    assert stored == produced
    assert sorted(g19["policy_index"].tolist()) == list(range(25)) and str(g19["pillow_version"])


def test_every_operation_equals_the_reference(g19):
    for k in range(3):
        frame = g19[f"frame{k}"]
        H, W = frame.shape[:2]
        for i, (op, idx, sign) in enumerate(zip(g19["op_name"].tolist(), g19["op_index"].tolist(), g19["op_sign"].tolist())):
            plan = AUG.make_plan([[((op, idx, sign), None)]], size=(H, W))
            assert np.array_equal(_run(frame[None, None], plan)[0, 0], g19[f"op_out{k}"][i]), (k, op, idx, sign)


def test_the_whole_policy_equals_the_reference(g19):
    clip = g19["policy_clip"]
    T, H, W = clip.shape[:3]
    seen = set()
    for seed, index, want in zip(g19["policy_seed"].tolist(), g19["policy_index"].tolist(), g19["policy_out"]):
        rng = random.Random(seed)
        plan = AUG.draw_plan(1, T, rng, size=(H, W))
        assert random.Random(seed).randint(0, 24) == index
        seen.add(index)
        assert np.array_equal(_run(clip[None], plan)[0], want), (seed, index)
        assert np.array_equal(_run(clip, plan[0]), want)                         # a 4-D clip with a [T, 2, 8] plan
    assert len(seen) == 25


def test_policy_tables():
    assert len(AUG.IMAGENET_POLICY) == 25 and len(AUG.OPS) == 10
    assert {r[1] for r in AUG.IMAGENET_POLICY} | {r[4] for r in AUG.IMAGENET_POLICY} == set(AUG.OPS)
    assert AUG.RANGES["posterize"].tolist() == [8, 8, 7, 7, 6, 6, 5, 5, 4, 4]
    assert AUG.RANGES["solarize"][0] == 256 and AUG.RANGES["rotate"][9] == 30 and abs(AUG.RANGES["shearX"][9] - 0.3) < 1e-15
    assert set(AUG.SIGNED_OPS) == {"rotate", "shearX", "color", "contrast", "sharpness"}


def _replay(B, T, seed, flip_p):
    """the reference's draw order, restated: -> (policy index, [[fired1, sign1, fired2, sign2] per frame], flip) per clip"""
    r = random.Random(seed)
    clips = []
    for _ in range(B):
        idx = r.randint(0, 24)
        p1, o1, _, p2, o2, _ = AUG.IMAGENET_POLICY[idx]
        frames = []
        for _ in range(T):
            row = []
            for p, op in ((p1, o1), (p2, o2)):
                hit = r.random() < p
                row += [hit, r.choice([-1, 1]) if hit and op in AUG.SIGNED_OPS else 1]
            frames.append(row)
        clips.append((idx, frames, None if flip_p is None else r.random() < flip_p))
    return clips, r.random()


@pytest.mark.parametrize("flip_p", [None, 0.5])
def test_draw_plan_consumes_the_draws_in_the_reference_order(flip_p):
    B, T = 40, 3
    rng = random.Random(77)
    got = AUG.draw_plan(B, T, rng, flip_p, size=(9, 11))
    clips, next_draw = _replay(B, T, 77, flip_p)
    assert rng.random() == next_draw                                             # exactly as many draws, no more
    plan, flips = (got, None) if flip_p is None else got
    assert plan.dtype == torch.int32 and tuple(plan.shape) == (B, T, 2, 8) and not plan.is_cuda
    if flip_p is not None:
        assert flips.dtype == torch.bool and flips.tolist() == [c[2] for c in clips] and 0 < int(flips.sum()) < B
        other = AUG.draw_plan(B, T, random.Random(77), None, size=(9, 11))         # one draw more per clip: the streams part
        assert torch.equal(other[0], plan[0]) and not torch.equal(other, plan)
    for b, (idx, frames, _) in enumerate(clips):
        row = AUG.IMAGENET_POLICY[idx]
        for t, (hit1, sign1, hit2, sign2) in enumerate(frames):
            for s, (hit, sign, op, mi) in enumerate(((hit1, sign1, row[1], row[2]), (hit2, sign2, row[4], row[5]))):
                want = AUG.encode_slot(op, mi, sign, (9, 11)) if hit else [0] * 8
                assert plan[b, t, s].tolist() == want, (b, t, s)


def test_plan_encoding():
    enc = AUG.encode_slot
    assert enc(None) == [0] * 8
    assert enc("posterize", 8) == [1, 0xF0, 0, 0, 0, 0, 0, 0] and enc("posterize", 0)[1] == 0xFF and enc("posterize", 5)[1] == 0xFC
    assert enc("solarize", 0)[:2] == [2, 256] and enc("solarize", 9)[:2] == [2, 0]
    assert enc("solarize", 5)[1] == math.ceil(256 - 5 * 256 / 9) == 114 and enc("solarize", 4)[1] == 143
    assert enc("invert", 4) == [3] + [0] * 7 and enc("autocontrast", 5)[0] == 4 and enc("equalize", 9) == [5] + [0] * 7
    for code, op in ((6, "color"), (7, "contrast"), (8, "sharpness")):
        for idx in (0, 4, 8):
            for sign in (-1, 1):
                slot = enc(op, idx, sign)
                want = np.float32(1 + np.linspace(0.0, 0.9, 10)[idx] * sign)
                assert slot[0] == code and struct.pack("<i", slot[1]) == want.tobytes() and slot[2:] == [0] * 6
    assert struct.unpack("<f", struct.pack("<i", enc("color", 0, -1)[1]))[0] == 1.0
    m = np.linspace(0, 0.3, 10)[5] * -1
    slot = enc("shearX", 5, -1)
    assert slot[0] == 10 and struct.pack("<ii", slot[1], slot[2]) == struct.pack("<d", m) and slot[3:] == [0] * 5
    # rotate by 0 degrees is the identity map in fixed point; the size travels with the slot
    assert enc("rotate", 0, 1, (5, 7)) == [9, 65536, 0, 32768, 0, 65536, 32768, 5 << 16 | 7]
    slot = enc("rotate", 9, 1, (20, 28))
    a = -math.radians(30.0)
    c, s = round(math.cos(a), 15), round(math.sin(a), 15)
    assert slot[1] == slot[5] == math.floor(c * 65536 + 0.5) and slot[2] == -slot[4] == math.floor(s * 65536 + 0.5)
    assert slot[3] == math.floor((c * -14.0 + s * -10.0 + 14.0 + c * 0.5 + s * 0.5) * 65536 + 0.5) and slot[7] == 20 << 16 | 28
    assert enc("rotate", 9, -1, (20, 28))[2] == -slot[2]
    plan = AUG.make_plan([[(("invert",), None), (None, ("color", 4, -1))]] * 2, size=(4, 4))
    assert tuple(plan.shape) == (2, 2, 2, 8) and plan.dtype == torch.int32
    assert plan[1, 0].tolist() == [enc("invert"), [0] * 8] and plan[0, 1].tolist() == [[0] * 8, enc("color", 4, -1)]


def test_argument_errors():
    with pytest.raises(ValueError, match="unknown operation"):
        AUG.make_plan([[(("brightness", 3, 1), None)]])
    with pytest.raises(ValueError, match="unknown operation"):
        AUG.encode_slot("shearY", 1, 1)
    for bad in (-1, 10, 2.0, True):
        with pytest.raises(ValueError, match="magnitude index"):
            AUG.encode_slot("rotate", bad, 1)
    for bad in (0, 2, -2, 0.5):
        with pytest.raises(ValueError, match="sign"):
            AUG.encode_slot("color", 3, bad)
    with pytest.raises(ValueError, match="size"):
        AUG.encode_slot("rotate", 3, 1, (0, 5))
    with pytest.raises(ValueError, match="two slots"):
        AUG.make_plan([[(None,)]])
    with pytest.raises(ValueError, match="same T"):
        AUG.make_plan([[(None, None)], [(None, None), (None, None)]])
    with pytest.raises(ValueError):
        AUG.draw_plan(0, 4, random.Random(0))
    with pytest.raises(ValueError, match="backend"):
        AUG.ClipAutoAugment(backend="torch")
    aug = AUG.ClipAutoAugment()
    clip = torch.zeros(2, 3, 5, 7, 3, dtype=torch.uint8)
    plan = AUG.make_plan([[(None, None)] * 3] * 2, size=(5, 7))
    assert torch.equal(aug(clip, plan), clip)
    with pytest.raises(ValueError, match="uint8"):
        aug(clip.float(), plan)
    with pytest.raises(ValueError, match="dimensions"):
        aug(clip[0, 0], plan)
    with pytest.raises(ValueError, match="channels"):
        aug(clip[..., :2], plan)
    with pytest.raises(ValueError, match="int32"):
        aug(clip, plan.long())
    with pytest.raises(ValueError, match=r"\[2, 3, 2, 8\]"):
        aug(clip, plan[:1])
    with pytest.raises(ValueError, match="frame size"):
        aug(clip, AUG.make_plan([[(("rotate", 3, 1), None)] * 3] * 2, size=(7, 5)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AUG.ClipAutoAugment(backend="hip")(clip, plan)


def test_channel_3_passes_through_and_codes_outside_the_table_do_nothing():
    g = torch.Generator().manual_seed(5)
    clip = torch.randint(0, 256, (2, 2, 9, 11, 4), dtype=torch.uint8, generator=g)
    choices = [[(("rotate", 8, 1), ("equalize",)), (("shearX", 5, -1), ("invert",))],
               [(("sharpness", 7, 1), ("color", 4, -1)), (("solarize", 5), ("contrast", 8, 1))]]
    plan = AUG.make_plan(choices, size=(9, 11))
    aug = AUG.ClipAutoAugment()
    out4 = aug(clip, plan)
    out3 = aug(clip[..., :3].contiguous(), plan)
    assert torch.equal(out4[..., 3], clip[..., 3]) and torch.equal(out4[..., :3], out3) and not torch.equal(out3, clip[..., :3])
    odd = plan.clone()
    odd[..., 0] = torch.tensor([11, -1])
    assert torch.equal(aug(clip, odd), clip)


# ---- live against Pillow's public calls -----------------------------------------------------------------------------------------

def _live_frames(H, W):
    g = np.random.RandomState(1000 * H + W)
    ramp = (np.add.outer(3 * np.arange(H), 2 * np.arange(W))[..., None] + np.array([0, 40, 90])) % 256
    flat1 = g.randint(0, 256, (H, W, 3))
    flat1[..., 2] = 200
    return {"noise": g.randint(0, 256, (H, W, 3)).astype(np.uint8), "ramp": ramp.astype(np.uint8),
            "narrow": g.randint(100, 120, (H, W, 3)).astype(np.uint8), "flat": np.full((H, W, 3), 91, dtype=np.uint8),
            "flat channel": flat1.astype(np.uint8)}


def _pillow(op, img, mag, sign):
    """the reference's ops.py calls, spelled with Pillow's public interface"""
    from PIL import Image, ImageEnhance, ImageOps
    x = Image.fromarray(img)
    if op == "posterize":
        return ImageOps.posterize(x, int(mag))
    if op == "solarize":
        return ImageOps.solarize(x, mag)
    if op == "invert":
        return ImageOps.invert(x)
    if op == "autocontrast":
        return ImageOps.autocontrast(x)
    if op == "equalize":
        return ImageOps.equalize(x)
    if op in ("color", "contrast", "sharpness"):
        enhancer = {"color": ImageEnhance.Color, "contrast": ImageEnhance.Contrast, "sharpness": ImageEnhance.Sharpness}[op]
        return enhancer(x).enhance(1 + mag * sign)
    if op == "rotate":
        rot = x.convert("RGBA").rotate(mag * sign)
        return Image.composite(rot, Image.new("RGBA", rot.size, (128,) * 4), rot).convert(x.mode)
    return x.transform(x.size, Image.AFFINE, (1, mag * sign, 0, 0, 1, 0), Image.BICUBIC, fillcolor=(128, 128, 128))


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_live_sweep_against_pillow(size):
    pytest.importorskip("PIL")
    H, W = size
    frames = _live_frames(H, W)
    names = list(frames) if H * W <= 40 * 56 else ["noise", "ramp"]              # the large sizes: the two textured frames
    stack = np.stack([frames[n] for n in names])[None]                           # one clip, a frame per kind
    for op in AUG.OPS:
        unsigned = op not in AUG.SIGNED_OPS
        for idx in range(10) if op in ("posterize", "solarize") or not unsigned else (0,):
            for sign in (1,) if unsigned else (-1, 1):
                plan = AUG.make_plan([[((op, idx, sign), None)] * len(names)], size=size)
                got = _run(stack, plan)[0]
                for k, n in enumerate(names):
                    want = np.array(_pillow(op, frames[n], AUG.RANGES[op][idx], sign))
                    assert np.array_equal(got[k], want), (op, idx, sign, n)
