#!/usr/bin/env python3
"""Generate tests/golden/g19_autoaugment.npz from the REFERENCE implementation (dataloader/ops.py and dataloader/autoaugment.py,
loaded unmodified by file path - dataloader/__init__.py is avoided, it needs cv2; ``np.int`` is shimmed, numpy dropped it), on
whatever Pillow is installed (its version is stored).  Run in the build container only:

    python tests/golden/make_golden_autoaugment.py

G19, data only - inputs, seeds and the reference's outputs:

  part 1  every (operation, magnitude index, sign) the 25 sub-policies of ImageNetPolicy can produce, applied by the reference's
          own SubPolicy(1.0, op, idx, 0.0, "invert", 0) - so the magnitude comes from ITS range table - to three one-frame clips:

    frame0 [20, 28, 3] noise      frame1 [16, 24, 3] values 90..139      frame2 [12, 16, 3] noise with channel 1 flat (77)
    op_name [N] str, op_index [N], op_sign [N] (1 for the unsigned operations), op_seed [N]: random.seed(op_seed) in front of the
    call makes random.choice([-1, 1]) return op_sign;  op_out0 / op_out1 / op_out2 [N, H, W, 3] the outputs

  part 2  ImageNetPolicy()(clip, False) on ONE 4-frame clip policy_clip [4, 20, 28, 3] under 25 random.seed values, one per
          sub-policy index (of the seeds below 400 that draw the index, the one under which most of the 8 coin flips fire):

    policy_seed [25], policy_index [25] (0..24, each once), policy_out [25, 4, 20, 28, 3]

  pillow_version str
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np

sys.dont_write_bytecode = True
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden import REF  # noqa: E402  (where the reference lies: see make_golden.py)
SIGNED = ("rotate", "shearX", "color", "contrast", "sharpness")


def load_reference():
    if not hasattr(np, "int"):
        np.int = int                                             # autoaugment.py:70
    pkg = types.ModuleType("refdl")
    pkg.__path__ = [os.path.join(REF, "dataloader")]
    sys.modules["refdl"] = pkg
    mods = {}
    for name in ("ops", "autoaugment"):
        spec = importlib.util.spec_from_file_location("refdl." + name, os.path.join(REF, "dataloader", name + ".py"))
        mods[name] = importlib.util.module_from_spec(spec)
        sys.modules["refdl." + name] = mods[name]
        spec.loader.exec_module(mods[name])
    return mods["autoaugment"]


def seed_for_sign(sign):
    """the first seed under which SubPolicy's draws - random() for p1, then the operation's choice([-1, 1]) - give this sign"""
    for s in range(1000):
        r = random.Random(s)
        r.random()
        if r.choice([-1, 1]) == sign:
            return s
    raise AssertionError


def fired(aa, seed, T):
    """how many of the 2 * T coin flips of the policy fire under this seed, and the sub-policy index it draws"""
    r = random.Random(seed)
    idx = r.randint(0, 24)
    rows = rows_of(aa)
    p1, op1, _, p2, op2, _ = rows[idx]
    n = 0
    for _ in range(T):
        for p, op in ((p1, op1), (p2, op2)):
            if r.random() < p:
                n += 1
                if op in SIGNED:
                    r.choice([-1, 1])
    return n, idx


_ROWS = []


def rows_of(aa):
    """(p1, op1, idx1, p2, op2, idx2) of the 25 SubPolicy calls, recorded from ImageNetPolicy.__init__ itself"""
    if not _ROWS:
        real = aa.SubPolicy

        class Recorder(real):
            def __init__(self, p1, o1, i1, p2, o2, i2, fillcolor=(128, 128, 128)):
                _ROWS.append((p1, o1, i1, p2, o2, i2))
                super().__init__(p1, o1, i1, p2, o2, i2, fillcolor)
        aa.SubPolicy = Recorder
        try:
            aa.ImageNetPolicy()
        finally:
            aa.SubPolicy = real
    return _ROWS


def main():
    import PIL
    aa = load_reference()
    rows = rows_of(aa)
    assert len(rows) == 25
    g = np.random.RandomState(19)
    frame0 = g.randint(0, 256, (20, 28, 3)).astype(np.uint8)
    frame1 = g.randint(90, 140, (16, 24, 3)).astype(np.uint8)
    frame2 = g.randint(0, 256, (12, 16, 3)).astype(np.uint8)
    frame2[..., 1] = 77
    frames = (frame0, frame1, frame2)

    cases = []
    for p1, o1, i1, p2, o2, i2 in rows:
        for op, idx in ((o1, i1), (o2, i2)):
            for sign in ((-1, 1) if op in SIGNED else (1,)):
                if (op, idx, sign) not in cases:
                    cases.append((op, idx, sign))
    cases.sort()
    outs, seeds = ([], [], []), []
    for op, idx, sign in cases:
        seed = seed_for_sign(sign)
        seeds.append(seed)
        sub = aa.SubPolicy(1.0, op, idx, 0.0, "invert", 0)
        for k, f in enumerate(frames):
            random.seed(seed)
            outs[k].append(sub(f[None].copy())[0])

    T = 4
    policy_clip = g.randint(0, 256, (T, 20, 28, 3)).astype(np.uint8)
    best = {}
    for s in range(400):
        n, idx = fired(aa, s, T)
        if idx not in best or n > best[idx][0]:
            best[idx] = (n, s)
    assert sorted(best) == list(range(25))
    policy = aa.ImageNetPolicy()
    p_seed, p_out = [], []
    for idx in range(25):
        seed = best[idx][1]
        random.seed(seed)
        p_out.append(policy(policy_clip.copy(), False))
        p_seed.append(seed)

    path = os.path.join(OUT, "g19_autoaugment.npz")
    np.savez_compressed(
        path, frame0=frame0, frame1=frame1, frame2=frame2, op_name=np.array([c[0] for c in cases]),
        op_index=np.array([c[1] for c in cases], dtype=np.int64), op_sign=np.array([c[2] for c in cases], dtype=np.int64),
        op_seed=np.array(seeds, dtype=np.int64), op_out0=np.stack(outs[0]), op_out1=np.stack(outs[1]), op_out2=np.stack(outs[2]),
        policy_clip=policy_clip, policy_seed=np.array(p_seed, dtype=np.int64), policy_index=np.arange(25, dtype=np.int64),
        policy_out=np.stack(p_out), pillow_version=np.array(PIL.__version__))
    print(f"wrote {path}  ({os.path.getsize(path) / 1024:.1f} KiB), {len(cases)} operation cases, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
