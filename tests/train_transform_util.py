"""Shared by the training-transform tests: the reference's ``aug_clip_transform`` (dataloader/aff2compdataset.py:72-74, applied at
163-164) chained by hand out of the numpy restatements the other tests already hold to the reference -
``augment.apply_slot`` per frame (pinned to Pillow by tests/golden/g19_autoaugment.npz), then ``clip_util.reference_transform``
with the flip (RandomClipFlip, NumpyToTensor, Normalize).  Nothing of the code under test is called."""
import numpy as np
import torch

import avformer_amd as A
from clip_util import STATS, reference_transform


def augmented_clips(clips_u8: np.ndarray, plan: torch.Tensor) -> np.ndarray:
    """uint8 [B, T, H, W, C] -> the same, channels 0..2 of every frame through the two slots of its plan"""
    x, pl = clips_u8.copy(), plan.numpy()
    for b in range(x.shape[0]):
        for t in range(x.shape[1]):
            img = x[b, t, :, :, 0:3]
            for s in range(2):
                img = A.augment.apply_slot(img, pl[b, t, s])
            x[b, t, :, :, 0:3] = img
    return x


def reference_chain(clips_u8: np.ndarray, plan: torch.Tensor, flip=None, k=None, layout="cthw", dtype=torch.float32,
                    augmented=None) -> torch.Tensor:
    """the planes of the training transform; ``augmented``: the result of ``augmented_clips`` where a caller shares it"""
    x = augmented_clips(clips_u8, plan) if augmented is None else augmented
    mean, std = STATS[x.shape[-1]]
    fl = None if flip is None else np.asarray(flip)
    return reference_transform(x, mean, std, fl, k, layout, bf16=dtype == torch.bfloat16)


def front_end(C, k, layout="cthw", dtype=torch.float32, backend="torch"):
    mean, std = STATS[C]
    return A.clip.ClipFrontEnd(mean, std, channels=k, layout=layout, out_dtype=dtype, backend=backend)
