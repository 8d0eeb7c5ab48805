"""Whole-video inference, the loop of the reference's test_aff2.py, from banks that stay on the device.

test_aff2.py labels every frame of the validation and test videos (76-77: a sequential sampler over ``np.nonzero(test_ids)``,
batch size 1), keeps the [len(dataset), 21] rows (79, 117) and writes one text file per video (87-115).  Its own comment (82)
says "takes 5+ hours for test and val": neighbouring samples share 15 of their 16 frames, and the S-Former - by far the largest
part of the video stream - runs on every frame of every clip.  Here it runs once per frame
(``FrozenVideoModel.frame_features`` -> ``frames.FeatureBank``), and a batch is ``index [B]`` alone: the token tensor of the
temporal stack comes straight from the feature bank (``frames.FeatureClipAssembler``), the audio features from the waveform
bank (``audio_bank.AudioAssembler``).

    feature_bank = model.video_model.video_model.frame_features(frame_bank, front_end)      # once per data set split
    assembler = frames.FeatureClipAssembler(16, 3, backend="hip")
    out = predict_bank(model, feature_bank, assembler, audio=lambda i: audio_assembler.features(audio_bank, i, mel))
    write_predictions("results/au", "AU", names, feature_bank.video_db_nr, out)

Not here: the frame-count interpolation of postprocess/postprocess.py.
"""
from __future__ import annotations

import os
from typing import Callable, Mapping, Optional, Sequence, Union

import torch

from . import ops
from .metrics import EvalMetrics

# test_aff2.py:87-90, the first line of every file of a task
HEADERS = {"AU": "AU1,AU2,AU4,AU6,AU7,AU10,AU12,AU15,AU23,AU24,AU25,AU26",
           "VA": "valence,arousal",
           "EX": "Neutral,Anger,Disgust,Fear,Happiness,Sadness,Surprise"}
# test_aff2.py:34-44: au_to_str, ex_to_str, va_to_str
ROW_FORMATS = {"AU": ",".join(["{:d}"] * 12), "EX": "{:d}", "VA": "{:.3f},{:.3f}"}


@torch.no_grad()
def predict_bank(model, feature_bank, assembler, batch_size: int = 64, audio: Optional[Callable] = None,
                 indices: Optional[torch.Tensor] = None) -> dict:
    """The rows and decisions of every labelled frame: ``{'logits': fp32 [F, 21], 'au': uint8 [F, 12], 'ex': int64 [F],
    'va': fp32 [F, 2]}``, resident on the bank's device (test_aff2.py:79, 117); a row not listed in ``indices`` stays zero.

    ``model`` takes ``{'clip_bank': (feature_bank, index, assembler)}`` (``TwoStreamAuralVisualFormer``), plus
    ``'audio_features': audio(index)`` when its ``modes`` name them: ``audio`` is a callable ``index -> audio_features``, e.g.
    ``lambda i: audio_assembler.features(audio_bank, i, mel)``.  Batches are consecutive runs of ``batch_size`` entries of
    ``indices`` (int64 [n] in [0, F); default: all of ``range(F)``, test_aff2.py:76).  Inside the loop nothing waits for the
    device.  The decisions are ``EvalMetrics``' rule, one launch over the finished rows.  The model runs in eval mode and is left
    in the mode it came in."""
    F, dev = len(feature_bank), feature_bank.device
    needs_audio = "audio_features" in getattr(model, "modes", ())
    if needs_audio and audio is None:
        raise ValueError("the model's modes name 'audio_features': predict_bank needs audio=, a callable index -> audio_features")
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be an integer of at least 1, got {batch_size!r}")
    if indices is None:
        indices = torch.arange(F, dtype=torch.int64, device=dev)
    else:
        indices = torch.as_tensor(indices)
        if indices.dtype != torch.int64 or indices.dim() != 1:
            raise ValueError("indices must be an int64 tensor [n]")
        if indices.numel() and not bool(((indices >= 0) & (indices < F)).all()):      # before the loop: index_copy_ checks nothing
            raise ValueError(f"indices must lie in [0, {F})")
        indices = indices.to(dev)
    logits = torch.zeros((F, 21), dtype=torch.float32, device=dev)
    was_training = model.training
    model.eval()
    try:
        for i in range(0, indices.numel(), batch_size):
            index = indices[i:i + batch_size]
            x = {'clip_bank': (feature_bank, index, assembler)}
            if audio is not None:
                x['audio_features'] = audio(index)
            logits.index_copy_(0, index, model(x).detach().float())                    # test_aff2.py:117
    finally:
        model.train(was_training)
    au = torch.zeros((F, 12), dtype=torch.uint8, device=dev)
    ex = torch.zeros(F, dtype=torch.int64, device=dev)
    va = torch.zeros((F, 2), dtype=torch.float32, device=dev)
    ops.eval_update(logits, None, None, None, None, EvalMetrics()._cfg(), state=None, pred_au=au, pred_ex=ex, pred_va=va)
    return {'logits': logits, 'au': au, 'ex': ex, 'va': va}


def write_predictions(directory: str, task: str, video_names: Union[Mapping[int, str], Sequence[str]], video_db_nr: torch.Tensor,
                      decisions: Mapping[str, torch.Tensor]) -> list:
    """One text file ``<directory>/<video name>.txt`` per video, as test_aff2.py:100-115 writes them: the task's header line
    (87-90), then one row per frame of the video in frame order - ``au_to_str`` / ``"{:d}"`` / ``"{:.3f},{:.3f}"`` (34-44).
    ``task`` is 'AU', 'EX' or 'VA'; ``video_names[nr]`` names video ``nr`` of ``video_db_nr`` int32 [F] (equal numbers need not be
    neighbours); ``decisions`` is what ``predict_bank`` returns.  One device-to-host copy.  Returns the paths, in the order the
    videos first appear."""
    task = task.upper()
    if task not in HEADERS:
        raise ValueError(f"task must be one of {sorted(HEADERS)}, got {task!r}")
    rows = decisions[task.lower()].detach().cpu()
    nr = video_db_nr.detach().cpu().tolist()
    if rows.shape[0] != len(nr):
        raise ValueError(f"decisions[{task.lower()!r}] has {rows.shape[0]} rows, video_db_nr {len(nr)}")
    rows, fmt = rows.tolist(), ROW_FORMATS[task]
    lines = {}
    for frame, n in enumerate(nr):
        r = rows[frame]
        lines.setdefault(n, []).append(fmt.format(*r) if task != "EX" else fmt.format(r))
    os.makedirs(directory, exist_ok=True)
    paths = []
    for n, body in lines.items():
        path = os.path.join(directory, f"{video_names[n]}.txt")
        with open(path, "w") as f:
            f.write(HEADERS[task] + "\n" + "\n".join(body) + "\n")
        paths.append(path)
    return paths
