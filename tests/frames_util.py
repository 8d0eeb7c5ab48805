"""Shared by the frame-bank tests: an independent numpy restatement of how the reference's data set assembles the clip of a sample,
and the test banks.

The reference's data set class (dataloader/aff2compdataset.py) cannot be imported here - it needs lmdb and cv2 -, so the
assembler's parity is unpinned by a reference fixture; it is held bytewise to this restatement of the cited lines instead:

  clip = np.zeros((clip_len, H, W, C), uint8)                                   (aff2compdataset.py:122-125)  init all frames black
  label_frame = clip_len * dilation                                             (:45)
  _range = range(index - label_frame + dilation,
                 index - label_frame + dilation * (clip_len + 1), dilation)     (:126-127)
  for clip_i, all_i in enumerate(_range):                                       (:128)
      if all_i < 0 or all_i >= len(self) or video_db_nr[all_i] != video_db_nr[index]: continue        (:129-132)
      try: clip[clip_i] = img  except: pass                                     (:142-155)  a failed decode leaves the slot black

``present[all_i] == 0`` stands for the failed decode.  The loop and its three ``continue`` conditions are kept as a loop.  One
point is this project's own definition and not the reference's: an ``index`` outside ``[0, F)`` (where the reference's
``video_db_nr[index]`` raises, or wraps for a small negative index) gives an all-black clip."""
import numpy as np
import torch

VIDEOS = (7, 1, 20, 12)                      # frames per video: a one-frame video, and both sides of every boundary exist
F_SMALL = sum(VIDEOS)                        # 40


def video_numbers(lengths=VIDEOS) -> np.ndarray:
    """int32 [sum(lengths)]: the video of every frame.  The numbers are not sorted and not dense, as in the reference's table"""
    names = (5, 2, 9, 4, 11, 3)
    return np.concatenate([np.full(n, names[i % len(names)] + 10 * (i // len(names)), dtype=np.int32) for i, n in enumerate(lengths)])


def boundary_indices(lengths=VIDEOS):
    """0, F - 1, the first and last frame of every video, -1 and F"""
    F = sum(lengths)
    out, start = [0, F - 1, -1, F], 0
    for n in lengths:
        out += [start, start + n - 1]
        start += n
    return sorted(set(out))


def reference_table(video_db_nr: np.ndarray, present, index, clip_len: int, dilation: int) -> np.ndarray:
    """int64 [B, clip_len]: the bank frame the loop copies into every slot, -1 where it leaves the slot black"""
    F = len(video_db_nr)
    table = np.full((len(index), clip_len), -1, dtype=np.int64)
    label_frame = clip_len * dilation
    for b, idx in enumerate(int(i) for i in index):
        if idx < 0 or idx >= F:                                                 # this project's definition: all black
            continue
        nr = video_db_nr[idx]
        _range = range(idx - label_frame + dilation, idx - label_frame + dilation * (clip_len + 1), dilation)
        for clip_i, all_i in enumerate(_range):
            if all_i < 0 or all_i >= F or video_db_nr[all_i] != nr:
                continue                                                        # leave frame black
            if present is not None and not present[all_i]:
                continue                                                        # loading an image fails: leave that frame black
            table[b, clip_i] = all_i
    return table


def reference_clips(frames: np.ndarray, video_db_nr: np.ndarray, present, index, clip_len: int, dilation: int) -> np.ndarray:
    """uint8 [B, clip_len, H, W, C], sample by sample as ``__getitem__`` builds them"""
    table = reference_table(video_db_nr, present, index, clip_len, dilation)
    clips = np.zeros((len(index), clip_len) + frames.shape[1:], dtype=np.uint8)
    for b in range(table.shape[0]):
        for t in range(clip_len):
            if table[b, t] >= 0:
                clips[b, t] = frames[table[b, t]]
    return clips


def random_frames(F, H, W, C, seed) -> torch.Tensor:
    """uint8 [F, H, W, C] without a zero byte: a black slot cannot be mistaken for a frame"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(1, 256, (F, H, W, C), dtype=torch.uint8, generator=g)


def holes(F, missing) -> np.ndarray:
    """uint8 [F]: 1, and 0 at ``missing``"""
    p = np.ones(F, dtype=np.uint8)
    p[list(missing)] = 0
    return p
