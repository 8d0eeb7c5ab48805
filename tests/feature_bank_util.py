"""Shared by the feature-bank tests: a numpy restatement of avf_feature_clip_tokens / FeatureClipAssembler.tokens on
``frames_util.reference_table`` - row pick, then cat, then one fp32 add -, its mutations (each breaks one clause of the rule and
must be told apart from it by the test inputs), the test banks and the case grid of the GPU kernel."""
import numpy as np
import torch

from frames_util import VIDEOS, boundary_indices, holes, reference_table, video_numbers

F_BANK = sum(VIDEOS)                                                            # 40 frames: videos of 7, 1, 20 and 12
MISSING = (3, 7, 8, 20, 27, 39)                                                 # absent frames, the one-frame video among them
INDEX = boundary_indices() + [13, 14, 30, F_BANK + 100]                         # both sides of every boundary, -1, F, F + 100
MUTATIONS = ("dilation_off_by_one", "last_slot_not_label", "present_ignored", "video_of_neighbour", "pos_shifted_by_n_lead")

# (D, T, d, B, n_lead, pos, present, pad): a dozen combinations that cover every value of every axis -
# D 4 / 260 / 512, T 1 / 3 / 16, d 1 / 3 / 5, B 1 / 7 / 65, n_lead 0 / 1, pos and present there / null, ldf = D and D + 8
GRID = ((512, 16, 3, 65, 1, True, True, 0),
        (512, 16, 3, 7, 1, True, True, 8),
        (512, 16, 1, 65, 1, True, False, 0),
        (260, 3, 5, 7, 1, True, True, 8),
        (260, 16, 1, 65, 0, False, True, 0),
        (260, 3, 1, 7, 0, True, False, 8),
        (4, 1, 1, 1, 0, False, False, 0),
        (4, 3, 3, 7, 1, False, True, 8),
        (4, 16, 5, 65, 0, True, True, 8),
        (512, 1, 5, 1, 1, True, True, 0),
        (260, 1, 3, 1, 1, False, False, 8),
        (512, 3, 5, 65, 0, False, True, 8),
        (1536, 3, 1, 7, 1, True, True, 8))                                      # wider than one pass of a workgroup: the column loop's
                                                                                # second and third trip (tformer's TFormer is 1536 wide)


def grid_id(case):
    D, T, d, B, n_lead, pos, present, pad = case
    return f"D{D}-T{T}-d{d}-B{B}-lead{n_lead}-pos{int(pos)}-present{int(present)}-pad{pad}"


def reference_tokens(feat, black, video_db_nr, present, index, T, d, lead=None, pos=None, mutate=None):
    """fp32 [B, n_lead + T, D].  ``lead`` [n_lead, D] or None, ``pos`` [>= n_lead + T, D] or None.  ``mutate``: one of MUTATIONS"""
    index = np.asarray(index, dtype=np.int64)
    if mutate == "dilation_off_by_one":
        table = reference_table(video_db_nr, present, index, T, d + 1)
    elif mutate == "last_slot_not_label":                                       # the clip ends one dilation early
        table = reference_table(video_db_nr, present, index - d, T, d)
    elif mutate == "present_ignored":
        table = reference_table(video_db_nr, None, index, T, d)
    elif mutate == "video_of_neighbour":                                        # each slot is checked against the slot after it
        table = _table_checked_against_neighbour(video_db_nr, present, index, T, d)
    else:
        table = reference_table(video_db_nr, present, index, T, d)
    B, D = len(index), black.shape[0]                                           # feat may carry padding columns behind D
    rows = np.empty((B, T, D), dtype=np.float32)
    for b in range(B):
        for t in range(T):
            rows[b, t] = black if table[b, t] < 0 else feat[table[b, t], :D]
    n_lead = 0 if lead is None else lead.shape[0]
    x = rows if n_lead == 0 else np.concatenate([np.broadcast_to(lead[None], (B, n_lead, D)), rows], axis=1)
    if pos is None:
        return np.ascontiguousarray(x, dtype=np.float32)
    p = pos[n_lead:2 * n_lead + T] if mutate == "pos_shifted_by_n_lead" else pos[:n_lead + T]
    assert p.shape[0] == n_lead + T, "pos is too short"
    return (x + p[None]).astype(np.float32)


def _table_checked_against_neighbour(video_db_nr, present, index, T, d):
    F = len(video_db_nr)
    table = np.full((len(index), T), -1, dtype=np.int64)
    for b, idx in enumerate(int(i) for i in index):
        if idx < 0 or idx >= F:
            continue
        for t in range(T):
            a = idx - d * (T - 1 - t)
            nb = min(a + d, idx)                                                # the next slot's frame (the label for the last)
            if a < 0 or a >= F or video_db_nr[a] != video_db_nr[nb]:
                continue
            if present is not None and not present[a]:
                continue
            table[b, t] = a
    return table


def slot_kinds(video_db_nr, present, index, T, d):
    """which kinds of slot the inputs hold - the vacuity guard of the tests reads it off ``reference_table``"""
    F = len(video_db_nr)
    table = reference_table(video_db_nr, present, index, T, d)
    kinds = dict(real=False, before_start=False, other_video=False, absent=False, label_outside=False, all_real=False)
    for b, idx in enumerate(int(i) for i in index):
        if idx < 0 or idx >= F:
            kinds["label_outside"] = True
            assert (table[b] == -1).all()
            continue
        kinds["all_real"] |= bool((table[b] >= 0).all())
        for t in range(T):
            a = idx - d * (T - 1 - t)
            if table[b, t] >= 0:
                kinds["real"] = True
            elif a < 0:
                kinds["before_start"] = True
            elif video_db_nr[a] != video_db_nr[idx]:
                kinds["other_video"] = True
            elif present is not None and not present[a]:
                kinds["absent"] = True
    return kinds


def make_case(case, seed=0):
    """the numpy inputs of one GRID case: feat [F, D + pad] with NaN in the padding columns and in the rows of absent frames"""
    D, T, d, B, n_lead, with_pos, with_present, pad = case
    g = np.random.default_rng(1000 + seed)
    F = F_BANK
    feat = g.standard_normal((F, D + pad)).astype(np.float32)
    feat[:, D:] = np.nan
    present = holes(F, MISSING) if with_present else None
    if with_present:
        feat[list(MISSING)] = np.nan
    black = g.standard_normal(D).astype(np.float32)
    nr = video_numbers()
    pool = INDEX
    index = np.array([pool[i % len(pool)] for i in range(B)] if B > 1 else [30], dtype=np.int64)
    if B >= len(pool):                                                          # beyond the pool: every label once more, shuffled
        index[len(pool):] = g.integers(-2, F + 2, size=B - len(pool))
    lead = g.standard_normal((n_lead, D)).astype(np.float32) if n_lead else None
    pos = g.standard_normal((n_lead + T + 2, D)).astype(np.float32) if with_pos else None   # two rows more than needed, as a longer table
    return dict(feat=feat, black=black, video_db_nr=nr, present=present, index=index, lead=lead, pos=pos, D=D, T=T, d=d, B=B,
                n_lead=n_lead, ldf=D + pad)


def torch_bank(c, device="cpu"):
    """the FeatureBank of a case (contiguous [F, D]: the module level has no row stride) and its index / lead / pos tensors"""
    import avformer_amd as A
    D = c["D"]
    feat = torch.from_numpy(np.ascontiguousarray(c["feat"][:, :D]))
    bank = A.frames.FeatureBank(feat, torch.from_numpy(c["black"]), torch.from_numpy(c["video_db_nr"]),
                                None if c["present"] is None else torch.from_numpy(c["present"])).to(device)
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)
    return bank, t(c["index"]), t(c["lead"]), t(c["pos"])


def want_tokens(c, mutate=None):
    return reference_tokens(c["feat"], c["black"], c["video_db_nr"], c["present"], c["index"], c["T"], c["d"], c["lead"], c["pos"],
                            mutate=mutate)
