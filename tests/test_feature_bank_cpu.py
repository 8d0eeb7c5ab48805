"""CPU (no GPU needed): ``frames.FeatureBank`` / ``FeatureClipAssembler(backend="torch")`` - the definition the HIP kernel of
csrc/feature_bank.hip is held to - against the numpy restatement of tests/feature_bank_util.py, bit for bit, over the grid the GPU
test runs; the restatement's mutations are refused; argument validation; ``predict.write_predictions``."""
import numpy as np
import pytest
import torch

import avformer_amd as A
from feature_bank_util import GRID, MUTATIONS, grid_id, make_case, slot_kinds, torch_bank, want_tokens

FR = A.frames
FLAGSHIP = GRID[0]                                                              # D 512, T 16, d 3, B 65, cls row, pos, holes


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("case", GRID, ids=grid_id)
def test_torch_backend_is_the_restatement_bit_for_bit(case):
    c = make_case(case)
    bank, index, lead, pos = torch_bank(c)
    got = FR.FeatureClipAssembler(c["T"], c["d"]).tokens(bank, index, lead, pos)
    want = torch.from_numpy(want_tokens(c))
    assert got.dtype == torch.float32 and tuple(got.shape) == (c["B"], c["n_lead"] + c["T"], c["D"])
    assert bool(torch.isfinite(got).all())                                      # no absent row was used
    assert torch.equal(_bits(got), _bits(want))
    # the parameter shapes TFormer holds: [1, n_lead, D] and [1, P, D]
    got3 = FR.FeatureClipAssembler(c["T"], c["d"]).tokens(bank, index, None if lead is None else lead[None],
                                                          None if pos is None else pos[None])
    assert torch.equal(_bits(got3), _bits(want))


def test_inputs_hold_every_kind_of_slot():
    """the vacuity guard: read off frames_util.reference_table"""
    union = {}
    for case in GRID:
        D, T, d, B, n_lead, with_pos, with_present, pad = case
        c = make_case(case)
        kinds = slot_kinds(c["video_db_nr"], c["present"], c["index"], T, d)
        assert kinds["real"], case
        if B >= 7 and T >= 3:
            assert kinds["before_start"] and kinds["other_video"] and kinds["label_outside"], (case, kinds)
            if with_present:
                assert kinds["absent"], (case, kinds)
        if B == 65 and not with_present and d * (T - 1) < 20:                   # the longest video has 20 frames
            assert kinds["all_real"], (case, kinds)
        union = {k: union.get(k, False) or v for k, v in kinds.items()}
    assert all(union.values()), union
    # the case the mutations are tried on holds every kind a clip of 46 frames can have (no video is that long)
    c = make_case(FLAGSHIP)
    kinds = slot_kinds(c["video_db_nr"], c["present"], c["index"], c["T"], c["d"])
    assert all(v for k, v in kinds.items() if k != "all_real"), kinds


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_mutated_restatement_is_refused(mutation):
    c = make_case(FLAGSHIP)
    bank, index, lead, pos = torch_bank(c)
    got = FR.FeatureClipAssembler(c["T"], c["d"]).tokens(bank, index, lead, pos)
    wrong = torch.from_numpy(want_tokens(c, mutate=mutation))
    assert wrong.shape == got.shape
    assert not torch.equal(_bits(got), _bits(wrong)), mutation


def test_source_table_is_the_clip_assemblers():
    """one copy of the rule: both assemblers give the table of frames_util.reference_table"""
    from frames_util import reference_table
    c = make_case(FLAGSHIP)
    bank, index, _, _ = torch_bank(c)
    frames = FR.FrameBank(torch.zeros(len(bank), 1, 1, 1, dtype=torch.uint8), bank.video_db_nr, bank.present)
    want = torch.from_numpy(reference_table(c["video_db_nr"], c["present"], c["index"], c["T"], c["d"]))
    assert torch.equal(FR.FeatureClipAssembler(c["T"], c["d"]).source_table(bank, index), want)
    assert torch.equal(FR.ClipAssembler(c["T"], c["d"]).source_table(frames, index), want)


def test_feature_bank_validation():
    F, D = 6, 8
    feat, black, nr = torch.zeros(F, D), torch.zeros(D), torch.zeros(F, dtype=torch.int32)
    bank = FR.FeatureBank(feat, black, nr, torch.ones(F, dtype=torch.bool))
    assert len(bank) == F and bank.device == feat.device and bank.dim == D
    moved = bank.to("cpu")
    assert isinstance(moved, FR.FeatureBank) and len(moved) == F and moved.present is not None
    for args, word in (((feat.double(), black, nr), "features must be a float32"),
                       ((feat[0], black, nr), "features must be a float32"),
                       ((torch.zeros(F, 6), torch.zeros(6), nr), "multiple of 4"),
                       ((torch.zeros(0, D), black, torch.zeros(0, dtype=torch.int32)), "at least one frame"),
                       ((feat, torch.zeros(D + 4), nr), "black must be"),
                       ((feat, black.double(), nr), "black must be"),
                       ((feat, black, nr.long()), "video_db_nr must be"),
                       ((feat, black, nr[:-1]), "video_db_nr must be"),
                       ((feat, black, nr, torch.ones(F)), "present must be"),
                       ((feat, black, nr, torch.ones(F + 1, dtype=torch.uint8)), "present must be"),
                       ((torch.zeros(F, 2 * D)[:, ::2], black, nr), "features must be contiguous"),
                       ((feat, torch.zeros(2 * D)[::2], nr), "black must be contiguous")):
        with pytest.raises(ValueError, match=word):
            FR.FeatureBank(*args)


def test_assembler_validation():
    F, D, T = 6, 8, 4
    bank = FR.FeatureBank(torch.zeros(F, D), torch.zeros(D), torch.zeros(F, dtype=torch.int32))
    index = torch.tensor([0, 5])
    for kw, word in (({"backend": "cuda"}, "backend must be"), ({"clip_len": 0}, "clip_len must be"), ({"dilation": 0}, "dilation must be"),
                     ({"clip_len": True}, "clip_len must be"), ({"dilation": 2.0}, "dilation must be")):
        with pytest.raises(ValueError, match=word):
            FR.FeatureClipAssembler(**kw)
    asm = FR.FeatureClipAssembler(T, 2)
    frames = FR.FrameBank(torch.zeros(F, 1, 1, 1, dtype=torch.uint8), bank.video_db_nr)
    for args, word in (((frames, index), "bank must be a FeatureBank"),
                       ((bank, index.int()), "index must be an int64"),
                       ((bank, index[:0]), "index must be an int64"),
                       ((bank, index[None]), "index must be an int64"),
                       ((bank, index, torch.zeros(1, D + 4)), "lead must be"),
                       ((bank, index, torch.zeros(2, 1, D)), "lead must be"),
                       ((bank, index, torch.zeros(1, D).double()), "lead must be"),
                       ((bank, index, torch.zeros(1, 1, D), torch.zeros(1, T, D)), "pos has 4 rows, the tokens need 5"),
                       ((bank, index, None, torch.zeros(T - 1, D)), "pos has 3 rows, the tokens need 4")):
        with pytest.raises(ValueError, match=word):
            asm.tokens(*args)
    out = asm.tokens(bank, index, torch.zeros(1, 1, D), torch.zeros(1, T + 3, D))   # a longer positional table: its first rows
    assert tuple(out.shape) == (2, T + 1, D)


def test_hip_backend_on_a_cpu_bank_raises_without_touching_a_library(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(A._lib, "load", boom)
    bank = FR.FeatureBank(torch.zeros(6, 8), torch.zeros(8), torch.zeros(6, dtype=torch.int32))
    asm = FR.FeatureClipAssembler(4, 2, backend="hip")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        asm.tokens(bank, torch.tensor([0, 5]))
    assert tuple(asm.source_table(bank, torch.tensor([0, 5])).shape) == (2, 4)   # the table is plain torch with either backend


def test_model_side_refusals_on_the_cpu():
    """what needs no device: the shape checks of forward_tokens / forward_bank / frame_features come before any launch"""
    torch.manual_seed(0)
    t = A.TFormer(num_patches=4, dim=32, depth=1, heads=2, mlp_dim=64, dim_head=16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        t.forward_tokens(torch.zeros(2, 5, 32))
    m = A.FrozenVideoModel()
    bank = FR.FeatureBank(torch.zeros(6, 512), torch.zeros(512), torch.zeros(6, dtype=torch.int32))
    index = torch.tensor([0, 5])
    with pytest.raises(ValueError, match="clips of 4 frames, t_former takes 16"):
        m.forward_bank(bank, index, FR.FeatureClipAssembler(4, 3))
    narrow = FR.FeatureBank(torch.zeros(6, 256), torch.zeros(256), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match="256 wide, t_former takes 512"):
        m.forward_bank(narrow, index, FR.FeatureClipAssembler(16, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_bank(bank, index, FR.FeatureClipAssembler(16, 3))
    frames = FR.FrameBank(torch.zeros(6, 8, 8, 3, dtype=torch.uint8), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match="layout='tchw'"):
        m.frame_features(frames, A.clip.ClipFrontEnd())
    with pytest.raises(ValueError, match="keeps 1 channels"):
        m.frame_features(frames, A.clip.ClipFrontEnd(channels=1, layout="tchw"))
    with pytest.raises(ValueError, match="chunk must be"):
        m.frame_features(frames, A.clip.ClipFrontEnd(layout="tchw"), chunk=0)
    model = A.build_model("avformer", task="AU")
    with pytest.raises(ValueError, match="audio="):
        A.predict_bank(model, bank, FR.FeatureClipAssembler(16, 3))
    with pytest.raises(ValueError, match="both 'clip' and 'clip_bank'"):
        model({'clip': None, 'clip_bank': None, 'audio_features': None})


# ---- write_predictions --------------------------------------------------------------------------------------------------------
# two videos, interleaved in the bank: video 9 owns frames 0, 1, 4 and video 2 owns frames 2, 3
NR = torch.tensor([9, 9, 2, 2, 9], dtype=torch.int32)
NAMES = {9: "video_nine", 2: "2-30-640x360"}


def _read(path):
    with open(path) as f:
        return f.read()


def test_write_predictions_au(tmp_path):
    au = torch.zeros(5, 12, dtype=torch.uint8)
    au[0, 0] = au[1, 11] = au[2, 5] = au[4, 3] = 1
    au[3] = 1
    paths = A.write_predictions(str(tmp_path / "au"), "AU", NAMES, NR, {"au": au})
    assert [p.split("/")[-1] for p in paths] == ["video_nine.txt", "2-30-640x360.txt"]
    head = "AU1,AU2,AU4,AU6,AU7,AU10,AU12,AU15,AU23,AU24,AU25,AU26\n"         # test_aff2.py:87
    assert _read(paths[0]) == head + "1,0,0,0,0,0,0,0,0,0,0,0\n0,0,0,0,0,0,0,0,0,0,0,1\n0,0,0,1,0,0,0,0,0,0,0,0\n"
    assert _read(paths[1]) == head + "0,0,0,0,0,1,0,0,0,0,0,0\n1,1,1,1,1,1,1,1,1,1,1,1\n"


def test_write_predictions_ex(tmp_path):
    ex = torch.tensor([4, 0, 6, 1, 3])
    paths = A.write_predictions(str(tmp_path), "ex", NAMES, NR, {"ex": ex})
    head = "Neutral,Anger,Disgust,Fear,Happiness,Sadness,Surprise\n"           # test_aff2.py:89
    assert _read(paths[0]) == head + "4\n0\n3\n"
    assert _read(paths[1]) == head + "6\n1\n"


def test_write_predictions_va(tmp_path):
    va = torch.tensor([[0.602, 0.389], [-0.024, 0.279], [-0.0001, 0.0004], [1.0, -1.0], [0.12349, -0.9996]])
    paths = A.write_predictions(str(tmp_path), "VA", ["", "", "two", "", "", "", "", "", "", "nine"], NR, {"va": va})   # names as a sequence
    head = "valence,arousal\n"                                                 # test_aff2.py:88
    assert [p.split("/")[-1] for p in paths] == ["nine.txt", "two.txt"]
    assert _read(paths[0]) == head + "0.602,0.389\n-0.024,0.279\n0.123,-1.000\n"
    assert _read(paths[1]) == head + "-0.000,0.000\n1.000,-1.000\n"


def test_write_predictions_refusals(tmp_path):
    with pytest.raises(ValueError, match="task must be"):
        A.write_predictions(str(tmp_path), "MT", NAMES, NR, {})
    with pytest.raises(ValueError, match="has 4 rows, video_db_nr 5"):
        A.write_predictions(str(tmp_path), "EX", NAMES, NR, {"ex": torch.zeros(4, dtype=torch.int64)})
