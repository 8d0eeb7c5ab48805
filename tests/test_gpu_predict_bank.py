"""-m gpu: whole-video inference at the module level - ``FrozenVideoModel.frame_features`` / ``forward_bank``, the avformer's
``x['clip_bank']`` and ``predict.predict_bank`` - against the path they replace: ``ClipAssembler.normalized`` then
``FrozenVideoModel.forward`` on the assembled clips.

The inputs: 60 random 112 x 112 x 3 frames over two videos (35 + 25), frame 19 absent, T = 16, d = 3, and five labels -
0 (first frame of video 0: 15 slots before the bank), 34 (the label with the most real slots: a clip spans 46 frames and the
longer video has 35, so NO label has all 16 real; this one has 11, and its slot 34 - 15 is the absent frame), 36 (second frame of
video 1: every other slot lies across the boundary), 20 (one frame after the hole) and -1 (an all-black clip).  The direct path
sends 80 frames through the backbone, the bank path 60 + 1.

Bounds.  The two paths run the same ops on the same frames; they differ in the batch the S-Former sees (80 frames of clips against
60 + 1 of the bank), for which the conv plan may pick another tile, and then a frame's sums are rounded in another order.  With R
the direct path on ``backend="torch"`` and e_direct = rel_fro(direct on hip, R) measured here, the bank path on hip is held to
rel_fro(bank, R) <= min(1.5e-2, 3 * e_direct): the project's bf16 output cap and its convention of three
times the measured error of the existing path (tests/golden/lowp_measured.json).  With ``backend="torch"`` on both sides the bound
is the project's parity tolerance on logits, 1e-3.  Measured on an MI355X: DESIGN.md section 9 (FEATBANKSTAT)."""
import pytest
import torch

import backbone_util as bu
from frames_util import holes, video_numbers
from gpu_util import rel_fro

pytestmark = pytest.mark.gpu

CAP = 1.5e-2
T, DIL = 16, 3
VIDEOS2 = (35, 25)
HOLE = 19
LABELS = (0, 34, 36, 20, -1)


@pytest.fixture(scope="module")
def A():
    import avformer_amd as A
    assert A.ops.device_ok()
    return A


def _freeze(m):
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _bound(e_direct):
    return min(CAP, 3.0 * e_direct)


def _frames(F, seed):
    """uint8 [F, 112, 112, 3], random: a colour of its own per frame, a 7 x 7 pattern of 16 x 16 blocks on it, pixel noise on top.
    (Pure pixel noise averages out in the S-Former's pooled features: every frame would give nearly the same row, and a wrong
    gather would go unseen.)"""
    g = torch.Generator().manual_seed(seed)
    colour = torch.randint(0, 192, (F, 1, 1, 3), generator=g)
    coarse = torch.randint(0, 48, (F, 7, 7, 3), generator=g).repeat_interleave(16, dim=1).repeat_interleave(16, dim=2)
    fine = torch.randint(0, 16, (F, 112, 112, 3), generator=g)
    return (colour + coarse + fine).clamp(1, 255).to(torch.uint8)              # no zero byte: no frame is black by accident


@pytest.fixture(scope="module")
def world(A):
    """the shared inputs, and every path's output computed once"""
    torch.manual_seed(77)
    model = _freeze(bu.randomize_batchnorm(A.FrozenVideoModel(), 78).eval()).cuda()
    F = sum(VIDEOS2)
    bank = A.frames.FrameBank(_frames(F, seed=79), torch.from_numpy(video_numbers(VIDEOS2)),
                              torch.from_numpy(holes(F, (HOLE,)))).to("cuda")
    index = torch.tensor(LABELS, device="cuda")
    table = A.frames.ClipAssembler(T, DIL).source_table(bank, index).cpu()
    assert int((table[1] >= 0).sum()) == 11 and HOLE not in table[1].tolist() and 34 - 15 == HOLE      # the hole is one of its slots
    assert table[2].tolist()[-2:] == [-1, 36] and table[0].tolist() == [-1] * 15 + [0] and bool((table[4] == -1).all())
    assert bool((table[3] >= 0).sum() == 7)
    fe_clip = A.clip.ClipFrontEnd(backend="hip").cuda()                                     # [B, 3, T, H, W], what forward takes
    fe_frame = A.clip.ClipFrontEnd(layout="tchw", channels=3, backend="hip").cuda()         # [n, 1, 3, H, W], what s_former takes
    clips = A.frames.ClipAssembler(T, DIL, backend="hip").normalized(bank, index, fe_clip)
    asm_hip, asm_torch = A.frames.FeatureClipAssembler(T, DIL, backend="hip"), A.frames.FeatureClipAssembler(T, DIL)
    w = dict(A=A, model=model, bank=bank, index=index, fe_frame=fe_frame, asm_hip=asm_hip, asm_torch=asm_torch)
    with torch.no_grad():
        model.s_former.set_backend("torch", stem="torch")
        w["direct_torch"] = model(clips)                                                    # R
        w["feat_torch"] = model.frame_features(bank, fe_frame)
        w["bank_torch"] = model.forward_bank(w["feat_torch"], index, asm_torch)
        model.s_former.set_backend("hip", stem="hip")
        w["direct_hip"] = model(clips)
        w["feat_hip"] = model.frame_features(bank, fe_frame)
        w["bank_hip"] = model.forward_bank(w["feat_hip"], index, asm_hip)
        w["bank_hip_off_by_one"] = model.forward_bank(w["feat_hip"], index + 1, asm_hip)   # the neighbouring labels: must be told apart
    torch.cuda.synchronize()
    w["e_direct"] = rel_fro(w["direct_hip"], w["direct_torch"])
    return w


def test_hip_backend_bank_path_within_three_times_the_direct_paths_error(world):
    w = world
    R, e_direct = w["direct_torch"], w["e_direct"]
    e_bank = rel_fro(w["bank_hip"], R)
    print(f"FEATBANKSTAT hip bf16: e_direct {e_direct:.3e}  e_bank {e_bank:.3e}  bound {_bound(e_direct):.3e}  "
          f"bank vs direct on hip {rel_fro(w['bank_hip'], w['direct_hip']):.3e}")
    fb = w["feat_hip"]
    assert tuple(fb.features.shape) == (60, 512) and fb.features.dtype == torch.float32 and tuple(fb.black.shape) == (512,)
    assert fb.video_db_nr is w["bank"].video_db_nr and fb.present is w["bank"].present
    assert tuple(R.shape) == (5, 512) and bool(torch.isfinite(w["bank_hip"]).all()) and float(R.abs().mean()) > 0.05
    # the comparison can fail: the rows of the labels one frame further on lie outside the bound
    e_off = rel_fro(w["bank_hip_off_by_one"], R)
    print(f"FEATBANKSTAT sensitivity: labels + 1 against R {e_off:.3e}  rows of labels 34 / 20 {rel_fro(R[1], R[3]):.3e}  "
          f"of labels 0 / -1 {rel_fro(R[0], R[4]):.3e}")
    assert e_direct > 0.0 and e_off > _bound(e_direct), (e_off, e_direct)
    assert e_bank <= _bound(e_direct), (e_bank, e_direct)


def test_absent_rows_are_never_read(world):
    w = world
    A = w["A"]
    fb = w["feat_hip"]
    feat = fb.features.clone()
    feat[HOLE] = float("nan")
    trapped = A.frames.FeatureBank(feat, fb.black, fb.video_db_nr, fb.present)
    with torch.no_grad():
        for asm in (w["asm_hip"], w["asm_torch"]):
            got = w["model"].forward_bank(trapped, w["index"], asm)
            assert torch.equal(got, w["bank_hip"])


def test_torch_backend_on_both_sides(world):
    w = world
    e = rel_fro(w["bank_torch"], w["direct_torch"])
    print(f"FEATBANKSTAT torch backend both sides: rel_fro(bank, direct) {e:.3e}  bit-equal {torch.equal(w['bank_torch'], w['direct_torch'])}")
    assert e <= 1e-3, e


def test_chunking(world):
    w = world
    with torch.no_grad():
        small = w["model"].frame_features(w["bank"], w["fe_frame"], chunk=7)                # 8 full chunks and one of 4
        got = w["model"].forward_bank(small, w["index"], w["asm_hip"])
    keep = torch.ones(60, dtype=torch.bool)
    keep[HOLE] = False
    same = torch.equal(small.features.cpu()[keep], w["feat_hip"].features.cpu()[keep]) and torch.equal(small.black, w["feat_hip"].black)
    e_feat = rel_fro(small.features.cpu()[keep], w["feat_hip"].features.cpu()[keep])
    e = rel_fro(got, w["bank_hip"])
    print(f"FEATBANKSTAT chunk 7 vs 256: features bit-equal {same} rel_fro {e_feat:.3e}  forward_bank rel_fro {e:.3e}  "
          f"bound {_bound(w['e_direct']):.3e}")
    assert e <= _bound(w["e_direct"]) and e_feat <= _bound(w["e_direct"]), (e, e_feat, w["e_direct"])
    assert rel_fro(got, w["direct_torch"]) <= _bound(w["e_direct"])


def test_refusals(world):
    w = world
    A, model, fb, index = w["A"], w["model"], w["feat_hip"], w["index"]
    with pytest.raises(ValueError, match="clips of 8 frames, t_former takes 16"):
        model.forward_bank(fb, index, A.frames.FeatureClipAssembler(8, DIL, backend="hip"))
    narrow = A.frames.FeatureBank(fb.features[:, :256].contiguous(), fb.black[:256].contiguous(), fb.video_db_nr, fb.present)
    with pytest.raises(ValueError, match="256 wide, t_former takes 512"):
        model.forward_bank(narrow, index, w["asm_hip"])
    for asm in (w["asm_hip"], w["asm_torch"]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_bank(fb.to("cpu"), index.cpu(), asm)
    with pytest.raises(ValueError, match="layout='tchw'"):
        model.frame_features(w["bank"], A.clip.ClipFrontEnd(backend="hip").cuda())


@pytest.fixture(scope="module")
def avformer(A, world):
    """the registry's avformer on the frozen video stream (identity audio backbone: it takes [B, 512] audio features), its
    [B, 21] rows from clips - on both S-Former backends - and from the bank"""
    w = world
    torch.manual_seed(80)
    m = A.build_model("avformer", task="AU", video_backbone="resnet18_frozen")
    bu.randomize_batchnorm(m.video_model, 81)
    m = _freeze(m.cuda().eval())
    audio_table = torch.randn(60, 512, generator=torch.Generator().manual_seed(82)).cuda()

    def audio(i):                                                               # a stub: any label's features, -1 among them
        return audio_table.index_select(0, i.clamp(0, 59))
    index = w["index"]
    fe_clip = A.clip.ClipFrontEnd(backend="hip").cuda()
    fe_frame = A.clip.ClipFrontEnd(layout="tchw", channels=3, backend="hip").cuda()
    clips = A.frames.ClipAssembler(T, DIL, backend="hip").normalized(w["bank"], index, fe_clip)
    video = m.video_model.video_model
    with torch.no_grad():
        video.s_former.set_backend("torch")
        ref = m({'clip': clips, 'audio_features': audio(index)})
        video.s_former.set_backend("hip")
        direct = m({'clip': clips, 'audio_features': audio(index)})
        fb = video.frame_features(w["bank"], fe_frame)
        banked = m({'clip_bank': (fb, index, w["asm_hip"]), 'audio_features': audio(index)})
    return dict(model=m, audio=audio, fb=fb, ref=ref, direct=direct, banked=banked)


def test_whole_model_clip_bank_against_clip(world, avformer):
    a = avformer
    e_direct, e_bank = rel_fro(a["direct"], a["ref"]), rel_fro(a["banked"], a["ref"])
    print(f"FEATBANKSTAT avformer [B, 21]: e_direct {e_direct:.3e}  e_bank {e_bank:.3e}  bound {_bound(e_direct):.3e}  "
          f"bank vs clip on hip {rel_fro(a['banked'], a['direct']):.3e}")
    assert tuple(a["banked"].shape) == (5, 21) and a["banked"].dtype == torch.float32
    assert bool((a["banked"][:, 12:] == 0).all()) and float(a["banked"][:, :12].abs().mean()) > 1e-3
    assert e_bank <= _bound(e_direct), (e_bank, e_direct)


def test_predict_bank_rows_and_decisions(world, avformer):
    w, a = world, avformer
    A, m, fb, asm = w["A"], a["model"], a["fb"], w["asm_hip"]
    out = A.predict_bank(m, fb, asm, batch_size=16, audio=a["audio"])            # 16, 16, 16 and a ragged 12
    assert not m.training
    logits = out["logits"]
    assert logits.is_cuda and tuple(logits.shape) == (60, 21) and logits.dtype == torch.float32
    with torch.no_grad():
        for lo, hi in ((16, 32), (48, 60)):
            idx = torch.arange(lo, hi, device="cuda")
            direct = m({'clip_bank': (fb, idx, asm), 'audio_features': a["audio"](idx)})
            assert torch.equal(logits[lo:hi], direct), (lo, hi)
    ex, au, va = A.EvalMetrics().predictions_torch(logits)
    assert out["au"].dtype == torch.uint8 and out["ex"].dtype == torch.int64 and out["va"].dtype == torch.float32
    assert torch.equal(out["au"], au) and torch.equal(out["ex"], ex) and torch.equal(out["va"], va)
    assert 0 < int(au.sum()) < au.numel()                                        # both decisions occur
    # a subset: the other rows stay zero, the listed ones are those of a direct call on the same batch
    some = torch.tensor([3, 36, 50])
    part = A.predict_bank(m, fb, asm, batch_size=64, audio=a["audio"], indices=some)
    rest = torch.ones(60, dtype=torch.bool)
    rest[some] = False
    with torch.no_grad():
        direct = m({'clip_bank': (fb, some.cuda(), asm), 'audio_features': a["audio"](some.cuda())})
    assert torch.equal(part["logits"][some.cuda()], direct)
    for k in ("logits", "au", "ex", "va"):
        assert not bool(part[k].cpu()[rest].any()), k
    with pytest.raises(ValueError, match=r"indices must lie in \[0, 60\)"):
        A.predict_bank(m, fb, asm, audio=a["audio"], indices=torch.tensor([0, 60]))
