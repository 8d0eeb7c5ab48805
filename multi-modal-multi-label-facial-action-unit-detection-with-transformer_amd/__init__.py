"""MI355X-native implementation of the aural-visual transformer hot path of
ColinWine/Multi-modal-Multi-label-Facial-Action-Unit-Detection-with-Transformer.

The compute lives in ``lib/libavformer_hip.so`` (hand-written HIP for gfx950, C ABI in
``include/avformer_hip.h``); this package is the host-side mirror of the reference's
``Transformer`` / head / loss / model-registry surface.
"""
from . import _build, _cabi, _lib, audio, audio_bank, augment, backbone, checkpoint, clip, dp, frames, graphs, metrics, ops, optim, predict, vggface2  # noqa: F401
from ._lib import get_f32_arithmetic, set_f32_arithmetic  # noqa: F401
from .backbone import FrozenAudioModel, FrozenBasicBlock, FrozenResFormer, FrozenVideoModel  # noqa: F401
from .vggface2 import FrozenBottleneck, FrozenVGGFace2, VGGFormer  # noqa: F401
from .heads import AU_former, ResFormerTokens, TFormer, VA_former, former_AU_head, tformer_AU_head  # noqa: F401
from .loss import AULoss, CCCLoss, CrossEntropyEX, DiceAULoss, FocalLoss_Ori, MultiTaskLoss  # noqa: F401
from .metrics import AccF1Metric, CCCMetric, EvalMetrics, MultiLabelAccF1, evaluate  # noqa: F401
from .predict import predict_bank, write_predictions  # noqa: F401
from .models import (MODEL_REGISTRY, AudioFormer, SyntheticAVFormer, TwoStreamAuralVisualFormer,  # noqa: F401
                     VisualFormer, build_model)
from .transformer import Transformer  # noqa: F401

__all__ = ["Transformer", "AU_former", "VA_former", "tformer_AU_head", "former_AU_head", "TFormer", "AULoss", "CCCLoss", "CrossEntropyEX",
           "DiceAULoss", "FocalLoss_Ori", "MultiTaskLoss", "AccF1Metric", "CCCMetric", "EvalMetrics", "MultiLabelAccF1", "evaluate",
           "ResFormerTokens", "TwoStreamAuralVisualFormer", "SyntheticAVFormer", "AudioFormer", "VisualFormer", "MODEL_REGISTRY",
           "build_model", "FrozenAudioModel", "FrozenBasicBlock", "FrozenResFormer", "FrozenVideoModel", "FrozenBottleneck", "FrozenVGGFace2", "VGGFormer", "ops", "optim", "predict_bank", "write_predictions", "set_f32_arithmetic", "get_f32_arithmetic"]
