"""MI355X-native forward path of the Swin-UNet IR/visible image-fusion network.

Public surface = the reference's module API (a013 `MyModel`, a012 `SelfAndCrossBlockPair`,
a001 `WindowAttention` and the inner modules needed for state_dict compatibility), implemented
by hand-written HIP kernels behind a C-ABI (`include/swinfuse.h`, `libswinfuse.so`).
"""
from .config import CONFIGS, FusionConfig, load_recipe_into, synthetic_pair  # noqa: F401
from .data import PairLoader, ResidentPairs, sample_crop_params  # noqa: F401
from .imaging import JpegBatch, PngBatch, decode_jpeg, decode_png, encode_jpeg, encode_png, jpeg_info, png_info  # noqa: F401
from .inference import test_fusion  # noqa: F401
from .loss import MyLoss  # noqa: F401
from .metrics import (COMPARATIVE_DEFAULTS, COMPARATIVE_NAMES, FEATURE_DEFAULTS, FEATURE_NAMES, FIDELITY_DEFAULTS, FIDELITY_NAMES,  # noqa: F401
                      METRIC_NAMES, PERCEPTION_DEFAULTS, PERCEPTION_NAMES, STRUCTURE_DEFAULTS, STRUCTURE_NAMES, FusionMetrics,
                      fusion_comparative, fusion_feature, fusion_fidelity, fusion_metrics, fusion_perception, fusion_structure)
from .modules import (AddAndLayerNormWithOtherModule, AutoPathMLP, AutoPathWinAtt, BasicBlock, MyModel,  # noqa: F401
                      MyPadding, NormalAndShiftWinsBlockPair, PatchMergingAndLinearLayer, SelfAndCrossBlockPair,
                      StateRecorder, WindowAttention, get_encoder_or_decoder_block)

from .optim import FusedAdam  # noqa: F401
from .parallel import DataParallelStep, TorchCollective  # noqa: F401
from .training import fractional_epoch, load_training_state, save_training_state, train_step, validate  # noqa: F401

__version__ = "0.1.0"
