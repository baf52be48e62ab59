"""MI355X-native 2D Gaussian splatting trainer: Python host-side binding of the C ABI.

The product is `lib/libsplat2d_hip.so` (hand-written HIP for gfx950 behind include/splat2d.h).
The package only binds it with ctypes for tests and bench.py; `Trainer` holds the same state the
reference keeps in main()'s locals (/root/reference/main.cpp:272-278, :310-317) and exposes the
three passes under the reference's names.  There is no CPU path here: importing works anywhere,
but every compute call needs the built library and a gfx950 device and raises otherwise.

One module per concern, re-exported here: _abi (constants, structures, the signature table of the C ABI), _runtime (loading the
library, one HIP runtime per process), _handle (what the two handles share), trainer (Trainer), multi (MultiTrainer), coarse
(CoarseTrainer: include/splat2d_coarse.h, with the signatures of its two symbols), backdrop (BackdropTrainer:
include/splat2d_backdrop.h, likewise), weights (WeightedTrainer: include/splat2d_weights.h, likewise); torch_op, torch_backdrop and distributed import torch and are imported by name.

The package name starts with a digit, so import it with
    importlib.import_module("2dgaussiansplatting_amd")
"""
from . import _build
from ._abi import (ABI_SYMBOLS, ABI_VERSION, ADAM_DTYPE, OPTIM_GROUPS, ROWS_ADAM, ROWS_GRADS, ROWS_SPLATS, SEED_SOURCES,
                   SIGNATURES, SPLAT_DTYPE, STATUS_NAMES, STRUCTS, _Config, _LossConfig, _LossTerms, _OptimConfig,
                   _PruneConfig, _RelocateConfig, _SeedConfig, _Stats, _ViewConfig)
from ._abi import (S2D_ABI_VERSION, S2D_BWD_DENSITY_STATS, S2D_BWD_SKIP_OPACITY_GRAD, S2D_CFG_ADAM_FP32, S2D_CFG_COUNT_PAIRS,
                   S2D_CFG_COVERAGE, S2D_CFG_DETERMINISTIC, S2D_CFG_EXACT_EXP, S2D_CFG_FP16_IMAGES, S2D_CFG_GENERIC_BINNING,
                   S2D_CFG_REFERENCE_ORDER, S2D_E_HIP, S2D_E_INVALID, S2D_E_NOMEM, S2D_E_NONFINITE, S2D_E_STATE,
                   S2D_FB_SKIP_IMAGE, S2D_MULTI_REPLICATED, S2D_MULTI_SHARE_GPU, S2D_OK, S2D_ROWS_ADAM, S2D_ROWS_GRADS,
                   S2D_ROWS_SPLATS, S2D_SEED_CALLER, S2D_SEED_ERROR, S2D_SEED_SQUARED, S2D_SEED_TARGET_EDGES,
                   S2D_STEP_DENSITY_STATS, S2D_STEP_OPTIMIZE_OPACITY, S2D_VIEW_BWD_FROM_TARGET, S2D_VIEW_RGBA8,
                   S2D_VIEW_RGBA32F)
from ._handle import S2DError
from ._runtime import hip_runtimes_mapped, load_library, use_library
from .backdrop import BackdropTrainer
from .coarse import CoarseTrainer
from .multi import MultiTrainer
from .trainer import Trainer
from .weights import WeightedTrainer

__all__ = ["Trainer", "MultiTrainer", "CoarseTrainer", "BackdropTrainer", "WeightedTrainer", "S2DError", "load_library", "use_library", "hip_runtimes_mapped",
           "SPLAT_DTYPE", "ADAM_DTYPE", "STATUS_NAMES"]
