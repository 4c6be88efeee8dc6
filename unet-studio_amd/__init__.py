"""MI355X-native engine for the UNet3d hot path of UNet-Studio (unet.hpp / unet.cpp / train.cpp step loop).

Host-side mirror of the reference's operator surface over libunet_hip.so (include/unet_hip.h).
Importing this package loads the HIP library; if it is missing the import fails -- there is no fallback.
"""
from . import engine  # noqa: F401  (raises ImportError when libunet_hip.so is absent)
from .engine import DTYPE_BF16, DTYPE_F32, IMPL_AUTO, IMPL_DIRECT, Plan, UNetError  # noqa: F401
from .unet3d import SGD, UNet3d  # noqa: F401
from .train import SyntheticVolumes, Trainer, TrainingParam  # noqa: F401
from . import augment  # noqa: F401
from . import space  # noqa: F401  (the module: space.EXPORTS the symbols of include/unet_space.h)
from .space import NativeVolume, model_to_image_map, to_model_space  # noqa: F401
from . import tiles  # noqa: F401  (the module: tiles.EXPORTS the symbols of include/unet_tiles.h)
from .tiles import canvas_dims, plan_tiles  # noqa: F401
from . import mirror  # noqa: F401  (the module: mirror.EXPORTS the symbols of include/unet_mirror.h)
from . import ensemble  # noqa: F401  (the module: ensemble.EXPORTS the symbols of include/unet_ensemble.h)
from .evaluate import EvaluateUNet  # noqa: F401
from .augment import AugmentedVolumes, PrefetchedVolumes, visual_perception_augmentation  # noqa: F401
from . import nz  # noqa: F401
from .nz import NzError  # noqa: F401
from . import qc  # noqa: F401  (the module: qc.qc() is the reference's qc(), qc.EXPORTS the symbols of include/unet_qc.h)
from .qc import QcStat, calculate_qc, qc_counts, run_qc  # noqa: F401
from . import feed  # noqa: F401  (the module: feed.EXPORTS the symbols of include/unet_feed.h)
from .feed import TrainingFeed  # noqa: F401
from . import postproc  # noqa: F401  (the module: postproc.EXPORTS the symbols of include/unet_postproc.h)
from .postproc import parse_chain, run_postproc  # noqa: F401
from . import preproc  # noqa: F401  (the module: preproc.EXPORTS the symbols of include/unet_preproc.h)
from .preproc import run_preproc  # noqa: F401
from . import components  # noqa: F401  (the module: components.EXPORTS the symbols of include/unet_components.h)
from . import atlas  # noqa: F401  (the module: atlas.EXPORTS the symbols of include/unet_atlas.h)
from . import register  # noqa: F401  (the module: register.EXPORTS the symbols of include/unet_register.h)
from . import table  # noqa: F401  (the module: table.EXPORTS the symbols of include/unet_table.h)
from . import distance  # noqa: F401  (the module: distance.EXPORTS the symbols of include/unet_distance.h)
from . import instances  # noqa: F401  (the module: instances.EXPORTS the symbols of include/unet_instances.h)
from . import morph  # noqa: F401  (the module: morph.EXPORTS the symbols of include/unet_morph.h)
from . import connectivity  # noqa: F401  (the module: connectivity.EXPORTS the symbols of include/unet_connectivity.h)
from . import stats  # noqa: F401  (the module: stats.EXPORTS the symbols of include/unet_stats.h)
from . import calib  # noqa: F401  (the module: calib.EXPORTS the symbols of include/unet_calib.h)
from . import recal  # noqa: F401  (the module: recal.EXPORTS the symbols of include/unet_recal.h)
from . import patches  # noqa: F401  (the module: patches.EXPORTS the symbols of include/unet_patches.h)
from . import coreg  # noqa: F401  (the module: coreg.EXPORTS the symbols of include/unet_coreg.h)
from . import start  # noqa: F401  (the module: start.EXPORTS the symbols of include/unet_start.h)
from . import warp  # noqa: F401  (the module: warp.EXPORTS the symbols of include/unet_warp.h)
from . import cowarp  # noqa: F401  (the module: cowarp.EXPORTS the symbols of include/unet_cowarp.h)
from . import deform  # noqa: F401  (the module: deform.EXPORTS the symbols of include/unet_deform.h)
from . import bias  # noqa: F401  (the module: bias.EXPORTS the symbols of include/unet_bias.h)
from .patches import WindowFeed, to_canvas  # noqa: F401


def save_to_file(model, file_name):
    """bool save_to_file(UNet3d& model, const char* file_name) -- main.cpp:207-233 (`.nz`: gzip + MATLAB Level-4 records, nz.py)"""
    return nz.save_to_file(model, file_name)


def load_from_file(file_name, device="cuda:0", dtype="bf16"):
    """load_from_file (main.cpp:157-206): builds UNet3d(channels[0], channels[1], architecture) on `device` and fills
    parameters() from tensor0..N; raises NzError with the reference's messages."""
    return nz.load_from_file(file_name, lambda i, o, a: UNet3d(i, o, a, device=device, dtype=dtype))


def default_feature(out_count):
    """The reference's default architecture string (train.cpp:1054-1069)."""
    out = "conv%d,ks1,stride1" % out_count
    nl = "norm,leaky_relu"
    enc = []
    for i, c in enumerate([16, 32, 64, 128, 256, 256]):
        enc.append("conv%d,ks3,stride%d+%s+conv%d,ks3,stride1+%s" % (c, 1 if i == 0 else 2, nl, c, nl))
    enc[-1] += "+conv_trans256,ks2,stride2"
    dec = ["conv%d,ks3,stride1+%s+conv%d,ks3,stride1+%s+%s+conv_trans%d,ks2,stride2" % (c, nl, c, nl, out, up)
           for c, up in [(256, 128), (128, 64), (64, 32), (32, 16)]]
    dec.append("conv16,ks3,stride1+%s+conv16,ks3,stride1+%s+%s" % (nl, nl, out))
    return "\n".join(enc + dec)
