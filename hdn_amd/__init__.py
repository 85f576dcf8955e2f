"""hdn_amd — MI355X-native implementation of HDN's per-frame homography-estimation hot path.

Hand-written gfx950 HIP kernels behind a C ABI (include/hdn_hip.h, hdn_amd/libhdn_hip.so), exposed under
the reference's own Python signatures.  See DESIGN.md and INTEGRATION.md.
"""
from .xcorr import xcorr_depthwise, xcorr_depthwise_backward, xcorr_depthwise_circular, xcorr_depthwise_multi, xcorr_fast, xcorr_slow  # noqa: F401
from .homography import DLT_solve, transform, transformer, Homo_STN, dlt_warp, dlt_solve_backward, transformer_backward  # noqa: F401
from .share_feature import PreShareFeature, PreShareFeatureTrain, fold_params  # noqa: F401
from .homo_model import HomoModelBuilder, track_proj  # noqa: F401
from .logpolar import STN_Polar, STN_PolarTrain, logpolar_sample_backward  # noqa: F401
from .affine import affine_sample, affine_sample_backward  # noqa: F401
from .triplet import TripletMarginLossL1, triplet_l1, triplet_l1_backward, triplet_l1_mean, triplet_l1_mean_backward  # noqa: F401
from .corner import corner_losses, corner_losses_backward, training_outputs  # noqa: F401
from .losses import (kalyo_l1_loss, select_cross_entropy_loss, select_l1_loss, select_l1_loss_c,  # noqa: F401
                     select_xr_focal_fuse_smooth_l1_loss_top_k, supervised_losses, supervised_losses_backward)
from .simi_geometry import (combine_affine_c0_v2, combine_affine_lt0, get_polar_from_two_para_loc, lp_pick, polar_pick,  # noqa: F401
                            similarity_warps)
from .simi_train import SimiTrainConfig, simi_training_forward  # noqa: F401
from .optim import GatedAMSGrad, grad_norm  # noqa: F401
from .heads import MultiBAN, MultiCircBAN  # noqa: F401
from .conv_train import conv3x3_valid, depthwise_xcorr_train_forward  # noqa: F401
from .bn_train import batchnorm_relu_train  # noqa: F401
from .refine import homo_refine, refine_warp  # noqa: F401

__version__ = "0.1.0"
from .backbone import optimize_similarity_model, restore_similarity_model  # noqa: F401
from .batched_tracker import track_videos  # noqa: F401
