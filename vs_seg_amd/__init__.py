"""vs_seg_amd — MI355X-native (gfx950) hot path of KCL-BMEIS/VS_Seg behind the reference's own Python interfaces.

    from vs_seg_amd import UNet2d5_spvPA, Dice_spvPA, sliding_window_inference, Adam, AdamW, SGD

`UNet2d5_spvPA` / `Dice_spvPA` mirror ref:params/networks/nets/unet2d5_spvPA.py and ref:params/losses/dice_spvPA.py;
`sliding_window_inference` mirrors the MONAI 0.4.0 function called at ref:params/VSparams.py:568-574.  All compute is
in `libvsseg_hip.so` (hand-written HIP, C ABI in include/vsseg_hip.h); there is no CPU fallback.
"""
from ._lib import VssegError, fx_status  # noqa: F401
from .inferers import compute_dice_score, sliding_window_inference  # noqa: F401
from .losses.dice_spvPA import Dice_spvPA, check_ce, check_ce_topk, check_region, topk_count  # noqa: F401
from .metrics import MEASUREMENT_FIELDS, compute_measurements, compute_surface_dice, compute_surface_distances, compute_surface_metrics, surface_metric_fields, voxel_spacing  # noqa: F401
from .networks.nets.unet2d5_spvPA import UNet2d5_spvPA  # noqa: F401
from .optim import SGD, Adam, AdamW, check_optimizer, poly_lr  # noqa: F401
from .postprocess import binary_close, binary_dilate, binary_erode, binary_open, connected_components, fill_holes, keep_largest_component, min_component_voxels, remove_small_components  # noqa: F401

__all__ = ["UNet2d5_spvPA", "Dice_spvPA", "check_ce", "check_ce_topk", "check_region", "topk_count", "sliding_window_inference", "compute_dice_score", "compute_surface_distances", "compute_surface_metrics", "compute_surface_dice", "surface_metric_fields", "compute_measurements", "MEASUREMENT_FIELDS", "voxel_spacing", "connected_components", "keep_largest_component", "fill_holes", "remove_small_components", "min_component_voxels", "binary_dilate", "binary_erode", "binary_close", "binary_open", "Adam", "AdamW", "SGD", "check_optimizer", "poly_lr", "fx_status", "VssegError"]
