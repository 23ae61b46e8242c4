"""Post-processing of a two-class prediction on the device: 3-D connected components of its foreground, "keep the largest connected component"
(MONAI's `KeepLargestConnectedComponent` after `AsDiscrete`), "fill holes" (`FillHoles`) and "remove small components" (`RemoveSmallObjects`), through
`vsseg_components_label` / `vsseg_keep_largest_component` / `vsseg_fill_holes` / `vsseg_remove_small_components` (csrc/components.hip).

Conventions: the foreground is the argmax over the two class channels as `compute_dice_score` and `argmax_segmentation` read it (ties and NaN are
background); connectivity 6, 18 or 26 (26 = `skimage.measure.label` with full connectivity, which MONAI uses); a component's label is 1 + the smallest
linear index `(x * Y + y) * Z + z` of its voxels; the largest component has the most voxels, ties going to the smallest label.  The filtered
prediction is a one-hot fp32 [B,2,X,Y,Z] tensor, so that `compute_dice_score`, `compute_surface_distances`, `argmax_segmentation` and
`VSparams.export_segmentation` take it like any other prediction.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from . import _lib as L
from . import _volume as V


def _route(name: str, outputs: torch.Tensor, connectivity, return_stats: bool, extra: tuple = (), labels: bool = False, caller: str = ""):
    """The body of the four calls: vsseg_<name> once per volume, `extra` between connectivity and scratch.  (result, stats or None): the one-hot fp32 [B,2,X,Y,Z]
    prediction (a view of channels-last storage), or with `labels` the int32 [B,X,Y,Z] labels."""
    B, dims = V.check_prediction("outputs", outputs)
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    lg, _ = V.on_device(caller or name, "outputs", outputs)
    stream = torch.cuda.current_stream(lg.device).cuda_stream
    nv = dims[0] * dims[1] * dims[2]
    scratch = V.scratch("components_scratch_bytes", lg.device, dims, stream)
    out = torch.empty((B, *dims) if labels else (B, *dims, 2), dtype=torch.int32 if labels else torch.float32, device=lg.device)
    stats = torch.empty((B, 4), dtype=torch.int64, device=lg.device) if return_stats else None
    V.each_volume(name, B, stream, (lg, 2 * nv), 2, L.i3(dims), connectivity, *extra, scratch.data_ptr(), scratch.numel(), (out, nv if labels else 2 * nv), (stats, 4))
    return (out if labels else out.permute(0, 4, 1, 2, 3)), stats


def connected_components(outputs: torch.Tensor, connectivity: int = 26) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels int32 [B,X,Y,Z], stats int64 [B,4]) on the device for `outputs` [B,2,X,Y,Z] logits or probabilities in any layout.  labels: 0 on the
    background, 1 + the smallest linear index of its component on a foreground voxel.  stats: foreground voxels, number of components, voxels of the
    largest component, its label (0 when there is no foreground).  No host synchronisation."""
    return _route("components_label", outputs, connectivity, True, labels=True, caller="connected_components")


def _one_hot(name: str, outputs, connectivity, return_stats: bool, extra: tuple = ()):
    result, stats = _route(name, outputs, connectivity, return_stats, extra)
    return (result, stats) if return_stats else result


def keep_largest_component(outputs: torch.Tensor, connectivity: int = 26, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] (logits or probabilities, any layout) reduced to the largest connected component of its foreground: fp32
    [B,2,X,Y,Z] (a view of channels-last storage, as `sliding_window_inference` returns), channel 1 = 1.0 on the kept component and 0.0 elsewhere,
    channel 0 = 1 - channel 1.  `outputs` is not written.  With `return_stats` also the int64 [B,4] statistics of `connected_components`.  No host
    synchronisation."""
    return _one_hot("keep_largest_component", outputs, connectivity, return_stats)


def min_component_voxels(min_mm3: float, spacing) -> int:
    """The voxel threshold of --min_component_mm3: ceil(min_mm3 / (sx * sy * sz)), the voxel volume formed in fp64 from the fp32 spacing as `vsseg_measurements`
    forms it (so that a component is kept exactly when the volume `--measurements` would report for it reaches min_mm3).  0 mm3 = 0 voxels = off."""
    sx, sy, sz = (float(np.float32(v)) for v in spacing)
    if not (isinstance(min_mm3, (int, float)) and not isinstance(min_mm3, bool) and math.isfinite(min_mm3) and min_mm3 >= 0):
        raise ValueError(f"min_mm3 must be a finite number >= 0, got {min_mm3!r}")
    if not all(math.isfinite(v) and v > 0 for v in (sx, sy, sz)):
        raise ValueError(f"spacing must be three positive finite extents, got {spacing!r}")
    return int(math.ceil(float(min_mm3) / (sx * sy * sz)))


def fill_holes(outputs: torch.Tensor, connectivity: int = 6, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] (logits or probabilities, any layout) with the holes of its foreground P filled (MONAI's `FillHoles`,
    `scipy.ndimage.binary_fill_holes`): fp32 [B,2,X,Y,Z] (a view of channels-last storage), channel 1 = 1.0 on P and on every connected component of
    the complement of P that holds no voxel on the border of the volume (an index equal to 0 or to dim - 1), channel 0 = 1 - channel 1.
    `connectivity` is that of the BACKGROUND: 6 (scipy's default, the dual of a 26-connected foreground), 18 or 26 (MONAI's default).  A tunnel through a
    ring is not a hole; a volume with an extent of 1 or 2 along an axis has none; an empty prediction stays empty.  `outputs` is not written.  With
    `return_stats` also int64 [B,4] on the device: |P|, the number of holes, the filled voxels |H|, |P| + |H|.  No host synchronisation."""
    return _one_hot("fill_holes", outputs, connectivity, return_stats)


def remove_small_components(outputs: torch.Tensor, min_voxels: int, connectivity: int = 26, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] reduced to the connected components of its foreground P with at least `min_voxels` voxels (strictly smaller
    ones are removed: `skimage.morphology.remove_small_objects`, MONAI's `RemoveSmallObjects`): the same one-hot fp32 [B,2,X,Y,Z] as
    `keep_largest_component` returns.  `min_voxels` <= 1 keeps P.  `outputs` is not written.  With `return_stats` also int64 [B,4] on the device: |P|,
    the number of components of P, the kept voxels, the kept components.  No host synchronisation: the threshold goes to the device as an argument."""
    if isinstance(min_voxels, bool) or not isinstance(min_voxels, int) or not 0 <= min_voxels < 2**63:
        raise ValueError(f"min_voxels must be an integer >= 0, got {min_voxels!r}")
    return _one_hot("remove_small_components", outputs, connectivity, return_stats, (min_voxels,))
