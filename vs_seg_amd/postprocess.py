"""Post-processing of a two-class prediction on the device: 3-D connected components of its foreground, "keep the largest connected component"
(MONAI's `KeepLargestConnectedComponent` after `AsDiscrete`), "fill holes" (`FillHoles`) and "remove small components" (`RemoveSmallObjects`), through
`vsseg_components_label` / `vsseg_keep_largest_component` / `vsseg_fill_holes` / `vsseg_remove_small_components` (csrc/components.hip); and ball morphology at a
radius in mm, `binary_dilate` / `binary_erode` / `binary_close` / `binary_open`, through `vsseg_ball_morphology` (csrc/ball.hip).

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


MAX_BALL_REACH = 32  # voxels per axis that a ball may reach (csrc/ball.hip)


def check_radius_mm(radius_mm, spacing=None, what: str = "radius_mm") -> float:
    """`radius_mm` as a float once it is a finite number >= 0 whose ball reaches at most 32 voxels along every axis of `spacing` (None: not checked)."""
    if isinstance(radius_mm, bool) or not isinstance(radius_mm, (int, float, np.integer, np.floating)) or not math.isfinite(radius_mm) or radius_mm < 0:
        raise ValueError(f"{what} must be a finite number >= 0 (mm), got {radius_mm!r}")
    radius_mm = float(radius_mm)
    for axis, s in enumerate(spacing or ()):
        reach = math.floor(radius_mm / float(np.float32(s)))  # the fp32 spacing that the library is given
        if reach > MAX_BALL_REACH:
            raise ValueError(f"{what} = {radius_mm} reaches {reach} voxels along axis {axis} (spacing {s} mm); at most {MAX_BALL_REACH} are supported")
    return radius_mm


def _ball(caller: str, op: int, outputs, radius_mm, spacing, return_stats: bool):
    """The body of the four ball operations: vsseg_ball_morphology with `op` once per volume."""
    B, dims = V.check_prediction("outputs", outputs)
    spacing = V.spacing3(spacing)
    radius_mm = check_radius_mm(radius_mm, spacing)
    lg, _ = V.on_device(caller, "outputs", outputs)
    stream = torch.cuda.current_stream(lg.device).cuda_stream
    nv = dims[0] * dims[1] * dims[2]
    scratch = V.scratch("ball_scratch_bytes", lg.device, dims, stream)
    out = torch.empty((B, *dims, 2), dtype=torch.float32, device=lg.device)
    stats = torch.empty((B, 4), dtype=torch.int64, device=lg.device) if return_stats else None
    V.each_volume("ball_morphology", B, stream, (lg, 2 * nv), 2, L.i3(dims), V.float3(spacing), op, radius_mm, scratch.data_ptr(), scratch.numel(), (out, 2 * nv), (stats, 4))
    result = out.permute(0, 4, 1, 2, 3)
    return (result, stats) if return_stats else result


def binary_dilate(outputs: torch.Tensor, radius_mm: float, spacing=None, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] (logits or probabilities, any layout) with its foreground P dilated by a ball of `radius_mm` mm: every voxel of the
    volume that has a voxel of P at an offset d with (sx dx)^2 + (sy dy)^2 + (sz dz)^2 <= radius_mm^2 (a tie belongs; `spacing` = mm per voxel, None = 1 mm; outside
    the volume there is no foreground: `scipy.ndimage.binary_dilation` with that ball and border_value 0).  Returns the one-hot fp32 [B,2,X,Y,Z] of
    `keep_largest_component`; `outputs` is not written.  With `return_stats` also int64 [B,4] on the device: |P|, |result|, voxels added, voxels removed.  The
    ball may reach 32 voxels per axis; radius 0 returns the one-hot of P.  No host synchronisation."""
    return _ball("binary_dilate", L.OP_DILATE, outputs, radius_mm, spacing, return_stats)


def binary_erode(outputs: torch.Tensor, radius_mm: float, spacing=None, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] with its foreground P eroded by a ball of `radius_mm` mm: every voxel of P that has no background voxel OF THE VOLUME
    at a ball offset (the ball of `binary_dilate`).  Positions outside the volume are ignored, they are not background (`scipy.ndimage.binary_erosion` with
    border_value 1): a tumour cut by the field of view does not shrink at the cut.  The same one-hot result and statistics as `binary_dilate`."""
    return _ball("binary_erode", L.OP_ERODE, outputs, radius_mm, spacing, return_stats)


def binary_close(outputs: torch.Tensor, radius_mm: float, spacing=None, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] with its foreground closed by a ball of `radius_mm` mm: `binary_erode` of `binary_dilate`, both with the same ball.
    Fragments less than about 2 * radius_mm apart are bridged and gaps narrower than that are filled; the result contains P (also at the border of the volume)
    and closing it again changes nothing.  The same one-hot result and statistics as `binary_dilate`."""
    return _ball("binary_close", L.OP_CLOSE, outputs, radius_mm, spacing, return_stats)


def binary_open(outputs: torch.Tensor, radius_mm: float, spacing=None, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] with its foreground opened by a ball of `radius_mm` mm: `binary_dilate` of `binary_erode`, both with the same ball.
    Spurs and islands into which the ball does not fit are removed; the result lies inside P and opening it again changes nothing.  The same one-hot result and
    statistics as `binary_dilate`."""
    return _ball("binary_open", L.OP_OPEN, outputs, radius_mm, spacing, return_stats)
