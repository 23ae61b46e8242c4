"""Surface-distance metrics next to `compute_dice_score`: the 95th-percentile Hausdorff distance and the average symmetric surface distance
of the argmax segmentation against the label, computed on the device (`vsseg_surface_distances`, csrc/surface.hip), and with them the normalised
surface Dice at tolerances in mm (`compute_surface_metrics` / `compute_surface_dice`, `vsseg_surface_metrics`: the same edge pass and distance transform).

Conventions (those of MONAI's `compute_hausdorff_distance(directed=False)` / `compute_average_surface_distance(symmetric=True)`): the
prediction mask is the argmax over the two class channels (ties -> class 0), the label mask `(int)label == 1`, as `compute_dice_score` reads
them; distances run from edge voxels (mask AND NOT its 6-connected erosion, outside the volume = background) to the nearest edge voxel of the
other mask, in mm.  Both masks empty: NaN; one empty: +inf.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import _volume as V

MEASUREMENT_FIELDS = ("voxels_pred", "voxels_label", "volume_pred_mm3", "volume_label_mm3", "centroid_distance_mm", "max_diameter_pred_mm", "max_diameter_label_mm",
                      "max_axial_diameter_pred_mm", "max_axial_diameter_label_mm")  # the nine outputs of vsseg_measurements, in order


def voxel_spacing(affine) -> Tuple[float, float, float]:
    """Voxel extents in mm: the column norms of the 3x3 block of a 4x4 affine (e.g. the RAS affine `load_case` keeps as label_meta["affine"])."""
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError(f"expected a 4x4 affine, got shape {a.shape}")
    return tuple(float(v) for v in np.linalg.norm(a[:3, :3], axis=0))


def _surface(caller: str, name: str, predicted_probabilities, label, spacing, percentile, columns: int, extra: tuple = ()) -> torch.Tensor:
    """The body of `compute_surface_distances` and `compute_surface_metrics`: vsseg_<name> once per volume, `extra` between percentile and scratch."""
    percentile = V.percentile100(percentile)
    sp = V.float3(V.spacing3(spacing))
    B, dims = V.check_prediction("predicted_probabilities", predicted_probabilities)
    lg, lab = V.on_device(caller, "predicted_probabilities", predicted_probabilities, label, B, dims)
    stream = torch.cuda.current_stream(lg.device).cuda_stream
    nv = dims[0] * dims[1] * dims[2]
    scratch = V.scratch("surface_scratch_bytes", lg.device, dims, stream)
    out = torch.empty((B, columns), dtype=torch.float32, device=lg.device)
    V.each_volume(name, B, stream, (lg, 2 * nv), 2, (lab, nv), L.i3(dims), sp, percentile, *extra, scratch.data_ptr(), scratch.numel(), (out, columns))
    return out


def compute_surface_distances(predicted_probabilities: torch.Tensor, label: torch.Tensor, spacing: Optional[Sequence[float]] = None,
                              percentile: Optional[float] = 95.0) -> torch.Tensor:
    """[B,2] fp32 on the device: column 0 the Hausdorff distance at `percentile` (None: the maximum), column 1 the average symmetric surface
    distance, in mm for voxel extents `spacing` (x, y, z; None: voxel units).  `predicted_probabilities` [B,2,X,Y,Z] logits or probabilities in
    any layout (as `compute_dice_score` takes them), `label` [B,1,X,Y,Z].  No host synchronisation."""
    return _surface("compute_surface_distances", "surface_distances", predicted_probabilities, label, spacing, percentile, 2)


MAX_TOLERANCES = 8  # of one vsseg_surface_metrics call


def check_tolerances(tolerances, what="tolerances", distinct=False) -> Tuple[float, ...]:
    """`tolerances` (mm) as a tuple of at most MAX_TOLERANCES finite floats >= 0, in the order given; ValueError (naming `what`) otherwise, and with
    `distinct` also for a repeated value."""
    if isinstance(tolerances, (str, bytes)):
        raise ValueError(f"{what} must be a sequence of finite numbers >= 0 (mm), got {tolerances!r}")
    try:
        tol = tuple(float(t) for t in tolerances)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a sequence of finite numbers >= 0 (mm), got {tolerances!r}") from None
    if not all(math.isfinite(t) and t >= 0 for t in tol):
        raise ValueError(f"{what} must be finite numbers >= 0 (mm), got {tolerances!r}")
    if len(tol) > MAX_TOLERANCES:
        raise ValueError(f"{what}: at most {MAX_TOLERANCES} values, got {len(tol)}")
    if distinct and len(set(tol)) != len(tol):
        raise ValueError(f"{what}: the values must be distinct, got {tolerances!r}")
    return tuple(t + 0.0 for t in tol)  # (-0.0 -> 0.0)


def surface_metric_fields(tolerances=()) -> Tuple[str, ...]:
    """The column names of `compute_surface_metrics(..., tolerances=tolerances)`."""
    return ("hd", "assd", "masd") + tuple(f"{name}_{t:g}mm" for t in check_tolerances(tolerances) for name in ("nsd", "surface_precision", "surface_recall"))


def compute_surface_metrics(predicted_probabilities: torch.Tensor, label: torch.Tensor, spacing: Optional[Sequence[float]] = None, percentile: Optional[float] = 95.0,
                            tolerances: Sequence[float] = ()) -> torch.Tensor:
    """[B, 3 + 3T] fp32 on the device, the columns named by `surface_metric_fields(tolerances)`: the two columns of `compute_surface_distances` (the same bits), the
    mean of the two directed mean surface distances, and per tolerance tau (mm, at most 8) the normalised surface Dice (the share of both boundaries that lies
    within tau of the other boundary; MONAI's `compute_surface_dice`), the surface precision (that share of the prediction's boundary) and the surface recall (of
    the label's).  A distance equal to tau counts.  Both masks empty: NaN; one empty: hd, assd, masd +inf, nsd 0, the fraction over the empty boundary NaN and the
    other 0.  One edge pass and one distance transform serve every column (vsseg_surface_metrics, csrc/surface.hip).  No host synchronisation."""
    tol = check_tolerances(tolerances)
    tl = (ctypes.c_float * max(len(tol), 1))(*tol)
    return _surface("compute_surface_metrics", "surface_metrics", predicted_probabilities, label, spacing, percentile, 3 + 3 * len(tol), (tl, len(tol)))


def compute_surface_dice(predicted_probabilities: torch.Tensor, label: torch.Tensor, spacing: Optional[Sequence[float]] = None, tolerances: Sequence[float] = (1.0,)) -> torch.Tensor:
    """[B, T] fp32 on the device: the normalised surface Dice at every tolerance (mm), the nsd columns of `compute_surface_metrics`."""
    return compute_surface_metrics(predicted_probabilities, label, spacing, 95.0, tolerances)[:, 3::3]


def compute_measurements(predicted_probabilities: torch.Tensor, label: Optional[torch.Tensor] = None, spacing: Optional[Sequence[float]] = None) -> torch.Tensor:
    """[B,9] fp64 on the device, the columns named by MEASUREMENT_FIELDS: voxel counts, volumes (mm^3), the distance between the centres of mass, the
    largest 3-D diameter and the largest diameter within an axial (equal z) slice, each of the argmax prediction and of the label, for voxel extents
    `spacing` (x, y, z in mm; None: voxel units).  `predicted_probabilities` [B,2,X,Y,Z] logits or probabilities in any layout, `label` [B,1,X,Y,Z] or
    None (the label columns and the centroid distance are then NaN).  Empty mask: its diameters and the centroid distance are NaN.  Y * Z <= 2^18.
    No host synchronisation (vsseg_measurements, csrc/measure.hip)."""
    sp = V.float3(V.spacing3(spacing))
    B, dims = V.check_prediction("predicted_probabilities", predicted_probabilities)
    lg, lab = V.on_device("compute_measurements", "predicted_probabilities", predicted_probabilities, label, B, dims)
    stream = torch.cuda.current_stream(lg.device).cuda_stream
    nv = dims[0] * dims[1] * dims[2]
    scratch = V.scratch("measure_scratch_bytes", lg.device, dims, stream)
    n = len(MEASUREMENT_FIELDS)
    out = torch.empty((B, n), dtype=torch.float64, device=lg.device)
    V.each_volume("measurements", B, stream, (lg, 2 * nv), 2, (lab, nv), L.i3(dims), sp, scratch.data_ptr(), scratch.numel(), (out, n))
    return out
