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
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .inferers import _as_cl

_SCRATCH_CACHE: Dict[tuple, torch.Tensor] = {}  # (device, dims, stream) -> scratch of vsseg_surface_distances
_MEASURE_SCRATCH_CACHE: Dict[tuple, torch.Tensor] = {}  # ... of vsseg_measurements

MEASUREMENT_FIELDS = ("voxels_pred", "voxels_label", "volume_pred_mm3", "volume_label_mm3", "centroid_distance_mm", "max_diameter_pred_mm", "max_diameter_label_mm",
                      "max_axial_diameter_pred_mm", "max_axial_diameter_label_mm")  # the nine outputs of vsseg_measurements, in order


def voxel_spacing(affine) -> Tuple[float, float, float]:
    """Voxel extents in mm: the column norms of the 3x3 block of a 4x4 affine (e.g. the RAS affine `load_case` keeps as label_meta["affine"])."""
    a = np.asarray(affine, dtype=np.float64)
    if a.shape != (4, 4):
        raise ValueError(f"expected a 4x4 affine, got shape {a.shape}")
    return tuple(float(v) for v in np.linalg.norm(a[:3, :3], axis=0))


def _scratch(device, dims, stream, cache=_SCRATCH_CACHE, what="surface_scratch_bytes") -> torch.Tensor:
    key = (str(device), tuple(dims), stream)
    buf = cache.get(key)
    if buf is None:
        nbytes = int(getattr(L.lib(), "vsseg_" + what)(L.i3(dims)))
        if nbytes < 0:
            L.check(nbytes, what)
        while len(cache) >= 4:
            cache.pop(next(iter(cache)))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)  # (the caching allocator's blocks are 512-byte aligned)
        cache[key] = buf
    return buf


def _spacing3(spacing) -> Tuple[float, float, float]:
    if spacing is None:
        return (1.0, 1.0, 1.0)
    try:
        spacing = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"spacing must be three positive numbers (mm) or None, got {spacing!r}") from None
    if len(spacing) != 3 or not all(math.isfinite(s) and s > 0 for s in spacing):
        raise ValueError(f"spacing must be three positive finite numbers (mm) or None, got {spacing!r}")
    return spacing


def compute_surface_distances(predicted_probabilities: torch.Tensor, label: torch.Tensor, spacing: Optional[Sequence[float]] = None,
                              percentile: Optional[float] = 95.0) -> torch.Tensor:
    """[B,2] fp32 on the device: column 0 the Hausdorff distance at `percentile` (None: the maximum), column 1 the average symmetric surface
    distance, in mm for voxel extents `spacing` (x, y, z; None: voxel units).  `predicted_probabilities` [B,2,X,Y,Z] logits or probabilities in
    any layout (as `compute_dice_score` takes them), `label` [B,1,X,Y,Z].  No host synchronisation."""
    if percentile is None:
        percentile = 100.0  # numpy.percentile at 100 is the maximum
    try:
        percentile = float(percentile)
    except (TypeError, ValueError):
        raise ValueError(f"percentile must be a number in [0, 100] or None, got {percentile!r}") from None
    if not 0.0 <= percentile <= 100.0:
        raise ValueError(f"percentile must be in [0, 100], got {percentile}")
    spacing = _spacing3(spacing)
    if predicted_probabilities.dim() != 5 or predicted_probabilities.shape[1] != 2:
        raise ValueError(f"expected predicted_probabilities [B,2,X,Y,Z], got {tuple(predicted_probabilities.shape)}")
    B, _, X, Y, Z = predicted_probabilities.shape
    if tuple(label.shape) != (B, 1, X, Y, Z):
        raise ValueError(f"expected label [B,1,X,Y,Z] = {(B, 1, X, Y, Z)}, got {tuple(label.shape)}")
    if not (predicted_probabilities.is_cuda and label.is_cuda):
        raise RuntimeError("vs_seg_amd.compute_surface_distances runs on an MI355X only; there is no CPU fallback")
    if label.device != predicted_probabilities.device:
        raise ValueError(f"predicted_probabilities on {predicted_probabilities.device}, label on {label.device}")
    lib = L.lib()
    stream = torch.cuda.current_stream(predicted_probabilities.device).cuda_stream
    lg = _as_cl(predicted_probabilities)  # [B,X,Y,Z,2] fp32: a view of the sliding window's channels-last output, no copy
    lab = label.detach()
    if lab.dtype != torch.float32 or not lab.is_contiguous():
        lab = lab.to(torch.float32).contiguous()
    dims = (int(X), int(Y), int(Z))
    nv = dims[0] * dims[1] * dims[2]
    scratch = _scratch(lg.device, dims, stream)
    sp = (ctypes.c_float * 3)(*spacing)
    out = torch.empty((B, 2), dtype=torch.float32, device=lg.device)
    for b in range(B):
        L.check(lib.vsseg_surface_distances(lg.data_ptr() + 8 * b * nv, 2, lab.data_ptr() + 4 * b * nv, L.i3(dims), sp, percentile, scratch.data_ptr(), scratch.numel(),
                                            out.data_ptr() + 8 * b, stream), "surface_distances")
    return out


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
    if percentile is None:
        percentile = 100.0
    try:
        percentile = float(percentile)
    except (TypeError, ValueError):
        raise ValueError(f"percentile must be a number in [0, 100] or None, got {percentile!r}") from None
    if not 0.0 <= percentile <= 100.0:
        raise ValueError(f"percentile must be in [0, 100], got {percentile}")
    spacing = _spacing3(spacing)
    tol = check_tolerances(tolerances)
    if predicted_probabilities.dim() != 5 or predicted_probabilities.shape[1] != 2:
        raise ValueError(f"expected predicted_probabilities [B,2,X,Y,Z], got {tuple(predicted_probabilities.shape)}")
    B, _, X, Y, Z = predicted_probabilities.shape
    if tuple(label.shape) != (B, 1, X, Y, Z):
        raise ValueError(f"expected label [B,1,X,Y,Z] = {(B, 1, X, Y, Z)}, got {tuple(label.shape)}")
    if not (predicted_probabilities.is_cuda and label.is_cuda):
        raise RuntimeError("vs_seg_amd.compute_surface_metrics runs on an MI355X only; there is no CPU fallback")
    if label.device != predicted_probabilities.device:
        raise ValueError(f"predicted_probabilities on {predicted_probabilities.device}, label on {label.device}")
    lib = L.lib()
    stream = torch.cuda.current_stream(predicted_probabilities.device).cuda_stream
    lg = _as_cl(predicted_probabilities)  # [B,X,Y,Z,2] fp32
    lab = label.detach()
    if lab.dtype != torch.float32 or not lab.is_contiguous():
        lab = lab.to(torch.float32).contiguous()
    dims = (int(X), int(Y), int(Z))
    nv = dims[0] * dims[1] * dims[2]
    scratch = _scratch(lg.device, dims, stream)
    sp = (ctypes.c_float * 3)(*spacing)
    tl = (ctypes.c_float * max(len(tol), 1))(*tol)
    n = 3 + 3 * len(tol)
    out = torch.empty((B, n), dtype=torch.float32, device=lg.device)
    for b in range(B):
        L.check(lib.vsseg_surface_metrics(lg.data_ptr() + 8 * b * nv, 2, lab.data_ptr() + 4 * b * nv, L.i3(dims), sp, percentile, tl, len(tol), scratch.data_ptr(), scratch.numel(),
                                          out.data_ptr() + 4 * n * b, stream), "surface_metrics")
    return out


def compute_surface_dice(predicted_probabilities: torch.Tensor, label: torch.Tensor, spacing: Optional[Sequence[float]] = None, tolerances: Sequence[float] = (1.0,)) -> torch.Tensor:
    """[B, T] fp32 on the device: the normalised surface Dice at every tolerance (mm), the nsd columns of `compute_surface_metrics`."""
    return compute_surface_metrics(predicted_probabilities, label, spacing, 95.0, tolerances)[:, 3::3]


def compute_measurements(predicted_probabilities: torch.Tensor, label: Optional[torch.Tensor] = None, spacing: Optional[Sequence[float]] = None) -> torch.Tensor:
    """[B,9] fp64 on the device, the columns named by MEASUREMENT_FIELDS: voxel counts, volumes (mm^3), the distance between the centres of mass, the
    largest 3-D diameter and the largest diameter within an axial (equal z) slice, each of the argmax prediction and of the label, for voxel extents
    `spacing` (x, y, z in mm; None: voxel units).  `predicted_probabilities` [B,2,X,Y,Z] logits or probabilities in any layout, `label` [B,1,X,Y,Z] or
    None (the label columns and the centroid distance are then NaN).  Empty mask: its diameters and the centroid distance are NaN.  Y * Z <= 2^18.
    No host synchronisation (vsseg_measurements, csrc/measure.hip)."""
    spacing = _spacing3(spacing)
    if predicted_probabilities.dim() != 5 or predicted_probabilities.shape[1] != 2:
        raise ValueError(f"expected predicted_probabilities [B,2,X,Y,Z], got {tuple(predicted_probabilities.shape)}")
    B, _, X, Y, Z = predicted_probabilities.shape
    if label is not None and tuple(label.shape) != (B, 1, X, Y, Z):
        raise ValueError(f"expected label [B,1,X,Y,Z] = {(B, 1, X, Y, Z)}, got {tuple(label.shape)}")
    if not (predicted_probabilities.is_cuda and (label is None or label.is_cuda)):
        raise RuntimeError("vs_seg_amd.compute_measurements runs on an MI355X only; there is no CPU fallback")
    if label is not None and label.device != predicted_probabilities.device:
        raise ValueError(f"predicted_probabilities on {predicted_probabilities.device}, label on {label.device}")
    lib = L.lib()
    stream = torch.cuda.current_stream(predicted_probabilities.device).cuda_stream
    lg = _as_cl(predicted_probabilities)  # [B,X,Y,Z,2] fp32
    lab = None
    if label is not None:
        lab = label.detach()
        if lab.dtype != torch.float32 or not lab.is_contiguous():
            lab = lab.to(torch.float32).contiguous()
    dims = (int(X), int(Y), int(Z))
    nv = dims[0] * dims[1] * dims[2]
    scratch = _scratch(lg.device, dims, stream, _MEASURE_SCRATCH_CACHE, "measure_scratch_bytes")
    sp = (ctypes.c_float * 3)(*spacing)
    n = len(MEASUREMENT_FIELDS)
    out = torch.empty((B, n), dtype=torch.float64, device=lg.device)
    for b in range(B):
        L.check(lib.vsseg_measurements(lg.data_ptr() + 8 * b * nv, 2, None if lab is None else lab.data_ptr() + 4 * b * nv, L.i3(dims), sp, scratch.data_ptr(), scratch.numel(),
                                       out.data_ptr() + 8 * n * b, stream), "measurements")
    return out
