"""Post-processing of a two-class prediction on the device: 3-D connected components of its foreground and "keep the largest connected component"
(MONAI's `KeepLargestConnectedComponent` after `AsDiscrete`), through `vsseg_components_label` / `vsseg_keep_largest_component` (csrc/components.hip).

Conventions: the foreground is the argmax over the two class channels as `compute_dice_score` and `argmax_segmentation` read it (ties and NaN are
background); connectivity 6, 18 or 26 (26 = `skimage.measure.label` with full connectivity, which MONAI uses); a component's label is 1 + the smallest
linear index `(x * Y + y) * Z + z` of its voxels; the largest component has the most voxels, ties going to the smallest label.  The filtered
prediction is a one-hot fp32 [B,2,X,Y,Z] tensor, so that `compute_dice_score`, `compute_surface_distances`, `argmax_segmentation` and
`VSparams.export_segmentation` take it like any other prediction.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from . import _lib as L
from .inferers import _as_cl

_SCRATCH_CACHE: Dict[tuple, torch.Tensor] = {}  # (device, dims, stream) -> scratch of vsseg_components_label / vsseg_keep_largest_component


def _scratch(device, dims, stream) -> torch.Tensor:
    key = (str(device), tuple(dims), stream)
    buf = _SCRATCH_CACHE.get(key)
    if buf is None:
        nbytes = int(L.lib().vsseg_components_scratch_bytes(L.i3(dims)))
        if nbytes < 0:
            L.check(nbytes, "components_scratch_bytes")
        while len(_SCRATCH_CACHE) >= 4:
            _SCRATCH_CACHE.pop(next(iter(_SCRATCH_CACHE)))
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)  # (the caching allocator's blocks are 512-byte aligned)
        _SCRATCH_CACHE[key] = buf
    return buf


def _checked(name: str, outputs: torch.Tensor, connectivity) -> Tuple[int, Tuple[int, int, int]]:
    if not isinstance(outputs, torch.Tensor) or outputs.dim() != 5 or outputs.shape[1] != 2:
        raise ValueError(f"expected outputs [B,2,X,Y,Z], got {tuple(outputs.shape) if isinstance(outputs, torch.Tensor) else type(outputs).__name__}")
    if isinstance(connectivity, bool) or not isinstance(connectivity, int) or connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    if not outputs.is_cuda:
        raise RuntimeError(f"vs_seg_amd.{name} runs on an MI355X only; there is no CPU fallback")
    B, _, X, Y, Z = outputs.shape
    return int(B), (int(X), int(Y), int(Z))


def connected_components(outputs: torch.Tensor, connectivity: int = 26) -> Tuple[torch.Tensor, torch.Tensor]:
    """(labels int32 [B,X,Y,Z], stats int64 [B,4]) on the device for `outputs` [B,2,X,Y,Z] logits or probabilities in any layout.  labels: 0 on the
    background, 1 + the smallest linear index of its component on a foreground voxel.  stats: foreground voxels, number of components, voxels of the
    largest component, its label (0 when there is no foreground).  No host synchronisation."""
    B, dims = _checked("connected_components", outputs, connectivity)
    lib = L.lib()
    stream = torch.cuda.current_stream(outputs.device).cuda_stream
    lg = _as_cl(outputs)  # [B,X,Y,Z,2] fp32: a view of the sliding window's channels-last output, no copy
    nv = dims[0] * dims[1] * dims[2]
    scratch = _scratch(lg.device, dims, stream)
    labels = torch.empty((B, *dims), dtype=torch.int32, device=lg.device)
    stats = torch.empty((B, 4), dtype=torch.int64, device=lg.device)
    for b in range(B):
        L.check(lib.vsseg_components_label(lg.data_ptr() + 8 * b * nv, 2, L.i3(dims), connectivity, scratch.data_ptr(), scratch.numel(), labels.data_ptr() + 4 * b * nv,
                                           stats.data_ptr() + 32 * b, stream), "components_label")
    return labels, stats


def keep_largest_component(outputs: torch.Tensor, connectivity: int = 26, return_stats: bool = False):
    """The prediction `outputs` [B,2,X,Y,Z] (logits or probabilities, any layout) reduced to the largest connected component of its foreground: fp32
    [B,2,X,Y,Z] (a view of channels-last storage, as `sliding_window_inference` returns), channel 1 = 1.0 on the kept component and 0.0 elsewhere,
    channel 0 = 1 - channel 1.  `outputs` is not written.  With `return_stats` also the int64 [B,4] statistics of `connected_components`.  No host
    synchronisation."""
    B, dims = _checked("keep_largest_component", outputs, connectivity)
    lib = L.lib()
    stream = torch.cuda.current_stream(outputs.device).cuda_stream
    lg = _as_cl(outputs)
    nv = dims[0] * dims[1] * dims[2]
    scratch = _scratch(lg.device, dims, stream)
    out = torch.empty((B, *dims, 2), dtype=torch.float32, device=lg.device)
    stats = torch.empty((B, 4), dtype=torch.int64, device=lg.device) if return_stats else None
    for b in range(B):
        L.check(lib.vsseg_keep_largest_component(lg.data_ptr() + 8 * b * nv, 2, L.i3(dims), connectivity, scratch.data_ptr(), scratch.numel(), out.data_ptr() + 8 * b * nv,
                                                 stats.data_ptr() + 32 * b if return_stats else None, stream), "keep_largest_component")
    filtered = out.permute(0, 4, 1, 2, 3)
    return (filtered, stats) if return_stats else filtered
