"""What the whole-volume analysis calls of `metrics.py` and `postprocess.py` share: argument checks, the scratch cache and the loop over the batch around
the one-volume-per-call entry points of csrc/surface.hip, csrc/measure.hip and csrc/components.hip."""
from __future__ import annotations

import ctypes
import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib as L
from .inferers import _as_cl

_SCRATCH: Dict[tuple, torch.Tensor] = {}  # (scratch-bytes entry point, device, dims, stream) -> scratch buffer


def scratch(what: str, device, dims, stream) -> torch.Tensor:
    """The cached scratch buffer of the entry points whose size `vsseg_<what>` reports; at most four live buffers per `what`, the oldest goes first."""
    key = (what, str(device), tuple(dims), stream)
    buf = _SCRATCH.get(key)
    if buf is None:
        nbytes = int(getattr(L.lib(), "vsseg_" + what)(L.i3(dims)))
        if nbytes < 0:
            L.check(nbytes, what)
        family = [k for k in _SCRATCH if k[0] == what]
        for k in family[:len(family) - 3]:
            del _SCRATCH[k]
        buf = torch.empty(nbytes, dtype=torch.uint8, device=device)  # (the caching allocator's blocks are 512-byte aligned)
        _SCRATCH[key] = buf
    return buf


def spacing3(spacing) -> Tuple[float, float, float]:
    if spacing is None:
        return (1.0, 1.0, 1.0)
    try:
        spacing = tuple(float(s) for s in spacing)
    except (TypeError, ValueError):
        raise ValueError(f"spacing must be three positive numbers (mm) or None, got {spacing!r}") from None
    if len(spacing) != 3 or not all(math.isfinite(s) and s > 0 for s in spacing):
        raise ValueError(f"spacing must be three positive finite numbers (mm) or None, got {spacing!r}")
    return spacing


def percentile100(percentile) -> float:
    if percentile is None:
        return 100.0  # numpy.percentile at 100 is the maximum
    try:
        percentile = float(percentile)
    except (TypeError, ValueError):
        raise ValueError(f"percentile must be a number in [0, 100] or None, got {percentile!r}") from None
    if not 0.0 <= percentile <= 100.0:
        raise ValueError(f"percentile must be in [0, 100], got {percentile}")
    return percentile


def float3(values):
    return (ctypes.c_float * 3)(*values)


def check_prediction(arg: str, prediction) -> Tuple[int, Tuple[int, int, int]]:
    """(B, dims) of the two-class prediction `prediction` [B,2,X,Y,Z], the caller's argument `arg`."""
    if not isinstance(prediction, torch.Tensor) or prediction.dim() != 5 or prediction.shape[1] != 2:
        raise ValueError(f"expected {arg} [B,2,X,Y,Z], got {tuple(prediction.shape) if isinstance(prediction, torch.Tensor) else type(prediction).__name__}")
    B, _, X, Y, Z = prediction.shape
    return int(B), (int(X), int(Y), int(Z))


def on_device(caller: str, arg: str, prediction: torch.Tensor, label: Optional[torch.Tensor] = None, B=None, dims=None):
    """(channels-last fp32 view [B,X,Y,Z,2] of `prediction`, fp32 contiguous `label` or None) once both are known to lie on one GPU; a `label` is first held to
    [B,1,X,Y,Z], so that a wrong shape is reported wherever the tensors lie."""
    if label is not None and tuple(label.shape) != (B, 1, *dims):
        raise ValueError(f"expected label [B,1,X,Y,Z] = {(B, 1, *dims)}, got {tuple(label.shape)}")
    if not (prediction.is_cuda and (label is None or label.is_cuda)):
        raise RuntimeError(f"vs_seg_amd.{caller} runs on an MI355X only; there is no CPU fallback")
    if label is None:
        return _as_cl(prediction), None  # a view of the sliding window's channels-last output, no copy
    if label.device != prediction.device:
        raise ValueError(f"{arg} on {prediction.device}, label on {label.device}")
    lab = label.detach()
    if lab.dtype != torch.float32 or not lab.is_contiguous():
        lab = lab.to(torch.float32).contiguous()
    return _as_cl(prediction), lab


def each_volume(name: str, B: int, stream, *args) -> None:
    """vsseg_<name>(*args, stream) once per volume b of the batch.  An argument (tensor, n) stands for the address of the tensor's b-th volume of n elements,
    (None, n) for NULL; every other argument goes as it is."""
    fn = getattr(L.lib(), "vsseg_" + name)

    def at(a, b):
        if not isinstance(a, tuple):
            return a
        return None if a[0] is None else a[0].data_ptr() + a[0].element_size() * a[1] * b

    for b in range(B):
        L.check(fn(*[at(a, b) for a in args], stream), name)
