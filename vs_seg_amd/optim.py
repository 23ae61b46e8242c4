"""Fused optimisers over the model's flat parameter buffer: one HIP launch instead of 178 per-tensor updates.

`Adam`: semantics = torch.optim.Adam(params, lr, weight_decay) exactly as constructed at ref:params/VSparams.py:388-391 (coupled
L2 decay, bias correction, eps outside the sqrt-of-v̂); `param_groups[i]["lr"]` stays mutable for the halving schedule
(ref:params/VSparams.py:517-523) and `zero_grad()` / `step()` keep their meaning (ref :457, :462).

Beyond the reference: `AdamW` (decoupled decay, torch.optim.AdamW), `SGD` (momentum, Nesterov, torch.optim.SGD with dampening 0) and, on all three,
`max_grad_norm`: the L2 norm of `grad_scale * g` over the whole flat gradient is reduced on the device in a fixed order (fp64, csrc/optim.hip), the coefficient of
torch.nn.utils.clip_grad_norm_ is left in a device record and the update kernel multiplies it in — no host read, `p.grad` itself stays unclipped.  A NaN / Inf norm
skips the update: parameters and optimiser state stay bitwise untouched.  `poly_lr` is the closed form of nnU-Net's polynomial schedule, `check_optimizer` the range
check of the command-line flags.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib as L

OPTIMIZERS = ("adam", "adamw", "sgd")
LR_SCHEDULES = ("halving", "poly")
DEFAULT_MOMENTUM, DEFAULT_POLY_POWER, DEFAULT_WEIGHT_DECAY = 0.99, 0.9, 1e-7


def check_optimizer(optimizer: str = "adam", momentum=None, nesterov: bool = False, weight_decay: float = DEFAULT_WEIGHT_DECAY, clip_grad_norm: float = 0.0, lr_schedule: str = "halving", poly_power=None) -> dict:
    """The optimiser settings as a dict of checked values, or ValueError.  `momentum` / `poly_power` None: not given (0.99 for sgd, 0.9 for poly).  Rejected: an unknown
    optimiser or schedule; momentum outside [0, 1) or not finite; Nesterov without momentum; a clip norm that is negative or not finite (0: off); a poly power that is <= 0
    or not finite; weight decay < 0 or not finite; and the flags that would silently do nothing — momentum or Nesterov with adam / adamw, a poly power without the poly
    schedule."""
    if optimizer not in OPTIMIZERS:
        raise ValueError(f"optimizer must be one of {', '.join(OPTIMIZERS)} (got {optimizer!r})")
    if lr_schedule not in LR_SCHEDULES:
        raise ValueError(f"lr_schedule must be one of {', '.join(LR_SCHEDULES)} (got {lr_schedule!r})")
    try:
        mu = None if momentum is None else float(momentum)
        power = None if poly_power is None else float(poly_power)
        wd, clip = float(weight_decay), float(clip_grad_norm)
    except (TypeError, ValueError):
        raise ValueError(f"momentum, weight_decay, clip_grad_norm and poly_power must be numbers (got {momentum!r}, {weight_decay!r}, {clip_grad_norm!r}, {poly_power!r})") from None
    nesterov = bool(nesterov)
    if optimizer != "sgd":
        if mu is not None:
            raise ValueError(f"momentum = {momentum!r} has no effect with optimizer {optimizer}: it is SGD's (adam / adamw have betas)")
        if nesterov:
            raise ValueError(f"nesterov has no effect with optimizer {optimizer}: give optimizer sgd as well")
        mu = DEFAULT_MOMENTUM  # unused
    else:
        mu = DEFAULT_MOMENTUM if mu is None else mu
        if not (math.isfinite(mu) and 0.0 <= mu < 1.0):
            raise ValueError(f"momentum must be in [0, 1) (got {momentum!r})")
        if nesterov and mu == 0.0:
            raise ValueError("nesterov needs momentum > 0")
    if not (math.isfinite(wd) and wd >= 0.0):
        raise ValueError(f"weight_decay must be finite and >= 0 (got {weight_decay!r})")
    if not (math.isfinite(clip) and clip >= 0.0):
        raise ValueError(f"clip_grad_norm must be finite and >= 0, 0 meaning off (got {clip_grad_norm!r})")
    if lr_schedule != "poly":
        if power is not None:
            raise ValueError(f"poly_power = {poly_power!r} has no effect without lr_schedule poly")
        power = DEFAULT_POLY_POWER
    else:
        power = DEFAULT_POLY_POWER if power is None else power
        if not (math.isfinite(power) and power > 0.0):
            raise ValueError(f"poly_power must be finite and > 0 (got {poly_power!r})")
    return dict(optimizer=optimizer, momentum=mu, nesterov=nesterov, weight_decay=wd, clip_grad_norm=clip, lr_schedule=lr_schedule, poly_power=power)


def poly_lr(lr0: float, epoch: int, num_epochs: int, power: float = DEFAULT_POLY_POWER) -> float:
    """lr0 * (1 - epoch / num_epochs) ** power: the learning rate of epoch `epoch` (0-based) under torch.optim.lr_scheduler.PolynomialLR(total_iters=num_epochs, power)
    stepped once per epoch, and nnU-Net's PolyLRScheduler; 0 from epoch num_epochs on."""
    if num_epochs <= 0:
        raise ValueError(f"num_epochs must be positive (got {num_epochs!r})")
    return float(lr0) * (1.0 - min(int(epoch), int(num_epochs)) / int(num_epochs)) ** float(power)


def _check_max_grad_norm(max_grad_norm):
    if max_grad_norm is None:
        return None
    v = float(max_grad_norm)
    if not (math.isfinite(v) and v > 0.0):
        raise ValueError(f"max_grad_norm must be finite and > 0, or None for no clipping (got {max_grad_norm!r})")
    return v


class _FlatOptimizer(torch.optim.Optimizer):
    """What the fused optimisers share: one flat parameter buffer per group (all of one vs_seg_amd model's parameters), `grad_scale` (multiplied into the gradient
    inside the kernel: the data-parallel mean without an extra pass — DataParallelTrainer sets it to 1 / world and skips its own division), and the gradient-norm
    clipping of `max_grad_norm`.

    Clipping: `step()` launches vsseg_grad_norm on the flat gradient — after the all-reduce, of grad_scale * g, so every rank forms the same bits — and hands the
    device record to the update kernel.  `last_grad_norm` is a device fp64 scalar view of the norm of the last step, `grad_norm_stats()` one host read of the running
    statistics."""

    def __init__(self, params, defaults, max_grad_norm=None):
        self.max_grad_norm = _check_max_grad_norm(max_grad_norm)
        super().__init__(params, defaults)
        name = f"vs_seg_amd.optim.{type(self).__name__}"
        self._owners = []
        for group in self.param_groups:
            owners = {id(getattr(p, "_vsseg_owner", None)): getattr(p, "_vsseg_owner", None) for p in group["params"]}
            if None in owners.values() or len(owners) != 1:
                raise ValueError(f"{name} updates the flat parameter buffer of one vs_seg_amd model per group; use torch.optim.{type(self).__name__} for other parameters")
            owner = next(iter(owners.values()))
            if len(group["params"]) != len(owner._params):
                raise ValueError(f"pass model.parameters() (all of them) to {name}")
            self._owners.append(owner)
        if self.max_grad_norm is not None and len(self.param_groups) != 1:
            raise ValueError(f"{name}: max_grad_norm clips the norm over one parameter group (one model)")
        self.grad_scale = 1.0  # multiplied into the gradient inside the kernel (data-parallel mean without an extra pass)
        self._clip_record = self._clip_scratch = None

    def _measure(self, gflat, stream):
        """Launch the norm of grad_scale * gflat and return the device address of the clip record (None: clipping is off)."""
        if self.max_grad_norm is None:
            return None
        lib = L.lib()
        need = int(lib.vsseg_grad_norm_scratch_bytes(gflat.numel()))
        if need < 0:
            L.check(need, "grad_norm_scratch_bytes")
        if self._clip_record is None or self._clip_record.device != gflat.device:
            self._clip_record = torch.zeros(ctypes.sizeof(L.ClipRecord) // 8, dtype=torch.float64, device=gflat.device)  # vsseg_clip_record, zeroed = statistics reset
        if self._clip_scratch is None or self._clip_scratch.device != gflat.device or self._clip_scratch.numel() * 8 < need:
            self._clip_scratch = torch.empty((need + 7) // 8, dtype=torch.float64, device=gflat.device)
        L.check(lib.vsseg_grad_norm(gflat.data_ptr(), gflat.numel(), float(self.grad_scale), self.max_grad_norm, self._clip_scratch.data_ptr(), self._clip_scratch.numel() * 8,
                                    self._clip_record.data_ptr(), stream), "grad_norm")
        return self._clip_record.data_ptr()

    @property
    def last_grad_norm(self):
        """Device fp64 scalar (a view of the clip record): the L2 norm of grad_scale * g of the last step; None before the first clipped step."""
        return None if self._clip_record is None else self._clip_record[0]

    def grad_norm_stats(self, reset: bool = True) -> dict:
        """steps, clipped (coefficient < 1), skipped (NaN / Inf norm), mean_norm and max_norm over the finite norms since the last reset.  One host read."""
        if self._clip_record is None:
            return dict(steps=0, clipped=0, skipped=0, mean_norm=0.0, max_norm=0.0)
        rec = L.ClipRecord.from_buffer_copy(self._clip_record.cpu().numpy().tobytes())
        if reset:
            self._clip_record.zero_()
        finite = rec.steps - rec.skipped
        return dict(steps=int(rec.steps), clipped=int(rec.clipped), skipped=int(rec.skipped), mean_norm=rec.norm_sum / finite if finite else 0.0, max_norm=float(rec.norm_max))

    def _flat_tensor(self, st, key, flat):
        """A state tensor spanning the whole flat parameter buffer, kept in `Optimizer.state` under the group's first parameter so that `state_dict()` /
        `load_state_dict()` carry it like torch's per-tensor state."""
        t = st.get(key)
        if t is None or t.numel() != flat.numel():
            st[key] = torch.zeros_like(flat)
        elif t.device != flat.device or t.dtype != flat.dtype or t.shape != flat.shape:  # the model moved (or a checkpoint was loaded on another device): keep the values
            st[key] = t.to(flat).reshape(flat.shape)
        return st[key]


class Adam(_FlatOptimizer):
    """torch.optim.Adam over the flat buffer.  With `decoupled_weight_decay=False` and `max_grad_norm=None` (the defaults) `step()` is one vsseg_adam launch, as the
    reference's optimiser needs.  `decoupled_weight_decay=True`: torch.optim.AdamW.  `max_grad_norm`: see _FlatOptimizer; on a skipped step (NaN / Inf norm) the
    parameters and both moments stay untouched, but the host step counter of the bias correction still advances — the host does not know that the step was skipped."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, max_grad_norm=None):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=bool(decoupled_weight_decay)), max_grad_norm)

    def _flat_state(self, group, flat):
        """m / v / step of one group live in `Optimizer.state` under the group's first parameter (flat tensors spanning the whole
        parameter buffer), so `state_dict()` / `load_state_dict()` carry them like torch.optim.Adam's per-tensor moments."""
        st = self.state[group["params"][0]]
        m = st.get("exp_avg")
        if m is None or m.numel() != flat.numel():
            st["step"], st["exp_avg"], st["exp_avg_sq"] = 0, torch.zeros_like(flat), torch.zeros_like(flat)
        elif m.device != flat.device or m.dtype != flat.dtype:  # the model moved (or a checkpoint was loaded on another device): keep the moments
            st["exp_avg"], st["exp_avg_sq"] = m.to(flat), st["exp_avg_sq"].to(flat)
        if torch.is_tensor(st["step"]):
            st["step"] = int(st["step"])
        return st

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        lib = L.lib()
        stream = torch.cuda.current_stream().cuda_stream
        for group, owner in zip(self.param_groups, self._owners):
            flat, gflat = owner.flat_parameters()
            st = self._flat_state(group, flat)
            if all(p.grad is None for p in group["params"]):
                continue
            st["step"] += 1
            b1, b2 = group["betas"]
            t = st["step"]
            decoupled = bool(group.get("decoupled_weight_decay", False))
            if not decoupled and self.max_grad_norm is None:
                L.check(lib.vsseg_adam(flat.data_ptr(), gflat.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), flat.numel(), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                       float(group["weight_decay"]), 1.0 - b1**t, 1.0 - b2**t, float(self.grad_scale), stream), "adam")
            else:
                record = self._measure(gflat, stream)
                L.check(lib.vsseg_adam_clipped(flat.data_ptr(), gflat.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), flat.numel(), float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                                               float(group["weight_decay"]), 1.0 - b1**t, 1.0 - b2**t, float(self.grad_scale), int(decoupled), record, stream), "adam_clipped")
            torch.autograd.graph.increment_version(flat)  # the kernel wrote through the raw pointer: let version-keyed caches (eval weight packing) see it
        return loss


class AdamW(Adam):
    """torch.optim.AdamW over the flat buffer: `Adam` with decoupled weight decay and torch's default decay of 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled_weight_decay=True, max_grad_norm=max_grad_norm)


class SGD(_FlatOptimizer):
    """torch.optim.SGD(lr, momentum, dampening=0, weight_decay, nesterov) over the flat buffer: one vsseg_sgd launch (plus the two of the norm with `max_grad_norm`).
    The momentum buffer lives in `Optimizer.state` under the group's first parameter as `momentum_buffer` (zero-initialised: mu * 0 + g is torch's first step); with
    momentum 0 there is none.  nnU-Net's recipe: SGD(lr 1e-2, momentum 0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=12) with `poly_lr`."""

    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0, nesterov=False, max_grad_norm=None):
        mu = float(momentum)
        if not (math.isfinite(mu) and 0.0 <= mu < 1.0):
            raise ValueError(f"momentum must be in [0, 1) (got {momentum!r})")
        if nesterov and mu == 0.0:
            raise ValueError("nesterov needs momentum > 0")
        super().__init__(params, dict(lr=lr, momentum=mu, weight_decay=weight_decay, nesterov=bool(nesterov)), max_grad_norm)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        lib = L.lib()
        stream = torch.cuda.current_stream().cuda_stream
        for group, owner in zip(self.param_groups, self._owners):
            flat, gflat = owner.flat_parameters()
            if all(p.grad is None for p in group["params"]):
                continue
            mu = float(group["momentum"])
            buf = self._flat_tensor(self.state[group["params"][0]], "momentum_buffer", flat) if mu > 0.0 else None
            record = self._measure(gflat, stream)
            L.check(lib.vsseg_sgd(flat.data_ptr(), gflat.data_ptr(), None if buf is None else buf.data_ptr(), flat.numel(), float(group["lr"]), mu, float(group["weight_decay"]), int(bool(group["nesterov"])),
                                  float(self.grad_scale), record, stream), "sgd")
            torch.autograd.graph.increment_version(flat)
        return loss
