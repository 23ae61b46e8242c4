"""fp64 CPU oracle of the Dice + top-k cross-entropy loss (Dice_spvPA(ce_weight=lam, ce_foreground_weight=w_fg, ce_topk=P)):

    loss = oracle.vsseg_oracle.dice_spvpa(...) + lam * F.cross_entropy(logits, y, weight=[1, w_fg], reduction='none').flatten().topk(K).values.mean()

with K = max(1, floor(N * P / 100)) and torch autograd for the gradients; the hand-written value / gradient of include/vsseg_hip.h (threshold, n_gt, n_eq, tie share),
which is order-independent and defined with ties; the key the radix select ranks a value by; and the select itself by numpy's sort."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vsseg_oracle as O
from tests.ce_oracle import classes


def count(voxels: int, pct: float) -> int:
    return max(1, int(math.floor(voxels * pct / 100.0)))


def values(logits: torch.Tensor, label: torch.Tensor, w_fg: float) -> torch.Tensor:
    """v_i = w[y_i] * (-log softmax(x_i)[y_i]), [B, X, Y, Z]."""
    return F.cross_entropy(logits, classes(label), weight=torch.tensor([1.0, w_fg], dtype=logits.dtype), reduction="none")


def topk_torch(logits: torch.Tensor, label: torch.Tensor, w_fg: float, k: int) -> torch.Tensor:
    return values(logits, label, w_fg).flatten().topk(k).values.mean()


def topk_by_hand(logits: torch.Tensor, label: torch.Tensor, w_fg: float, k: int):
    """(value, d value / d logits, (t, n_gt, n_eq, share), c) by the formulas of include/vsseg_hip.h, no autograd and no sort of the gradient:
    value = (S_gt + (K - n_gt) t) / K; gradient w[y] / K * c * (softmax(x) - onehot(y)) from the other class's probability, c = 1 above t, (K - n_gt) / n_eq at t, 0 below."""
    y = classes(label)
    x0, x1 = logits[:, 0], logits[:, 1]
    fg = y == 1
    z = torch.where(fg, x0 - x1, x1 - x0)
    w = torch.where(fg, torch.full_like(z, w_fg), torch.ones_like(z))
    v = w * (torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs())))
    t = v.flatten().sort(descending=True).values[k - 1]
    n_gt, n_eq = int((v > t).sum()), int((v == t).sum())
    share = (k - n_gt) / n_eq
    c = torch.where(v > t, torch.ones_like(v), torch.where(v == t, torch.full_like(v, share), torch.zeros_like(v)))
    m = torch.maximum(x0, x1)
    e0, e1 = torch.exp(x0 - m), torch.exp(x1 - m)
    p0, p1 = e0 / (e0 + e1), e1 / (e0 + e1)
    g = c * torch.where(fg, w_fg * p0, -p1) / k
    return (v[v > t].sum() + (k - n_gt) * t) / k, torch.stack([g, -g], 1), (float(t), n_gt, n_eq, share), c


def loss_and_grads(logits, atts, label, *, supervised_attention, hardness_weighting, ce_weight, ce_foreground_weight, ce_topk):
    """fp64: (loss, d loss / d logits, [d loss / d att_i], extras).  extras: the Dice-only gradient of the logits, the per-voxel top-k gradient had the voxel been selected
    (c = 1), the values v, the threshold t and K — what a test needs to accept either side for a voxel within rounding of the threshold."""
    lg = logits.detach().double().cpu().requires_grad_(True)
    at = [a.detach().double().cpu().requires_grad_(True) for a in atts]
    y = label.detach().double().cpu()
    k = count(lg.shape[0] * lg[0, 0].numel(), ce_topk)
    dice = O.dice_spvpa(lg, at, y, supervised_attention=supervised_attention, hardness_weighting=hardness_weighting)
    (gdice,) = torch.autograd.grad(dice, lg, retain_graph=True)
    loss = dice + ce_weight * topk_torch(lg, y, ce_foreground_weight, k)
    loss.backward()
    v = values(lg.detach(), y, ce_foreground_weight)
    t = float(v.flatten().topk(k).values[-1])
    p = torch.softmax(lg.detach(), 1)
    fg = classes(y) == 1
    g = ce_weight / k * torch.where(fg, ce_foreground_weight * p[:, 0], -p[:, 1])
    return float(loss.detach()), lg.grad, [a.grad for a in at], dict(dice_grad=gdice, selected_grad=gdice + torch.stack([g, -g], 1), values=v, threshold=t, k=k)


def key_of(values32: np.ndarray) -> np.ndarray:
    """uint32 keys of fp32 values as the select ranks them: the bit pattern, -0 as 0, a NaN as 0xFFFFFFFF."""
    a = np.ascontiguousarray(values32, dtype=np.float32)
    u = a.view(np.uint32).copy()
    u[u == 0x80000000] = 0
    u[np.isnan(a)] = 0xFFFFFFFF
    return u


def select(values32: np.ndarray, k: int):
    """(threshold_bits, n_gt, n_eq) of the k-th largest key, by sorting."""
    u = np.sort(key_of(values32).reshape(-1))
    t = int(u[u.size - k])
    return t, int((u > t).sum()), int((u == t).sum())
