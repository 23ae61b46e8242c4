"""fp64 CPU oracle of the Dice + cross-entropy loss (Dice_spvPA(ce_weight=lam, ce_foreground_weight=w_fg)):

    loss = oracle.vsseg_oracle.dice_spvpa(...) + lam * F.cross_entropy(logits, y, weight=[1, w_fg]),   y = ((int)label == 1)

with torch autograd for the gradients, and the hand-written value / gradient formulas of the kernels (softplus of the logit difference, the gradient from the other
class's probability, the weighted normaliser) so that a CPU test can hold them against F.cross_entropy."""
import torch
import torch.nn.functional as F

from oracle import vsseg_oracle as O

ATT_SHAPES = [(2, 1, 1, 1, 1), (2, 1, 2, 2, 2), (2, 1, 4, 4, 4), (2, 1, 8, 8, 8), (2, 1, 16, 16, 8), (2, 1, 32, 32, 8)]  # the six maps of a (2, 1, 32, 32, 8) label


def classes(label: torch.Tensor) -> torch.Tensor:
    """[B, 1, X, Y, Z] float label -> [B, X, Y, Z] int64 class: 1 where (int)label == 1, else 0 (the cast of the Dice kernels)."""
    return (label[:, 0].to(torch.int64) == 1).to(torch.int64)


def ce_torch(logits: torch.Tensor, label: torch.Tensor, w_fg: float) -> torch.Tensor:
    return F.cross_entropy(logits, classes(label), weight=torch.tensor([1.0, w_fg], dtype=logits.dtype))


def ce_by_hand(logits: torch.Tensor, label: torch.Tensor, w_fg: float):
    """(value, d value / d logits) by the formulas of include/vsseg_hip.h, no autograd: softplus(z) = max(z, 0) + log1p(exp(-|z|)), z = x[1-y] - x[y];
    gradient w[y] / W * (softmax(x) - onehot(y)) formed from the other class's probability; W = N_bg + w_fg * N_fg."""
    y = classes(label)
    x0, x1 = logits[:, 0], logits[:, 1]
    fg = y == 1
    z = torch.where(fg, x0 - x1, x1 - x0)
    v = torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))
    w = torch.where(fg, torch.full_like(z, w_fg), torch.ones_like(z))
    W = w.sum()
    m = torch.maximum(x0, x1)
    e0, e1 = torch.exp(x0 - m), torch.exp(x1 - m)
    p0, p1 = e0 / (e0 + e1), e1 / (e0 + e1)
    c = torch.where(fg, w_fg * p0, -p1) / W
    return (w * v).sum() / W, torch.stack([c, -c], 1)


def loss_and_grads(logits, atts, label, *, supervised_attention, hardness_weighting, ce_weight, ce_foreground_weight):
    """fp64: (loss, d loss / d logits, [d loss / d att_i])."""
    lg = logits.detach().double().cpu().requires_grad_(True)
    at = [a.detach().double().cpu().requires_grad_(True) for a in atts]
    y = label.detach().double().cpu()
    loss = O.dice_spvpa(lg, at, y, supervised_attention=supervised_attention, hardness_weighting=hardness_weighting) + ce_weight * ce_torch(lg, y, ce_foreground_weight)
    loss.backward()
    return float(loss.detach()), lg.grad, [a.grad for a in at]
