"""fp64 CPU oracle of the region and focal options of the loss (Dice_spvPA(tversky_beta=, focal_tversky_gamma=, batch_dice=, ce_focal_gamma=)), a restatement of their
definition on top of oracle.vsseg_oracle with torch autograd for the gradients:

    I, G, P            the three sums of a ratio (per sample and class for the logits, hardness-weighted when that is on; per level and sample for the attention maps),
                       summed over the samples first with batch_dice
    T                  (2 I + eps) / (2 a_P P + 2 a_G G + eps), eps = 1e-5; (a_P, a_G) = (1 - beta, beta) for the foreground class and the attention maps, (beta, 1 - beta)
                       for the background class
    term               u = 1 - T when gamma == 1, max(u, 1e-7)^gamma otherwise
    loss               mean over the logits ratios + sum over the levels of 1 / L times the mean over the level's ratios
    focal term         + ce_weight * sum w[y] q^gamma_c softplus(z) / W, z = x[1-y] - x[y], q = sigmoid(z), w = (1, w_fg), W = N_bg + w_fg N_fg

and the hand-written value and gradient of the focal term (the formulas of include/vsseg_hip.h, no autograd) so that a CPU test can hold them against autograd."""
import torch
import torch.nn.functional as F

from oracle import vsseg_oracle as O
from tests import ce_oracle as CO

EPS, FLOOR = 1e-5, 1e-7


def ratios_mean(inp, target, w, a_p, a_g, gamma, pooled):
    """Mean of the terms of the ratios of inp / target [B, C, ...]; a_p, a_g: one weight per channel; w: the voxel weight or None."""
    ax = list(range(2, inp.dim()))
    w = torch.ones_like(inp) if w is None else w
    inter, ground, pred = torch.sum(w * target * inp, ax), torch.sum(w * target, ax), torch.sum(w * inp, ax)
    if pooled:
        inter, ground, pred = inter.sum(0, keepdim=True), ground.sum(0, keepdim=True), pred.sum(0, keepdim=True)
    a_p, a_g = torch.tensor(a_p, dtype=inp.dtype), torch.tensor(a_g, dtype=inp.dtype)
    u = 1.0 - (2.0 * inter + EPS) / (2.0 * a_p * pred + 2.0 * a_g * ground + EPS)
    term = u if gamma == 1.0 else torch.clamp(u, min=FLOOR) ** gamma
    return term.mean()


def region_spvpa(logits, att_maps, target, *, supervised_attention=True, hardness_weighting=True, tversky_beta=0.5, focal_tversky_gamma=1.0, batch_dice=False):
    """oracle.vsseg_oracle.dice_spvpa with the ratio above in the place of the Dice ratio."""
    beta, alpha = float(tversky_beta), 1.0 - float(tversky_beta)
    total = torch.zeros((), dtype=logits.dtype)
    if supervised_attention:
        L = len(att_maps)
        g = target
        for level in range(L):
            total = total + ratios_mean(att_maps[L - level - 1], g, None, [alpha], [beta], focal_tversky_gamma, batch_dice) / L
            if level < L - 1:
                cur, nxt = att_maps[L - level - 1].shape, att_maps[L - level - 2].shape
                assert all(a % b == 0 for a, b in zip(cur, nxt))
                ratio = [a // b for a, b in zip(cur, nxt)][2:5]
                g = F.max_pool3d(g, kernel_size=ratio, stride=ratio)
    p, onehot = torch.softmax(logits, 1), O.one_hot(target, 2).to(logits.dtype)
    w = 0.6 * torch.abs(p - onehot) + 0.4 if hardness_weighting else None  # not detached, as in the reference
    return total + ratios_mean(p, onehot, w, [beta, alpha], [alpha, beta], focal_tversky_gamma, batch_dice)


def _softplus(z):
    return torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))


def _z_w(logits, label, w_fg):
    fg = CO.classes(label) == 1
    x0, x1 = logits[:, 0], logits[:, 1]
    z = torch.where(fg, x0 - x1, x1 - x0)
    return fg, z, torch.where(fg, torch.full_like(z, w_fg), torch.ones_like(z))


def focal_ce(logits, label, w_fg, gamma_c):
    """The focal cross-entropy with autograd: sum w q^gamma_c softplus(z) / W, q^gamma_c = exp(-gamma_c softplus(-z))."""
    _, z, w = _z_w(logits, label, w_fg)
    return (w * torch.exp(-gamma_c * _softplus(-z)) * _softplus(z)).sum() / w.sum()


def focal_ce_by_hand(logits, label, w_fg, gamma_c):
    """(value, d value / d logits), no autograd: dz = w / W q^gamma_c (gamma_c (1 - q) softplus(z) + q) to the other class's logit, -dz to the label's own."""
    fg, z, w = _z_w(logits, label, w_fg)
    e = torch.exp(-z.abs())
    q = torch.where(z > 0, 1.0 / (1.0 + e), e / (1.0 + e))
    py = torch.where(z > 0, e / (1.0 + e), 1.0 / (1.0 + e))
    sp, qg = _softplus(z), torch.exp(-gamma_c * _softplus(-z))
    W = w.sum()
    dz = w / W * qg * (gamma_c * py * sp + q)
    c = torch.where(fg, dz, -dz)  # y = 1: the other class is 0
    return (w * qg * sp).sum() / W, torch.stack([c, -c], 1)


def loss_fp64(lg, at, y, *, supervised_attention, hardness_weighting, tversky_beta=None, focal_tversky_gamma=1.0, batch_dice=False, ce_weight=0.0, ce_foreground_weight=1.0,
              ce_focal_gamma=0.0, ce_topk_k=0):
    """The whole loss on fp64 tensors.  tversky_beta None with gamma 1 and no pooling: the reference's Dice ratio.  ce_topk_k: K of the top-k term (0: off)."""
    if tversky_beta is None and focal_tversky_gamma == 1.0 and not batch_dice:
        loss = O.dice_spvpa(lg, at, y, supervised_attention=supervised_attention, hardness_weighting=hardness_weighting)
    else:
        loss = region_spvpa(lg, at, y, supervised_attention=supervised_attention, hardness_weighting=hardness_weighting, tversky_beta=0.5 if tversky_beta is None else tversky_beta,
                            focal_tversky_gamma=focal_tversky_gamma, batch_dice=batch_dice)
    if ce_weight > 0 and ce_focal_gamma > 0:
        loss = loss + ce_weight * focal_ce(lg, y, ce_foreground_weight, ce_focal_gamma)
    elif ce_weight > 0 and ce_topk_k > 0:
        v = F.cross_entropy(lg, CO.classes(y), weight=torch.tensor([1.0, ce_foreground_weight], dtype=lg.dtype), reduction="none")
        loss = loss + ce_weight * v.flatten().topk(ce_topk_k).values.mean()
    elif ce_weight > 0:
        loss = loss + ce_weight * CO.ce_torch(lg, y, ce_foreground_weight)
    return loss


def loss_and_grads(logits, atts, label, **kw):
    """fp64: (loss, d loss / d logits, [d loss / d att_i])."""
    lg = logits.detach().double().cpu().requires_grad_(True)
    at = [a.detach().double().cpu().requires_grad_(True) for a in atts]
    loss = loss_fp64(lg, at, label.detach().double().cpu(), **kw)
    loss.backward()
    return float(loss.detach()), lg.grad, [a.grad if a.grad is not None else torch.zeros_like(a) for a in at]
