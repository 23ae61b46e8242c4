"""`Dice_spvPA` — drop-in for ref:params/losses/dice_spvPA.py:170-297 on fused gfx950 kernels.

loss = sum_l (1/L) Dice(att_{L-1-l}, G_l) + Dice_softmax_onehot(logits, target; weight w),  G_{l+1} = MaxPool3d(G_l),
w = 0.6 |softmax(x) - onehot(target)| + 0.4 (differentiable, ref :279-283).

Forward = label pyramid + per-sample fp64 reductions (logits read once); backward = one elementwise kernel for the
logits and one per supervised attention map.  Returns a 0-dim tensor supporting `.backward()` / `.item()`
(ref call sites: params/VSparams.py:460-463, 488-492).

Beyond the reference: `ce_weight` adds a voxel-wise cross-entropy term on the final logits (MONAI's DiceCELoss, nnU-Net's default loss),
loss += ce_weight * F.cross_entropy(logits, target == 1, weight=[1, ce_foreground_weight]) — one more reduction pass forward, its gradient
formed inside the Dice backward kernel (include/vsseg_hip.h).  0 (the default) issues exactly the launches of the plain Dice loss.
`ce_topk` = P > 0 averages that term over the hardest P percent of the voxels of the batch only (nnU-Net's Dice + TopK loss, DC_and_topk_loss with k = 10):
loss += ce_weight * F.cross_entropy(..., reduction='none').flatten().topk(K).values.mean(), K = max(1, floor(N * P / 100)) — divided by K, not by the class-weight sum.
The K voxels are found by a radix select on the GPU (csrc/topk.hip); the backward compares each voxel's value with the threshold the select left in device memory.

For small lesions (include/vsseg_hip.h states the formulas): `tversky_beta` = beta replaces every Dice ratio by the Tversky index (2I + eps) / (2 a_P P + 2 a_G G + eps) —
beta weights the false negatives, 1 - beta the false positives of the foreground and of the attention maps, mirrored for the background class; beta = 0.5 is the Dice ratio
(Salehi 2017, MONAI's TverskyLoss).  `focal_tversky_gamma` = gamma raises every term to max(1 - T, 1e-7)^gamma (Abraham 2019).  `batch_dice` forms one ratio per class and per
level over the pooled sums of the batch (nnU-Net's batch_dice; the samples of this rank).  `ce_focal_gamma` = gamma_c > 0 weights every voxel of the cross-entropy term by
(1 - p_y)^gamma_c (MONAI's DiceFocalLoss; needs ce_weight > 0, not together with ce_topk).  The region options need no pass of their own — the sums are the same — and the
focal term replaces the plain term's one reduction pass.  With all four at their defaults the launches are exactly those of before.
"""
from __future__ import annotations

import math
from typing import List, Optional, Sequence, Tuple

import torch
from torch.nn.modules.loss import _Loss

from .. import _lib as L


def check_ce(ce_weight: float, ce_foreground_weight: float = 1.0) -> Tuple[float, float]:
    """The two numbers of the cross-entropy term as floats, or ValueError: ce_weight finite and >= 0 (0: the term is off), ce_foreground_weight finite and > 0,
    and not a foreground weight without the term — a flag that would silently do nothing."""
    try:
        lam, wfg = float(ce_weight), float(ce_foreground_weight)
    except (TypeError, ValueError):
        raise ValueError(f"ce_weight and ce_foreground_weight must be numbers (got {ce_weight!r}, {ce_foreground_weight!r})") from None
    if not math.isfinite(lam) or lam < 0:
        raise ValueError(f"ce_weight must be finite and >= 0 (got {ce_weight!r})")
    if not math.isfinite(wfg) or wfg <= 0:
        raise ValueError(f"ce_foreground_weight must be finite and > 0 (got {ce_foreground_weight!r})")
    if lam == 0 and wfg != 1:
        raise ValueError(f"ce_foreground_weight = {ce_foreground_weight!r} has no effect without the cross-entropy term: give ce_weight > 0 as well")
    return lam, wfg


def check_ce_topk(ce_topk: float, ce_weight: float) -> float:
    """The percentage of the top-k cross-entropy term as a float, or ValueError: finite and in [0, 100] (0: off, the mean over every voxel), and not a percentage
    without the term (ce_weight > 0) — a flag that would silently do nothing."""
    try:
        pct, lam = float(ce_topk), float(ce_weight)
    except (TypeError, ValueError):
        raise ValueError(f"ce_topk and ce_weight must be numbers (got {ce_topk!r}, {ce_weight!r})") from None
    if not math.isfinite(pct) or pct < 0 or pct > 100:
        raise ValueError(f"ce_topk must be a percentage in [0, 100] (got {ce_topk!r})")
    if pct > 0 and not lam > 0:
        raise ValueError(f"ce_topk = {ce_topk!r} has no effect without the cross-entropy term: give ce_weight > 0 as well")
    return pct


def check_region(tversky_beta=None, focal_tversky_gamma: float = 1.0, batch_dice: bool = False, ce_focal_gamma: float = 0.0, ce_weight: float = 0.0, ce_topk: float = 0.0):
    """The options for small lesions as (region, ce_focal_gamma), or ValueError.  region is None when every region option is at its default (the reference's Dice ratio per
    sample), else (beta, gamma, pooled) with beta = 0.5 where only the exponent or the pooling was asked for.  tversky_beta in (0, 1), focal_tversky_gamma in [0.25, 4],
    ce_focal_gamma in [0, 5] (0: off), all finite; batch_dice a bool; the focal exponent needs the cross-entropy term (ce_weight > 0) — a flag that would silently do nothing —
    and is refused together with ce_topk: they are two different selections of the hard voxels."""
    try:
        beta = None if tversky_beta is None else float(tversky_beta)
        gamma, gc, lam, pct = float(focal_tversky_gamma), float(ce_focal_gamma), float(ce_weight), float(ce_topk)
    except (TypeError, ValueError):
        raise ValueError(f"tversky_beta, focal_tversky_gamma and ce_focal_gamma must be numbers (got {tversky_beta!r}, {focal_tversky_gamma!r}, {ce_focal_gamma!r})") from None
    if beta is not None and not (math.isfinite(beta) and 0.0 < beta < 1.0):
        raise ValueError(f"tversky_beta must be in (0, 1) (got {tversky_beta!r})")
    if not (math.isfinite(gamma) and 0.25 <= gamma <= 4.0):
        raise ValueError(f"focal_tversky_gamma must be in [0.25, 4] (got {focal_tversky_gamma!r})")
    if not isinstance(batch_dice, (bool, int)) or batch_dice not in (0, 1):
        raise ValueError(f"batch_dice must be True or False (got {batch_dice!r})")
    if not (math.isfinite(gc) and 0.0 <= gc <= 5.0):
        raise ValueError(f"ce_focal_gamma must be in [0, 5] (got {ce_focal_gamma!r})")
    if gc > 0 and not lam > 0:
        raise ValueError(f"ce_focal_gamma = {ce_focal_gamma!r} has no effect without the cross-entropy term: give ce_weight > 0 as well")
    if gc > 0 and pct > 0:
        raise ValueError("ce_focal_gamma and ce_topk are two different selections of the hard voxels: give one of them")
    on = beta is not None or gamma != 1.0 or bool(batch_dice)
    return ((0.5 if beta is None else beta, gamma, bool(batch_dice)) if on else None), gc


def topk_count(voxels: int, ce_topk: float) -> int:
    """K = max(1, floor(N * P / 100)): how many of the N voxels of a batch the top-k term averages over (nnU-Net: int(num_voxels * k / 100))."""
    return min(int(voxels), max(1, int(math.floor(int(voxels) * float(ce_topk) / 100.0))))


def _cl_logits(x: torch.Tensor) -> torch.Tensor:
    """[B,2,X,Y,Z] -> contiguous channels-last [B,X,Y,Z,2] fp32 (zero-copy when the tensor came from vs_seg_amd's network)."""
    v = x.detach().permute(0, 2, 3, 4, 1)
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.to(torch.float32).contiguous()
    return v


def _c1(x: torch.Tensor) -> torch.Tensor:
    v = x.detach()
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.to(torch.float32).contiguous()
    return v


class _State:
    """What the forward leaves for the backward: channels-last logits, labels (full resolution + the pyramid), the coefficients of vsseg_dice_finalize
    (and, with the cross-entropy term, the two of vsseg_dice_ce_finalize or, with ce_topk, the eight of vsseg_dice_ce_topk_finalize; None without it).
    topk_rec: with ce_topk, the first 32 bytes of the select's record as four int64 on the device (threshold_bits | passes_done << 32, n_gt, n_eq, K).
    opts: the vsseg_loss_opts record when a region option or the focal term is on (vsseg_loss_finalize / vsseg_loss_pred_bwd[_to]), else None; npred: the number of
    logits coefficients in front of the attention maps' (6 per sample with a region option, else 4)."""
    __slots__ = ("lg", "lab", "labels", "coef", "ce_coef", "topk", "topk_rec", "hardness", "nl", "shape", "att_shapes", "loss", "opts", "npred")


def _dice_forward(logits, target, supervised, hardness, atts, ce=(0.0, 1.0), ce_topk=0.0, region=None, ce_focal=0.0) -> _State:
    lib = L.lib()
    stream = torch.cuda.current_stream().cuda_stream
    dev = logits.device
    B, Cc, X, Y, Z = logits.shape
    if Cc != 2:
        raise NotImplementedError("Dice_spvPA HIP path: 2-class logits (the configuration VSparams uses)")
    if target.shape != (B, 1, X, Y, Z):
        raise AssertionError(f"ground truth has differing shape ({tuple(target.shape)}) from input ({tuple(logits.shape)})")
    lg, lab = _cl_logits(logits), _c1(target)
    nvox = X * Y * Z
    nl = len(atts) if supervised else 0
    ce_on = ce[0] > 0
    topk_on = ce_on and ce_topk > 0
    nsums = B * 6 + max(nl, 1) * B * 3
    nce = (L.topk_scratch_bytes() // 8 if topk_on else 3) if ce_on else 0  # the three sums of the plain term, or the record and histograms of the select
    sums = torch.empty(nsums + nce, dtype=torch.float64, device=dev)  # [pred | att levels | CE], zeroed through the C ABI (no ATen fill kernels on the step)
    L.check(lib.vsseg_memset_zero(sums.data_ptr(), sums.numel() * 8, stream), "memset_zero")
    pred_sums, att_sums, ce_sums = sums[: B * 6], sums[B * 6 : nsums], sums[nsums:]
    labels: List[torch.Tensor] = []
    plan = _fused_plan(B, (X, Y, Z), [tuple(a.shape) for a in atts], lg, lab, [_c1(a) for a in atts]) if nl else None
    if plan is not None:
        # fewer passes and launches (csrc/loss.hip): a level whose next level pools (2, 2, 1) computes its sums, the logits' sums (finest level) and the next level's label
        # in one pass; the remaining coarse levels are one launch.  Same sums (fixed-point, order-independent up to the fp32 partial sums of a thread).
        g, gdims = lab, (X, Y, Z)
        for level in range(plan):
            ac = _c1(atts[nl - level - 1])
            ndims = tuple(atts[nl - level - 2].shape[2:])
            g2 = torch.empty((B, 1, *ndims), dtype=torch.float32, device=dev)
            L.check(lib.vsseg_dice_level_sums(lg.data_ptr() if level == 0 else None, ac.data_ptr(), g.data_ptr(), B, L.i3(gdims), int(hardness), pred_sums.data_ptr(), att_sums.data_ptr() + 8 * level * B * 3,
                                              g2.data_ptr(), stream), "dice_level_sums")
            labels.append(g)
            g, gdims = g2, ndims
        td = L.DiceTailDesc()
        td.n, td.nlevels, td.src, td.sdims, td.sums = B, nl - plan, g.data_ptr(), L.i3(gdims), att_sums.data_ptr() + 8 * plan * B * 3
        for j, level in enumerate(range(plan, nl)):
            a = atts[nl - level - 1]
            adims = tuple(a.shape[2:])
            assert all(x % y == 0 for x, y in zip(gdims, adims)), "attention-map pyramid must divide (ref dice_spvPA.py:273)"
            gl = g if adims == gdims else torch.empty((B, 1, *adims), dtype=torch.float32, device=dev)
            td.att[j], td.label[j] = _c1(a).data_ptr(), (None if gl is g else gl.data_ptr())
            td.dims[j][0], td.dims[j][1], td.dims[j][2] = adims
            labels.append(gl)
        L.check(lib.vsseg_dice_tail_sums(td, stream), "dice_tail_sums")
    else:
        L.check(lib.vsseg_dice_pred_sums(lg.data_ptr(), 2, lab.data_ptr(), B, nvox, int(hardness), pred_sums.data_ptr(), stream), "dice_pred_sums")
    if nl and plan is None:
        g, gdims = lab, (X, Y, Z)
        for level in range(nl):  # finest attention map first (ref :256-277)
            a = atts[nl - level - 1]
            adims = tuple(a.shape[2:])
            if adims != gdims:
                assert all(x % y == 0 for x, y in zip(gdims, adims)), "attention-map pyramid must divide (ref dice_spvPA.py:273)"
                ratio = tuple(x // y for x, y in zip(gdims, adims))
                g2 = torch.empty((B, 1, *adims), dtype=torch.float32, device=dev)
                L.check(lib.vsseg_maxpool_label(g.data_ptr(), B, L.i3(gdims), L.i3(ratio), g2.data_ptr(), stream), "maxpool_label")
                g, gdims = g2, adims
            ac = _c1(a)
            if tuple(ac.shape) != (B, 1, *adims):
                raise AssertionError(f"ground truth has differing shape ({(B, 1, *gdims)}) from input ({tuple(ac.shape)})")
            L.check(lib.vsseg_dice_att_sums(ac.data_ptr(), g.data_ptr(), B, adims[0] * adims[1] * adims[2], att_sums.data_ptr() + 8 * level * B * 3, stream), "dice_att_sums")
            labels.append(g)
    loss = torch.empty((), dtype=torch.float32, device=dev)  # vsseg_dice_finalize assigns the loss and every coefficient it is asked for
    focal_on = ce_on and ce_focal > 0
    npred = B * 6 if region is not None else B * 4
    coef = torch.empty(npred + max(nl, 1) * B * 2, dtype=torch.float32, device=dev)
    st = _State()
    st.topk, st.topk_rec, st.opts, st.npred = topk_on, None, None, npred
    if region is not None or focal_on:  # the record-driven entry points: any combination of the region options with no / the plain / the top-k / the focal cross-entropy term
        o = st.opts = L.LossOpts()
        if region is not None:
            o.region, o.tversky_beta, o.focal_tversky_gamma, o.batch_dice = 1, region[0], region[1], int(region[2])
        o.ce_mode = (L.CE_FOCAL if focal_on else L.CE_TOPK if topk_on else L.CE_PLAIN) if ce_on else L.CE_NONE
        o.ce_weight, o.ce_foreground_weight, o.ce_focal_gamma = ce[0], ce[1], (ce_focal if focal_on else 0.0)
        if focal_on:  # the plain term's pass with the focal factor: the same three sums
            L.check(lib.vsseg_ce_focal_sums(lg.data_ptr(), 2, lab.data_ptr(), B, nvox, ce_focal, ce_sums.data_ptr(), stream), "ce_focal_sums")
        elif topk_on:
            L.check(lib.vsseg_ce_topk_select(lg.data_ptr(), 2, lab.data_ptr(), B, nvox, ce[1], topk_count(B * nvox, ce_topk), ce_sums.data_ptr(), stream), "ce_topk_select")
            st.topk_rec = ce_sums[:4].view(torch.int64)
        elif ce_on:
            L.check(lib.vsseg_ce_sums(lg.data_ptr(), 2, lab.data_ptr(), B, nvox, ce_sums.data_ptr(), stream), "ce_sums")
        st.ce_coef = torch.empty(8 if topk_on else 2, dtype=torch.float32, device=dev) if ce_on else None
        L.check(lib.vsseg_loss_finalize(pred_sums.data_ptr(), att_sums.data_ptr(), B, nl, ce_sums.data_ptr() if ce_on else None, nvox, o, loss.data_ptr(), coef.data_ptr(),
                                        st.ce_coef.data_ptr() if ce_on else None, stream), "loss_finalize")
    elif topk_on:  # three histogram passes over logits and label leave the threshold, the counts and the sum in ce_sums; the finalize leaves the backward's coefficients
        L.check(lib.vsseg_ce_topk_select(lg.data_ptr(), 2, lab.data_ptr(), B, nvox, ce[1], topk_count(B * nvox, ce_topk), ce_sums.data_ptr(), stream), "ce_topk_select")
        st.ce_coef = torch.empty(8, dtype=torch.float32, device=dev)
        L.check(lib.vsseg_dice_ce_topk_finalize(pred_sums.data_ptr(), att_sums.data_ptr(), B, nl, ce_sums.data_ptr(), ce[0], ce[1], loss.data_ptr(), coef.data_ptr(), st.ce_coef.data_ptr(), stream), "dice_ce_topk_finalize")
        st.topk_rec = ce_sums[:4].view(torch.int64)
    elif ce_on:  # one more pass over logits and label; the finalize decodes its three sums too and leaves the two gradient coefficients on the device
        L.check(lib.vsseg_ce_sums(lg.data_ptr(), 2, lab.data_ptr(), B, nvox, ce_sums.data_ptr(), stream), "ce_sums")
        st.ce_coef = torch.empty(2, dtype=torch.float32, device=dev)
        L.check(lib.vsseg_dice_ce_finalize(pred_sums.data_ptr(), att_sums.data_ptr(), B, nl, ce_sums.data_ptr(), nvox, ce[0], ce[1], loss.data_ptr(), coef.data_ptr(), st.ce_coef.data_ptr(), stream), "dice_ce_finalize")
    else:
        st.ce_coef = None
        L.check(lib.vsseg_dice_finalize(pred_sums.data_ptr(), att_sums.data_ptr(), B, nl, loss.data_ptr(), coef.data_ptr(), stream), "dice_finalize")
    st.lg, st.lab, st.labels, st.coef, st.hardness, st.nl, st.shape = lg, lab, labels, coef, int(hardness), nl, (B, X, Y, Z)
    st.att_shapes = [tuple(a.shape) for a in atts]
    st.loss = loss
    return st


def _fused_plan(B, dims, att_shapes, lg, lab, acs) -> Optional[int]:
    """How many of the finest levels take the fused pass of csrc/loss.hip (vsseg_dice_level_sums: the level is made of 2 x 2 x 4 blocks and the next one pools (2, 2, 1)),
    the rest going to the one tail launch; None when not even the finest level qualifies or a level is too many for the tail (the generic sequence is used)."""
    nl = len(att_shapes)
    if tuple(att_shapes[nl - 1][2:]) != tuple(dims) or any(t.data_ptr() % 16 for t in (lg, lab, *acs)):
        return None
    k, g = 0, tuple(dims)
    while k + 1 < nl:
        nxt = tuple(att_shapes[nl - k - 2][2:])
        if tuple(att_shapes[nl - k - 1][2:]) != g or g[0] % 2 or g[1] % 2 or g[2] % 4 or nxt != (g[0] // 2, g[1] // 2, g[2]) or (B * nxt[0] * nxt[1] * nxt[2]) % 4:
            break
        k, g = k + 1, nxt
    if k == 0 or nl - k > L.DICE_MAX_LEVELS:
        return None
    if any(s[2] * s[3] * s[4] >= (1 << 22) for s in att_shapes[: nl - k]):  # the tail launch takes levels of < 2^22 voxels per sample
        return None
    return k


def _att_backward(st: _State, level: int, gs_ptr, dst: torch.Tensor):
    B = st.shape[0]
    shp = st.att_shapes[st.nl - level - 1]
    L.check(L.lib().vsseg_dice_att_bwd(st.labels[level].data_ptr(), B, shp[2] * shp[3] * shp[4], st.coef.data_ptr() + 4 * (st.npred + level * B * 2), 1.0 / st.nl, gs_ptr, dst.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "dice_att_bwd")


class _DiceFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, supervised, hardness, ce, owner, *atts):
        ctx.st = st = _dice_forward(logits, target, supervised, hardness, atts, ce[:2], ce[2], owner.region, owner.ce_focal_gamma)
        owner.topk_record = st.topk_rec  # (the Dice_spvPA object: the record of its last call, None without ce_topk)
        return st.loss

    @staticmethod
    def backward(ctx, gout):
        lib = L.lib()
        st = ctx.st
        stream = torch.cuda.current_stream().cuda_stream
        B, X, Y, Z = st.shape
        dev = st.lg.device
        gs = gout.detach().to(torch.float32).contiguous()
        dlog = torch.empty((B, X, Y, Z, 2), dtype=torch.float32, device=dev)
        if st.opts is not None:
            L.check(lib.vsseg_loss_pred_bwd(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), None if st.ce_coef is None else st.ce_coef.data_ptr(), st.opts, gs.data_ptr(), dlog.data_ptr(),
                                            stream), "loss_pred_bwd")
        elif st.ce_coef is None:
            L.check(lib.vsseg_dice_pred_bwd(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), gs.data_ptr(), dlog.data_ptr(), stream), "dice_pred_bwd")
        elif st.topk:
            L.check(lib.vsseg_dice_ce_topk_pred_bwd(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), st.ce_coef.data_ptr(), gs.data_ptr(), dlog.data_ptr(), stream), "dice_ce_topk_pred_bwd")
        else:
            L.check(lib.vsseg_dice_ce_pred_bwd(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), st.ce_coef.data_ptr(), gs.data_ptr(), dlog.data_ptr(), stream), "dice_ce_pred_bwd")
        datts: List[Optional[torch.Tensor]] = [None] * len(st.att_shapes)
        for level in range(st.nl):
            i = st.nl - level - 1
            d = torch.empty(st.att_shapes[i], dtype=torch.float32, device=dev)
            _att_backward(st, level, gs.data_ptr(), d)
            datts[i] = d
        return (dlog.permute(0, 4, 1, 2, 3), None, None, None, None, None, *datts)


class Dice_spvPA(_Loss):
    def __init__(self, include_background: bool = True, to_onehot_y: bool = False, sigmoid: bool = False, softmax: bool = False, other_act=None, squared_pred: bool = False,
                 jaccard: bool = False, reduction="mean", supervised_attention=True, hardness_weighting=True, ce_weight: float = 0.0, ce_foreground_weight: float = 1.0,
                 ce_topk: float = 0.0, tversky_beta: Optional[float] = None, focal_tversky_gamma: float = 1.0, batch_dice: bool = False, ce_focal_gamma: float = 0.0) -> None:
        super().__init__(reduction=getattr(reduction, "value", reduction))
        if other_act is not None and not callable(other_act):
            raise TypeError(f"other_act must be None or callable but is {type(other_act).__name__}.")
        if int(sigmoid) + int(softmax) + int(other_act is not None) > 1:
            raise ValueError("Incompatible values: more than 1 of [sigmoid=True, softmax=True, other_act is not None].")
        self.ce_weight, self.ce_foreground_weight = check_ce(ce_weight, ce_foreground_weight)  # beyond the reference: + ce_weight * cross-entropy on the final logits
        self.ce_topk = check_ce_topk(ce_topk, self.ce_weight)  # ... over the hardest ce_topk percent of the voxels only (0: over all of them)
        # for small lesions: the Tversky ratio, its focal exponent, one ratio over the batch, the focal cross-entropy (region: None with the first three at their defaults)
        self.region, self.ce_focal_gamma = check_region(tversky_beta, focal_tversky_gamma, batch_dice, ce_focal_gamma, self.ce_weight, self.ce_topk)
        self.tversky_beta, self.focal_tversky_gamma, self.batch_dice = (None, 1.0, False) if self.region is None else self.region
        self.topk_record = None  # with ce_topk: the select's record of the last call (device tensor of four int64: threshold_bits | passes_done << 32, n_gt, n_eq, K)
        # the reference's Dice_spvPA.forward ignores every option except the two below (it builds its inner Dice objects with fixed options)
        self.include_background, self.to_onehot_y, self.sigmoid, self.softmax = include_background, to_onehot_y, sigmoid, softmax
        self.other_act, self.squared_pred, self.jaccard = other_act, squared_pred, jaccard
        self.supervised_attention = supervised_attention
        self.hardness_weighting = hardness_weighting

    def forward(self, input, target: torch.Tensor, smooth: float = 1e-5) -> torch.Tensor:
        x, att_maps = input
        if not x.is_cuda:
            raise RuntimeError("vs_seg_amd.Dice_spvPA runs on an MI355X only (got a CPU tensor); there is no CPU fallback")
        if smooth != 1e-5:
            raise NotImplementedError("smooth is fixed at 1e-5 (the value the reference always uses)")
        atts: Sequence[torch.Tensor] = list(att_maps) if self.supervised_attention else []
        return _DiceFn.apply(x, target, bool(self.supervised_attention), bool(self.hardness_weighting), (self.ce_weight, self.ce_foreground_weight, self.ce_topk), self, *atts)

    def forward_backward_into(self, input, target: torch.Tensor, landing):
        """The loss AND its gradients in one call, outside autograd (the fused train step of vs_seg_amd.parallel.DataParallelTrainer): d(loss)/d(logits) and
        d(loss)/d(att_i) are written where `landing` says — `(descriptor of the staged gradient of the logits, [fp32 buffer per attention map or None])`, as
        UNet2d5_spvPA.train_forward_landing hands it out — in the layout and dtype the network's backward reads, instead of fp32 tensors that the backward
        would copy and cast (7 passes per step).  The values are those of `loss.backward()` (upstream gradient 1).  Returns (loss, indices of the attention
        maps whose buffer was written)."""
        x, att_maps = input
        if not x.is_cuda:
            raise RuntimeError("vs_seg_amd.Dice_spvPA runs on an MI355X only (got a CPU tensor); there is no CPU fallback")
        atts: Sequence[torch.Tensor] = list(att_maps) if self.supervised_attention else []
        glogits_dst, gatt_bufs = landing
        with torch.no_grad():
            st = _dice_forward(x, target, bool(self.supervised_attention), bool(self.hardness_weighting), atts, (self.ce_weight, self.ce_foreground_weight), self.ce_topk, self.region, self.ce_focal_gamma)
            self.topk_record = st.topk_rec
            B, X, Y, Z = st.shape
            stream = torch.cuda.current_stream().cuda_stream
            if st.opts is not None:
                L.check(L.lib().vsseg_loss_pred_bwd_to(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), None if st.ce_coef is None else st.ce_coef.data_ptr(), st.opts, None, glogits_dst,
                                                       stream), "loss_pred_bwd_to")
            elif st.ce_coef is None:
                L.check(L.lib().vsseg_dice_pred_bwd_to(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), None, glogits_dst, stream), "dice_pred_bwd_to")
            elif st.topk:
                L.check(L.lib().vsseg_dice_ce_topk_pred_bwd_to(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), st.ce_coef.data_ptr(), None, glogits_dst, stream), "dice_ce_topk_pred_bwd_to")
            else:
                L.check(L.lib().vsseg_dice_ce_pred_bwd_to(st.lg.data_ptr(), 2, st.lab.data_ptr(), B, X * Y * Z, st.hardness, st.coef.data_ptr(), st.ce_coef.data_ptr(), None, glogits_dst, stream), "dice_ce_pred_bwd_to")
            written, coarse = [], []
            for level in range(st.nl):
                i = st.nl - level - 1
                buf = gatt_bufs[i]
                if buf is None:
                    continue  # this map has no gradient path in the network
                nv = st.att_shapes[i][2] * st.att_shapes[i][3] * st.att_shapes[i][4]
                if buf.numel() != B * nv or buf.dtype != torch.float32:
                    raise AssertionError(f"gradient buffer of attention map {i} does not match its shape {st.att_shapes[i]}")
                if nv * B >= (1 << 22) or len(coarse) == L.DICE_MAX_LEVELS:
                    _att_backward(st, level, None, buf)  # a level large enough to fill the GPU: its own launch
                else:
                    coarse.append((level, buf, nv))
                written.append(i)
            if coarse:  # the coarse levels: one launch
                bd = L.DiceBwdLevelsDesc()
                bd.n, bd.nlevels, bd.gscale = B, len(coarse), None
                for j, (level, buf, nv) in enumerate(coarse):
                    bd.label[j], bd.datt[j], bd.nvox[j] = st.labels[level].data_ptr(), buf.data_ptr(), nv
                    bd.coef[j] = st.coef.data_ptr() + 4 * (st.npred + level * B * 2)
                L.check(L.lib().vsseg_dice_att_bwd_levels(bd, stream), "dice_att_bwd_levels")
        return st.loss, written
