"""fp64 definitions of the Dice loss kernels (csrc/loss.hip), a restatement of their launch arithmetic, the case tables of tests/test_gpu_dice.py and the bars it
holds the kernels to.  Nothing of the package under test is imported here: torch, numpy, and the suite's own helpers.  tests/test_dice_host.py ties the definitions
to oracle.vsseg_oracle (dice, dice_spvpa and autograd of them), the restated constants to the source text, every case row to the path it declares, and plants faults.

Layouts (the C ABI's, voxel axes flattened): logits [B, nvox, 2], label and attention map [B, nvox]; everything fp64 unless said otherwise.

    p = softmax(l)            g_c = [(int)label == c]            w_c = 0.6 |p_c - g_c| + 0.4 with hardness weighting, else 1
    (I_c, G_c, P_c) = sum_v (w_c g_c p_c,  w_c g_c,  w_c p_c)                                   per sample: six sums, order (I0, G0, P0, I1, G1, P1)
    (I, G, P)       = sum_v (G_l a,  G_l,  a)     G_0 = label, G_{l+1} = MaxPool3d(ratio)(G_l)   per level and sample
    f = 1 - (2 I + eps) / (G + P + eps)           loss = sum_{b,c} f / (2 n) + sum_{l,b} f / (L n)
    coef = (df/dI, df/dG) * weight = (-2 / D, (2 I + eps) / D^2) * weight,  D = G + P + eps      prediction block [b][c][2], then [l][b][2]
    d loss / d p_c = A_c g_c t_c + B_c (g_c s_c + t_c),   s_c = 0.6 sign(p_c - g_c),  t_c = w_c + p_c s_c         (s = 0, t = 1 without hardness)
    d loss / d l_c = p_c (dp_c - sum_k dp_k p_k)          d loss / d a = A G_l + B
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.helpers import synth_input

F64 = torch.float64
U24, U23 = 2.0 ** -24, 2.0 ** -23  # half an fp32 ulp (one rounding, relative) / one ulp
SMOOTH = 1e-5
FX_DICE = 2.0 ** 32  # csrc/loss.hip VSSEG_FX_DICE: the sums are 64-bit integers of this scale
FX_STAT = 2.0 ** 20  # csrc/common.h VSSEG_FX_STAT: the scale of vsseg_ce_sums


# ---------------------------------------------------------------------------------------------------------------------------------------------
# definitions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def onehot(label):
    """[...] float label -> (g0, g1): the cast of the kernels, (int)label == c."""
    cls = label.to(torch.int64)
    return (cls == 0).to(F64), (cls == 1).to(F64)


def softmax2(logits):
    l0, l1 = logits[..., 0].to(F64), logits[..., 1].to(F64)
    m = torch.maximum(l0, l1)
    e0, e1 = torch.exp(l0 - m), torch.exp(l1 - m)
    return e0 / (e0 + e1), e1 / (e0 + e1)


def pred_terms(logits, label, hardness):
    """The six terms of every voxel, [B, nvox, 6] (all >= 0: the sum of their magnitudes is their sum)."""
    (p0, p1), (g0, g1) = softmax2(logits), onehot(label)
    w0 = 0.6 * (p0 - g0).abs() + 0.4 if hardness else torch.ones_like(p0)
    w1 = 0.6 * (p1 - g1).abs() + 0.4 if hardness else torch.ones_like(p1)
    return torch.stack([w0 * g0 * p0, w0 * g0, w0 * p0, w1 * g1 * p1, w1 * g1, w1 * p1], -1)


def pred_sums(logits, label, hardness):
    """[B, 6] = (I0, G0, P0, I1, G1, P1) per sample."""
    return pred_terms(logits, label, hardness).sum(1)


def pool(label5, ratio):
    """MaxPool3d(ratio) of a [B, 1, X, Y, Z] label."""
    ratio = tuple(int(r) for r in ratio)
    return F.max_pool3d(label5.to(F64), kernel_size=ratio, stride=ratio)


def pyramid_labels(label5, level_dims):
    """G_l for level dims listed finest first: each level pools the previous one by the per-axis ratio (1, 1, 1 where the dims repeat)."""
    out, g = [], label5.to(F64)
    for d in level_dims:
        cur = tuple(g.shape[2:])
        assert all(c % t == 0 for c, t in zip(cur, d)), f"{cur} -> {tuple(d)} does not divide"
        if tuple(d) != cur:
            g = pool(g, [c // t for c, t in zip(cur, d)])
        out.append(g)
    return out


def pool_from(src5, dims):
    """The tail launch's label: level dims straight from the source (a max-pool of a max-pool is the max-pool over the product window)."""
    cur = tuple(src5.shape[2:])
    return src5.to(F64) if tuple(dims) == cur else pool(src5, [c // t for c, t in zip(cur, dims)])


def att_sums(att, g):
    """[B, 3] = (I, G, P) of an attention map [B, nvox] against its level's label [B, nvox]."""
    att, g = att.to(F64).reshape(att.shape[0], -1), g.to(F64).reshape(g.shape[0], -1)
    return torch.stack([(g * att).sum(1), g.sum(1), att.sum(1)], 1)


def finalize(psums, asums=None):
    """psums [B, 6], asums [L, B, 3] or None -> (loss, coef): coef in the layout of dice_finalize_kernel, B*4 + max(L, 1)*B*2 numbers, the prediction block
    [b][c][2] then [l][b][2], with 1/(2n) and 1/(L n) folded in (the last B*2 are unused and left 0 when L = 0)."""
    n = psums.shape[0]
    nl = 0 if asums is None else asums.shape[0]
    coef = torch.zeros(n * 4 + max(nl, 1) * n * 2, dtype=F64)
    total = torch.zeros((), dtype=F64)
    s = psums.to(F64).reshape(n, 2, 3)
    D, num, wgt = s[..., 1] + s[..., 2] + SMOOTH, 2.0 * s[..., 0] + SMOOTH, 1.0 / (2.0 * n)
    total = total + (wgt * (1.0 - num / D)).sum()
    coef[: n * 4] = torch.stack([-2.0 / D * wgt, num / (D * D) * wgt], -1).reshape(-1)
    if nl:
        a = asums.to(F64)
        D, num, wgt = a[..., 1] + a[..., 2] + SMOOTH, 2.0 * a[..., 0] + SMOOTH, 1.0 / (float(nl) * n)
        total = total + (wgt * (1.0 - num / D)).sum()
        coef[n * 4:] = torch.stack([-2.0 / D * wgt, num / (D * D) * wgt], -1).reshape(-1)
    return total, coef


def dlogits(logits, label, hardness, coef_pred, gs=1.0):
    """d loss / d logits [B, nvox, 2] from the prediction block of the coefficients ([B*4] or [B, 2, 2]) and the upstream gradient gs."""
    (p0, p1), (g0, g1) = softmax2(logits), onehot(label)
    c = coef_pred.to(F64).reshape(-1, 2, 2) * float(gs)
    A0, B0, A1, B1 = (c[:, i, j].reshape(-1, 1) for i in (0, 1) for j in (0, 1))
    if hardness:
        d0, d1 = p0 - g0, p1 - g1
        w0, w1 = 0.6 * d0.abs() + 0.4, 0.6 * d1.abs() + 0.4
        s0, s1 = 0.6 * torch.sign(d0), 0.6 * torch.sign(d1)
    else:
        w0, w1, s0, s1 = torch.ones_like(p0), torch.ones_like(p1), torch.zeros_like(p0), torch.zeros_like(p1)
    t0, t1 = w0 + p0 * s0, w1 + p1 * s1
    dp0 = A0 * g0 * t0 + B0 * (g0 * s0 + t0)
    dp1 = A1 * g1 * t1 + B1 * (g1 * s1 + t1)
    dot = dp0 * p0 + dp1 * p1
    return torch.stack([p0 * (dp0 - dot), p1 * (dp1 - dot)], -1)


def datt(g, coef_level, gs=1.0):
    """d loss / d att [B, nvox] = A G + B from one level's [B, 2] slice of the coefficients."""
    c = coef_level.to(F64).reshape(-1, 2) * float(gs)
    return c[:, :1] * g.to(F64).reshape(c.shape[0], -1) + c[:, 1:]


def datt_fp32(g, coef_level32, gs32=None):
    """The same as the kernels round it: fl32(fl32(A gs) g + fl32(B gs)) from the fp32 coefficients on the device.  With g in {0, 1} the product is exact,
    so a fused multiply-add and a separate multiply and add give the same bits."""
    c = coef_level32.detach().cpu().to(torch.float32).reshape(-1, 2)
    if gs32 is not None:
        c = c * torch.tensor(gs32, dtype=torch.float32)
    g = g.detach().cpu().to(torch.float32).reshape(c.shape[0], -1)
    assert bool(((g == 0) | (g == 1)).all())
    return c[:, :1] * g + c[:, 1:]


def argmax2(logits):
    """[..., 2] -> int64 class: 1 where l1 > l0, else 0 — ties, and a NaN in either logit, go to class 0."""
    return (logits[..., 1] > logits[..., 0]).to(torch.int64)


def hard_counts(logits, label):
    """(|pred & label|, |pred|, |label|) over every voxel."""
    pr, (_, g1) = argmax2(logits).to(F64), onehot(label)
    return torch.stack([(pr * g1).sum(), pr.sum(), g1.sum()])


def loss_by_hand(logits5, atts, label5, supervised, hardness):
    """(loss, d logits [B, 2, X, Y, Z], [d att_i in the order of atts]) of Dice_spvPA from the definitions above, no autograd.  atts: coarsest first."""
    B = logits5.shape[0]
    lg = logits5.to(F64).permute(0, 2, 3, 4, 1).reshape(B, -1, 2)
    lab = label5.to(F64).reshape(B, -1)
    nl = len(atts) if supervised else 0
    labels = pyramid_labels(label5, [tuple(atts[nl - l - 1].shape[2:]) for l in range(nl)])
    asums = torch.stack([att_sums(atts[nl - l - 1], labels[l]) for l in range(nl)]) if nl else None
    loss, coef = finalize(pred_sums(lg, lab, hardness), asums)
    dl = dlogits(lg, lab, hardness, coef[: B * 4]).reshape(B, *logits5.shape[2:], 2).permute(0, 4, 1, 2, 3)
    da = [None] * len(atts)
    for l in range(nl):
        i = nl - l - 1
        da[i] = datt(labels[l], coef[B * 4 + l * B * 2: B * 4 + (l + 1) * B * 2]).reshape(atts[i].shape)
    return loss, dl, da


# ---------------------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic, READ FROM csrc/loss.hip and csrc/common.h (grid_for) and losses/dice_spvPA.py (_fused_plan).  A restatement for the case audit, not a
# second source of truth: tests/test_dice_host.py reads the constants back from the source text, and whoever retunes a launch there updates it here.
# ---------------------------------------------------------------------------------------------------------------------------------------------
DICE_THREADS = 512
DICE_TAIL_THREADS = 1024
TAIL_BLOCK_CAP = 48         # workgroups per level of the tail launch
TAIL_VOX_PER_BLOCK = 8192   # ... one per this many voxels where the level is the source level (win == 1)
TAIL_LANES_PER_BLOCK = 2048  # ... one per this many lanes (voxels * T) where it pools
BWD_LEVELS_BLOCK_CAP = 256  # workgroups per level of vsseg_dice_att_bwd_levels, one per BWD_LEVELS_VOX voxels
BWD_LEVELS_VOX = 2048
BWD_THREADS, BWD_GRID_CAP = 256, 2048  # dice_pred_bwd_kernel / dice_att_bwd_kernel: grid_for((nvox + 3) / 4, 256, 2048)
DICE_MAX_LEVELS = 8
TAIL_MAX_VOX = 1 << 22


def grid_for(items, block, cap=256 * 16):
    return max(1, min((items + block - 1) // block, cap))


def dice_blocks(items, n):
    want = (items + DICE_THREADS * 2 - 1) // (DICE_THREADS * 2)
    cap = 1 if n >= 512 else 512 // n
    return max(1, min(want, cap))


def vec16(nvox, pitch=2, ptrs=()):
    """The condition of the 16-byte path of the sums and backward kernels: pitch 2, nvox a multiple of 4, every base pointer 16-byte aligned."""
    return pitch == 2 and nvox % 4 == 0 and all(p % 16 == 0 for p in ptrs)


def sums_launch(nvox, n, pitch=2, ptrs=()):
    """vsseg_dice_pred_sums / vsseg_dice_att_sums / vsseg_ce_sums: workgroups per sample, the path, and the grid-stride rounds of the busiest thread."""
    blocks = dice_blocks(nvox // 4, n)
    vec = vec16(nvox, pitch, ptrs)
    items = nvox // 4 if vec else nvox
    return {"blocks": blocks, "cap": 1 if n >= 512 else 512 // n, "vector": vec, "rounds": -(-items // (blocks * DICE_THREADS)), "workgroups": blocks}


def level_launch(dims, n):
    """vsseg_dice_level_sums: a thread owns a 2 x 2 x 4 block."""
    items = (dims[0] // 2) * (dims[1] // 2) * (dims[2] // 4)
    blocks = dice_blocks(items * 2, n)
    return {"items": items, "blocks": blocks, "rounds": -(-items // (blocks * DICE_THREADS)), "workgroups": blocks}


def tail_plan(sdims, levels):
    """vsseg_dice_tail_sums: per level the window, the lanes T that share it, voxels per workgroup and round, workgroups, whether the win == 1 loop can take
    16-byte loads (aligned pointers assumed), and first[]."""
    out, first, nb = [], [], 0
    for d in levels:
        assert all(s % t == 0 for s, t in zip(sdims, d))
        win = math.prod(s // t for s, t in zip(sdims, d))
        nvox = math.prod(d)
        T = 1
        while T < 64 and T * 2 <= win:
            T *= 2
        blocks = min(TAIL_BLOCK_CAP, -(-nvox // TAIL_VOX_PER_BLOCK) if win == 1 else -(-nvox * T // TAIL_LANES_PER_BLOCK))
        first.append(nb)
        nb += blocks
        vpb = DICE_TAIL_THREADS // T
        vec = win == 1 and nvox % 4 == 0
        rounds = -(-(nvox // 4) // (blocks * DICE_TAIL_THREADS)) if vec else -(-nvox // (blocks * vpb * 4))
        # workgroup lb starts at item lb * 1024 of nvox / 4 (16-byte loop) or at voxel lb * vpb * 4: `busy` of the level's workgroups have anything to do
        busy = min(blocks, -(-(nvox // 4) // DICE_TAIL_THREADS) if vec else -(-nvox // (vpb * 4)))
        out.append({"win": win, "T": T, "vpb": vpb, "blocks": blocks, "busy": busy, "nvox": nvox, "vector": vec, "rounds": rounds})
    first += [nb] * (DICE_MAX_LEVELS + 1 - len(levels))
    return out, first


def bwd_launch(nvox, pitch=2, ptrs=()):
    """dice_pred_bwd_kernel / dice_att_bwd_kernel: grid, path and the rounds of the busiest thread."""
    grid = grid_for((nvox + 3) // 4, BWD_THREADS, BWD_GRID_CAP)
    vec = vec16(nvox, pitch, ptrs)
    return {"grid": grid, "vector": vec, "rounds": -(-(nvox // 4 if vec else nvox) // (grid * BWD_THREADS))}


def bwd_levels_blocks(nvox):
    return min(BWD_LEVELS_BLOCK_CAP, -(-nvox // BWD_LEVELS_VOX))


def fused_plan(B, dims, att_dims, aligned=True):
    """losses/dice_spvPA.py `_fused_plan` for a pyramid (att_dims: (X, Y, Z) per map, coarsest first): how many of the finest levels take the fused pass, or None."""
    nl = len(att_dims)
    if tuple(att_dims[nl - 1]) != tuple(dims) or not aligned:
        return None
    k, g = 0, tuple(dims)
    while k + 1 < nl:
        nxt = tuple(att_dims[nl - k - 2])
        if tuple(att_dims[nl - k - 1]) != g or g[0] % 2 or g[1] % 2 or g[2] % 4 or nxt != (g[0] // 2, g[1] // 2, g[2]) or (B * math.prod(nxt)) % 4:
            break
        k, g = k + 1, nxt
    if k == 0 or nl - k > DICE_MAX_LEVELS:
        return None
    if any(math.prod(s) >= TAIL_MAX_VOX for s in att_dims[: nl - k]):
        return None
    return k


# ---------------------------------------------------------------------------------------------------------------------------------------------
# bars
# ---------------------------------------------------------------------------------------------------------------------------------------------
# Per-term relative error of dice_pred_terms for a case whose largest |l0 - l1| is d, from named pieces.  __expf(x) is v_exp_f32(fl(log2e) * x) (hip math
# header), x = l - max(l0, l1): 0 for the larger logit (e = 1 exactly), -|l0 - l1| for the other.
def e_arg(d):
    """Relative error of e_other from its argument: the rounding of l - m, the fp32 constant log2 e and the rounding of their product each move the argument of 2^x
    by at most 2^-24 |x log2 e|, i.e. e by the relative amount 2^-24 |x| <= 2^-24 d."""
    return 3.0 * U24 * d


E_EXP = U23  # v_exp_f32: 1 ulp
E_RCP = U23  # 1.f / x: held to 1 ulp (the build's division is correctly rounded: 1/2 ulp)
ABS_E = 3.0 * U24 / math.e + E_EXP  # ABSOLUTE error of e_other = e * (e_arg(|x|) + E_EXP) <= max_x (x exp(-x)) * 3 * 2^-24 + 2^-23, whatever d
REL_SUM = ABS_E + 2.0 * U24         # e0 + e1 in [1, 2]: one of them is exactly 1, the other off by ABS_E, one rounding of a number <= 2; relative to a sum >= 1
REL_INV = REL_SUM + E_RCP
ABS_P = ABS_E + REL_INV + U24       # absolute error of either p: p_max = 1 * inv (exact product); p_other = e * inv <= 1/2
ABS_W = 0.6 * (ABS_P + U24) + (0.6 + 1.0 + 0.4 + 1.0) * U24  # w = 0.6f * |p - g| + 0.4f: the subtraction, the two constants, the product and the sum (all <= 1)
REL_W = ABS_W / 0.4                 # w >= 0.4
CHAIN = 15.0 * U24                  # fp32 adds of a thread's terms before they go to fp64: 16 voxels in the level kernel (4 in the 16-byte loop, 1 in the scalar loop)


def rel_p(d):
    """Relative error of a probability: p_other = e_other * inv carries e_other's relative error, the reciprocal's and one product."""
    return e_arg(d) + E_EXP + REL_INV + U24


def rel_term(d, hardness):
    """Relative error of one summand w g p (the largest of the three kinds), with the fp32 chain it is added in."""
    return (REL_W if hardness else 0.0) + rel_p(d) + 2.0 * U24 + CHAIN


def max_logit_gap(logits):
    return float((logits[..., 0].to(F64) - logits[..., 1].to(F64)).abs().max())


def sum_bound(logits, label, hardness, workgroups):
    """Bar of the six prediction sums, [B, 6]: (per-term relative error at the case's largest |l0 - l1|) * sum|term| + workgroups * 2^-33 (each workgroup's
    partial sum is rounded once to the 2^-32 grid).  fp64 accumulation of at most 2^22 fp32 partials adds below 2^-30 relative: folded into the chain piece."""
    terms = pred_terms(logits, label, hardness)
    return rel_term(max_logit_gap(logits), hardness) * terms.abs().sum(1) + workgroups * 2.0 ** -33


def ce_bound(logits, label, workgroups):
    """Bar of (S_bg, S_fg) of vsseg_ce_sums where this suite launches it for its launch shape.  Per voxel, v = max(z, 0) + log1p(exp(-|z|)), absolute: 2^-24 |z|
    (z), e off by ABS_E and 1 + e rounded (2 * 2^-24) under a log of slope <= 1, v_log_f32 1 ulp of a log2 <= 1 and the ln 2 product (3 * 2^-24), the two-term
    series below 2^-12 (smaller), the final sum 2^-24 v; then three fp32 adds of four voxels' values and 2^-21 per workgroup (2^-20 grid)."""
    z = (logits[..., 0].to(F64) - logits[..., 1].to(F64)).abs()
    fg = onehot(label)[1]
    per = U24 * z + ABS_E + 2 * U24 + 3 * U24 + U24 * (z + 1.0) + 3 * U24 * (z + 1.0)
    return torch.stack([(per * (1 - fg)).sum(), (per * fg).sum()]) + workgroups * 2.0 ** -21


def ce_sums(logits, label):
    """(S_bg, S_fg, N_fg) over the whole batch."""
    l0, l1 = logits[..., 0].to(F64), logits[..., 1].to(F64)
    fg = onehot(label)[1]
    z = torch.where(fg == 1, l0 - l1, l1 - l0)
    v = torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))
    return torch.stack([(v * (1 - fg)).sum(), (v * fg).sum(), fg.sum()])


def fx_encode(x, scale=FX_DICE):
    """Real numbers -> the int64 pattern vsseg_fx_add leaves (round to nearest on the grid of the scale), as an int64 tensor."""
    return torch.round(torch.as_tensor(x, dtype=F64) * scale).to(torch.int64)


def fx_decode(i, scale=FX_DICE):
    return i.to(torch.int64).to(F64) / scale


def ulp32(x):
    """Spacing of the fp32 numbers at |x| (fp64 tensor in, fp64 out)."""
    x = np.asarray(x, dtype=np.float64)
    a = np.abs(np.atleast_1d(x)).astype(np.float32)
    return torch.from_numpy(np.spacing(np.maximum(a, np.float32(2.0 ** -126))).astype(np.float64)).reshape(x.shape)


def loss_bound(psums, pbound, asums=None):
    """Bar of the loss where a Dice denominator is small: the finalisation evaluated at sums +- bound.  f = 1 - (2I + eps) / (G + P + eps) is monotone in each sum
    (falling in I, rising in G and P), so the extremes are at the corners; attention sums are exact.  Plus one fp32 rounding of the loss."""
    lo, _ = finalize((psums + pbound * torch.tensor([1.0, -1.0, -1.0] * 2, dtype=F64)).clamp(min=0.0), asums)
    hi, _ = finalize((psums + pbound * torch.tensor([-1.0, 1.0, 1.0] * 2, dtype=F64)).clamp(min=0.0), asums)
    mid, _ = finalize(psums, asums)
    return float(torch.maximum(hi - mid, mid - lo)) + U24 * abs(float(mid)) + 2.0 ** -60


# ---------------------------------------------------------------------------------------------------------------------------------------------
# comparison helpers (the GPU test uses exactly these; tests/test_dice_host.py plants faults against them)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _first_mismatches(got, want, bad, k=4):
    """'(sample, level, voxel, got, want)' of the first few bad elements of a [sample, level, voxel]-shaped comparison."""
    idx = torch.nonzero(bad.reshape(bad.shape))[:k]
    return "; ".join(f"(sample {int(i[0])}, level {int(i[1])}, voxel {int(i[2])}, got {got[tuple(i)].item()!r}, want {want[tuple(i)].item()!r})" for i in idx)


def _as3(t, level):
    """A [sample, ...] tensor as [sample, 1, voxel]; `level` only names the level in the message."""
    return t.reshape(t.shape[0], 1, -1) if t.dim() else t.reshape(1, 1, 1)


def assert_equal(got, want, what="", level=0):
    """Element-for-element equality (of values: -0 == 0); got and want are [sample, voxel...] tensors of any dtype, compared in fp64 (or int64)."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    if got.dtype != torch.int64 or want.dtype != torch.int64:
        got, want = got.to(F64), want.to(F64)
    bad = ~(got == want)
    if bool(bad.any()):
        g3, w3, b3 = _as3(got, level), _as3(want, level), _as3(bad, level)
        msg = _first_mismatches(g3, w3, b3).replace("level 0", f"level {level}")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ: {msg}")


def assert_within(got, want, bound, what="", level=0):
    """|got - want| <= bound element for element (bound a tensor or a number); prints and returns the largest |got - want| / bound."""
    got, want = got.detach().cpu().to(F64), want.detach().cpu().to(F64)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    bound = torch.as_tensor(bound, dtype=F64).expand(want.shape) if not torch.is_tensor(bound) else bound.to(F64).expand(want.shape)
    err = (got - want).abs()
    bad = ~(err <= bound)  # (a NaN fails)
    ratio = float((err / bound.clamp(min=1e-300)).max()) if got.numel() else 0.0
    print(f"within[{what}]: largest |got - want| / bound = {ratio:.3g}")
    if bool(bad.any()):
        g3, w3, b3 = _as3(got, level), _as3(want, level), _as3(bad, level)
        msg = _first_mismatches(g3, w3, b3).replace("level 0", f"level {level}")
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound (largest error / bound {ratio:.3g}): {msg}")
    return ratio


def check_grad(dt, got, ref, what=""):
    """A gradient tensor [B, ...] against its fp64 definition at the project's elementwise bar, PER SAMPLE and absolute: fp32 within 2e-5 max|ref| of the sample,
    bf16 within one correct rounding of that (tests/rounding.py).  Absolute on purpose: at a saturated voxel the fp32 sign(p - g) is 0 where fp64 has +-0.6, and
    the gradient there is about 1e-8 of the sample's largest."""
    from tests.rounding import assert_one_rounding

    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    worst = 0.0
    for b in range(ref.shape[0]):
        e = 2e-5 * float(ref[b].abs().max())
        if dt == "bf16":
            assert_one_rounding(got[b], ref[b], e=e, what=f"{what} sample {b}")
        else:
            worst = max(worst, assert_within(got[b:b + 1], ref[b:b + 1], e + 1e-300, what=f"{what} sample {b}"))
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs (generated on the CPU, identically by the host audit and by the GPU test)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def make_label(seed, n, nvox, kind="mixed", q=0.3):
    """[n, nvox] fp32 in {0, 1}.  'mixed': a share q of foreground; 'special': sample 0 all foreground, sample 1 (if any) empty, the rest mixed;
    'sparse' (the pooling rows: q about 1 / window, so that pooled labels are neither all 0 nor all 1): sample b has the share q (b + 1), and of three
    or more samples sample 1 is empty."""
    rng = np.random.default_rng(1000 + seed)
    u = rng.random((n, nvox))
    if kind == "sparse":
        lab = (u < q * (np.arange(n).reshape(n, 1) + 1.0)).astype(np.float32)
        if n > 2:
            lab[1] = 0.0
    else:
        lab = (u < q).astype(np.float32)
    if kind == "special":
        lab[0] = 1.0
        if n > 1:
            lab[1] = 0.0
    return torch.from_numpy(lab)


def make_logits(seed, n, nvox, kind="synth"):
    """[n, nvox, 2] fp32.  'synth': 2 * synth_input.  'saturated': l1 = l0 + one of (+40, -40, +20, -20, 0): p rounds to 0 or 1 in fp32 (at 20 not yet in
    fp64), and ties."""
    lg = 2.0 * synth_input(seed, (n, nvox, 2))
    if kind == "saturated":
        rng = np.random.default_rng(2000 + seed)
        diff = torch.from_numpy(np.array([40.0, -40.0, 20.0, -20.0, 0.0], np.float32)[rng.integers(0, 5, (n, nvox))])
        lg[..., 1] = lg[..., 0] + diff
    return lg


def make_att(seed, n, nvox):
    """[n, nvox] fp32, dyadic: k / 256 with k in 0..256.  Every sum of them (and of g * a) is a multiple of 2^-8 below 2^16: exact in fp32 in any order, and
    exact on the 2^-32 grid of the fixed point."""
    rng = np.random.default_rng(3000 + seed)
    return torch.from_numpy((rng.integers(0, 257, (n, nvox)) / 256.0).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# case tables.  Each row names the paths it is there for (`want`): tests/test_dice_host.py checks the declaration against the restated launch arithmetic.
# ---------------------------------------------------------------------------------------------------------------------------------------------
NVOX = (1, 3, 4, 5, 1023, 1024, 4100, 4101)
OFF_LOGITS, OFF_LABEL = 8, 4  # bytes a deliberately offset pointer is moved by: float2 rows stay 8-byte aligned, floats 4-byte aligned


def _sums_rows():
    rows = []
    for nvox in NVOX:
        for n in (1, 2, 3, 5):
            for pitch in (2, 8):
                rows.append({"name": f"v{nvox}_n{n}_p{pitch}", "nvox": nvox, "n": n, "pitch": pitch, "offset": False, "label": "mixed", "logits": "synth",
                             "want": {"vector": pitch == 2 and nvox % 4 == 0}})
    for nvox in (4, 1024, 4100):  # a multiple of 4 that the offset pointers force into the scalar loop
        for n in (1, 3):
            rows.append({"name": f"v{nvox}_n{n}_offset", "nvox": nvox, "n": n, "pitch": 2, "offset": True, "label": "mixed", "logits": "synth", "want": {"vector": False}})
    rows.append({"name": "special_vec", "nvox": 1024, "n": 3, "pitch": 2, "offset": False, "label": "special", "logits": "synth", "want": {"vector": True}})
    rows.append({"name": "special_scalar", "nvox": 1023, "n": 3, "pitch": 2, "offset": False, "label": "special", "logits": "synth", "want": {"vector": False}})
    rows.append({"name": "saturated_vec", "nvox": 1024, "n": 2, "pitch": 2, "offset": False, "label": "special", "logits": "saturated", "want": {"vector": True}})
    rows.append({"name": "saturated_scalar", "nvox": 1023, "n": 2, "pitch": 2, "offset": False, "label": "mixed", "logits": "saturated", "want": {"vector": False}})
    # dice_blocks at its cap 512 / n = 8: a thread of the 16-byte loop takes a second round (10 000 items on 4 096 threads), of the scalar loop a tenth
    rows.append({"name": "cap8_vec", "nvox": 40000, "n": 64, "pitch": 2, "offset": False, "label": "mixed", "logits": "synth", "ce": True, "want": {"vector": True, "blocks": 8, "at_cap": True, "min_rounds": 2}})
    rows.append({"name": "cap8_scalar", "nvox": 40001, "n": 64, "pitch": 2, "offset": False, "label": "mixed", "logits": "synth", "ce": True, "want": {"vector": False, "blocks": 8, "at_cap": True, "min_rounds": 2}})
    rows.append({"name": "cap1", "nvox": 3000, "n": 512, "pitch": 2, "offset": False, "label": "mixed", "logits": "synth", "ce": True, "want": {"vector": True, "blocks": 1, "at_cap": True, "min_rounds": 2}})
    return rows


SUMS_CASES = _sums_rows()

POOL_RATIOS = ((2, 2, 1), (2, 2, 2), (3, 1, 3), (1, 5, 1), (8, 8, 8), (1, 1, 1))
POOL_DST = (3, 5, 7)  # odd destination extents
POOL_CASES = [{"name": f"r{r[0]}{r[1]}{r[2]}_n{n}", "ratio": r, "dst": POOL_DST, "n": n} for r in POOL_RATIOS for n in (1, 3)]

LEVEL_DIMS = ((2, 2, 4), (6, 10, 4), (4, 2, 12), (32, 32, 12))
LEVEL_CASES = [{"name": f"{d[0]}x{d[1]}x{d[2]}_n{n}", "dims": d, "n": n, "want": {"blocks": 2 if d == (32, 32, 12) else 1}} for d in LEVEL_DIMS for n in (1, 3)]

TAIL_ROWS = {
    # name: (source dims, level dims in descriptor order, what the row is there for).  `ragged`: the levels whose window is not a multiple of T (the lanes of a
    # window then take unequal numbers of voxels); 576 = 9 * 64 is not one of them, 9, 27 and 135 are.
    "win_1_8_64_576": ((12, 4, 12), ((12, 4, 12), (6, 2, 6), (3, 1, 3), (1, 1, 1)), {"win": (1, 8, 64, 576), "T": (1, 8, 64, 64), "ragged": (), "vector": (0,)}),
    "win_1_9_135_odd": ((9, 3, 5), ((9, 3, 5), (3, 1, 5), (1, 1, 1)), {"win": (1, 9, 135), "T": (1, 8, 64), "ragged": (1, 2), "scalar_win1": (0,)}),
    "unordered": ((6, 6, 6), ((2, 2, 2), (3, 3, 3)), {"win": (27, 8), "T": (16, 8), "ragged": (0,)}),
    "win1_two_workgroups": ((24, 24, 16), ((24, 24, 16),), {"win": (1,), "T": (1,), "vector": (0,), "blocks": (2,), "busy": (2,)}),
    # (the launcher gives a pooling level one workgroup per 2 048 lanes and a workgroup takes 4 096 lanes a round: of exactly two workgroups the second starts at
    # voxel nvox and has nothing to do; the row after this one has levels of six workgroups, three of them with voxels)
    "win64_two_workgroups": ((16, 16, 16), ((4, 4, 4),), {"win": (64,), "T": (64,), "blocks": (2,), "busy": (1,)}),
    "pool_many_workgroups": ((48, 16, 16), ((24, 8, 4), (12, 4, 4)), {"win": (16, 64), "T": (16, 64), "blocks": (6, 6), "busy": (3, 3)}),
    "eight_levels": ((4, 4, 4), ((4, 4, 4), (4, 4, 2), (4, 2, 2), (2, 2, 2), (2, 2, 1), (2, 1, 1), (1, 1, 1), (4, 4, 4)), {"win": (1, 2, 4, 8, 16, 32, 64, 1), "nlevels": 8}),
}
TAIL_CASES = [{"name": f"{k}_n{n}", "row": k, "n": n} for k in TAIL_ROWS for n in (1, 3)]

def _seed(name):
    return sum(map(ord, name))


def sparse_q(wins):
    """Foreground share of a pooling row's source label: 0.7 / the middle window (so that the pooled labels of that level are about half ones); 0.3 if nothing pools."""
    w = sorted(x for x in wins if x > 1)
    return min(0.3, 0.7 / w[(len(w) - 1) // 2]) if w else 0.3


def pool_inputs(case):
    """[n, 1, X, Y, Z] fp32 source label of a POOL_CASES row."""
    src = tuple(d * r for d, r in zip(case["dst"], case["ratio"]))
    return make_label(_seed(case["name"]), case["n"], math.prod(src), "sparse", sparse_q([math.prod(case["ratio"])])).reshape(case["n"], 1, *src)


def level_inputs(case):
    """(logits [n, nvox, 2], attention map [n, nvox], label [n, 1, X, Y, Z]) of a LEVEL_CASES row."""
    n, d = case["n"], case["dims"]
    nvox, s = math.prod(d), _seed(case["name"])
    return make_logits(s, n, nvox), make_att(s, n, nvox), make_label(s, n, nvox, "sparse", 0.15).reshape(n, 1, *d)


def tail_inputs(case):
    """(source label [n, 1, X, Y, Z], [attention map [n, nvox_l] per level]) of a TAIL_CASES row."""
    sdims, levels, _ = TAIL_ROWS[case["row"]]
    n, s = case["n"], _seed(case["name"])
    q = sparse_q([math.prod(a // b for a, b in zip(sdims, d)) for d in levels])
    return make_label(s, n, math.prod(sdims), "sparse", q).reshape(n, 1, *sdims), [make_att(s + 1 + i, n, math.prod(d)) for i, d in enumerate(levels)]


def argmax_inputs(nvox, pitch=2):
    """Logits [nvox, pitch] with ties (every 5th voxel: l1 = l0, which must go to class 0), a NaN in either channel of two voxels, and a sentinel in channels
    2.. that would win every comparison; label [nvox] in {0, 1}."""
    lg = torch.full((nvox, pitch), 1e30)
    lg[:, :2] = 2.0 * synth_input(77 + nvox % 1000, (nvox, 2))
    lg[::5, 1] = lg[::5, 0]
    if nvox > 2:  # (a single voxel is the tie)
        lg[nvox // 2, 1] = float("nan")
        lg[nvox // 3, 0] = float("nan")
    return lg, make_label(78, 1, nvox)[0]


BWD_BIG = BWD_GRID_CAP * BWD_THREADS * 4 + 1028  # one voxel quad more than a full grid of the backward takes in a round, and then some: a second round
ATT_BWD_NVOX = (1, 135, 2049, 9216)
GS = 0.37  # the upstream gradient of the rows that have one
BWD_COEF = [-0.3, 0.02, -0.25, 0.015, -0.31, 0.021, -0.2, 0.017, -0.28, 0.019, -0.22, 0.016]  # [sample][class][A, B]: every one different
BWD_LAYOUTS = ("f32x2", "bf16x2", "bf16x8", "f32x8")


def _bwd_rows():
    """The rows of the logits-gradient kernels: every entry of NVOX at n = 1 and 3 with pitch 2 and 8, hardness on and off, without and with an upstream gradient,
    and two rows of offset pointers; the saturated logits; and the row whose threads take a second round.  `ce`: the cross-entropy entry points are called too."""
    rows = []
    for nvox in NVOX:
        for n in (1, 3):
            for pitch in (2, 8):
                for hard in (1, 0):
                    for gs in (False, True):
                        rows.append({"n": n, "nvox": nvox, "kind": "synth", "pitch": pitch, "hard": hard, "gs": gs, "offset": False, "ce": pitch == 2 and hard == 1 and gs})
            rows.append({"n": n, "nvox": nvox, "kind": "synth", "pitch": 2, "hard": 1, "gs": True, "offset": True, "ce": False})
            rows.append({"n": n, "nvox": nvox, "kind": "synth", "pitch": 8, "hard": 0, "gs": False, "offset": True, "ce": False})
    for nvox in (1023, 1024):
        for hard in (1, 0):
            rows.append({"n": 3, "nvox": nvox, "kind": "saturated", "pitch": 2, "hard": hard, "gs": True, "offset": False, "ce": False})
        rows.append({"n": 3, "nvox": nvox, "kind": "saturated", "pitch": 8, "hard": 1, "gs": False, "offset": True, "ce": False})
    rows.append({"n": 1, "nvox": BWD_BIG, "kind": "synth", "pitch": 2, "hard": 1, "gs": False, "offset": False, "ce": False, "layouts": ("bf16x2",)})
    return rows


BWD_ROWS = _bwd_rows()


def bwd_inputs(row):
    """(logits [n, nvox, 2], label [n, nvox], the prediction block of the coefficients [n * 4] fp32) of a BWD_ROWS row."""
    n, nvox = row["n"], row["nvox"]
    s = 500 + nvox % 997 + n
    return make_logits(s, n, nvox, row["kind"]), make_label(s, n, nvox, "special" if row["kind"] == "saturated" else "mixed"), torch.tensor(BWD_COEF[: n * 4])


FINALIZE_ROWS = [(n, nl) for n in (1, 3) for nl in (0, 1, 4)]


def hand_sums(n, nl):
    """Sums of a finalisation row as (int64 patterns of the prediction sums [n, 6], of the attention sums [nl, n, 3] or None), on the 2^-32 grid: sample 0 ordinary;
    of three samples, sample 1 has no foreground (G1 = 0, P1 tiny) and sample 2 is predicted perfectly (I = G = P); of the levels, level 1 has an all-zero
    attention map and level 3 neither label nor map in sample 0."""
    ps = torch.tensor([[900.25, 1000.0, 1010.5, 40.125, 55.0, 44.5], [4095.9999, 4096.0, 4095.9999, 0.0, 0.0, 1.5e-7], [3000.0, 3000.0, 3000.0, 1096.0, 1096.0, 1096.0]], dtype=F64)[:n]
    a = torch.tensor([[[20.5, 64.0, 41.25], [0.0, 0.0, 3.0 / 256], [7.0, 7.0, 7.0]], [[0.0, 17.0, 0.0], [0.0, 5.0, 0.0], [0.0, 1.0, 0.0]],
                      [[1.5, 2.0, 2.75], [0.0, 0.0, 0.5], [1.0, 1.0, 1.0]], [[0.0, 0.0, 0.0], [0.25, 1.0, 0.25], [0.0, 1.0, 0.0]]], dtype=F64)[:nl, :n]
    return fx_encode(ps), (fx_encode(a) if nl else None)


ARGMAX_ROWS = [(nvox, pitch) for nvox in (1, 1000003) for pitch in (2, 8)]

# Module rows: (B, label dims, attention-map dims coarsest first, the plan _fused_plan must answer)
MODULE_ROWS = {
    "pyr_12_4_12": (3, (12, 4, 12), ((3, 1, 3), (6, 2, 6), (12, 4, 12)), None),
    "pyr_6_10_4": (1, (6, 10, 4), ((1, 5, 1), (3, 5, 2), (6, 10, 4)), None),
    "pyr_9_3_5": (2, (9, 3, 5), ((3, 1, 1), (9, 3, 5)), None),
    "fused_b1": (1, (32, 32, 12), ((4, 4, 4), (8, 8, 12), (16, 16, 12), (32, 32, 12)), 2),
    "fused_b3": (3, (32, 32, 12), ((4, 4, 4), (8, 8, 12), (16, 16, 12), (32, 32, 12)), 2),
    "ten_levels": (3, (8, 8, 4), ((1, 1, 1), (1, 1, 1), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (4, 2, 2), (4, 4, 2), (4, 4, 4), (8, 8, 4)), None),
}


def module_inputs(name):
    """CPU tensors of a module row: label [B, 1, X, Y, Z] in {0, 1} with an empty-foreground sample where B > 1 (sample 0), logits [B, 2, X, Y, Z] = 2 *
    synth_input, dyadic attention maps [B, 1, x, y, z] (coarsest first)."""
    B, dims, att_dims, _ = MODULE_ROWS[name]
    seed = sum(map(ord, name))
    nvox = math.prod(dims)
    lab = make_label(seed, B, nvox)
    if B > 1:
        lab[0] = 0.0
    logits = 2.0 * synth_input(seed + 1, (B, 2, *dims))
    atts = [make_att(seed + 2 + i, B, math.prod(d)).reshape(B, 1, *d) for i, d in enumerate(att_dims)]
    return lab.reshape(B, 1, *dims), logits, atts


def module_bars(name, supervised, hardness):
    """What the end-to-end test holds a module row to: the fp64 sums and their bounds, whether every Dice denominator G + P is at least 1 (then the loss bar is
    5e-6, that of test_gpu_ce_loss.py), else the bar propagated through the finalisation; and the largest bound / denominator (the gradients' 5e-5 needs <= 1e-5)."""
    B, dims, att_dims, plan = MODULE_ROWS[name]
    lab5, logits5, atts = module_inputs(name)
    lg = logits5.to(F64).permute(0, 2, 3, 4, 1).reshape(B, -1, 2)
    lab = lab5.reshape(B, -1)
    ps = pred_sums(lg, lab, hardness)
    wg = max(sums_launch(math.prod(dims), B)["workgroups"], level_launch(dims, B)["workgroups"] if plan else 0)
    pb = sum_bound(lg, lab, hardness, wg)
    nl = len(atts) if supervised else 0
    labels = pyramid_labels(lab5, [att_dims[nl - l - 1] for l in range(nl)])
    asums = torch.stack([att_sums(atts[nl - l - 1], labels[l]) for l in range(nl)]) if nl else None
    D = ps.reshape(B, 2, 3)[..., 1] + ps.reshape(B, 2, 3)[..., 2]
    dens = [float(D.min())] + ([float((asums[..., 1] + asums[..., 2]).min())] if nl else [])
    rel = float((pb.reshape(B, 2, 3) / (D.unsqueeze(-1) + SMOOTH)).max())
    big = min(dens) >= 1.0
    return {"big_denominators": big, "loss_bar": 5e-6 if big else loss_bound(ps, pb, asums), "rel_sums": rel, "min_denominator": min(dens)}
