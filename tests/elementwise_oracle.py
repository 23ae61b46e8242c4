"""fp64 definitions of the streaming elementwise kernels (csrc/elementwise.hip), the comparison helpers of tests/test_gpu_elementwise.py, and a restatement
of the launch arithmetic that test's shapes were derived from.  Nothing of the package under test is imported here: torch, and the suite's own bf16
comparison (tests/rounding.py).

Layout: every activation is a 2-D fp64 tensor [voxels, channels] (the channels-last tensors of the C ABI with their voxel axes flattened); per-channel
vectors are [channels].  Gradients are written out as closed-form sums, not taken from autograd (tests/test_elementwise_host.py holds them against autograd).

    z = y*scale + shift            scale = gamma*invstd, shift = beta - mean*scale, invstd = 1/sqrt(var + eps)
    d = keep * z / (1 - p)         keep in {0, 1}
    out = (d > 0 ? d : alpha*d) + residual            residual: nothing, a tensor, or x1*rw + rb with a ONE-channel x1
    dz = keep * (d > 0 ? g : alpha*g) / (1 - p)       g = d(loss)/d(out)
    dbeta = sum dz   dgamma = sum dz*xhat   dalpha = sum over d < 0 of g*d   d(residual bias) = sum g      xhat = (y - mean)*invstd
    dy = gamma*invstd * (dz - mean(dz) - xhat*mean(dz*xhat))
"""
import math
from math import gcd

import torch

from tests.rounding import assert_one_rounding

F64 = torch.float64
U24, U23 = 2.0 ** -24, 2.0 ** -23  # half an fp32 ulp (one rounding, relative) / one ulp


# ---------------------------------------------------------------------------------------------------------------------------------------------
# definitions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def bn_stats(y):
    """Training-mode statistics over the voxel axis: (mean, biased variance, unbiased variance for the running update)."""
    n = y.shape[0]
    mean = y.sum(0) / n
    var = (y * y).sum(0) / n - mean * mean
    var = torch.clamp(var, min=0.0)
    return mean, var, (var * n / (n - 1) if n > 1 else var)


def bn_stats_from_sums(s, q, count):
    """The same from sum(y) and sum(y^2) (what the sharded statistics buffer holds)."""
    mean = s / count
    var = torch.clamp(q / count - mean * mean, min=0.0)
    return mean, var, (var * count / (count - 1) if count > 1 else var)


def bn_fold(mean, var, gamma, beta, eps):
    """(invstd, scale, shift) of the folded affine."""
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * invstd
    return invstd, scale, beta - mean * scale


def running_update(rm, rv, mean, var_unbiased, momentum):
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var_unbiased


def fold_eval(gamma, beta, rm, rv, eps):
    scale = gamma / torch.sqrt(rv + eps)
    return scale, beta - rm * scale


def keep_bits(keep_bytes, c):
    """[voxels*c/8] uint8 keep bytes (bit j of byte i = element 8*i + j of the pitch-free [voxel][c] order) -> [voxels, c] fp64 mask."""
    b = keep_bytes.to(torch.int64).reshape(-1, 1)
    return ((b >> torch.arange(8).reshape(1, 8)) & 1).to(F64).reshape(-1, c)


def prelu(d, alpha):
    return torch.where(d > 0, d, alpha * d)


def bn_act_fwd(y, scale, shift, alpha, keep=None, p=0.0, res=None, x1=None, rw=None, rb=None):
    z = y * scale + shift
    d = z if keep is None else keep * z / (1.0 - p)
    out = prelu(d, alpha)
    if res is not None:
        out = out + res
    if x1 is not None:
        out = out + x1.reshape(-1, 1) * rw + rb
    return out


def bn_act_bwd(y, g, mean, invstd, gamma, scale, shift, alpha, keep=None, p=0.0):
    """All gradients of the block, and for every per-channel sum the sum of the magnitudes of its summands (`abs_*`, for the derived bounds)."""
    n = y.shape[0]
    keep = torch.ones_like(y) if keep is None else keep
    z = y * scale + shift
    d = keep * z / (1.0 - p)
    dz = keep * torch.where(d > 0, g, alpha * g) / (1.0 - p)
    xhat = (y - mean) * invstd
    neg = (d < 0).to(F64)
    r = {"z": z, "dz": dz, "dbeta": dz.sum(0), "dgamma": (dz * xhat).sum(0), "dalpha": (neg * g * d).sum(), "dres_bias": g.sum(0),
         "abs_dbeta": dz.abs().sum(0), "abs_dgamma": (dz * xhat).abs().sum(0), "abs_dalpha": (neg * g * d).abs().sum(), "abs_dres_bias": g.abs().sum(0)}
    r["mean_dz"], r["mean_dzx"] = r["dbeta"] / n, r["dgamma"] / n
    r["dy"] = gamma * invstd * (dz - r["mean_dz"] - xhat * r["mean_dzx"])
    return r


def att_fwd(x, att):
    return x * (1.0 + att.reshape(-1, 1))


def att_bwd(x, att, g, datt_ext=None):
    """(dx, d(pre-sigmoid), its sum = the bias gradient of the convolution in front of the sigmoid)."""
    dot = (g * x).sum(1)
    if datt_ext is not None:
        dot = dot + datt_ext
    dpre = dot * att * (1.0 - att)
    return g * (1.0 + att.reshape(-1, 1)), dpre, dpre.sum()


def channel_sum(t):
    return t.sum(0)


def add(dst, src):
    return dst + src


def copy(src):
    return src.clone()


def merge_residual_grads(dw, db, dwr, dbr, cout, cin, taps, centre):
    """The centre tap of a [cout, cin, taps] weight gradient and its bias gradient added to those of the 1x1x1 residual convolution."""
    return dwr + dw.reshape(cout * cin, taps)[:, centre], dbr + db


def gather(src, m, m2=None):
    """dst[i] = src[m[i]] (0 where m[i] < 0) + src[m2[i]] (where m2 is given and >= 0)."""
    out = torch.where(m >= 0, src[m.clamp(min=0).long()], torch.zeros((), dtype=F64))
    if m2 is not None:
        out = out + torch.where(m2 >= 0, src[m2.clamp(min=0).long()], torch.zeros((), dtype=F64))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------
# comparison helpers (the GPU test uses exactly these; tests/test_elementwise_host.py plants faults against them)
# ---------------------------------------------------------------------------------------------------------------------------------------------
def check_out(dt, got, ref, what=""):
    """An output tensor against its fp64 definition: fp32 within 2e-5 max|ref| (the accumulator bar of tests/test_gpu_ops.py `_tol`), bf16 within ONE correct
    rounding of that (tests/rounding.py).  Returns max |got - ref| / max|ref|."""
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    scale = float(ref.abs().max()) + 1e-12
    err = float((got - ref).abs().max()) / scale
    print(f"check_out[{what}, {dt}]: max |got - ref| = {err:.3g} of max|ref| (bar {'one bf16 rounding of ' if dt == 'bf16' else ''}2e-5)")
    if dt == "bf16":
        assert_one_rounding(got, ref, what=what)
    else:
        assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
        assert err <= 2e-5, f"{what}: max |got - ref| = {err:.3g} of max|ref|, bar 2e-5"
    return err


def sum_bound(chain, abs_terms, ref, extra=0.0):
    """Derived bar of a per-channel fp32-accumulated sum: (chain + 8) * 2^-24 * sum|term| (the per-thread accumulation chain and the fp32 roundings inside one
    summand) + 2^-23 |ref| (the fp32 roundings of the per-channel constants in the summands) + one final fp32 rounding of the result (2^-24 |ref|)."""
    return (chain + 8) * U24 * abs_terms + U23 * ref.abs() + U24 * ref.abs() + extra


def check_sum(got, ref, bound, what=""):
    """|got - ref| <= bound, element for element; returns the largest error / bound."""
    got, ref, bound = (torch.as_tensor(t).detach().cpu().to(F64).reshape(-1) for t in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, f"{what}: shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(bound.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite result"
    ratio = (got - ref).abs() / bound.clamp(min=1e-300)
    i = int(ratio.argmax())
    print(f"check_sum[{what}]: largest |got - ref| / bound = {float(ratio[i]):.3g} (|err| {float((got - ref).abs()[i]):.3g}, bound {float(bound[i]):.3g}, ref {float(ref[i]):.6g})")
    assert float(ratio[i]) <= 1.0, f"{what}: channel {i}: got {float(got[i])!r}, ref {float(ref[i])!r}, |err| {float((got - ref).abs()[i]):.3g} > bound {float(bound[i]):.3g}"
    return float(ratio[i])


def check_bwd(dt, got, ref, chain, mean, invstd, count):
    """The backward of one BN case: `got` holds dy [voxels, c] and the vectors dgamma, dbeta, dalpha, dres_bias, mean_dz, mean_dzx as the kernels left them,
    `ref` is bn_act_bwd(...).  dgamma carries the extra term of the fp32 mean the kernel subtracts: |mean| invstd 2^-24 sum|dz|."""
    worst = {"dy": check_out(dt, got["dy"], ref["dy"], "bn_act_bwd_apply dy")}
    extra_g = mean.abs() * invstd * U24 * ref["abs_dbeta"]
    worst["dgamma"] = check_sum(got["dgamma"], ref["dgamma"], sum_bound(chain, ref["abs_dgamma"], ref["dgamma"], extra_g), "dgamma")
    worst["dbeta"] = check_sum(got["dbeta"], ref["dbeta"], sum_bound(chain, ref["abs_dbeta"], ref["dbeta"]), "dbeta")
    worst["dalpha"] = check_sum(got["dalpha"], ref["dalpha"], sum_bound(chain, ref["abs_dalpha"], ref["dalpha"]), "dalpha")
    worst["dres_bias"] = check_sum(got["dres_bias"], ref["dres_bias"], sum_bound(chain, ref["abs_dres_bias"], ref["dres_bias"]), "d(residual bias)")
    worst["mean_dz"] = check_sum(got["mean_dz"], ref["mean_dz"], sum_bound(chain, ref["abs_dbeta"] / count, ref["mean_dz"]), "mean_dz")
    worst["mean_dzx"] = check_sum(got["mean_dzx"], ref["mean_dzx"], sum_bound(chain, ref["abs_dgamma"] / count, ref["mean_dzx"], extra_g / count), "mean_dzx")
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------------------
# launch arithmetic, READ FROM csrc/elementwise.hip (block_for_cgs, vsseg_bn_act_bwd_reduce, vsseg_bn_act_bwd_apply, bn_fwd_grid, vsseg_channel_sum) and
# csrc/common.h (grid_for).  It is a restatement for the case audit, not a second source of truth: whoever retunes a grid there updates it here, and the
# audit (tests/test_elementwise_host.py) then says which shapes of BN_CASES to re-pick.
# ---------------------------------------------------------------------------------------------------------------------------------------------
STAT_SHARDS = 256
FX_GRAD_RANGE = 256.0  # |one workgroup's partial sum| must stay below 2^52 / 2^44 (csrc/common.h)


def block_for_cgs(cgs):
    blk = 64 * (cgs // gcd(cgs, 64))
    while blk < 256 and (blk * 2) % cgs == 0:
        blk *= 2
    return 0 if blk > 1024 else blk


def grid_for(items, block, cap=256 * 16):
    return max(1, min((items + block - 1) // block, cap))


def reduce_grid(c, nvox):
    cgs = c // 8
    blk, items = block_for_cgs(cgs), nvox * cgs
    cap = min(256 * 8, max(192, min(items // (blk * 16), 256 * 3 if c <= 16 else 65536 // (3 * c))))
    return grid_for((items + 1) // 2, blk, cap)


def apply_grid(c, nvox):
    cgs = c // 8
    return grid_for((nvox * cgs + 1) // 2, block_for_cgs(cgs), 256 * 8)


def bn_fwd_grid(c, nvox):
    cgs = c // 8
    g = grid_for(nvox * cgs, 256, 16384)
    return (g + cgs - 1) // cgs * cgs


def channel_sum_grid(c, nvox):
    cgs = (c + 7) // 8
    return grid_for(nvox * cgs, block_for_cgs(cgs), 2048)


def thread_paths(grid, blk, cgs, nvox, unroll=2):
    """How the threads of a (grid x blk) launch walk nvox voxels: every thread owns one 8-channel group and the voxels slot, slot + step, ... ; the backward
    kernels take them two at a time (`for (; v + step < nvox; v += 2*step)`) and finish with a scalar tail.  Counts are in voxel slots (cgs threads each)."""
    assert (grid * blk) % cgs == 0
    step = grid * blk // cgs
    live = min(step, nvox)
    hi, nhi = (nvox + step - 1) // step, (nvox - 1) % step + 1  # slot s holds ceil((nvox - s) / step) voxels: hi for s < nhi, hi - 1 for the other live slots
    per_counts = {hi: nhi}
    if live > nhi:
        per_counts[hi - 1] = live - nhi
    r = {"block": blk, "grid": grid, "step": step, "idle": step - live, "body_then_tail": 0, "body_only": 0, "tail_only": 0, "chain": max(per_counts)}
    for k, cnt in per_counts.items():
        if k == 0 or cnt == 0:
            continue
        if unroll == 1:
            r["body_only"] += cnt
        elif k == 1:
            r["tail_only"] += cnt
        elif k % unroll == 0:
            r["body_only"] += cnt
        else:
            r["body_then_tail"] += cnt
    return r


def bn_launches(c, nvox):
    cgs = c // 8
    blk = block_for_cgs(cgs)
    return {"reduce": thread_paths(reduce_grid(c, nvox), blk, cgs, nvox), "apply": thread_paths(apply_grid(c, nvox), blk, cgs, nvox),
            "fwd": thread_paths(bn_fwd_grid(c, nvox), 256, cgs, nvox, unroll=1)}


# name -> (channels, (n, x, y, z), sliced, what the backward reduce launch must reach).  `sliced`: every tensor is the channel slice [8, 8 + c) of rows of 96.
BN_CASES = {
    "c160_15vox": (160, (1, 5, 3, 1), False, {"block": 320, "grid": 1, "idle": 1, "tail_only": 15, "body_only": 0, "body_then_tail": 0}),
    "c48_630vox": (48, (2, 7, 9, 5), False, {"block": 384, "grid": 5, "step": 320, "body_only": 310, "tail_only": 10, "idle": 0}),
    "c48_27600vox": (48, (2, 23, 25, 24), False, {"block": 384, "grid": 192, "step": 12288, "body_then_tail": 3024, "body_only": 12288 - 3024, "chain": 3}),
    "c16_210vox": (16, (2, 5, 7, 3), False, {"block": 256}),
    "c32_210vox": (32, (2, 5, 7, 3), False, {"block": 256}),
    "c64_210vox": (64, (2, 5, 7, 3), False, {"block": 256}),
    "c80_210vox": (80, (2, 5, 7, 3), False, {"block": 320}),
    "c96_210vox": (96, (2, 5, 7, 3), False, {"block": 384}),
    "c80_sliced": (80, (2, 5, 7, 3), True, {"block": 320}),
}
EXACT_CASE = (16, (1, 96, 96, 64))  # grid > STAT_SHARDS in the backward reduce; channel_sum's grid is capped, its threads loop
NETWORK_BLOCKS = {2: 256, 4: 256, 6: 384, 8: 256, 10: 320, 12: 384, 20: 320}  # 8-channel groups of the network's layers -> block size


# ---------------------------------------------------------------------------------------------------------------------------------------------
# inputs of the BN cases (generated on the CPU, identically by the host audit and by the GPU test)
# ---------------------------------------------------------------------------------------------------------------------------------------------
KINK_MARGIN = 1e-4  # min |z| >= KINK_MARGIN * max |z|: two orders above the fp32 error of y*scale + shift, 3 * 2^-24 (|y*scale| + |shift|)
EPS, MOMENTUM, ALPHA = 1e-5, 0.1, 0.2


def _rt(x, dt):
    return x.to(torch.bfloat16).to(F64) if dt == "bf16" else x.to(torch.float32).to(F64)


def split_sums(s, parts=(0.5, 0.3)):
    """A sum as three addends (for three shards of a statistics buffer), each on the 2^-20 grid of the fixed-point statistics; returns (addends, their total)."""
    fx = 2.0 ** 20
    a = [torch.round(s * f * fx) / fx for f in parts]
    a.append(torch.round((s - sum(a)) * fx) / fx)
    return a, sum(a)


def make_bn_case(name, dt, seed=0):
    """Inputs of one BN case, values representable in dt, as fp64 [voxels, c]: y, dout, residual tensor; gamma, beta, running statistics; the statistics as the
    test writes them into three shards, and mean / var / invstd / scale / shift defined from those.  The PReLU backward is discontinuous at z = 0 and the
    kernel decides the branch on the fp32 z: elements with |z| below 2 * KINK_MARGIN * max|z| are redrawn (with 1.3 M elements no seed avoids them), then the
    margin is ASSERTED over every element, kept or dropped."""
    c, shape, _, _ = BN_CASES[name]
    nvox = math.prod(shape)
    gen = torch.Generator().manual_seed(1000 + 17 * seed + sum(map(ord, name)))
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)  # noqa: E731
    gamma, beta = _rt(torch.rand(c, generator=gen, dtype=F64) + 0.5, "fp32"), _rt(rnd(c) * 0.1, "fp32")
    rm, rv = _rt(rnd(c) * 0.1, "fp32"), _rt(torch.rand(c, generator=gen, dtype=F64) + 0.5, "fp32")
    centre, spread = _rt(rnd(c) * 0.3, "fp32"), _rt(torch.rand(c, generator=gen, dtype=F64) + 0.75, "fp32")
    y = _rt(rnd(nvox, c) * spread + centre, dt)
    for _ in range(16):
        (s_parts, s), (q_parts, q) = split_sums(y.sum(0)), split_sums((y * y).sum(0))
        mean, var, var_unb = bn_stats_from_sums(s, q, float(nvox))
        invstd, scale, shift = bn_fold(mean, var, gamma, beta, EPS)
        z = y * scale + shift
        bad = z.abs() < 2 * KINK_MARGIN * float(z.abs().max())
        if not bool(bad.any()):
            break
        y = torch.where(bad, _rt(rnd(nvox, c) * spread + centre, dt), y)
    assert float(z.abs().min()) >= KINK_MARGIN * float(z.abs().max()), f"{name}/{dt}: an element within {KINK_MARGIN} max|z| of the PReLU kink"
    return {"c": c, "shape": shape, "nvox": nvox, "y": y, "dout": _rt(rnd(nvox, c), dt), "res": _rt(rnd(nvox, c), dt), "gamma": gamma, "beta": beta, "rm": rm, "rv": rv,
            "s_parts": s_parts, "q_parts": q_parts, "mean": mean, "var": var, "var_unb": var_unb, "invstd": invstd, "scale": scale, "shift": shift, "alpha": ALPHA}


EXACT_VALUES = (-1.0, -0.5, 0.0, 0.5, 1.0)


def exact_design(ch, unit):
    """Per channel, the designed sum of dout over the voxels of each value of y, in the order of EXACT_VALUES (all non-zero multiples of 4 * unit), and the sums
    they give with alpha = 1/2: dz = g for y > 0 and g/2 for y <= 0 (y = 0 takes the alpha branch), dz*xhat = dz*y, g*d = g*y for y < 0."""
    cls = [4 * unit * k for k in (1 + ch % 3, -2, 1 + ch % 4, 1, 2 + ch % 2)]
    b, d, z, h, a = cls
    return cls, {"dbeta": a + h + (b + d + z) / 2, "dgamma": a + h / 2 - b / 2 - d / 4, "dalpha": -b - d / 2, "dres_bias": a + b + d + z + h}


def make_exact_case(seed=1, shape=None):  # seed: the largest workgroup partial sum is 166 of the 256 a fixed-point slot takes (host audit)
    """The exact-arithmetic case: y, dout in {-1, -1/2, 0, 1/2, 1}, mean 0, invstd 1, gamma 1, scale 1, shift 0, alpha 1/2, no dropout.  Every summand is a
    multiple of 1/4, so every fp32 partial sum and every fixed-point add is exact and the sums equal the fp64 definition bit for bit in any order.
    For dy to be exact too, mean(dz) and mean(dz*xhat) must be fp32 numbers, i.e. the sums multiples of count / 2^14: within every class of voxels with the same
    y, a few hundred values of dout at random places are overwritten so that the class sums to its designed value (exact_design).  The class sums are all
    non-zero, so a wrong factor on ANY class (the alpha branch at y = 0 among them) changes sum dz; with voxels in cancelling pairs it would not.
    Then dy = dz - mean_dz - y*mean_dzx is a multiple of 2^-15 below 2 in magnitude: exact in fp32."""
    c, shape = EXACT_CASE[0], shape or EXACT_CASE[1]
    nvox = math.prod(shape)
    assert nvox % 65536 == 0
    unit = nvox // 16384
    gen = torch.Generator().manual_seed(77 + seed)
    vals = torch.tensor(EXACT_VALUES, dtype=F64)
    y = vals[torch.randint(0, 5, (nvox, c), generator=gen)]
    g = vals[torch.randint(0, 5, (nvox, c), generator=gen)]
    for ch in range(c):
        for val, target in zip(EXACT_VALUES, exact_design(ch, unit)[0]):
            idx = torch.nonzero(y[:, ch] == val).reshape(-1)
            delta = target - float(g[idx, ch].sum())
            m = int(abs(delta)) + 64
            rows = idx[torch.randperm(idx.numel(), generator=gen)[:m]]
            want = float(g[rows, ch].sum()) + delta  # the new sum of the overwritten values: n1 of them +-1, one 0 or +-1/2, the rest 0
            n1 = int(abs(want))
            assert rows.numel() == m and n1 < m and (abs(want) - n1) in (0.0, 0.5)
            new = torch.zeros(m, dtype=F64)
            new[:n1] = math.copysign(1.0, want)
            new[n1] = math.copysign(abs(want) - n1, want)
            g[rows, ch] = new
    one, zero = torch.ones(c, dtype=F64), torch.zeros(c, dtype=F64)
    return {"c": c, "shape": shape, "nvox": nvox, "y": y, "dout": g, "mean": zero, "invstd": one, "gamma": one, "scale": one, "shift": zero, "alpha": 0.5}


def workgroup_partials(case, c, nvox):
    """Largest |partial sum| any workgroup of the backward reduce launch adds to a fixed-point slot (must stay below FX_GRAD_RANGE), from the launch arithmetic."""
    cgs = c // 8
    blk, grid = block_for_cgs(cgs), reduce_grid(c, nvox)
    per_blk, step = blk // cgs, grid * blk // cgs
    assert nvox % step == 0
    r = bn_act_bwd(case["y"], case["dout"], case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"], case["alpha"])
    neg = (r["z"] < 0).to(F64)
    worst = 0.0
    for t in (r["dz"], r["dz"] * case["y"], case["dout"], (neg * case["dout"] * r["z"]).sum(1, keepdim=True)):
        w = t.reshape(nvox // step, grid, per_blk, t.shape[1]).sum((0, 2))  # voxel = k*step + workgroup*per_blk + slot
        worst = max(worst, float(w.abs().max()))
    return worst
