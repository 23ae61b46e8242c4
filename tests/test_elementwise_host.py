"""CPU tests of tests/elementwise_oracle.py, the net under tests/test_gpu_elementwise.py:

* the closed-form definitions against torch fp64 autograd of the same composition (F.batch_norm(training=True) for the statistics path), 1e-10 relative;
* planted faults: an fp32 model of the kernels passes the comparison helpers the GPU test uses, and each subtly wrong variant of it is rejected by them;
* the case audit: the launch arithmetic restated from csrc/elementwise.hip says that every BN case of the GPU test reaches the code path it is there for
  (unrolled body then tail, tail only, idle threads, more workgroups than statistics shards).  A retuned grid fails here, not silently.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_oracle as EO

F64 = torch.float64


def _rel(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# oracle against autograd
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("res", ["none", "tensor", "conv1"])
def test_closed_form_gradients_equal_autograd(res, p):
    gen = torch.Generator().manual_seed(3)
    n, c = 211, 24
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)  # noqa: E731
    y = (rnd(n, c) * 1.5 + 0.3).requires_grad_(True)
    gamma, beta, alpha = (rnd(c).abs() + 0.5).requires_grad_(True), rnd(c).requires_grad_(True), torch.tensor([0.2], dtype=F64, requires_grad=True)
    keep = (torch.rand(n, c, generator=gen) >= p).to(F64)
    g = rnd(n, c)
    r, x1, rw, rb = rnd(n, c), rnd(n), rnd(c), rnd(c).requires_grad_(True)
    rm0, rv0 = rnd(c), rnd(c).abs() + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    # torch: batch_norm over [N, C] in training mode, dropout with the given mask, PReLU, residual
    z = F.batch_norm(y, rm, rv, gamma, beta, training=True, momentum=EO.MOMENTUM, eps=EO.EPS)
    out = F.prelu(z * keep / (1 - p), alpha)
    out = out + (r if res == "tensor" else x1.reshape(-1, 1) * rw + rb if res == "conv1" else 0.0)
    out.backward(g)
    # the oracle, from detached values
    yd = y.detach()
    mean, var, var_unb = EO.bn_stats(yd)
    invstd, scale, shift = EO.bn_fold(mean, var, gamma.detach(), beta.detach(), EO.EPS)
    o = EO.bn_act_fwd(yd, scale, shift, 0.2, keep, p, res=r if res == "tensor" else None, **(dict(x1=x1, rw=rw, rb=rb.detach()) if res == "conv1" else {}))
    b = EO.bn_act_bwd(yd, g, mean, invstd, gamma.detach(), scale, shift, 0.2, keep, p)
    erm, erv = EO.running_update(rm0, rv0, mean, var_unb, EO.MOMENTUM)
    assert _rel(o, out.detach()) < 1e-10
    assert _rel(erm, rm) < 1e-10 and _rel(erv, rv) < 1e-10
    assert _rel(b["dy"], y.grad) < 1e-10 and _rel(b["dgamma"], gamma.grad) < 1e-10 and _rel(b["dbeta"], beta.grad) < 1e-10 and _rel(b["dalpha"].reshape(1), alpha.grad) < 1e-10
    if res == "conv1":
        assert _rel(b["dres_bias"], rb.grad) < 1e-10
    assert _rel(b["dres_bias"], g.sum(0)) < 1e-10
    s, q = yd.sum(0), (yd * yd).sum(0)
    for a, e in zip(EO.bn_stats_from_sums(s, q, float(n)), (mean, var, var_unb)):
        assert _rel(a, e) < 1e-10


def test_eval_fold_attention_gate_and_plain_ops_equal_torch():
    gen = torch.Generator().manual_seed(4)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)  # noqa: E731
    n, c = 37, 24
    y, gamma, beta, rm, rv = rnd(n, c), rnd(c), rnd(c), rnd(c), rnd(c).abs() + 1e-3
    scale, shift = EO.fold_eval(gamma, beta, rm, rv, EO.EPS)
    assert _rel(y * scale + shift, F.batch_norm(y, rm, rv, gamma, beta, training=False, eps=EO.EPS)) < 1e-10
    x, pre, g, ext = rnd(n, c).requires_grad_(True), rnd(n).requires_grad_(True), rnd(n, c), rnd(n)
    att = torch.sigmoid(pre)
    out = att.reshape(-1, 1) * x + x
    ((out * g).sum() + (att * ext).sum()).backward()
    dx, dpre, dbias = EO.att_bwd(x.detach(), att.detach(), g, ext)
    assert _rel(EO.att_fwd(x.detach(), att.detach()), out.detach()) < 1e-10 and _rel(dx, x.grad) < 1e-10 and _rel(dpre, pre.grad) < 1e-10 and abs(float(dbias - pre.grad.sum())) < 1e-10
    assert torch.equal(EO.channel_sum(y), y.sum(0)) and torch.equal(EO.add(y, g), y + g) and torch.equal(EO.copy(y), y)
    dw, db, dwr, dbr = rnd(5, 3, 9), rnd(5), rnd(15), rnd(5)
    w2, b2 = EO.merge_residual_grads(dw, db, dwr, dbr, 5, 3, 9, 4)
    assert torch.equal(w2, dwr + dw[:, :, 4].reshape(-1)) and torch.equal(b2, dbr + db)
    src, m, m2 = rnd(11), torch.tensor([3, -1, 0, 10, -1]), torch.tensor([-1, -1, 2, 10, 5])
    assert torch.equal(EO.gather(src, m, m2), torch.stack([src[3], src[0] * 0, src[0] + src[2], src[10] * 2, src[5]]))
    assert torch.equal(EO.gather(src, m), torch.stack([src[3], src[0] * 0, src[0], src[10], src[0] * 0]))
    kb = torch.tensor([0b00000101, 0xFF, 0x80], dtype=torch.uint8)
    assert EO.keep_bits(kb, 24).tolist() == [[1, 0, 1, 0, 0, 0, 0, 0] + [1] * 8 + [0] * 7 + [1]]


# ---------------------------------------------------------------------------------------------------------------------------------------------
# planted faults
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _f32(*ts):
    return [t.to(torch.float32) if torch.is_tensor(t) else torch.tensor(t, dtype=torch.float32) for t in ts]


def kernel_model(case, dt, keep, p, fault=None):
    """What the kernels compute, in fp32 (fp32 per-channel vectors, fp32 arithmetic per element, fp32 sums; a bf16 output is rounded once), with one
    optional planted fault.  Returns (out with the residual tensor, the backward results as check_bwd takes them)."""
    y, g, res, mean, invstd, gamma, scale, shift = _f32(case["y"], case["dout"], case.get("res", case["y"] * 0), case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"])
    alpha, inv_keep, n, c = float(case["alpha"]), torch.tensor(1.0 / (1.0 - p), dtype=torch.float32), y.shape[0], y.shape[1]
    keep = torch.ones_like(y) if keep is None else keep.to(torch.float32)
    if fault == "neighbour_keep_byte":
        keep = torch.roll(keep, 8, 1)  # the byte of the next 8-channel group
    z = y * scale + shift
    d = torch.where(keep > 0, z * inv_keep, torch.zeros_like(z))
    pos = d >= 0 if fault == "prelu_branch_ge" else d > 0
    if fault == "residual_before_activation":
        d2 = d + res
        out = torch.where(d2 > 0, d2, alpha * d2)
    else:
        out = torch.where(pos, d, alpha * d) + res
    dz = torch.where(keep > 0, torch.where(pos, g, alpha * g) * inv_keep, torch.zeros_like(z))
    w = torch.ones(n, 1)
    if fault == "last_voxel_dropped":
        w[-1] = 0.0
    if fault == "voxel_counted_twice":
        w[n // 3] = 2.0
    s1, s2, s3, dal = (w * dz).sum(0), (w * dz * (y - mean)).sum(0) * invstd, (w * g).sum(0), (w * torch.where(d < 0, g * d, torch.zeros_like(d))).sum()
    mean_dz, mean_dzx = s1 / n, s2 / n
    k1 = gamma * invstd
    xc = (y - mean) if fault == "mean_dzx_without_invstd" else (y - mean) * invstd
    dy = k1 * dz - k1 * (xc * mean_dzx + mean_dz)
    store = (lambda t: t.to(torch.bfloat16).to(F64)) if dt == "bf16" else (lambda t: t.to(F64))
    return store(out), {"dy": store(dy), "dgamma": s2, "dbeta": s1, "dalpha": dal.reshape(1), "dres_bias": s3, "mean_dz": mean_dz, "mean_dzx": mean_dzx}


def _judge(case, dt, keep, p, fault, chain):
    """Run the model through the GPU test's comparison helpers; returns the list of checks that rejected it."""
    ref_out = EO.bn_act_fwd(case["y"], case["scale"], case["shift"], case["alpha"], keep, p, res=case.get("res"))
    ref = EO.bn_act_bwd(case["y"], case["dout"], case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"], case["alpha"], keep, p)
    out, got = kernel_model(case, dt, keep, p, fault)
    rejected = []
    try:
        EO.check_out(dt, out, ref_out, "bn_act_fwd")
    except AssertionError:
        rejected.append("out")
    try:
        EO.check_bwd(dt, got, ref, chain, case["mean"], case["invstd"], float(case["y"].shape[0]))
    except AssertionError as e:
        rejected.append("bwd: " + str(e).split(":")[0])
    return rejected


FAULTS = ["last_voxel_dropped", "voxel_counted_twice", "neighbour_keep_byte", "residual_before_activation", "mean_dzx_without_invstd"]


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["c48_630vox", "c48_27600vox"])
def test_planted_faults_are_rejected_by_the_comparison_helpers(name, dt):
    case = EO.make_bn_case(name, dt)
    chain = EO.bn_launches(case["c"], case["nvox"])["reduce"]["chain"]
    keep = (torch.rand(case["nvox"], case["c"], generator=torch.Generator().manual_seed(8)) >= 0.1).to(F64)
    assert _judge(case, dt, keep, 0.1, None, chain) == [], "the fault-free fp32 model must pass"
    for fault in FAULTS:
        rejected = _judge(case, dt, keep, 0.1, fault, chain)
        print(f"planted fault {fault} [{name}, {dt}]: caught by {rejected}")
        assert rejected, f"{fault} was not caught"


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_planted_prelu_branch_on_zero_is_rejected_by_the_exact_case(dt):
    """d >= 0 instead of d > 0 differs only where z == 0 on a kept element: the exact-arithmetic case has y = 0 in a fifth of its elements."""
    case = EO.make_exact_case(shape=(1, 32, 32, 64))
    ref = EO.bn_act_bwd(case["y"], case["dout"], case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"], case["alpha"])
    for fault, same in ((None, True), ("prelu_branch_ge", False)):
        _, got = kernel_model(case, dt, None, 0.0, fault)
        eq = all(torch.equal(got[k].to(F64).reshape(-1), ref[k].reshape(-1)) for k in ("dgamma", "dbeta", "dalpha", "dres_bias"))
        eq = eq and torch.equal(got["dy"], EO._rt(ref["dy"], dt))
        print(f"planted fault {fault}: exact comparison {'equal' if eq else 'differs (caught)'}")
        assert eq == same


# ---------------------------------------------------------------------------------------------------------------------------------------------
# case audit
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_block_sizes_of_the_network_are_all_exercised():
    for cgs, blk in EO.NETWORK_BLOCKS.items():
        assert EO.block_for_cgs(cgs) == blk, (cgs, EO.block_for_cgs(cgs), blk)
    used = {(c // 8) for c, _, _, _ in EO.BN_CASES.values()} | {EO.EXACT_CASE[0] // 8}
    assert set(EO.NETWORK_BLOCKS) <= used, f"no BN case for the group counts {set(EO.NETWORK_BLOCKS) - used}"


def test_every_bn_case_reaches_the_path_it_is_there_for():
    seen = {k: {"body_then_tail": 0, "body_only": 0, "tail_only": 0, "idle": 0} for k in ("reduce", "apply")}
    for name, (c, shape, sliced, expect) in EO.BN_CASES.items():
        nvox = math.prod(shape)
        la = EO.bn_launches(c, nvox)
        for k in ("reduce", "apply", "fwd"):
            r = la[k]
            print(f"{name:14s} {k:6s}: block {r['block']:4d} grid {r['grid']:5d} voxel step {r['step']:6d} | voxel slots: body+tail {r['body_then_tail']:6d} body only {r['body_only']:6d} "
                  f"tail only {r['tail_only']:6d} idle {r['idle']:6d} | chain {r['chain']}")
            assert r["body_then_tail"] + r["body_only"] + r["tail_only"] + r["idle"] == r["step"]
        for k, v in expect.items():
            assert la["reduce"][k] == v, f"{name}: the backward reduce launch has {k} = {la['reduce'][k]}, the case was picked for {v}: re-pick its shape"
        for k in seen:
            for path in seen[k]:
                seen[k][path] += la[k][path] > 0
        assert la["reduce"]["grid"] <= EO.STAT_SHARDS
    # the apply launch is capped at 2048 workgroups only: a thread of it takes the unrolled body AND the tail on the exact-arithmetic tensor alone
    ea = EO.bn_launches(EO.EXACT_CASE[0], math.prod(EO.EXACT_CASE[1]))["apply"]
    print(f"exact case     apply : block {ea['block']} grid {ea['grid']} voxel step {ea['step']} | voxel slots: body+tail {ea['body_then_tail']} body only {ea['body_only']}")
    seen["apply"]["body_then_tail"] += ea["body_then_tail"] > 0
    assert all(v > 0 for k in seen for v in seen[k].values()), f"a path of the backward kernels is reached by no case: {seen}"
    # the capped grid: without the cap of 192 the 27 600-voxel case would need 216 workgroups
    c, shape, _, _ = EO.BN_CASES["c48_27600vox"]
    assert (math.prod(shape) * (c // 8) + 1) // 2 > 192 * EO.block_for_cgs(c // 8)
    # odd voxel counts / ragged ends: no case is a whole number of unrolled trips for every thread
    for name, (c, shape, _, _) in EO.BN_CASES.items():
        r = EO.bn_launches(c, math.prod(shape))["reduce"]
        assert r["tail_only"] + r["body_then_tail"] > 0, name


def test_exact_case_shares_shards_and_stays_in_the_fixed_point_range():
    c, shape = EO.EXACT_CASE
    nvox = math.prod(shape)
    la = EO.bn_launches(c, nvox)
    r = la["reduce"]
    print(f"exact case: reduce block {r['block']} grid {r['grid']} voxel step {r['step']} chain {r['chain']}; apply grid {la['apply']['grid']}; channel_sum grid {EO.channel_sum_grid(c, nvox)}")
    assert r["grid"] > EO.STAT_SHARDS, "no two workgroups share a shard: re-pick the shape"
    smallest = next(v for v in range(2048, nvox + 1, 2048) if EO.reduce_grid(c, v) > EO.STAT_SHARDS)
    print(f"smallest voxel count (in steps of 2048) with grid > {EO.STAT_SHARDS}: {smallest}; the case has {nvox}: {r['grid'] - EO.STAT_SHARDS} shards shared")
    assert smallest <= nvox <= smallest * 9 // 8
    g = EO.channel_sum_grid(c, nvox)
    assert g == 2048 and nvox > g * EO.block_for_cgs(2) // 2, "channel_sum's threads no longer loop on this tensor"
    case = EO.make_exact_case()
    worst = EO.workgroup_partials(case, c, nvox)
    print(f"largest |workgroup partial sum| {worst} (range {EO.FX_GRAD_RANGE})")
    assert worst < 0.9 * EO.FX_GRAD_RANGE
    ref = EO.bn_act_bwd(case["y"], case["dout"], case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"], case["alpha"])
    for ch in range(c):
        cls, want = EO.exact_design(ch, nvox // 16384)
        assert all(v != 0 for v in cls) and all(float(ref[k][ch]) == want[k] for k in ("dbeta", "dgamma", "dres_bias")) and want["dgamma"] != 0
    assert float(ref["dalpha"]) == sum(EO.exact_design(ch, nvox // 16384)[1]["dalpha"] for ch in range(c)) != 0
    assert torch.equal(ref["mean_dz"].float().double(), ref["mean_dz"]) and torch.equal(ref["dy"].float().double(), ref["dy"])  # fp32 numbers: the kernel's dy is exact
    assert float((case["y"] == 0).double().mean()) > 0.15


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_no_bn_case_has_an_element_near_the_prelu_kink(dt):
    for name in EO.BN_CASES:
        case = EO.make_bn_case(name, dt)  # asserts the margin itself
        z = case["y"] * case["scale"] + case["shift"]
        fp32_err = 3 * 2.0 ** -24 * float(((case["y"] * case["scale"]).abs() + case["shift"].abs()).max())
        assert float(z.abs().min()) >= EO.KINK_MARGIN * float(z.abs().max()) > 50 * fp32_err, name
        assert torch.equal(EO._rt(case["y"], dt), case["y"]) and torch.equal(EO._rt(case["dout"], dt), case["dout"])
