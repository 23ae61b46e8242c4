"""-m gpu: every streaming kernel of csrc/elementwise.hip, driven through the C ABI, against its fp64 definition (tests/elementwise_oracle.py) at ragged
shapes: odd voxel counts, threads that take the unrolled body and then the tail, the tail only or nothing, more workgroups than statistics shards, channel
slices of wider rows.  tests/test_elementwise_host.py audits (from the launch arithmetic) that each BN case reaches the path it is named for, and plants faults
against the comparison helpers used here.

Bars.  Output tensors: fp32 within 2e-5 max|ref|, bf16 within ONE correct rounding of that (inputs are bf16 values on both sides).  Per-channel sums
(dgamma, dbeta, dalpha, d(residual bias), mean_dz, mean_dzx): the derived bound of elementwise_oracle.sum_bound, about a hundred times tighter than one dropped
voxel at 27 600 voxels.  Integer-valued data and the exact-arithmetic case: equality.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import elementwise_oracle as EO  # noqa: E402
from tests import gpu_harness as H  # noqa: E402
from tests.rounding import rne_bf16  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

F64 = torch.float64
SENT = -77.0  # sentinel of everything a kernel must not write (a bf16 number)
SEED, SALT = 0x1234ABCD5678, 7


def _dev(v2d, shape, dt, pitch=None, c0=0):
    """fp64 [voxels, c] -> device channels-last [n, x, y, z, pitch] of dt, the values in channels [c0, c0 + c), the sentinel everywhere else."""
    c = v2d.shape[1]
    t = torch.full((*shape, pitch or c), SENT, dtype=F64)
    t[..., c0:c0 + c] = v2d.reshape(*shape, c)
    return t.to(torch.float32).cuda().to(H.DT[dt]).contiguous()


def _host(t, c, c0=0):
    return t[..., c0:c0 + c].detach().cpu().to(F64).reshape(-1, c)


def _sentinel_intact(t, c, c0=0):
    o = t.detach().cpu().to(F64)
    return bool((o[..., :c0] == SENT).all()) and bool((o[..., c0 + c:] == SENT).all())


def _f32(v):
    return v.to(torch.float32).cuda().contiguous()


def _vec(n, fill=SENT):
    return torch.full((n,), fill, dtype=torch.float32, device="cuda")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# BatchNorm -> Dropout -> PReLU: finalize, forward, both backward passes
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["p0", "regenerated", "stored"])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("name", list(EO.BN_CASES))
def test_bn_dropout_prelu_at_ragged_shapes(name, dt, mode):
    """One BN case of elementwise_oracle.BN_CASES: statistics finalisation (three shards, stride >= c), forward without and with a residual tensor, keep bytes
    against vsseg_dropout_mask, backward reduce / finalize / apply.  `stored`: the backward passes read the forward's keep bytes and get ANOTHER seed.
    The sliced case runs every tensor as channels [8, 88) of its own 96-wide parent filled with a sentinel, the statistics with stride 96."""
    lib, S = L.lib(), H.stream()
    case = EO.make_bn_case(name, dt)
    c, shape, nvox, sliced = case["c"], case["shape"], case["nvox"], EO.BN_CASES[name][2]
    pitch, c0, stride = (96, 8, 96) if sliced else (c, 0, c)
    p, stored = (0.0 if mode == "p0" else 0.1), mode == "stored"
    chain = EO.bn_launches(c, nvox)["reduce"]["chain"]
    ycl, gcl, rcl = (_dev(case[k], shape, dt, pitch, c0) for k in ("y", "dout", "res"))
    # statistics in three shards of the fixed-point buffer
    stats = torch.zeros(L.STAT_SHARDS, 2, stride, dtype=F64, device="cuda")
    for sh, sp, qp in zip((0, 5, L.STAT_SHARDS - 1), case["s_parts"], case["q_parts"]):
        stats[sh, 0, :c] = H.stat_encode(sp).cuda()
        stats[sh, 1, :c] = H.stat_encode(qp).cuda()
    gamma, beta, alpha = _f32(case["gamma"]), _f32(case["beta"]), torch.tensor([case["alpha"]], device="cuda")
    rm, rv, nb = _f32(case["rm"]), _f32(case["rv"]), torch.zeros(1, dtype=torch.int64, device="cuda")
    vec = torch.zeros(6, c, device="cuda")  # mean, invstd, scale, shift, mean_dz, mean_dzx
    vp = [vec[i].data_ptr() for i in range(6)]
    L.check(lib.vsseg_bn_finalize(stats.data_ptr(), stride, c, float(nvox), gamma.data_ptr(), beta.data_ptr(), EO.EPS, EO.MOMENTUM, rm.data_ptr(), rv.data_ptr(), nb.data_ptr(), vp[0], vp[1], vp[2], vp[3], S), "bn_finalize")
    torch.cuda.synchronize()
    erm, erv = EO.running_update(case["rm"], case["rv"], case["mean"], case["var_unb"], EO.MOMENTUM)
    for what, got, ref in (("mean", vec[0], case["mean"]), ("invstd", vec[1], case["invstd"]), ("scale", vec[2], case["scale"]), ("shift", vec[3], case["shift"]), ("running_mean", rm, erm), ("running_var", rv, erv)):
        err = float((got.cpu().double() - ref).abs().max())
        print(f"bn_finalize {what}: max |got - ref| = {err:.3g} (bar 1e-5)")
        assert err <= 1e-5, what
    assert int(nb) == 1
    # forward: without a residual (keep_out NULL) and with one (keep bytes stored)
    keep_b = torch.zeros(nvox * c // 8, dtype=torch.uint8, device="cuda")
    mask = torch.full((nvox * c,), SENT, device="cuda")
    L.check(lib.vsseg_dropout_mask(mask.data_ptr(), nvox, c, p, SEED, SALT, S), "dropout_mask")
    outs = []
    for has_res in (0, 1):
        out = _dev(torch.zeros(nvox, c, dtype=F64), shape, dt, pitch, c0)
        L.check(lib.vsseg_bn_act_fwd(H.tdesc(ycl, c, c0), vp[2], vp[3], alpha.data_ptr(), p, SEED, SALT, H.tdesc(rcl, c, c0) if has_res else L.Tensor(), has_res, H.tdesc(out, c, c0), keep_b.data_ptr() if has_res else None, S), "bn_act_fwd")
        outs.append(out)
    torch.cuda.synchronize()
    keep = mask.cpu().to(F64).reshape(nvox, c)
    assert torch.equal(EO.keep_bits(keep_b.cpu(), c), keep), "keep bytes differ from vsseg_dropout_mask"
    if p > 0:
        assert 0.8 < float(keep.mean()) < 0.97 and (nvox * c < 5000 or 0.88 < float(keep.mean()) < 0.92)
    else:
        assert bool((keep == 1).all())
    for has_res, out in enumerate(outs):
        EO.check_out(dt, _host(out, c, c0), EO.bn_act_fwd(case["y"], case["scale"], case["shift"], case["alpha"], keep, p, res=case["res"] if has_res else None), f"bn_act_fwd res={has_res}")
        assert _sentinel_intact(out, c, c0), "bn_act_fwd wrote outside its channel slice"
    # backward
    ref = EO.bn_act_bwd(case["y"], case["dout"], case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"], case["alpha"], keep, p)
    sums = torch.zeros(L.STAT_SHARDS, 3, stride, dtype=F64, device="cuda")
    aacc = torch.zeros(L.STAT_SHARDS, dtype=F64, device="cuda")
    seed_b = SEED ^ 0x5A5A5A5A if stored else SEED  # stored: a regenerated mask would be a different one
    kptr = keep_b.data_ptr() if stored else None
    common = [vp[0], vp[1], gamma.data_ptr(), beta.data_ptr(), vp[2], vp[3], alpha.data_ptr(), p, seed_b, SALT]
    L.check(lib.vsseg_bn_act_bwd_reduce(H.tdesc(ycl, c, c0), H.tdesc(gcl, c, c0), *common, sums.data_ptr(), stride, aacc.data_ptr(), kptr, S), "bn_act_bwd_reduce")
    dg, db, da, drb = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(c, device="cuda")
    L.check(lib.vsseg_bn_act_bwd_finalize(sums.data_ptr(), stride, aacc.data_ptr(), c, float(nvox), dg.data_ptr(), db.data_ptr(), da.data_ptr(), vp[4], vp[5], drb.data_ptr(), S), "bn_act_bwd_finalize")
    dy = _dev(torch.zeros(nvox, c, dtype=F64), shape, dt, pitch, c0)
    L.check(lib.vsseg_bn_act_bwd_apply(H.tdesc(ycl, c, c0), H.tdesc(gcl, c, c0), *common, vp[4], vp[5], H.tdesc(dy, c, c0), kptr, S), "bn_act_bwd_apply")
    torch.cuda.synchronize()
    assert L.fx_status() is False
    assert bool((sums[:, :, c:].view(torch.int64) == 0).all()), "the statistics columns beyond c were written"
    for t in (ycl, gcl, rcl, dy):
        assert _sentinel_intact(t, c, c0), "a backward kernel wrote outside its channel slice"
    got = {"dy": _host(dy, c, c0), "dgamma": dg, "dbeta": db, "dalpha": da, "dres_bias": drb, "mean_dz": vec[4], "mean_dzx": vec[5]}
    EO.check_bwd(dt, got, ref, chain, case["mean"], case["invstd"], float(nvox))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# exact arithmetic: two workgroups per shard, capped grids
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def exact():
    case = EO.make_exact_case()
    case["ref"] = EO.bn_act_bwd(case["y"], case["dout"], case["mean"], case["invstd"], case["gamma"], case["scale"], case["shift"], case["alpha"])
    return case


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_exact_sums_when_workgroups_share_a_shard(exact, dt):
    """elementwise_oracle.make_exact_case: every summand is a multiple of 1/4, so the backward sums of the 288-workgroup launch (shards 0..31 receive two
    workgroups each) equal the fp64 definition exactly, as do mean_dz, mean_dzx and dy.  y = 0 takes the alpha branch and adds nothing to dalpha.
    The same tensors give the exact channel_sum (grid capped, threads loop) and add_inplace checks."""
    lib, S = L.lib(), H.stream()
    c, shape, nvox, ref = exact["c"], exact["shape"], exact["nvox"], exact["ref"]
    ycl, gcl = _dev(exact["y"], shape, dt), _dev(exact["dout"], shape, dt)
    vec = torch.zeros(6, c, device="cuda")
    vec[1], vec[2] = 1.0, 1.0  # mean 0, invstd 1, scale 1, shift 0
    vp = [vec[i].data_ptr() for i in range(6)]
    gamma, beta, alpha = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda"), torch.tensor([0.5], device="cuda")
    sums = torch.zeros(L.STAT_SHARDS, 3, c, dtype=F64, device="cuda")
    aacc = torch.zeros(L.STAT_SHARDS, dtype=F64, device="cuda")
    common = [vp[0], vp[1], gamma.data_ptr(), beta.data_ptr(), vp[2], vp[3], alpha.data_ptr(), 0.0, 0, 1]
    L.check(lib.vsseg_bn_act_bwd_reduce(H.tdesc(ycl), H.tdesc(gcl), *common, sums.data_ptr(), c, aacc.data_ptr(), None, S), "bn_act_bwd_reduce")
    dg, db, da, drb = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(c, device="cuda")
    L.check(lib.vsseg_bn_act_bwd_finalize(sums.data_ptr(), c, aacc.data_ptr(), c, float(nvox), dg.data_ptr(), db.data_ptr(), da.data_ptr(), vp[4], vp[5], drb.data_ptr(), S), "bn_act_bwd_finalize")
    dy = torch.full_like(ycl, SENT)
    L.check(lib.vsseg_bn_act_bwd_apply(H.tdesc(ycl), H.tdesc(gcl), *common, vp[4], vp[5], H.tdesc(dy), None, S), "bn_act_bwd_apply")
    torch.cuda.synchronize()
    assert L.fx_status() is False
    used = (sums.view(torch.int64) != 0).any(2).any(1)
    assert int(used.sum()) == L.STAT_SHARDS, "the launch no longer fills every shard: no shard is shared"
    for what, got, want in (("dgamma", dg, ref["dgamma"]), ("dbeta", db, ref["dbeta"]), ("dalpha", da, ref["dalpha"].reshape(1)), ("d(residual bias)", drb, ref["dres_bias"]),
                            ("mean_dz", vec[4], ref["mean_dz"]), ("mean_dzx", vec[5], ref["mean_dzx"]), ("mean_dz * count", vec[4].double() * nvox, ref["dbeta"])):
        assert torch.equal(got.cpu().double(), want), f"{what}: {got.cpu().tolist()} != {want.tolist()}"
    want_dy = rne_bf16(ref["dy"]) if dt == "bf16" else ref["dy"]
    assert torch.equal(_host(dy, c), want_dy), f"dy differs in {int((_host(dy, c) != want_dy).sum())} elements"
    # channel_sum (+=) and add_inplace on the same tensors
    out = torch.arange(1, c + 9, dtype=torch.float32, device="cuda")
    L.check(lib.vsseg_channel_sum(H.tdesc(ycl), out.data_ptr(), S), "channel_sum")
    L.check(lib.vsseg_add_inplace(H.tdesc(ycl), H.tdesc(gcl), S), "add_inplace")
    torch.cuda.synchronize()
    want = torch.arange(1, c + 9, dtype=F64)
    want[:c] += exact["y"].sum(0)
    assert torch.equal(out.cpu().double(), want)
    assert torch.equal(_host(ycl, c), exact["y"] + exact["dout"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
# forward with the one-channel residual convolution; eval fold
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("c", [16, 32])
def test_bn_act_fwd_with_one_channel_residual_convolution(c, dt, p):
    """vsseg_bn_act_fwd_res1 = PReLU(drop(BN(y))) + x1*rw + rb with a one-channel x1 of the same dtype; keep bytes as vsseg_bn_act_fwd writes them."""
    lib, S = L.lib(), H.stream()
    case = EO.make_bn_case(f"c{c}_210vox", dt)
    shape, nvox = case["shape"], case["nvox"]
    gen = torch.Generator().manual_seed(21)
    x1 = EO._rt(torch.randn(nvox, generator=gen, dtype=F64), dt)
    rw, rb = EO._rt(torch.randn(c, generator=gen, dtype=F64), "fp32"), EO._rt(torch.randn(c, generator=gen, dtype=F64), "fp32")
    scale, shift = EO._rt(case["scale"], "fp32"), EO._rt(case["shift"], "fp32")  # the fp32 vectors are the inputs here
    ycl, x1d = _dev(case["y"], shape, dt), x1.to(torch.float32).cuda().to(H.DT[dt])
    sc, sh, al, rwd, rbd = _f32(scale), _f32(shift), torch.tensor([case["alpha"]], device="cuda"), _f32(rw), _f32(rb)
    keep_ref = torch.zeros(nvox * c // 8, dtype=torch.uint8, device="cuda")
    tmp = torch.zeros_like(ycl)
    L.check(lib.vsseg_bn_act_fwd(H.tdesc(ycl), sc.data_ptr(), sh.data_ptr(), al.data_ptr(), p, SEED, SALT, L.Tensor(), 0, H.tdesc(tmp), keep_ref.data_ptr(), S), "bn_act_fwd")
    torch.cuda.synchronize()
    keep = EO.keep_bits(keep_ref.cpu(), c)
    ref = EO.bn_act_fwd(case["y"], scale, shift, case["alpha"], keep, p, x1=x1, rw=rw, rb=rb)
    for with_keep in (True, False):
        out = torch.full_like(ycl, SENT)
        keep_b = torch.zeros(nvox * c // 8 + 8, dtype=torch.uint8, device="cuda")
        L.check(lib.vsseg_bn_act_fwd_res1(H.tdesc(ycl), sc.data_ptr(), sh.data_ptr(), al.data_ptr(), p, SEED, SALT, x1d.data_ptr(), rwd.data_ptr(), rbd.data_ptr(), H.tdesc(out), keep_b.data_ptr() if with_keep else None, S), "bn_act_fwd_res1")
        torch.cuda.synchronize()
        EO.check_out(dt, _host(out, c), ref, f"bn_act_fwd_res1 keep_out={with_keep}")
        if with_keep:
            assert torch.equal(keep_b[:-8], keep_ref) and int(keep_b[-8:].sum()) == 0


@pytest.mark.parametrize("c", [1, 16, 63, 64, 65, 160])
def test_bn_fold_eval(c):
    """scale = gamma / sqrt(rv + eps), shift = beta - rm*scale at channel counts on either side of the 64-thread block, running variances from 1e-3 to 1e3.
    The build has no fast-math flag: sqrtf and the division are correctly rounded, so scale is three fp32 roundings from the definition (3 * 2^-24 relative)
    and shift within 2^-23 (|beta| + 4 |rm*scale|)."""
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(c)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)  # noqa: E731
    gamma, beta, rm = EO._rt(rnd(c), "fp32"), EO._rt(rnd(c), "fp32"), EO._rt(rnd(c) * 3, "fp32")
    rv = EO._rt(10.0 ** (torch.rand(c, generator=gen, dtype=F64) * 6 - 3), "fp32")
    rv[-1], rv[0] = EO._rt(torch.tensor(1e3, dtype=F64), "fp32"), EO._rt(torch.tensor(1e-3, dtype=F64), "fp32")
    scale, shift = _vec(c + 8), _vec(c + 8)
    gd, bd, rmd, rvd = _f32(gamma), _f32(beta), _f32(rm), _f32(rv)
    L.check(lib.vsseg_bn_fold_eval(gd.data_ptr(), bd.data_ptr(), rmd.data_ptr(), rvd.data_ptr(), EO.EPS, scale.data_ptr(), shift.data_ptr(), c, S), "bn_fold_eval")
    torch.cuda.synchronize()
    eps32 = float(torch.tensor(EO.EPS, dtype=torch.float32))  # the kernel's eps is the fp32 argument
    rs, rsh = EO.fold_eval(gamma, beta, rm, rv, eps32)
    EO.check_sum(scale[:c], rs, 3 * EO.U24 * rs.abs() + 1e-45, "bn_fold_eval scale")
    EO.check_sum(shift[:c], rsh, EO.U23 * (beta.abs() + 4 * (rm * rs).abs()) + 1e-45, "bn_fold_eval shift")
    assert bool((scale[c:] == SENT).all()) and bool((shift[c:] == SENT).all())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# sums, copies, merges, gathers: exact where the arithmetic allows
# ---------------------------------------------------------------------------------------------------------------------------------------------
SHAPE210 = (2, 5, 7, 3)


def _ints(gen, *size, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, size, generator=gen).to(F64)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("c,pitch", [(1, 8), (2, 8), (16, 16), (48, 48), (80, 96)])
def test_channel_sum_is_exact_on_integers(c, pitch, dt):
    """out[0..c) += per-channel sums; small integers sum exactly in fp32 in any order.  Padding channels hold 2^15: they must not leak into out[0..c), and out[c..] stays."""
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(100 + c)
    nvox = math.prod(SHAPE210)
    t = torch.full((nvox, pitch), 32768.0, dtype=F64)
    t[:, :c] = _ints(gen, nvox, c)
    tcl = _dev(t, SHAPE210, dt)
    pre = torch.arange(3, 3 + pitch + 8, dtype=F64)
    out = _f32(pre)
    L.check(lib.vsseg_channel_sum(H.tdesc(tcl, c, 0), out.data_ptr(), S), "channel_sum")
    torch.cuda.synchronize()
    want = pre.clone()
    want[:c] += EO.channel_sum(t[:, :c])
    assert torch.equal(out.cpu().double(), want)


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("sdt,ddt", [("fp32", "fp32"), ("fp32", "bf16"), ("bf16", "fp32"), ("bf16", "bf16")])
@pytest.mark.parametrize("c,sp,dp", [(3, 8, 16), (16, 16, 16)])
def test_pitched_copy_cast_and_add_inplace_are_exact_on_integers(c, sp, dp, sdt, ddt, add):
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(7)
    nvox = math.prod(SHAPE210)
    src, dst0 = _ints(gen, nvox, c), _ints(gen, nvox, c)
    scl, dcl = _dev(src, SHAPE210, sdt, sp), _dev(dst0, SHAPE210, ddt, dp)
    if add:
        L.check(lib.vsseg_add_inplace(H.tdesc(dcl, c, 0), H.tdesc(scl, c, 0), S), "add_inplace")
    else:
        L.check(lib.vsseg_copy_cast(H.tdesc(scl, c, 0), H.tdesc(dcl, c, 0), S), "copy_cast")
    torch.cuda.synchronize()
    assert torch.equal(_host(dcl, c), EO.add(dst0, src) if add else EO.copy(src))
    assert _sentinel_intact(dcl, c) and torch.equal(_host(scl, c), src) and _sentinel_intact(scl, c)


@pytest.mark.parametrize("add", [False, True])
def test_copy_and_add_into_bf16_round_to_nearest_even(add):
    """Non-integer fp32 source into a bf16 destination: one rounding of the exact value (the addends are multiples of 2^-8, so the fp32 sum is exact)."""
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(8)
    nvox, c = math.prod(SHAPE210), 3
    src = _ints(gen, nvox, c, lo=-1024, hi=1024) / 256.0 if add else EO._rt(torch.randn(nvox, c, generator=gen, dtype=F64), "fp32")
    dst0 = _ints(gen, nvox, c)
    scl, dcl = _dev(src, SHAPE210, "fp32", 8), _dev(dst0, SHAPE210, "bf16", 16)
    if add:
        L.check(lib.vsseg_add_inplace(H.tdesc(dcl, c, 0), H.tdesc(scl, c, 0), S), "add_inplace")
    else:
        L.check(lib.vsseg_copy_cast(H.tdesc(scl, c, 0), H.tdesc(dcl, c, 0), S), "copy_cast")
    torch.cuda.synchronize()
    want = rne_bf16(dst0 + src if add else src)
    assert float((want != (dst0 + src if add else src)).double().mean()) > 0.5  # the rounding is really exercised
    assert torch.equal(_host(dcl, c), want) and _sentinel_intact(dcl, c)


@pytest.mark.parametrize("cout,cin,taps,centre", [(16, 1, 9, 4), (32, 16, 27, 13), (5, 3, 1, 0)])
def test_merge_residual_grads_is_exact_on_integers(cout, cin, taps, centre):
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(cout)
    dw, db, dwr, dbr = _ints(gen, cout * cin * taps), _ints(gen, cout), _ints(gen, cout * cin), _ints(gen, cout)
    pad = torch.full((8,), SENT, dtype=F64)
    dwd, dbd, dwrd, dbrd = _f32(dw), _f32(db), _f32(torch.cat([dwr, pad])), _f32(torch.cat([dbr, pad]))
    L.check(lib.vsseg_merge_residual_grads(dwd.data_ptr(), dbd.data_ptr(), dwrd.data_ptr(), dbrd.data_ptr(), cout, cin, taps, centre, S), "merge_residual_grads")
    torch.cuda.synchronize()
    w2, b2 = EO.merge_residual_grads(dw, db, dwr, dbr, cout, cin, taps, centre)
    assert torch.equal(dwrd.cpu().double(), torch.cat([w2, pad])) and torch.equal(dbrd.cpu().double(), torch.cat([b2, pad]))
    assert torch.equal(dwd.cpu().double(), dw) and torch.equal(dbd.cpu().double(), db)


@pytest.mark.parametrize("ddt", ["fp32", "bf16"])
@pytest.mark.parametrize("n", [0, 1, 257, 100003])
def test_gather_cast_with_holes_and_a_second_map(n, ddt):
    """dst[i] = src[map[i]] + src[map2[i]], -1 = nothing.  The source holds multiples of 2^-8 (the fp32 sum of two is exact): fp32 exactly, bf16 one rounding."""
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(n + 1)
    src = _ints(gen, 1000, lo=-1024, hi=1024) / 256.0
    m = torch.randint(-250, 1000, (n,), generator=gen).clamp(min=-1).to(torch.int32)
    m2 = torch.randint(-250, 1000, (n,), generator=gen).clamp(min=-1).to(torch.int32)
    srcd, md, m2d = _f32(src), torch.cat([m, torch.zeros(1, dtype=torch.int32)]).cuda(), torch.cat([m2, torch.zeros(1, dtype=torch.int32)]).cuda()
    for second in (True, False):
        dst = torch.full((n + 8,), SENT, dtype=H.DT[ddt], device="cuda")
        L.check(lib.vsseg_gather_cast(srcd.data_ptr(), md.data_ptr(), m2d.data_ptr() if second else None, dst.data_ptr(), n, L.F32 if ddt == "fp32" else L.BF16, S), "gather_cast")
        torch.cuda.synchronize()
        ref = EO.gather(src, m, m2 if second else None)
        want = rne_bf16(ref) if ddt == "bf16" else ref
        assert torch.equal(dst[:n].cpu().double(), want) and bool((dst[n:] == SENT).all())
    if n > 100:
        assert int((m < 0).sum()) > 0 and int(((m >= 0) & (m2 < 0)).sum()) > 0 and int(((m < 0) & (m2 >= 0)).sum()) > 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# attention gate
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("c", [8, 24, 40, 160])
def test_attention_gate_at_an_odd_voxel_count(c, dt):
    """out = x (1 + att); dx = g (1 + att) (fresh, += or not produced), d(pre-sigmoid) = (sum_c g x + datt_ext) att (1 - att) in channel 0 of an 8-wide row and / or
    as a compact copy; 210 voxels, 1 / 4 (3 live) / 8 (5 live) / 32 lanes per voxel.  dbias = sum dpre within (1 + 8) 2^-24 sum|dpre| (one voxel per thread)."""
    lib, S = L.lib(), H.stream()
    gen = torch.Generator().manual_seed(60 + c)
    nvox = math.prod(SHAPE210)
    rnd = lambda *s: torch.randn(*s, generator=gen, dtype=F64)  # noqa: E731
    x, g, dx0 = EO._rt(rnd(nvox, c), dt), EO._rt(rnd(nvox, c), dt), EO._rt(rnd(nvox, c), dt)
    att, ext = EO._rt(torch.sigmoid(rnd(nvox)), "fp32"), EO._rt(rnd(nvox), "fp32")
    xcl, gcl, attd, extd = _dev(x, SHAPE210, dt), _dev(g, SHAPE210, dt), _f32(att), _f32(ext)
    out = torch.full_like(xcl, SENT)
    L.check(lib.vsseg_att_apply_fwd(H.tdesc(xcl), attd.data_ptr(), H.tdesc(out), S), "att_apply_fwd")
    torch.cuda.synchronize()
    EO.check_out(dt, _host(out, c), EO.att_fwd(x, att), "att_apply_fwd")
    rdx, rdpre, rdbias = EO.att_bwd(x, att, g, ext)
    for acc, wide in ((0, True), (1, False), (2, True)):
        dx = _dev(dx0, SHAPE210, dt)
        dpre = torch.full((*SHAPE210, 8), SENT, dtype=H.DT[dt], device="cuda")
        dpre1 = torch.full((nvox + 8,), SENT, dtype=H.DT[dt], device="cuda")
        dbias = torch.zeros(1, device="cuda")
        L.check(lib.vsseg_att_apply_bwd(H.tdesc(xcl), attd.data_ptr(), H.tdesc(gcl), extd.data_ptr(), H.tdesc(dx), acc, H.tdesc(dpre) if wide else L.Tensor(), dbias.data_ptr(), dpre1.data_ptr(), S), "att_apply_bwd")
        torch.cuda.synchronize()
        if acc == 2:
            assert torch.equal(_host(dx, c), dx0), "accumulate_dx = 2 must leave dx alone"
        else:
            EO.check_out(dt, _host(dx, c), rdx + dx0 if acc else rdx, f"att_apply_bwd dx accumulate={acc}")
        EO.check_out(dt, dpre1[:nvox].cpu().double().reshape(-1, 1), rdpre.reshape(-1, 1), f"att_apply_bwd dpre1 accumulate={acc}")
        assert bool((dpre1[nvox:] == SENT).all())
        if wide:
            assert torch.equal(dpre[..., 0].reshape(-1), dpre1[:nvox]) and float(dpre[..., 1:].float().abs().max()) == 0.0
        else:
            assert bool((dpre == SENT).all())
        EO.check_sum(dbias, rdbias.reshape(1), (1 + 8) * EO.U24 * rdpre.abs().sum().reshape(1), f"att_apply_bwd dbias accumulate={acc}")
