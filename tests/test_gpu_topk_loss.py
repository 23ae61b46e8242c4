"""-m gpu: the top-k cross-entropy term of the loss (Dice_spvPA(ce_weight=, ce_topk=); vsseg_topk_select / vsseg_ce_topk_select / vsseg_dice_ce_topk_finalize /
vsseg_dice_ce_topk_pred_bwd[_to]) against tests/topk_oracle.py: the radix select against numpy's sort of the keys, bit for bit, and loss and gradients against the fp64
CPU oracle = oracle.vsseg_oracle.dice_spvpa + ce_weight * F.cross_entropy(reduction='none').flatten().topk(K).values.mean() with autograd.

The bars are the ones tests/test_gpu_ce_loss.py holds the loss to: loss within 5e-6, gradients atol 2e-9 / rtol 2e-4.  The kernel ranks fp32 values, the oracle fp64 ones:
a voxel within |v - t| <= 1e-5 t + 1e-6 of the oracle's threshold (about 30 x the fp32 evaluation error of v at these magnitudes: a margin) may fall on either side, and
its gradient must then be the oracle's "selected" or "not selected" one; at most 4 voxels may lie in that band, asserted on the oracle's values first."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vs_seg_amd as V  # noqa: E402
from tests import ce_oracle as CO  # noqa: E402
from tests import gpu_harness as H  # noqa: E402
from tests import topk_oracle as TO  # noqa: E402
from tests.helpers import synth_input, synth_label  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

BIG, ODD = (2, 1, 32, 32, 8), (1, 1, 5, 3, 7)  # (16-byte loads, four voxels per thread, several workgroups per pass) / (odd voxel count: the scalar path)
PAIRS = [(1.0, 1.0), (0.5, 4.0)]  # (ce_weight, ce_foreground_weight)
ATOL, RTOL, LOSS_BAR = 2e-9, 2e-4, 5e-6


def _record(rec: torch.Tensor):
    """(threshold_bits, passes_done, n_gt, n_eq, K) of the first 32 bytes of the select's record (include/vsseg_hip.h), given as four int64."""
    r = [int(v) for v in rec.cpu().tolist()]
    return r[0] & 0xFFFFFFFF, (r[0] >> 32) & 0xFFFFFFFF, r[1], r[2], r[3]


# ---------------------------------------------------------------- A: the select is exact
def _select_inputs(name):
    rng = np.random.default_rng(123)
    if name == "random":  # an odd length spanning many workgroups: the scalar path
        return np.exp(3.0 * rng.standard_normal(100003)).astype(np.float32)
    if name == "equal":
        return np.full(5000, 0.7, np.float32)
    if name == "two_values":
        return rng.permutation(np.concatenate([np.full(3000, 1.5, np.float32), np.full(5000, 0.25, np.float32)]))
    if name == "lowest_digit":  # decided by the last digit alone
        j = np.repeat(np.arange(1024, dtype=np.uint32), 4)
        return rng.permutation((np.uint32(0x3F800000) + j).view(np.float32))
    if name == "magnitudes":  # denormals to 1e30, zeros, -0 and +inf
        a = (10.0 ** rng.uniform(-46.0, 30.0, 20001)).astype(np.float32)
        a[::97] = 0.0
        a[5::101] = -0.0
        a[7::1013] = np.inf
        a[11::503] = np.float32(1e-45)
        assert (a == 0).sum() > 300 and np.isinf(a).sum() > 10 and ((a > 0) & (a < 1e-38)).sum() > 100 and np.signbit(a).sum() > 100
        return a
    if name == "nans":
        a = np.exp(2.0 * rng.standard_normal(4099)).astype(np.float32)
        a[[3, 500, 501, 1777, 4000, 4097, 4098]] = np.nan
        return a
    raise KeyError(name)


@pytest.mark.parametrize("name", ["random", "equal", "two_values", "lowest_digit", "magnitudes", "nans"])
def test_select_equals_the_sorted_keys_bit_for_bit(name):
    lib = L.lib()
    a = _select_inputs(name)
    n = a.size
    v = torch.from_numpy(a).cuda()
    assert np.array_equal(v.cpu().numpy().view(np.uint32), a.view(np.uint32))
    for k in (1, 2, n // 10, n - 1, n):
        scratch = torch.zeros(L.topk_scratch_bytes() // 8, dtype=torch.int64, device="cuda")
        L.check(lib.vsseg_topk_select(v.data_ptr(), n, k, scratch.data_ptr(), H.stream()), "topk_select")
        t, passes, n_gt, n_eq, kk = _record(scratch[:4])
        want = TO.select(a, k)
        print(f"{name} n={n} k={k}: threshold {t:#010x} n_gt {n_gt} n_eq {n_eq}; sorted keys {want[0]:#010x} {want[1]} {want[2]}")
        assert (t, n_gt, n_eq) == want and kk == k and passes == 3
        assert n_gt < k <= n_gt + n_eq
        if name == "nans" and k <= 7:
            assert t == 0xFFFFFFFF and n_gt == 0 and n_eq == 7


# ---------------------------------------------------------------- B: loss and gradients against the fp64 oracle
def _inputs(shape, seed=32):
    """CPU tensors: label (sample 0 of a batch of two has no foreground), logits = 3 * N(0, 1), the attention maps of the golden loss test (none at the odd shape)."""
    y = synth_label(31, shape)
    logits = 3.0 * synth_input(seed, (shape[0], 2, *shape[2:]))
    atts = [torch.sigmoid(synth_input(40 + i, s)) for i, s in enumerate(CO.ATT_SHAPES)] if shape == BIG else []
    return y, logits, atts


@functools.lru_cache(maxsize=None)
def _oracle(shape, hard, pct, lam, w_fg):
    y, logits, atts = _inputs(shape)
    return TO.loss_and_grads(logits, atts, y, supervised_attention=bool(atts), hardness_weighting=hard, ce_weight=lam, ce_foreground_weight=w_fg, ce_topk=pct)


def _run(shape, hard, pct, lam, w_fg, inputs=None):
    y, logits, atts = inputs or _inputs(shape)
    y, logits = y.cuda(), logits.cuda().requires_grad_(True)
    atts = [a.cuda().requires_grad_(True) for a in atts]
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=bool(atts), hardness_weighting=hard, ce_weight=lam, ce_foreground_weight=w_fg, ce_topk=pct)
    loss = fn((logits, atts), y)
    assert loss.dim() == 0
    loss.backward()
    return loss, logits, atts, fn


@pytest.mark.parametrize("shape", [BIG, ODD])
@pytest.mark.parametrize("lam,w_fg", PAIRS)
@pytest.mark.parametrize("pct", [1.0, 10.0, 50.0])
@pytest.mark.parametrize("hard", [True, False])
def test_dice_topk_loss_and_gradients_match_the_fp64_oracle(hard, pct, lam, w_fg, shape):
    want, wlog, watts, ex = _oracle(shape, hard, pct, lam, w_fg)
    v, t, k = ex["values"], ex["threshold"], ex["k"]
    band = (v - t).abs() <= 1e-5 * t + 1e-6  # [B, X, Y, Z]
    assert 1 <= int(band.sum()) <= 4, f"{int(band.sum())} voxels within rounding of the oracle's threshold"  # (before the kernel is consulted)
    loss, logits, atts, fn = _run(shape, hard, pct, lam, w_fg)
    tb, passes, n_gt, n_eq, kk = _record(fn.topk_record)
    got = logits.grad.cpu().double()
    err = abs(loss.item() - want)
    print(f"{shape} hard={hard} P={pct} ce=({lam}, {w_fg}): K {k}, loss {loss.item():.9g} oracle {want:.9g} |diff| {err:.3g}; threshold {np.uint32(tb).view(np.float32):.9g} oracle {t:.9g}, "
          f"n_gt {n_gt} n_eq {n_eq}, {int(band.sum())} voxels in the band; max |dlogits diff| {float((got - wlog).abs().max()):.3g}, max |dlogits| {float(wlog.abs().max()):.3g}")
    assert kk == k == V.topk_count(v.numel(), pct) and passes == 3 and n_gt < k <= n_gt + n_eq
    assert abs(float(np.uint32(tb).view(np.float32)) - t) <= 1e-5 * t + 1e-6
    assert np.isfinite(loss.item()) and err < LOSS_BAR
    b2 = band[:, None].expand_as(got)
    out = ~b2
    np.testing.assert_allclose(got[out].numpy(), wlog[out].numpy(), atol=ATOL, rtol=RTOL)
    # in the band: the oracle's gradient had the voxel been selected, or had it not (per voxel: both channels on the same side)
    inb, sel, unsel = (g.permute(0, 2, 3, 4, 1)[band].numpy() for g in (got, ex["selected_grad"], ex["dice_grad"]))  # [voxels in the band, 2]
    ok = np.isclose(inb, sel, atol=ATOL, rtol=RTOL).all(1) | np.isclose(inb, unsel, atol=ATOL, rtol=RTOL).all(1)
    assert ok.all(), (inb, sel, unsel)
    for a, w in zip(atts, watts):
        np.testing.assert_allclose(a.grad.cpu().numpy(), w.numpy(), atol=ATOL, rtol=RTOL)


# ---------------------------------------------------------------- C, D: ties, P = 100
def _by_hand(y, logits, hard, lam, w_fg, k):
    """fp64: the oracle's Dice loss and gradient plus the hand-written top-k value and gradient (defined with ties, where torch.topk picks arbitrarily)."""
    dice, gdice, _ = CO.loss_and_grads(logits, [], y, supervised_attention=False, hardness_weighting=hard, ce_weight=0.0, ce_foreground_weight=1.0)
    val, g, info, _ = TO.topk_by_hand(logits.double(), y.double(), w_fg, k)
    return dice + lam * float(val), gdice + lam * g, info


def test_constant_logits_tie_every_voxel_and_give_the_plain_term():
    y = synth_label(31, BIG)
    logits = torch.full((2, 2, 32, 32, 8), 0.7)
    n = y.numel()
    loss, lg, _, fn = _run(BIG, True, 10.0, 0.5, 1.0, (y, logits, []))
    ploss, plg, _, _ = _run(BIG, True, 0.0, 0.5, 1.0, (y, logits, []))
    tb, passes, n_gt, n_eq, k = _record(fn.topk_record)
    assert (n_gt, n_eq, k, passes) == (0, n, V.topk_count(n, 10.0), 3) and abs(float(np.uint32(tb).view(np.float32)) - np.log(2.0)) < 1e-6
    assert abs(loss.item() - ploss.item()) < LOSS_BAR
    np.testing.assert_allclose(lg.grad.cpu().numpy(), plg.grad.cpu().numpy(), atol=ATOL, rtol=RTOL)
    want, wg, _ = _by_hand(y, logits, True, 0.5, 1.0, k)
    assert abs(loss.item() - want) < LOSS_BAR
    np.testing.assert_allclose(lg.grad.cpu().numpy(), wg.numpy(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("lam,w_fg", PAIRS)
def test_two_values_select_the_foreground_and_share_the_rest_among_the_background(lam, w_fg):
    """Logits (1, 0) everywhere: every foreground voxel is wrong (v = w_fg softplus(1)), every background voxel right (softplus(-1)); K > N_fg."""
    y = synth_label(31, BIG)
    logits = torch.zeros(2, 2, 32, 32, 8)
    logits[:, 0] = 1.0
    n, n_fg = y.numel(), int((y == 1).sum())
    loss, lg, _, fn = _run(BIG, True, 10.0, lam, w_fg, (y, logits, []))
    tb, passes, n_gt, n_eq, k = _record(fn.topk_record)
    assert 0 < n_fg < k and (n_gt, n_eq) == (n_fg, n - n_fg)
    want, wg, (t, o_gt, o_eq, share) = _by_hand(y, logits, True, lam, w_fg, k)
    assert (o_gt, o_eq) == (n_gt, n_eq) and abs(share - (k - n_fg) / (n - n_fg)) < 1e-15
    assert abs(loss.item() - want) < LOSS_BAR
    np.testing.assert_allclose(lg.grad.cpu().numpy(), wg.numpy(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("shape", [BIG, ODD])
def test_all_voxels_with_unit_weights_is_the_plain_term(shape):
    loss, lg, atts, fn = _run(shape, True, 100.0, 0.5, 1.0)
    ploss, plg, patts, _ = _run(shape, True, 0.0, 0.5, 1.0)
    n = lg[:, 0].numel()
    _, _, n_gt, n_eq, k = _record(fn.topk_record)
    assert k == n and n_gt + n_eq == n
    print(f"{shape}: P = 100 loss {loss.item():.9g}, plain term {ploss.item():.9g}")
    assert abs(loss.item() - ploss.item()) < LOSS_BAR
    np.testing.assert_allclose(lg.grad.cpu().numpy(), plg.grad.cpu().numpy(), atol=ATOL, rtol=RTOL)
    for a, b in zip(atts, patts):
        assert torch.equal(a.grad, b.grad)


# ---------------------------------------------------------------- E, G: off is today's loss; the two routes
def _both_routes(fn):
    """(loss, d logits [B,2,X,Y,Z], [d att]) of the autograd route and (loss, bf16 destination, buffers, written) of forward_backward_into, on the inputs of test B."""
    y, lg, atts = _inputs(BIG)
    y = y.cuda()
    lg_cl = lg.permute(0, 2, 3, 4, 1).contiguous().cuda()
    logits = lg_cl.permute(0, 4, 1, 2, 3).detach().requires_grad_(True)  # channels-last storage, as the network hands it out
    atts = [a.cuda().requires_grad_(True) for a in atts]
    loss = fn((logits, atts), y)
    loss.backward()
    rec = None if fn.topk_record is None else fn.topk_record.clone()
    dst = torch.zeros(2, 32, 32, 8, 2, device="cuda", dtype=torch.bfloat16)
    bufs = [torch.zeros(s[0], *s[2:], device="cuda") for s in CO.ATT_SHAPES]
    loss2, written = fn.forward_backward_into((logits.detach(), [a.detach() for a in atts]), y, (L.Tensor(dst.data_ptr(), L.BF16, 2, 2, 2, 32, 32, 8), bufs))
    rec2 = None if fn.topk_record is None else fn.topk_record.clone()
    return (loss.detach(), logits.grad, [a.grad for a in atts], rec), (loss2, dst, bufs, written, rec2)


def test_ce_topk_zero_is_todays_loss_bit_for_bit():
    without = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0))
    zero = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0, ce_topk=0.0))
    on = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0, ce_topk=10.0))
    for a, b in zip(without, zero):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for s, t in zip(a[2], b[2]):
            assert torch.equal(s, t)
    assert without[1][3] == zero[1][3] and zero[0][3] is None and zero[1][4] is None
    assert float(on[0][0]) != float(zero[0][0]) and not torch.equal(on[0][1], zero[0][1]) and not torch.equal(on[1][1], zero[1][1])
    for s, t in zip(on[0][2], zero[0][2]):  # (the attention-map terms are unchanged by the term)
        assert torch.equal(s, t)
    plain, pzero = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True)), _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_topk=0.0))
    assert torch.equal(plain[0][0], pzero[0][0]) and torch.equal(plain[0][1], pzero[0][1]) and torch.equal(plain[1][1], pzero[1][1])


@pytest.mark.parametrize("att", [True, False])
def test_loss_and_gradients_in_one_call_equal_the_autograd_route(att):
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=True, ce_weight=0.5, ce_foreground_weight=4.0, ce_topk=10.0)
    (loss, glog, gatts, rec), (loss2, dst, bufs, written, rec2) = _both_routes(fn)
    assert torch.equal(loss2, loss) and torch.equal(rec, rec2)
    assert torch.equal(dst, glog.permute(0, 2, 3, 4, 1).to(torch.bfloat16))
    assert written == ([5, 4, 3, 2, 1, 0] if att else [])
    for i in written:
        assert torch.equal(bufs[i].reshape(-1), gatts[i].reshape(-1))


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_train_step_with_the_term_is_bit_identical_on_both_routes(dtype):
    """DataParallelTrainer, two steps with dropout: the fused-loss route (gradient written where the backward reads it) against loss.backward(), bit for bit; and the
    top-k term is really in the step."""
    from tests.test_gpu_parallel import _batch, _model_dt
    from vs_seg_amd import parallel as DP

    x, y = _batch(0)
    res = []
    for fused in (True, False):
        m = _model_dt(dtype, 0.1)
        trainer = DP.DataParallelTrainer(m.train(), V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0, ce_topk=10.0), V.Adam(m.parameters(), lr=1e-3, weight_decay=1e-7))
        assert trainer.fused_loss
        trainer.fused_loss = fused
        losses = [float(trainer.step(x, y)) for _ in range(2)]
        flat, gflat = m.flat_parameters()
        torch.cuda.synchronize()
        res.append((losses, gflat.clone(), flat.clone(), m._bflat.clone()))
    assert res[0][0] == res[1][0] and all(np.isfinite(v) for v in res[0][0])
    for a, b in zip(res[0][1:], res[1][1:]):
        assert torch.equal(a, b)
    assert float(res[0][1].abs().max()) > 0
    m = _model_dt(dtype, 0.1)
    plain = DP.DataParallelTrainer(m.train(), V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0), V.Adam(m.parameters(), lr=1e-3, weight_decay=1e-7))
    first = float(plain.step(x, y))
    print(f"{dtype}: first loss {res[0][0][0]:.6f} with the top-k term, {first:.6f} with the plain one")
    assert first != res[0][0][0]


# ---------------------------------------------------------------- F: the staged layouts
@pytest.mark.parametrize("layout", ["bf16x2", "bf16x8", "f32x2", "f32x8"])
@pytest.mark.parametrize("nvox_dims", [(32, 32, 8), (5, 3, 7)])
def test_gradient_written_in_the_staged_layouts_equals_the_fp32_gradient_cast(layout, nvox_dims):
    """vsseg_dice_ce_topk_pred_bwd_to = vsseg_dice_ce_topk_pred_bwd followed by vsseg_copy_cast, bit for bit, in every layout the training plan stages the gradient in."""
    lib = L.lib()
    n, dims = 2, nvox_dims
    nvox = dims[0] * dims[1] * dims[2]
    lg = (2.0 * synth_input(32, (n, *dims, 2))).cuda().contiguous()
    lab = synth_label(31, (n, 1, *dims)).cuda().contiguous()
    coef = torch.tensor([-0.3, 0.02, -0.25, 0.015, -0.31, 0.021, -0.2, 0.017], device="cuda")
    tcoef = torch.tensor([0.011, 0.044, 0.37, 1.25, 4.0, 0.0, 0.0, 0.0], device="cuda")  # (k_bg, k_fg, tie share, threshold 1.25 as its bits, w_fg)
    want32, dice32 = torch.empty(n, *dims, 2, device="cuda"), torch.empty(n, *dims, 2, device="cuda")
    L.check(lib.vsseg_dice_ce_topk_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), tcoef.data_ptr(), None, want32.data_ptr(), H.stream()))
    L.check(lib.vsseg_dice_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), None, dice32.data_ptr(), H.stream()))
    # the term is there, above the threshold only: want32 - dice32 = k w[y] (softmax - onehot) where v > 1.25, 0 below, to the rounding of the fp32 sum
    p = torch.softmax(lg.double(), -1)
    fg = (lab.reshape(n, *dims) == 1)
    v = torch.where(fg, 4.0 * torch.nn.functional.softplus(lg[..., 0].double() - lg[..., 1].double()), torch.nn.functional.softplus(lg[..., 1].double() - lg[..., 0].double()))
    clear = (v - 1.25).abs() > 1e-4
    ce = torch.where(fg, 0.044 * p[..., 0], -0.011 * p[..., 1]) * (v > 1.25)
    diff = (want32.double() - dice32.double() - torch.stack([ce, -ce], -1))[clear]
    assert float(diff.abs().max()) <= 2e-7 and 0 < int((v > 1.25).sum()) < v.numel()
    dt = torch.bfloat16 if layout.startswith("bf16") else torch.float32
    pitch = int(layout[-1])
    got = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    want = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    tdt = L.BF16 if dt == torch.bfloat16 else L.F32
    flags = L.ZERO_PADDED if pitch == 8 else 0
    L.check(lib.vsseg_copy_cast(L.Tensor(want32.data_ptr(), L.F32, 2, 2, n, *dims), L.Tensor(want.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    L.check(lib.vsseg_dice_ce_topk_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), tcoef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got[..., :2], want[..., :2])
    if pitch == 8:  # bf16 rows are written whole (channels 2..7 = 0, as the cast pass writes them); fp32 rows keep what was there
        assert torch.equal(got[..., 2:], want[..., 2:]) if dt == torch.bfloat16 else float(got[..., 2:].min()) == 7.0
    assert lib.vsseg_dice_ce_topk_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), tcoef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 3, pitch, n, *dims), H.stream()) == L.EINVAL


# ---------------------------------------------------------------- H: run to run
def test_sixteen_workgroups_per_pass_give_the_same_bits_every_time():
    shape = (2, 1, 64, 64, 16)  # 131072 voxels: 32 workgroups in every histogram pass
    y = synth_label(31, shape).cuda()
    x = (3.0 * synth_input(32, (2, 2, *shape[2:]))).cuda()
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, ce_weight=1.0, ce_foreground_weight=4.0, ce_topk=10.0)
    res = []
    for _ in range(2):
        logits = x.clone().requires_grad_(True)
        loss = fn((logits, []), y)
        loss.backward()
        res.append((loss.detach().clone(), fn.topk_record.clone(), logits.grad.clone()))
    assert torch.isfinite(res[0][0]) and all(torch.equal(a, b) for a, b in zip(res[0], res[1]))
    _, passes, n_gt, n_eq, k = _record(res[0][1])
    assert passes == 3 and k == 13107 and n_gt < k <= n_gt + n_eq
    want, _, _, _ = TO.loss_and_grads(x, [], y, supervised_attention=False, hardness_weighting=True, ce_weight=1.0, ce_foreground_weight=4.0, ce_topk=10.0)
    assert abs(float(res[0][0]) - want) < LOSS_BAR


# ---------------------------------------------------------------- I: extreme logits
def test_loss_of_nan_logits_is_nan_and_sets_the_flag():
    V.fx_status(reset=True)
    y = synth_label(31, BIG).cuda()
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, hardness_weighting=True, ce_weight=0.5, ce_foreground_weight=4.0, ce_topk=10.0)
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda()
    logits[1, 0, 5, 6, 7] = float("nan")
    loss = fn((logits.requires_grad_(True), []), y)
    assert torch.isnan(loss).item()
    assert V.fx_status(reset=True) is True
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda().requires_grad_(True)
    loss = fn((logits, []), y)
    assert torch.isfinite(loss).item() and V.fx_status() is False
    V.fx_status(reset=True)


def test_select_alone_flags_a_nan_logit():
    """vsseg_ce_topk_select on its own (in the test above the Dice sums see the same NaN): the NaN takes the largest key, is selected, and sets the flag; the finalize
    returns a NaN loss and NaN coefficients."""
    lib = L.lib()
    V.fx_status(reset=True)
    n, nvox = 1, 64
    lg, zl = torch.zeros(n, nvox, 2, device="cuda"), torch.zeros(n, nvox, 2, device="cuda")
    lg[0, :, 1] = torch.linspace(-2.0, 2.0, nvox, device="cuda")
    lab = torch.zeros(n, nvox, device="cuda")
    lab[0, 3] = 1.0
    out = torch.zeros(1 + 4 + 8, device="cuda")

    def run(k):
        sums = torch.zeros(6 + L.topk_scratch_bytes() // 8, dtype=torch.float64, device="cuda")
        L.check(lib.vsseg_dice_pred_sums(zl.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, sums.data_ptr(), H.stream()))
        L.check(lib.vsseg_ce_topk_select(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 3.0, k, sums.data_ptr() + 48, H.stream()))
        L.check(lib.vsseg_dice_ce_topk_finalize(sums.data_ptr(), None, n, 0, sums.data_ptr() + 48, 2.0, 3.0, out.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 20, H.stream()))
        torch.cuda.synchronize()
        return out.clone(), _record(sums[6:10].view(torch.int64))

    o, (tb, passes, n_gt, n_eq, k) = run(8)
    assert V.fx_status() is False and torch.isfinite(o[:8]).all() and (passes, k) == (3, 8) and n_eq == 1 and n_gt == 7
    assert abs(float(o[5]) - 2.0 / 8) < 1e-8 and abs(float(o[6]) - 6.0 / 8) < 1e-8 and float(o[7]) == 1.0 and float(o[9]) == 3.0
    assert int(o[8:9].view(torch.int32)) == tb - (1 << 32 if tb >= 1 << 31 else 0)
    for k in (1, 8):  # the NaN is the threshold itself (K = 1) or above it
        lg[0, 9, 1] = float("nan")
        o, (tb, _, n_gt, n_eq, _) = run(k)
        assert (tb == 0xFFFFFFFF and n_eq == 1) if k == 1 else (n_gt == 7 and n_eq == 1)
        assert torch.isnan(o[0]) and torch.isnan(o[5:10]).all() and V.fx_status(reset=True) is True
        lg[0, 9, 1] = 0.0
    assert torch.isfinite(run(8)[0][:8]).all() and V.fx_status() is False


@pytest.mark.parametrize("lam,w_fg", PAIRS)
def test_logit_differences_of_100_stay_finite_and_in_range(lam, w_fg):
    """|z| = 100 everywhere, every voxel wrong: v = 100 w[y]; the fixed-point flag stays clear."""
    V.fx_status(reset=True)
    y = synth_label(31, BIG)
    fg = (y[:, 0] == 1)
    logits = torch.empty(2, 2, 32, 32, 8)
    logits[:, 0] = torch.where(fg, 50.0, -50.0)
    logits[:, 1] = -logits[:, 0]
    loss, lg, _, fn = _run(BIG, True, 10.0, lam, w_fg, (y, logits, []))
    _, _, _, _, k = _record(fn.topk_record)
    want, _, _ = _by_hand(y, logits, True, lam, w_fg, k)
    print(f"|z| = 100: loss {loss.item():.9g}, by hand {want:.9g}")
    assert np.isfinite(loss.item()) and abs(loss.item() - want) < LOSS_BAR * max(1.0, abs(want)) and want > 50.0 * lam
    assert torch.isfinite(lg.grad).all() and V.fx_status() is False


# ---------------------------------------------------------------- J: the three evaluations of v agree
def test_the_backward_selects_exactly_the_voxels_the_select_counted():
    """The backward through the C ABI with an all-zero Dice `coef`: only the cross-entropy gradient is written, and the number of voxels with a non-zero gradient is
    n_gt + n_eq of the record, exactly — the histogram passes and the backward computed every v to the same bits."""
    lib = L.lib()
    y, logits, _ = _inputs(BIG)
    n, nvox = 2, 32 * 32 * 8
    lg = logits.permute(0, 2, 3, 4, 1).contiguous().cuda()
    lab = y.cuda().contiguous()
    k = V.topk_count(n * nvox, 10.0)
    sums = torch.zeros(n * 6 + L.topk_scratch_bytes() // 8, dtype=torch.float64, device="cuda")
    out = torch.zeros(1 + n * 4 + 8, device="cuda")
    tcoef_at = out.data_ptr() + 4 * (1 + n * 4)
    L.check(lib.vsseg_ce_topk_select(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 4.0, k, sums.data_ptr() + 8 * n * 6, H.stream()))
    L.check(lib.vsseg_dice_ce_topk_finalize(sums.data_ptr(), None, n, 0, sums.data_ptr() + 8 * n * 6, 1.0, 4.0, out.data_ptr(), out.data_ptr() + 4, tcoef_at, H.stream()))
    zero_coef = torch.zeros(n * 4, device="cuda")
    for hard in (1, 0):
        g = torch.full((n, nvox, 2), 7.0, device="cuda")
        L.check(lib.vsseg_dice_ce_topk_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, hard, zero_coef.data_ptr(), tcoef_at, None, g.data_ptr(), H.stream()))
        torch.cuda.synchronize()
        tb, passes, n_gt, n_eq, kk = _record(sums[n * 6 : n * 6 + 4].view(torch.int64))
        nz = int(((g[..., 0] != 0) | (g[..., 1] != 0)).sum())
        print(f"K {kk}: n_gt {n_gt} n_eq {n_eq}, voxels with a gradient {nz}")
        assert kk == k and passes == 3 and n_gt < k <= n_gt + n_eq
        assert nz == n_gt + n_eq
        assert torch.equal(g[..., 0], -g[..., 1])


# ---------------------------------------------------------------- K: through the command line
def test_training_epochs_with_the_flag(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 2 --ce_weight 1 --ce_topk 10` over the synthetic debug cases of tools/make_debug_data.py: two training epochs and the validation
    pass at val_interval = 2 (the forward under no_grad, the same loss object)."""
    import importlib.util
    import logging

    from vs_seg_amd.params import VSparams

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_debug_data", os.path.join(root, "tools", "make_debug_data.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    data = os.path.join(str(tmp_path), "data") + os.sep
    gen.main(["--data_root", data, "--size", "64", "64", "32"])
    monkeypatch.chdir(root)  # --debug reads ./params/split_debug.csv
    argv = ["--debug", "--num_epochs", "2", "--data_root", data, "--compute_dtype", "fp32", "--train_batch_size", "2", "--ce_weight", "1", "--ce_topk", "10"]
    before = list(logging.getLogger().handlers)
    p = VSparams(argparse.ArgumentParser(), argv)
    try:
        p.create_results_folders()
        p.set_up_logger("training_log.txt")
        p.log_parameters()
        train_files, val_files, _ = p.load_T1_or_T2_data()
        ttf, vtf, _ = p.get_transforms()
        train_loader, val_loader = p.cache_transformed_train_data(train_files, ttf), p.cache_transformed_val_data(val_files, vtf)
        model, loss_fn = p.set_and_get_model(), p.set_and_get_loss_function()
        assert (loss_fn.ce_weight, loss_fn.ce_foreground_weight, loss_fn.ce_topk) == (1.0, 1.0, 10.0)
        losses, metrics = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
        print(f"epoch losses with the top-k term: {losses}, validation Dice {metrics}")
        assert len(losses) == 2 and np.isfinite(losses).all() and len(metrics) == 1 and np.isfinite(metrics).all()
        assert loss_fn.topk_record is not None and _record(loss_fn.topk_record)[1] == 3
        for h in p.logger.handlers:
            h.flush()
        log = open(os.path.join(p.logs_path, "training_log.txt")).read()
        saved = sorted(os.listdir(p.model_path))
    finally:
        for h in list(logging.getLogger().handlers):
            if h not in before:
                logging.getLogger().removeHandler(h)
                h.close()
    assert "ce_weight =" in log and "ce_topk =" in log
    assert "epoch 2 average loss" in log
    val = [ln for ln in log.splitlines() if "validation loss" in ln]
    assert len(val) == 1 and np.isfinite(float(val[0].rsplit(":", 1)[1]))
    best = [ln for ln in log.splitlines() if "best mean dice" in ln]
    assert len(best) == 1
    cur, top = float(best[0].split("current mean dice:")[1].split()[0]), float(best[0].split("best mean dice:")[1].split()[0])
    assert np.isfinite(cur) and cur <= top
    assert "last_epoch_model.pth" in saved and "best_metric_model.pth" in saved
    assert V.fx_status() is False
