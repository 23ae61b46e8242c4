"""-m gpu: the region and focal options of the loss (Dice_spvPA(tversky_beta=, focal_tversky_gamma=, batch_dice=, ce_focal_gamma=); vsseg_ce_focal_sums /
vsseg_loss_finalize / vsseg_loss_pred_bwd[_to]) against the fp64 CPU oracle of tests/region_oracle.py, a restatement of their definition with autograd.

The bars are the ones this loss is already held to (tests/test_gpu_ce_loss.py): loss within 5e-6, gradients of logits and attention maps atol 2e-9 / rtol 2e-4.  With the
top-k term the kernel ranks fp32 values and the oracle fp64 ones: as in tests/test_gpu_topk_loss.py a voxel within |v - t| <= 1e-5 t + 1e-6 of the oracle's threshold may
fall on either side, its gradient must then be the oracle's "selected" or "not selected" one, and at most 4 voxels may lie in that band (asserted on the oracle first)."""
import argparse
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import vs_seg_amd as V  # noqa: E402
from tests import ce_oracle as CO  # noqa: E402
from tests import gpu_harness as H  # noqa: E402
from tests import region_oracle as RO  # noqa: E402
from tests import topk_oracle as TO  # noqa: E402
from tests.helpers import synth_input, synth_label  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd import check_region  # noqa: E402

BIG, ODD = (2, 1, 32, 32, 8), (2, 1, 5, 3, 7)  # (16-byte loads, two workgroups per sample, sample 0 without foreground, six attention maps) / (odd voxel count: the scalar path)
ATOL, RTOL, LOSS_BAR = 2e-9, 2e-4, 5e-6
# the cross-entropy term beside the region term: keywords of Dice_spvPA
CE = {"none": {}, "plain": dict(ce_weight=0.25, ce_foreground_weight=8.0), "focal": dict(ce_weight=0.25, ce_foreground_weight=8.0, ce_focal_gamma=2.0),
      "topk": dict(ce_weight=1.0, ce_foreground_weight=4.0, ce_topk=10.0)}
ALL_ON = dict(tversky_beta=0.7, focal_tversky_gamma=0.75, batch_dice=True, ce_weight=0.25, ce_foreground_weight=8.0, ce_focal_gamma=2.0)


def _inputs(shape, scale):
    """CPU tensors: label (sample 0 has no foreground), logits = scale * synth_input, the attention maps of the golden loss test (none at the odd shape)."""
    y = synth_label(31, shape)
    logits = scale * synth_input(32, (shape[0], 2, *shape[2:]))
    atts = [torch.sigmoid(synth_input(40 + i, s)) for i, s in enumerate(CO.ATT_SHAPES)] if shape == BIG else []
    return y, logits, atts


def _oracle_kw(shape, kw):
    kw = dict(kw)
    pct = kw.pop("ce_topk", 0.0)
    if pct:
        kw["ce_topk_k"] = TO.count(shape[0] * shape[2] * shape[3] * shape[4], pct)
    return kw


@functools.lru_cache(maxsize=None)
def _oracle(shape, scale, att, hard, kw_items):
    y, logits, atts = _inputs(shape, scale)
    return RO.loss_and_grads(logits, atts if att else [], y, supervised_attention=att, hardness_weighting=hard, **_oracle_kw(shape, dict(kw_items)))


def _run(shape, scale, att, hard, kw):
    y, logits, atts = _inputs(shape, scale)
    y, logits = y.cuda(), logits.cuda().requires_grad_(True)
    atts = [a.cuda().requires_grad_(True) for a in atts] if att else []
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=hard, **kw)
    loss = fn((logits, atts), y)
    assert loss.dim() == 0
    loss.backward()
    return loss, logits, atts, fn


def _compare(shape, scale, att, hard, kw, loss_bar=lambda want: LOSS_BAR):
    want, wlog, watts = _oracle(shape, scale, att, hard, tuple(sorted(kw.items())))
    band = torch.zeros((shape[0], *shape[2:]), dtype=torch.bool)
    if kw.get("ce_topk"):  # the voxels within rounding of the oracle's threshold, and the oracle's gradient with such a voxel selected / not selected
        y, lg, _ = _inputs(shape, scale)
        v = TO.values(lg.double(), y.double(), kw["ce_foreground_weight"])
        k = TO.count(v.numel(), kw["ce_topk"])
        t = float(v.flatten().topk(k).values[-1])
        band = (v - t).abs() <= 1e-5 * t + 1e-6
        assert 1 <= int(band.sum()) <= 4, f"{int(band.sum())} voxels within rounding of the oracle's threshold"  # (before the kernel is consulted)
        rest = {a: b for a, b in kw.items() if not a.startswith("ce_")}
        _, unsel, _ = _oracle(shape, scale, att, hard, tuple(sorted(rest.items())))
        p = torch.softmax(lg.double(), 1)
        g = kw["ce_weight"] / k * torch.where(CO.classes(y) == 1, kw["ce_foreground_weight"] * p[:, 0], -p[:, 1])
        sel = unsel + torch.stack([g, -g], 1)
    loss, logits, atts, fn = _run(shape, scale, att, hard, kw)
    got = logits.grad.cpu().double()
    err = abs(loss.item() - want)
    print(f"{shape} x{scale} att={att} hard={hard} {kw}: loss {loss.item():.9g} oracle {want:.9g} |diff| {err:.3g} (bar {loss_bar(want):.3g}); max |dlogits diff| {float((got - wlog).abs().max()):.3g}, "
          f"max |dlogits| {float(wlog.abs().max()):.3g}, {int(band.sum())} voxels in the band")
    assert np.isfinite(loss.item()) and err < loss_bar(want)
    assert torch.isfinite(got).all()
    out = ~band[:, None].expand_as(got)
    np.testing.assert_allclose(got[out].numpy(), wlog[out].numpy(), atol=ATOL, rtol=RTOL)
    if band.any():
        inb, s, u = (x.permute(0, 2, 3, 4, 1)[band].numpy() for x in (got, sel, unsel))
        assert (np.isclose(inb, s, atol=ATOL, rtol=RTOL).all(1) | np.isclose(inb, u, atol=ATOL, rtol=RTOL).all(1)).all(), (inb, s, u)
    for a, w in zip(atts, watts):
        np.testing.assert_allclose(a.grad.cpu().numpy(), w.numpy(), atol=ATOL, rtol=RTOL)
    return loss, fn


# (shape, (beta, gamma), pooled, hardness, attention, cross-entropy term): every (beta, gamma) pooled and not, with hardness on and off, with attention on and off, and
# with each of the four cross-entropy modes, at both shapes — a chosen list, not the product
CASES = [
    (BIG, (0.7, 1.0), False, True, True, "none"),
    (BIG, (0.7, 0.75), True, True, True, "focal"),
    (BIG, (0.3, 1.5), False, False, True, "plain"),
    (BIG, (0.3, 1.5), True, True, False, "topk"),
    (BIG, (0.7, 0.75), False, False, False, "none"),
    (BIG, (0.7, 1.0), True, False, True, "topk"),
    (BIG, (0.3, 1.5), True, False, True, "focal"),
    (BIG, (0.7, 0.75), False, True, True, "plain"),
    (ODD, (0.7, 1.0), False, True, False, "focal"),
    (ODD, (0.7, 0.75), True, True, False, "plain"),
    (ODD, (0.3, 1.5), True, False, False, "none"),
    (ODD, (0.3, 1.5), False, True, False, "topk"),
    (ODD, (0.7, 1.0), True, False, False, "focal"),
]


@pytest.mark.parametrize("shape,bg,pooled,hard,att,ce", CASES)
def test_loss_and_gradients_match_the_fp64_oracle(shape, bg, pooled, hard, att, ce):
    kw = dict(tversky_beta=bg[0], focal_tversky_gamma=bg[1], batch_dice=pooled, **CE[ce])
    _, fn = _compare(shape, 3.0 if ce == "topk" else 2.0, att, hard, kw)
    assert (fn.topk_record is not None) == (ce == "topk")


@pytest.mark.parametrize("shape,att", [(BIG, True), (BIG, False), (ODD, False)])
@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("gamma_c,lam,w_fg", [(2.0, 0.25, 8.0), (0.5, 1.0, 1.0)])
def test_focal_term_alone_matches_the_fp64_oracle(shape, att, hard, gamma_c, lam, w_fg):
    _compare(shape, 2.0, att, hard, dict(ce_weight=lam, ce_foreground_weight=w_fg, ce_focal_gamma=gamma_c))


@pytest.mark.parametrize("kw", [ALL_ON, dict(ce_weight=1.0, ce_foreground_weight=1.0, ce_focal_gamma=2.0), dict(tversky_beta=0.3, focal_tversky_gamma=1.5, ce_weight=0.25, ce_foreground_weight=8.0, ce_focal_gamma=5.0)])
def test_large_logits_stay_finite_and_in_range(kw):
    """Logits 40 * N(0, 1): probabilities underflow in fp32 (log(q) of a rounded q = 0 is -inf) and a voxel's value is far from bounded by 1; the fixed-point flag stays clear."""
    V.fx_status(reset=True)
    _compare(BIG, 40.0, True, True, kw, lambda want: LOSS_BAR * max(1.0, abs(want)))
    assert _oracle(BIG, 40.0, True, True, tuple(sorted(kw.items())))[0] > 2.0 * kw["ce_weight"]  # (the term is large at these logits)
    assert V.fx_status() is False


def _perfect(shape, att_shapes, logit):
    """A prediction that is the label at +-logit and attention maps that are the label pyramid."""
    y = synth_label(31, shape)
    y[0, 0, 2:5, 2:5, 1:3] = 1.0  # both samples have a tumour
    x1 = torch.where(y[:, 0] > 0, logit, -logit)
    labels, g = [y], y
    for a, b in zip(att_shapes[::-1][:-1], att_shapes[::-1][1:]):
        g = F.max_pool3d(g, [p // q for p, q in zip(a[2:], b[2:])])
        labels.append(g)
    return y, torch.stack([-x1, x1], 1), labels[::-1]


@pytest.mark.parametrize("pooled", [False, True])
@pytest.mark.parametrize("gamma", [0.75, 0.25])
def test_saturated_perfect_prediction_has_no_nan_and_equals_the_oracle(pooled, gamma):
    """gamma < 1: the derivative gamma u^(gamma - 1) is unbounded at u = 0; below the floor 1e-7 the term is the constant 1e-7^gamma and every coefficient 0."""
    V.fx_status(reset=True)
    y, lg, atts = _perfect(BIG, CO.ATT_SHAPES, 60.0)
    kw = dict(supervised_attention=True, hardness_weighting=True, tversky_beta=0.7, focal_tversky_gamma=gamma, batch_dice=pooled)
    want, wlog, watts = RO.loss_and_grads(lg, atts, y, **kw)
    assert abs(want - 2.0 * 1e-7 ** gamma) < 1e-15 and float(wlog.abs().max()) == 0.0  # one floored term per ratio
    logits, a = lg.cuda().requires_grad_(True), [t.cuda().requires_grad_(True) for t in atts]
    loss = V.Dice_spvPA(to_onehot_y=True, softmax=True, **kw)((logits, a), y.cuda())
    loss.backward()
    print(f"pooled={pooled} gamma={gamma}: loss {loss.item():.9g} oracle {want:.9g}")
    assert np.isfinite(loss.item()) and abs(loss.item() - want) < LOSS_BAR and abs(loss.item() - want) <= 1e-6 * want
    assert torch.isfinite(logits.grad).all() and float(logits.grad.abs().max()) == 0.0
    for t, w in zip(a, watts):
        assert torch.isfinite(t.grad).all() and float(t.grad.abs().max()) == 0.0 and float(w.abs().max()) == 0.0
    assert V.fx_status() is False


@pytest.mark.parametrize("shape,att", [(BIG, True), (ODD, False)])
def test_new_path_at_beta_half_gamma_one_unpooled_is_todays_dice_loss(shape, att):
    new, nlog, natts, _ = _run(shape, 2.0, att, True, dict(tversky_beta=0.5))
    old, olog, oatts, _ = _run(shape, 2.0, att, True, {})
    assert abs(new.item() - old.item()) < LOSS_BAR
    np.testing.assert_allclose(nlog.grad.cpu().numpy(), olog.grad.cpu().numpy(), atol=ATOL, rtol=RTOL)
    for a, b in zip(natts, oatts):
        np.testing.assert_allclose(a.grad.cpu().numpy(), b.grad.cpu().numpy(), atol=ATOL, rtol=RTOL)


def test_pooled_and_unpooled_losses_differ_on_the_two_sample_input():
    kw = dict(tversky_beta=0.7)
    wp, wu = _oracle(BIG, 2.0, True, True, tuple(sorted(dict(kw, batch_dice=True).items())))[0], _oracle(BIG, 2.0, True, True, tuple(sorted(kw.items())))[0]
    assert abs(wp - wu) > 1e-2  # sample 0 has no foreground: its own ratios are those of an empty label
    p, u = _run(BIG, 2.0, True, True, dict(kw, batch_dice=True))[0].item(), _run(BIG, 2.0, True, True, kw)[0].item()
    assert abs(p - wp) < LOSS_BAR and abs(u - wu) < LOSS_BAR and abs((p - u) - (wp - wu)) < 2 * LOSS_BAR


def _opts(**kw):
    o = L.LossOpts()
    o.tversky_beta, o.focal_tversky_gamma, o.ce_foreground_weight = 0.5, 1.0, 1.0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


@pytest.mark.parametrize("layout", ["bf16x2", "bf16x8", "f32x2", "f32x8"])
@pytest.mark.parametrize("nvox_dims", [(32, 32, 8), (5, 3, 7)])
@pytest.mark.parametrize("mode", ["region+focal", "region", "focal", "region+topk"])
def test_gradient_written_in_the_staged_layouts_equals_the_fp32_gradient_cast(layout, nvox_dims, mode):
    """vsseg_loss_pred_bwd_to = vsseg_loss_pred_bwd followed by vsseg_copy_cast, bit for bit, in every layout the training plan stages the gradient in."""
    lib = L.lib()
    n, dims = 2, nvox_dims
    nvox = dims[0] * dims[1] * dims[2]
    lg = (2.0 * synth_input(32, (n, *dims, 2))).cuda().contiguous()
    lab = synth_label(31, (n, 1, *dims)).cuda().contiguous()
    region = mode.startswith("region")
    coef = torch.tensor([-0.3, 0.02, 0.03, -0.25, 0.015, 0.01, -0.31, 0.021, 0.04, -0.2, 0.017, 0.012] if region else [-0.3, 0.02, -0.25, 0.015, -0.31, 0.021, -0.2, 0.017], device="cuda")
    ce_coef = torch.tensor([0.011, 0.044, 0.5, 0.0, 4.0, 0.0, 0.0, 0.0], device="cuda")
    ce_coef[3:4].view(torch.int32).fill_(int(np.float32(0.4).view(np.int32)))  # the top-k threshold's bits: values above 0.4 are selected
    o = _opts(region=int(region), tversky_beta=0.7, focal_tversky_gamma=0.75, ce_mode=L.CE_FOCAL if "focal" in mode else L.CE_TOPK if "topk" in mode else L.CE_NONE, ce_weight=1.0,
              ce_foreground_weight=4.0, ce_focal_gamma=2.0 if "focal" in mode else 0.0)
    want32 = torch.empty(n, *dims, 2, device="cuda")
    L.check(lib.vsseg_loss_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), o, None, want32.data_ptr(), H.stream()))
    if mode == "region":  # the three coefficients are in: against A g t + B_G g s + B_P t by hand, fp64
        p = torch.softmax(lg.double(), -1)
        g = torch.stack([(lab.reshape(n, *dims) != 1), (lab.reshape(n, *dims) == 1)], -1).double()
        d = p - g
        s, w = 0.6 * torch.sign(d), 0.6 * d.abs() + 0.4
        t = w + p * s
        c = coef.double().reshape(n, 2, 3)[:, None, None, None]  # [n, 1, 1, 1, class, 3]
        dp = c[..., 0] * g * t + c[..., 1] * g * s + c[..., 2] * t
        hand = p * (dp - (dp * p).sum(-1, keepdim=True))
        np.testing.assert_allclose(want32.double().cpu().numpy(), hand.cpu().numpy(), atol=1e-7, rtol=2e-4)  # (fp32 rounding of terms of magnitude <= 0.4)
    dt = torch.bfloat16 if layout.startswith("bf16") else torch.float32
    pitch = int(layout[-1])
    got = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    want = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    tdt = L.BF16 if dt == torch.bfloat16 else L.F32
    flags = L.ZERO_PADDED if pitch == 8 else 0
    L.check(lib.vsseg_copy_cast(L.Tensor(want32.data_ptr(), L.F32, 2, 2, n, *dims), L.Tensor(want.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    L.check(lib.vsseg_loss_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), o, None, L.Tensor(got.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    torch.cuda.synchronize()
    assert torch.isfinite(want32).all() and float(want32.abs().max()) > 0
    assert torch.equal(got[..., :2], want[..., :2])
    if pitch == 8:  # bf16 rows are written whole (channels 2..7 = 0, as the cast pass writes them); fp32 rows keep what was there
        assert torch.equal(got[..., 2:], want[..., 2:]) if dt == torch.bfloat16 else float(got[..., 2:].min()) == 7.0
    # a destination that is not a 2-channel tensor of the right size is refused
    assert lib.vsseg_loss_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), o, None, L.Tensor(got.data_ptr(), tdt, 3, pitch, n, *dims), H.stream()) == L.EINVAL
    assert lib.vsseg_loss_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), o, None, L.Tensor(got.data_ptr(), tdt, 2, pitch, n + 1, *dims), H.stream()) == L.EINVAL


def _both_routes(fn):
    """(loss, d logits [B,2,X,Y,Z], [d att]) of the autograd route and (loss, bf16 destination, buffers, written) of forward_backward_into, on the golden loss inputs."""
    y, lg, atts = _inputs(BIG, 2.0)
    y = y.cuda()
    lg_cl = lg.permute(0, 2, 3, 4, 1).contiguous().cuda()
    logits = lg_cl.permute(0, 4, 1, 2, 3).detach().requires_grad_(True)  # channels-last storage, as the network hands it out
    atts = [a.cuda().requires_grad_(True) for a in atts]
    loss = fn((logits, atts), y)
    loss.backward()
    dst = torch.zeros(2, 32, 32, 8, 2, device="cuda", dtype=torch.bfloat16)
    bufs = [torch.zeros(s[0], *s[2:], device="cuda") for s in CO.ATT_SHAPES]
    bufs[2] = None  # a map without a gradient path is skipped
    loss2, written = fn.forward_backward_into((logits.detach(), [a.detach() for a in atts]), y, (L.Tensor(dst.data_ptr(), L.BF16, 2, 2, 2, 32, 32, 8), bufs))
    return (loss.detach(), logits.grad, [a.grad for a in atts]), (loss2, dst, bufs, written)


@pytest.mark.parametrize("att", [True, False])
@pytest.mark.parametrize("kw", [ALL_ON, dict(tversky_beta=0.3, focal_tversky_gamma=1.5), dict(ce_weight=0.5, ce_foreground_weight=4.0, ce_focal_gamma=2.0), dict(batch_dice=True, **CE["topk"])])
def test_loss_and_gradients_in_one_call_equal_the_autograd_route(att, kw):
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=True, **kw)
    (loss, glog, gatts), (loss2, dst, bufs, written) = _both_routes(fn)
    assert torch.isfinite(loss) and torch.equal(loss2, loss)
    assert torch.equal(dst, glog.permute(0, 2, 3, 4, 1).to(torch.bfloat16)) and float(dst.float().abs().max()) > 0
    assert written == ([5, 4, 3, 1, 0] if att else [])
    for i in written:
        assert torch.equal(bufs[i].reshape(-1), gatts[i].reshape(-1)) and float(bufs[i].abs().max()) > 0
    assert bufs[2] is None


def test_defaults_are_todays_loss_bit_for_bit():
    assert check_region(None, 1.0, False, 0.0, 0.5) == (None, 0.0)  # nothing on: the launches of before
    plain = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5))
    same = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, tversky_beta=None, focal_tversky_gamma=1.0, batch_dice=False, ce_focal_gamma=0.0))
    for a, b in zip(plain, same):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_sixteen_workgroups_add_up_to_the_same_bits_every_time():
    shape = (1, 1, 64, 64, 16)  # 16 workgroups in the sums passes
    y = synth_label(31, shape).cuda()
    x = (2.0 * synth_input(32, (1, 2, *shape[2:]))).cuda()
    kw = dict(supervised_attention=False, hardness_weighting=True, tversky_beta=0.7, focal_tversky_gamma=0.75, batch_dice=True, ce_weight=1.0, ce_foreground_weight=8.0, ce_focal_gamma=2.0)
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, **kw)
    res = []
    for _ in range(2):
        logits = x.clone().requires_grad_(True)
        loss = fn((logits, []), y)
        loss.backward()
        res.append((loss.detach(), logits.grad))
    assert torch.isfinite(res[0][0]) and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    want, _, _ = RO.loss_and_grads(x, [], y, **kw)
    assert abs(float(res[0][0]) - want) < LOSS_BAR


def test_nan_logit_in_the_focal_pass_sets_the_flag_and_the_reset_clears_it():
    """vsseg_ce_focal_sums on its own (the Dice sums see all-zero logits): values against the definition at z = 0, then a NaN logit — flag set, NaN loss and coefficients."""
    lib = L.lib()
    V.fx_status(reset=True)
    n, nvox = 1, 64
    lg, zl = torch.zeros(n, nvox, 2, device="cuda"), torch.zeros(n, nvox, 2, device="cuda")
    lab = torch.zeros(n, nvox, device="cuda")
    lab[0, 3] = 1.0
    sums = torch.zeros(6 + 3, dtype=torch.float64, device="cuda")
    out = torch.zeros(1 + 6 + 2, device="cuda")
    o = _opts(region=1, tversky_beta=0.7, focal_tversky_gamma=0.75, ce_mode=L.CE_FOCAL, ce_weight=2.0, ce_foreground_weight=3.0, ce_focal_gamma=2.0)

    def run():
        sums.zero_()
        L.check(lib.vsseg_dice_pred_sums(zl.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, sums.data_ptr(), H.stream()))
        L.check(lib.vsseg_ce_focal_sums(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 2.0, sums.data_ptr() + 48, H.stream()))
        L.check(lib.vsseg_loss_finalize(sums.data_ptr(), None, n, 0, sums.data_ptr() + 48, nvox, o, out.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 28, H.stream()))
        torch.cuda.synchronize()
        return out.clone()

    r = run()  # all-zero logits: every voxel's value is 0.5^2 log 2; W = 63 + 3
    assert V.fx_status() is False and torch.isfinite(r).all()
    assert abs(float(r[7]) - 2.0 / 66.0) < 1e-8 and abs(float(r[8]) - 6.0 / 66.0) < 1e-8
    region_only = torch.zeros(7, device="cuda")
    L.check(lib.vsseg_loss_finalize(sums.data_ptr(), None, n, 0, None, nvox, _opts(region=1, tversky_beta=0.7, focal_tversky_gamma=0.75), region_only.data_ptr(), region_only.data_ptr() + 4, None, H.stream()))
    assert abs(float(r[0]) - float(region_only[0]) - 2.0 * 0.25 * np.log(2.0)) < 1e-6 and torch.equal(r[1:7], region_only[1:7])
    lg[0, 9, 1] = float("nan")
    r = run()
    assert torch.isnan(r[0]) and torch.isnan(r[1:]).all() and V.fx_status(reset=True) is True
    lg[0, 9, 1] = 0.0
    assert torch.isfinite(run()).all() and V.fx_status() is False


def test_loss_of_nan_logits_is_nan():
    V.fx_status(reset=True)
    y = synth_label(31, BIG).cuda()
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, hardness_weighting=True, **ALL_ON)
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda()
    logits[1, 0, 5, 6, 7] = float("nan")
    loss = fn((logits.requires_grad_(True), []), y)
    assert torch.isnan(loss).item()
    assert V.fx_status(reset=True) is True
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda().requires_grad_(True)
    loss = fn((logits, []), y)
    assert torch.isfinite(loss).item() and V.fx_status() is False
    V.fx_status(reset=True)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_train_step_with_the_options_is_bit_identical_on_both_routes(dtype):
    """DataParallelTrainer, two steps with dropout: the fused-loss route (gradient written where the backward reads it) against loss.backward(), bit for bit; and the options
    are really in the step."""
    from tests.test_gpu_parallel import _batch, _model_dt
    from vs_seg_amd import parallel as DP

    x, y = _batch(0)
    kw = dict(tversky_beta=0.7, focal_tversky_gamma=0.75, batch_dice=True, ce_weight=0.5, ce_foreground_weight=4.0, ce_focal_gamma=2.0)
    res = []
    for fused in (True, False):
        m = _model_dt(dtype, 0.1)
        trainer = DP.DataParallelTrainer(m.train(), V.Dice_spvPA(to_onehot_y=True, softmax=True, **kw), V.Adam(m.parameters(), lr=1e-3, weight_decay=1e-7))
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
    plain = DP.DataParallelTrainer(m.train(), V.Dice_spvPA(to_onehot_y=True, softmax=True), V.Adam(m.parameters(), lr=1e-3, weight_decay=1e-7))
    first = float(plain.step(x, y))
    print(f"{dtype}: first loss {res[0][0][0]:.6f} with the options, {first:.6f} without")
    assert first != res[0][0][0]
    assert V.fx_status() is False


def test_training_epochs_with_the_four_flags(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 2 --tversky_beta 0.7 --focal_tversky_gamma 0.75 --batch_dice --ce_weight 0.5 --ce_foreground_weight 4 --ce_focal_gamma 2` over the
    synthetic debug cases of tools/make_debug_data.py: two training epochs and the validation pass at val_interval = 2 (the forward under no_grad)."""
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
    argv = ["--debug", "--num_epochs", "2", "--data_root", data, "--compute_dtype", "fp32", "--train_batch_size", "2", "--tversky_beta", "0.7", "--focal_tversky_gamma", "0.75", "--batch_dice",
            "--ce_weight", "0.5", "--ce_foreground_weight", "4", "--ce_focal_gamma", "2"]
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
        assert (loss_fn.tversky_beta, loss_fn.focal_tversky_gamma, loss_fn.batch_dice, loss_fn.ce_focal_gamma) == (0.7, 0.75, True, 2.0)
        losses, metrics = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
        print(f"epoch losses with the region and focal options: {losses}, validation Dice {metrics}")
        assert len(losses) == 2 and np.isfinite(losses).all() and len(metrics) == 1
        for h in p.logger.handlers:
            h.flush()
        log = open(os.path.join(p.logs_path, "training_log.txt")).read()
    finally:
        for h in list(logging.getLogger().handlers):
            if h not in before:
                logging.getLogger().removeHandler(h)
                h.close()
    for k in ("tversky_beta =", "focal_tversky_gamma =", "batch_dice =", "ce_focal_gamma ="):
        assert k in log
    assert "epoch 2 average loss" in log
    val = [ln for ln in log.splitlines() if "validation loss" in ln]
    assert len(val) == 1 and np.isfinite(float(val[0].rsplit(":", 1)[1]))
    assert V.fx_status() is False
