"""-m gpu: the cross-entropy term of the loss (Dice_spvPA(ce_weight=, ce_foreground_weight=), vsseg_ce_sums / vsseg_dice_ce_finalize / vsseg_dice_ce_pred_bwd[_to])
against the fp64 CPU oracle of tests/ce_oracle.py = oracle.vsseg_oracle.dice_spvpa + ce_weight * F.cross_entropy(weight=[1, ce_foreground_weight]) with autograd.

The bars are the ones tests/test_gpu_ops.py holds this loss to: loss within 5e-6, gradients atol 2e-9 / rtol 2e-4."""
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
from tests.helpers import synth_input, synth_label  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

BIG, ODD = (2, 1, 32, 32, 8), (2, 1, 5, 3, 7)  # (16-byte loads, four voxels per thread, two workgroups per sample) / (odd voxel count: the scalar path)
PAIRS = [(1.0, 1.0), (0.25, 8.0)]  # (ce_weight, ce_foreground_weight)


def _inputs(shape, scale):
    """CPU tensors: label (sample 0 has no foreground), logits = scale * synth_input, the attention maps of the golden loss test (none at the odd shape)."""
    y = synth_label(31, shape)
    logits = scale * synth_input(32, (shape[0], 2, *shape[2:]))
    atts = [torch.sigmoid(synth_input(40 + i, s)) for i, s in enumerate(CO.ATT_SHAPES)] if shape == BIG else []
    return y, logits, atts


@functools.lru_cache(maxsize=None)
def _oracle(shape, scale, att, hard, lam, w_fg):
    y, logits, atts = _inputs(shape, scale)
    return CO.loss_and_grads(logits, atts if att else [], y, supervised_attention=att, hardness_weighting=hard, ce_weight=lam, ce_foreground_weight=w_fg)


def _run(shape, scale, att, hard, lam, w_fg):
    y, logits, atts = _inputs(shape, scale)
    y, logits = y.cuda(), logits.cuda().requires_grad_(True)
    atts = [a.cuda().requires_grad_(True) for a in atts] if att else []
    loss = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=hard, ce_weight=lam, ce_foreground_weight=w_fg)((logits, atts), y)
    assert loss.dim() == 0
    loss.backward()
    return loss, logits, atts


def _compare(shape, scale, att, hard, lam, w_fg, loss_bar):
    loss, logits, atts = _run(shape, scale, att, hard, lam, w_fg)
    want, wlog, watts = _oracle(shape, scale, att, hard, lam, w_fg)
    err = abs(loss.item() - want)
    gerr = float((logits.grad.cpu().double() - wlog).abs().max())
    print(f"{shape} x{scale} att={att} hard={hard} ce=({lam}, {w_fg}): loss {loss.item():.9g} oracle {want:.9g} |diff| {err:.3g} (bar {loss_bar(want):.3g}); max |dlogits diff| {gerr:.3g}, "
          f"max |dlogits| {float(wlog.abs().max()):.3g}")
    assert np.isfinite(loss.item()) and err < loss_bar(want)
    np.testing.assert_allclose(logits.grad.cpu().numpy(), wlog.numpy(), atol=2e-9, rtol=2e-4)
    for a, w in zip(atts, watts):
        np.testing.assert_allclose(a.grad.cpu().numpy(), w.numpy(), atol=2e-9, rtol=2e-4)


@pytest.mark.parametrize("shape", [BIG, ODD])
@pytest.mark.parametrize("lam,w_fg", PAIRS)
@pytest.mark.parametrize("att", [True, False])
@pytest.mark.parametrize("hard", [True, False])
def test_dice_ce_loss_and_gradients_match_the_fp64_oracle(hard, att, lam, w_fg, shape):
    _compare(shape, 2.0, att, hard, lam, w_fg, lambda want: 5e-6)


@pytest.mark.parametrize("lam,w_fg", PAIRS)
def test_large_logits_stay_finite_and_in_range(lam, w_fg):
    """Logits 40 * N(0, 1): softmax probabilities underflow in fp32 (-log(p_y) = inf) and a voxel's value is far from bounded by 1; the fixed-point flag stays clear."""
    V.fx_status(reset=True)
    _compare(BIG, 40.0, True, True, lam, w_fg, lambda want: 5e-6 * max(1.0, abs(want)))
    assert _oracle(BIG, 40.0, True, True, lam, w_fg)[0] > 5.0 * lam
    assert V.fx_status() is False


@pytest.mark.parametrize("layout", ["bf16x2", "bf16x8", "f32x2", "f32x8"])
@pytest.mark.parametrize("nvox_dims", [(32, 32, 8), (5, 3, 7)])
def test_dice_ce_gradient_written_in_the_staged_layouts_equals_the_fp32_gradient_cast(layout, nvox_dims):
    """vsseg_dice_ce_pred_bwd_to = vsseg_dice_ce_pred_bwd followed by vsseg_copy_cast, bit for bit, in every layout the training plan stages the gradient in."""
    lib = L.lib()
    n, dims = 2, nvox_dims
    nvox = dims[0] * dims[1] * dims[2]
    lg = (2.0 * synth_input(32, (n, *dims, 2))).cuda().contiguous()
    lab = synth_label(31, (n, 1, *dims)).cuda().contiguous()
    coef = torch.tensor([-0.3, 0.02, -0.25, 0.015, -0.31, 0.021, -0.2, 0.017], device="cuda")
    ce_coef = torch.tensor([0.011, 0.044], device="cuda")
    want32, dice32 = torch.empty(n, *dims, 2, device="cuda"), torch.empty(n, *dims, 2, device="cuda")
    L.check(lib.vsseg_dice_ce_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), None, want32.data_ptr(), H.stream()))
    L.check(lib.vsseg_dice_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), None, dice32.data_ptr(), H.stream()))
    # the term is there: want32 - dice32 = k w[y] (softmax - onehot), to the rounding of the fp32 sum
    p = torch.softmax(lg.double(), -1)
    fg = (lab.reshape(n, *dims) == 1)
    ce = torch.where(fg, 0.044 * p[..., 0], -0.011 * p[..., 1])
    np.testing.assert_allclose((want32.double() - dice32.double()).cpu().numpy(), torch.stack([ce, -ce], -1).cpu().numpy(), atol=2e-7, rtol=0)
    dt = torch.bfloat16 if layout.startswith("bf16") else torch.float32
    pitch = int(layout[-1])
    got = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    want = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    tdt = L.BF16 if dt == torch.bfloat16 else L.F32
    flags = L.ZERO_PADDED if pitch == 8 else 0
    L.check(lib.vsseg_copy_cast(L.Tensor(want32.data_ptr(), L.F32, 2, 2, n, *dims), L.Tensor(want.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    L.check(lib.vsseg_dice_ce_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got[..., :2], want[..., :2])
    if pitch == 8:  # bf16 rows are written whole (channels 2..7 = 0, as the cast pass writes them); fp32 rows keep what was there
        assert torch.equal(got[..., 2:], want[..., 2:]) if dt == torch.bfloat16 else float(got[..., 2:].min()) == 7.0
    # a destination that is not a 2-channel tensor of the right size is refused
    assert lib.vsseg_dice_ce_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 3, pitch, n, *dims), H.stream()) == L.EINVAL
    assert lib.vsseg_dice_ce_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), ce_coef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 2, pitch, n + 1, *dims), H.stream()) == L.EINVAL


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
def test_dice_ce_loss_and_gradients_in_one_call_equal_the_autograd_route(att):
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=True, ce_weight=0.5, ce_foreground_weight=4.0)
    (loss, glog, gatts), (loss2, dst, bufs, written) = _both_routes(fn)
    assert torch.equal(loss2, loss)
    assert torch.equal(dst, glog.permute(0, 2, 3, 4, 1).to(torch.bfloat16))
    assert written == ([5, 4, 3, 1, 0] if att else [])
    for i in written:
        assert torch.equal(bufs[i].reshape(-1), gatts[i].reshape(-1))
    assert bufs[2] is None


def test_ce_weight_zero_is_the_plain_dice_loss_bit_for_bit():
    plain, zero = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True)), _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.0, ce_foreground_weight=1.0))
    on = _both_routes(V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5))
    for (a, b) in zip(plain, zero):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for s, t in zip(a[2], b[2]):
            assert (s is None and t is None) or torch.equal(s, t)
    assert plain[1][3] == zero[1][3]
    assert float(on[0][0]) != float(plain[0][0]) and float(on[1][0]) != float(plain[1][0]) and not torch.equal(on[0][1], plain[0][1])
    # (the attention-map terms are unchanged by the cross-entropy term)
    for s, t in zip(on[0][2], plain[0][2]):
        assert torch.equal(s, t)


def test_dice_ce_fused_passes_equal_the_pass_per_level_sequence(monkeypatch):
    """With the cross-entropy term, the fused Dice passes against the generic sequence, at the bars of test_dice_fused_passes_equal_the_pass_per_level_sequence."""
    from vs_seg_amd.losses import dice_spvPA as D

    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0)
    res = []
    for generic in (False, True):
        if generic:
            monkeypatch.setattr(D, "_fused_plan", lambda *a, **k: None)
        else:
            y, lg, _ = _inputs(BIG, 2.0)
            assert D._fused_plan(2, BIG[2:], CO.ATT_SHAPES, lg.permute(0, 2, 3, 4, 1).contiguous().cuda(), y.cuda(), []) is not None
        (loss, glog, gatts), (loss2, _, _, _) = _both_routes(fn)
        assert torch.equal(loss, loss2)
        res.append((float(loss), glog.clone(), [a.clone() for a in gatts]))
    assert abs(res[0][0] - res[1][0]) < 2e-6
    np.testing.assert_allclose(res[0][1].cpu().numpy(), res[1][1].cpu().numpy(), rtol=2e-5, atol=1e-10)
    for a, b in zip(res[0][2], res[1][2]):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=1e-10)


def test_sixteen_workgroups_add_up_to_the_same_bits_every_time():
    shape = (1, 1, 64, 64, 16)  # 16 workgroups in the sums pass
    y = synth_label(31, shape).cuda()
    x = (2.0 * synth_input(32, (1, 2, *shape[2:]))).cuda()
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, ce_weight=1.0, ce_foreground_weight=8.0)
    res = []
    for _ in range(2):
        logits = x.clone().requires_grad_(True)
        loss = fn((logits, []), y)
        loss.backward()
        res.append((loss.detach(), logits.grad))
    assert torch.isfinite(res[0][0]) and torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    want, _, _ = CO.loss_and_grads(x, [], y, supervised_attention=False, hardness_weighting=True, ce_weight=1.0, ce_foreground_weight=8.0)
    assert abs(float(res[0][0]) - want) < 5e-6


def test_dice_ce_loss_of_nan_logits_is_nan():
    """A NaN logit gives a NaN partial sum in vsseg_ce_sums: the sticky flag is set and the loss is NaN; after the reset a finite input is finite again."""
    V.fx_status(reset=True)
    y = synth_label(31, BIG).cuda()
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, hardness_weighting=True, ce_weight=0.5, ce_foreground_weight=4.0)
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda()
    logits[1, 0, 5, 6, 7] = float("nan")
    loss = fn((logits.requires_grad_(True), []), y)
    assert torch.isnan(loss).item()
    assert V.fx_status(reset=True) is True
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda().requires_grad_(True)
    loss = fn((logits, []), y)
    assert torch.isfinite(loss).item() and V.fx_status() is False
    V.fx_status(reset=True)


def test_ce_sums_alone_flag_a_nan_logit():
    """vsseg_ce_sums on its own (the Dice sums see the same NaN in the test above): flag set, vsseg_dice_ce_finalize returns NaN loss and coefficients."""
    lib = L.lib()
    V.fx_status(reset=True)
    n, nvox = 1, 64
    lg, zl = torch.zeros(n, nvox, 2, device="cuda"), torch.zeros(n, nvox, 2, device="cuda")
    lab = torch.zeros(n, nvox, device="cuda")
    lab[0, 3] = 1.0
    sums = torch.zeros(6 + 3, dtype=torch.float64, device="cuda")
    out = torch.zeros(1 + 4 + 2, device="cuda")

    def run():
        sums.zero_()
        L.check(lib.vsseg_dice_pred_sums(zl.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, sums.data_ptr(), H.stream()))
        L.check(lib.vsseg_ce_sums(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, sums.data_ptr() + 48, H.stream()))
        L.check(lib.vsseg_dice_ce_finalize(sums.data_ptr(), None, n, 0, sums.data_ptr() + 48, nvox, 2.0, 3.0, out.data_ptr(), out.data_ptr() + 4, out.data_ptr() + 20, H.stream()))
        torch.cuda.synchronize()
        return out.clone()

    o = run()  # all-zero logits: every voxel's value is log 2; W = 63 + 3
    assert V.fx_status() is False and torch.isfinite(o).all()
    assert abs(float(o[5]) - 2.0 / 66.0) < 1e-8 and abs(float(o[6]) - 6.0 / 66.0) < 1e-8
    dice_only = torch.zeros(5, device="cuda")
    L.check(lib.vsseg_dice_finalize(sums.data_ptr(), None, n, 0, dice_only.data_ptr(), dice_only.data_ptr() + 4, H.stream()))
    assert abs(float(o[0]) - float(dice_only[0]) - 2.0 * np.log(2.0)) < 1e-6 and torch.equal(o[1:5], dice_only[1:5])
    lg[0, 9, 1] = float("nan")
    o = run()
    assert torch.isnan(o[0]) and torch.isnan(o[5:]).all() and V.fx_status(reset=True) is True
    lg[0, 9, 1] = 0.0
    assert torch.isfinite(run()).all() and V.fx_status() is False


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
def test_train_step_with_the_term_is_bit_identical_on_both_routes(dtype):
    """DataParallelTrainer, two steps with dropout: the fused-loss route (gradient written where the backward reads it) against loss.backward(), bit for bit; and the term
    is really in the step."""
    from tests.test_gpu_parallel import _batch, _model_dt
    from vs_seg_amd import parallel as DP

    x, y = _batch(0)
    res = []
    for fused in (True, False):
        m = _model_dt(dtype, 0.1)
        trainer = DP.DataParallelTrainer(m.train(), V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=0.5, ce_foreground_weight=4.0), V.Adam(m.parameters(), lr=1e-3, weight_decay=1e-7))
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
    print(f"{dtype}: first loss {res[0][0][0]:.6f} with the term, {first:.6f} without")
    assert first != res[0][0][0]


def test_training_epochs_with_the_two_flags(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 2 --ce_weight 0.5 --ce_foreground_weight 4` over the synthetic debug cases of tools/make_debug_data.py: two training epochs and the
    validation pass at val_interval = 2 (the forward under no_grad)."""
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
    argv = ["--debug", "--num_epochs", "2", "--data_root", data, "--compute_dtype", "fp32", "--train_batch_size", "2", "--ce_weight", "0.5", "--ce_foreground_weight", "4"]
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
        assert (loss_fn.ce_weight, loss_fn.ce_foreground_weight) == (0.5, 4.0)
        losses, metrics = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
        print(f"epoch losses with the cross-entropy term: {losses}, validation Dice {metrics}")
        assert len(losses) == 2 and np.isfinite(losses).all() and len(metrics) == 1
        for h in p.logger.handlers:
            h.flush()
        log = open(os.path.join(p.logs_path, "training_log.txt")).read()
    finally:
        for h in list(logging.getLogger().handlers):
            if h not in before:
                logging.getLogger().removeHandler(h)
                h.close()
    assert "ce_weight =" in log and "ce_foreground_weight =" in log
    assert "epoch 2 average loss" in log
    val = [ln for ln in log.splitlines() if "validation loss" in ln]
    assert len(val) == 1 and np.isfinite(float(val[0].rsplit(":", 1)[1]))
    assert V.fx_status() is False
