"""CPU tests of the top-k cross-entropy term of the loss (Dice_spvPA(ce_topk=), --ce_topk): the range checks and the command-line flag, K from the shapes, the exported
entry points and their argument checks, and the hand-written value / gradient of tests/topk_oracle.py (threshold, n_gt, n_eq, tie share: what the kernels compute)
against torch.topk with autograd in fp64."""
import argparse

import numpy as np
import pytest
import torch

import vs_seg_amd as V
from tests import topk_oracle as TO
from tests.helpers import synth_input, synth_label
from vs_seg_amd import _lib as L

NAN, INF = float("nan"), float("inf")


def test_check_ce_topk_accepts_and_rejects():
    assert V.check_ce_topk(0.0, 0.0) == 0.0 and V.check_ce_topk(0, 1.0) == 0.0
    for pct in (10, 0.5, 100, 1e-3):
        assert V.check_ce_topk(pct, 1.0) == float(pct)
    for pct, lam in ((101, 1.0), (-1, 1.0), (NAN, 1.0), (INF, 1.0), ("x", 1.0), (None, 1.0), (100.0001, 1.0)):
        with pytest.raises(ValueError):
            V.check_ce_topk(pct, lam)
    with pytest.raises(ValueError, match="no effect"):  # a flag that would silently do nothing
        V.check_ce_topk(10, 0.0)
    # check_ce keeps its signature and return value
    assert V.check_ce(0.5, 4.0) == (0.5, 4.0)


def test_constructor_takes_the_keyword():
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    assert fn.ce_topk == 0.0 and fn.topk_record is None
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=1.0, ce_foreground_weight=4.0, ce_topk=10)
    assert (fn.ce_weight, fn.ce_foreground_weight, fn.ce_topk) == (1.0, 4.0, 10.0)
    for kw in (dict(ce_topk=10), dict(ce_weight=0.0, ce_topk=10), dict(ce_weight=1.0, ce_topk=101), dict(ce_weight=1.0, ce_topk=-1), dict(ce_weight=1.0, ce_topk=NAN)):
        with pytest.raises(ValueError):
            V.Dice_spvPA(to_onehot_y=True, softmax=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.Dice_spvPA(ce_weight=1.0, ce_topk=10)((torch.zeros(1, 2, 4, 4, 4), []), torch.zeros(1, 1, 4, 4, 4))


@pytest.mark.parametrize("n,pct,want", [(100, 10, 10), (1000, 0.05, 1), (7, 10, 1), (105, 10, 10), (109, 10, 10), (110, 10, 11), (4 * 384 * 128 * 128, 10, 2516582), (4 * 384 * 128 * 128, 100, 25165824),
                                         (2 * 32 * 32 * 8, 1, 163), (105, 50, 52), (3, 100, 3), (1, 1e-3, 1)])
def test_k_from_the_shapes(n, pct, want):
    """K = max(1, floor(N * P / 100)), N * P / 100 < 1 included."""
    assert V.topk_count(n, pct) == want == TO.count(n, pct)
    assert 1 <= V.topk_count(n, pct) <= n


def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


def test_command_line_flag_defaults_to_off_and_rejects_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    assert ap.get_default("ce_topk") == 0.0
    for bad in (["--ce_topk", "10"], ["--ce_weight", "0", "--ce_topk", "10"], ["--ce_weight", "1", "--ce_topk", "101"], ["--ce_weight", "1", "--ce_topk", "-1"],
                ["--ce_weight", "1", "--ce_topk", "nan"], ["--ce_weight", "1", "--ce_topk", "x"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in (["--ce_weight", "1", "--ce_topk", "10"], ["--ce_weight", "1", "--ce_topk", "0"], ["--ce_weight", "0.5", "--ce_foreground_weight", "4", "--ce_topk", "100"]):
        p = _parse(good)
        if p is not None:
            assert p.ce_topk == float(good[-1])


def test_flag_reaches_the_loss_function_and_the_log(monkeypatch):
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    for argv, pct in (([], 0.0), (["--ce_weight", "1"], 0.0), (["--ce_weight", "1", "--ce_topk", "10"], 10.0), (["--ce_weight", "0.5", "--ce_foreground_weight", "4", "--ce_topk", "2.5"], 2.5)):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        assert p.ce_topk == pct
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        fn = p.set_and_get_loss_function()
        assert isinstance(fn, V.Dice_spvPA) and fn.ce_topk == pct and fn.ce_weight == p.ce_weight
        p.log_parameters()
        assert any("ce_topk =" in ln for ln in lines) == (pct > 0)
        if pct > 0:
            assert any(ln.split() == ["ce_topk", "=", str(pct)] for ln in lines)


def test_library_exports_the_entry_points_and_checks_arguments_before_any_launch():
    lib = L.lib()
    assert lib.vsseg_version() >= 16
    for name in ("vsseg_topk_scratch_bytes", "vsseg_topk_select", "vsseg_ce_topk_select", "vsseg_dice_ce_topk_finalize", "vsseg_dice_ce_topk_pred_bwd", "vsseg_dice_ce_topk_pred_bwd_to"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes is not None
    nbytes = lib.vsseg_topk_scratch_bytes()
    assert nbytes == L.topk_scratch_bytes() and nbytes > 32 and nbytes % 8 == 0
    # null pointers, k < 1, k > n, a misaligned scratch
    assert lib.vsseg_topk_select(None, 8, 1, 16, None) == L.EINVAL and b"vsseg_topk_select" in lib.vsseg_last_error()
    assert lib.vsseg_topk_select(16, 8, 1, None, None) == L.EINVAL
    assert lib.vsseg_topk_select(16, 0, 1, 16, None) == L.EINVAL
    assert lib.vsseg_topk_select(16, 8, 0, 16, None) == L.EINVAL and b"k = 0" in lib.vsseg_last_error()
    assert lib.vsseg_topk_select(16, 8, -3, 16, None) == L.EINVAL
    assert lib.vsseg_topk_select(16, 8, 9, 16, None) == L.EINVAL and b"k = 9" in lib.vsseg_last_error()
    assert lib.vsseg_topk_select(16, 8, 1, 20, None) == L.EINVAL and b"aligned" in lib.vsseg_last_error()
    assert lib.vsseg_ce_topk_select(None, 2, 16, 1, 8, 1.0, 1, 16, None) == L.EINVAL and b"vsseg_ce_topk_select" in lib.vsseg_last_error()
    assert lib.vsseg_ce_topk_select(16, 2, None, 1, 8, 1.0, 1, 16, None) == L.EINVAL
    assert lib.vsseg_ce_topk_select(16, 2, 16, 1, 8, 1.0, 1, None, None) == L.EINVAL
    assert lib.vsseg_ce_topk_select(16, 3, 16, 1, 8, 1.0, 1, 16, None) == L.EINVAL
    assert lib.vsseg_ce_topk_select(16, 2, 16, 2, 8, 1.0, 0, 16, None) == L.EINVAL and b"k = 0" in lib.vsseg_last_error()
    assert lib.vsseg_ce_topk_select(16, 2, 16, 2, 8, 1.0, 17, 16, None) == L.EINVAL and b"k = 17" in lib.vsseg_last_error()
    for w in (0.0, -1.0, NAN, INF):
        assert lib.vsseg_ce_topk_select(16, 2, 16, 2, 8, w, 1, 16, None) == L.EINVAL and b"ce_foreground_weight" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_topk_finalize(16, 16, 1, 0, None, 1.0, 1.0, 16, 16, 16, None) == L.EINVAL and b"vsseg_dice_ce_topk_finalize" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_topk_finalize(16, 16, 1, 0, 16, 1.0, 1.0, 16, 16, None, None) == L.EINVAL
    for lam, w in ((-1.0, 1.0), (NAN, 1.0), (INF, 1.0), (1.0, 0.0), (1.0, NAN), (1.0, INF)):
        assert lib.vsseg_dice_ce_topk_finalize(16, 16, 1, 0, 16, lam, w, 16, 16, 16, None) == L.EINVAL and b"ce_weight" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_topk_pred_bwd(16, 2, 16, 1, 8, 1, 16, None, None, 16, None) == L.EINVAL and b"vsseg_dice_ce_topk_pred_bwd" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_topk_pred_bwd(None, 2, 16, 1, 8, 1, 16, 16, None, 16, None) == L.EINVAL
    assert lib.vsseg_dice_ce_topk_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, None, L.Tensor(16, L.F32, 3, 4, 1, 2, 2, 2), None) == L.EINVAL and b"2-channel" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_topk_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, None, L.Tensor(16, L.BF16, 2, 4, 1, 2, 2, 2), None) == L.EINVAL and b"layout" in lib.vsseg_last_error()


@pytest.mark.parametrize("shape", [(2, 1, 32, 32, 8), (1, 1, 5, 3, 7), (1, 1, 16, 16, 4)])
@pytest.mark.parametrize("pct", [1.0, 10.0, 50.0, 100.0])
@pytest.mark.parametrize("w_fg", [1.0, 4.0])
def test_hand_written_value_and_gradient_agree_with_torch_topk(shape, pct, w_fg):
    """Threshold, n_gt, n_eq and the tie share against torch.topk + autograd, fp64, to 1e-12, on inputs without ties (n_eq = 1: the share is K - n_gt = 1)."""
    B = shape[0]
    y = synth_label(31, shape).double()
    x = (3.0 * synth_input(32, (B, 2, *shape[2:]))).double().requires_grad_(True)
    k = TO.count(B * int(np.prod(shape[2:])), pct)
    want = TO.topk_torch(x, y, w_fg, k)
    want.backward()
    want = want.detach()
    got, ggot, (t, n_gt, n_eq, share), c = TO.topk_by_hand(x.detach(), y, w_fg, k)
    assert n_eq == 1 and n_gt == k - 1 and share == 1.0 and int((c > 0).sum()) == k
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert float((ggot - x.grad).abs().max()) <= 1e-12
    assert int((x.grad[:, 0] != 0).sum()) == k


def test_hand_written_value_with_ties_shares_what_is_left_of_k():
    """All voxels equal (constant logits, w_fg = 1): t is that value, n_gt = 0, n_eq = N, every voxel carries K / N of its gradient and the value is the plain mean."""
    x = torch.zeros(1, 2, 4, 4, 2, dtype=torch.float64)
    x[:, 1] = 0.75
    y = torch.zeros(1, 1, 4, 4, 2, dtype=torch.float64)
    got, g, (t, n_gt, n_eq, share), c = TO.topk_by_hand(x, y, 1.0, 8)
    v = float(torch.nn.functional.softplus(torch.tensor(0.75, dtype=torch.float64)))
    assert (n_gt, n_eq, share) == (0, 32, 0.25) and abs(t - v) < 1e-15 and abs(float(got) - v) < 1e-15
    p1 = float(torch.sigmoid(torch.tensor(0.75, dtype=torch.float64)))
    assert float((g[:, 1] - 0.25 * p1 / 8).abs().max()) < 1e-15 and float((g[:, 0] + g[:, 1]).abs().max()) == 0.0


def test_the_key_and_the_sorted_select_of_the_oracle():
    a = np.array([0.0, -0.0, 1.0, np.inf, np.nan, 1e-45, 2.0, 2.0], dtype=np.float32)
    u = TO.key_of(a)
    assert u[0] == 0 and u[1] == 0 and u[4] == 0xFFFFFFFF and u[3] == 0x7F800000 and u[5] == 1
    assert TO.select(a, 1) == (0xFFFFFFFF, 0, 1)
    assert TO.select(a, 2) == (0x7F800000, 1, 1)
    assert TO.select(a, 3) == (0x40000000, 2, 2) == TO.select(a, 4)
    assert TO.select(a, 8) == (0, 6, 2)
