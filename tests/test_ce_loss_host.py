"""CPU tests of the cross-entropy term of the loss (Dice_spvPA(ce_weight=, ce_foreground_weight=), --ce_weight / --ce_foreground_weight): the range checks, the
command-line flags, the exported entry points, and the hand-written formulas of tests/ce_oracle.py (the ones the kernels use) against F.cross_entropy in fp64."""
import argparse

import pytest
import torch

import vs_seg_amd as V
from tests import ce_oracle as CO
from tests.helpers import synth_input, synth_label
from vs_seg_amd import _lib as L

NAN, INF = float("nan"), float("inf")
BAD = [(-0.5, 1.0), (NAN, 1.0), (INF, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, NAN), (1.0, INF), (0.0, 4.0), (0.0, 0.5), ("x", 1.0), (1.0, None)]
GOOD = [(0.0, 1.0), (1.0, 1.0), (0.25, 8.0), (3, 0.5)]


def test_check_ce_accepts_and_rejects():
    assert V.check_ce(0.0) == (0.0, 1.0) and V.check_ce(0, 1) == (0.0, 1.0)
    for lam, w in GOOD:
        assert V.check_ce(lam, w) == (float(lam), float(w))
    for lam, w in BAD:
        with pytest.raises(ValueError):
            V.check_ce(lam, w)
    with pytest.raises(ValueError, match="no effect"):  # a flag that would silently do nothing
        V.check_ce(0.0, 4.0)


def test_constructor_takes_the_two_keywords():
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    assert fn.ce_weight == 0.0 and fn.ce_foreground_weight == 1.0
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, hardness_weighting=False, ce_weight=0.25, ce_foreground_weight=8)
    assert (fn.ce_weight, fn.ce_foreground_weight) == (0.25, 8.0) and not fn.supervised_attention and not fn.hardness_weighting
    for lam, w in BAD:
        with pytest.raises(ValueError):
            V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=lam, ce_foreground_weight=w)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # the term has no CPU path either
        V.Dice_spvPA(ce_weight=1.0)((torch.zeros(1, 2, 4, 4, 4), []), torch.zeros(1, 1, 4, 4, 4))


def test_library_exports_the_entry_points():
    lib = L.lib()
    assert lib.vsseg_version() >= 14
    for name in ("vsseg_ce_sums", "vsseg_dice_ce_finalize", "vsseg_dice_ce_pred_bwd", "vsseg_dice_ce_pred_bwd_to"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes
    # refused before any launch: null pointers, an odd pitch
    assert lib.vsseg_ce_sums(None, 2, None, 1, 8, None, None) == L.EINVAL and b"vsseg_ce_sums" in lib.vsseg_last_error()
    assert lib.vsseg_ce_sums(16, 3, 16, 1, 8, 16, None) == L.EINVAL
    assert lib.vsseg_dice_ce_finalize(16, 16, 1, 0, None, 8, 1.0, 1.0, 16, 16, 16, None) == L.EINVAL and b"vsseg_dice_ce_finalize" in lib.vsseg_last_error()
    for lam, w in ((-1.0, 1.0), (NAN, 1.0), (INF, 1.0), (1.0, 0.0), (1.0, NAN), (1.0, INF)):
        assert lib.vsseg_dice_ce_finalize(16, 16, 1, 0, 16, 8, lam, w, 16, 16, 16, None) == L.EINVAL and b"ce_weight" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_pred_bwd(16, 2, 16, 1, 8, 1, 16, None, None, 16, None) == L.EINVAL and b"vsseg_dice_ce_pred_bwd" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, None, L.Tensor(16, L.F32, 3, 4, 1, 2, 2, 2), None) == L.EINVAL and b"2-channel" in lib.vsseg_last_error()
    assert lib.vsseg_dice_ce_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, None, L.Tensor(16, L.BF16, 2, 4, 1, 2, 2, 2), None) == L.EINVAL and b"layout" in lib.vsseg_last_error()


def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


def test_command_line_flags_default_to_off_and_reject_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    assert ap.get_default("ce_weight") == 0.0 and ap.get_default("ce_foreground_weight") == 1.0
    for bad in (["--ce_weight", "-1"], ["--ce_weight", "nan"], ["--ce_weight", "inf"], ["--ce_weight", "x"], ["--ce_weight", "1", "--ce_foreground_weight", "0"],
                ["--ce_weight", "1", "--ce_foreground_weight", "-3"], ["--ce_weight", "1", "--ce_foreground_weight", "nan"], ["--ce_weight", "1", "--ce_foreground_weight", "inf"],
                ["--ce_foreground_weight", "4"], ["--ce_weight", "0", "--ce_foreground_weight", "4"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], ["--ce_weight", "0.5"], ["--ce_weight", "0.5", "--ce_foreground_weight", "4"], ["--ce_weight", "0", "--ce_foreground_weight", "1"]):
        p = _parse(good)
        if p is not None:
            assert p.ce_weight == (float(good[1]) if good else 0.0)


def test_flags_reach_the_loss_function_and_the_log(monkeypatch):
    """set_and_get_loss_function and log_parameters need no device: build the object past the device check."""
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    for argv, lam, w in (([], 0.0, 1.0), (["--ce_weight", "0.5", "--ce_foreground_weight", "4"], 0.5, 4.0), (["--ce_weight", "2"], 2.0, 1.0), (["--no_hardness", "--ce_weight", "0.25"], 0.25, 1.0)):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        assert (p.ce_weight, p.ce_foreground_weight) == (lam, w)
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        fn = p.set_and_get_loss_function()
        assert isinstance(fn, V.Dice_spvPA) and (fn.ce_weight, fn.ce_foreground_weight) == (lam, w)
        assert fn.supervised_attention and fn.hardness_weighting == ("--no_hardness" not in argv)
        p.log_parameters()
        for k in ("ce_weight =", "ce_foreground_weight ="):
            assert any(k in ln for ln in lines) == (lam > 0)
        if lam > 0:
            assert any(ln.split() == ["ce_weight", "=", str(lam)] for ln in lines) and any(ln.split() == ["ce_foreground_weight", "=", str(w)] for ln in lines)


@pytest.mark.parametrize("shape", [(2, 1, 32, 32, 8), (2, 1, 5, 3, 7), (1, 1, 16, 16, 4)])
@pytest.mark.parametrize("scale", [2.0, 40.0])
@pytest.mark.parametrize("w_fg", [1.0, 8.0])
def test_hand_written_formulas_agree_with_torch_cross_entropy(shape, scale, w_fg):
    """softplus of the logit difference, the gradient from the other class's probability and the weighted normaliser against F.cross_entropy autograd, fp64, to 1e-12
    (sample 0 of a batch of two has no foreground)."""
    B = shape[0]
    y = synth_label(31, shape).double()
    x = (scale * synth_input(32, (B, 2, *shape[2:]))).double().requires_grad_(True)
    want = CO.ce_torch(x, y, w_fg)
    want.backward()
    want = want.detach()
    got, ggot = CO.ce_by_hand(x.detach(), y, w_fg)
    assert abs(float(got) - float(want)) <= 1e-12 * max(1.0, abs(float(want)))
    assert float((ggot - x.grad).abs().max()) <= 1e-12
    n_fg = float(CO.classes(y).sum())
    assert (n_fg > 0) and (B == 1 or float(CO.classes(y)[0].sum()) == 0)
    if scale == 40.0:  # -log(p_y) is inf at these logits; the softplus form is not
        p = torch.softmax(x.detach().float(), 1)
        py = torch.where(CO.classes(y) == 1, p[:, 1], p[:, 0])
        assert torch.isinf(-torch.log(py)).any() and torch.isfinite(got)


def test_label_cast_is_the_one_of_the_dice_kernels():
    lab = torch.tensor([0.0, 1.0, 1.9, 2.0, -1.0, 0.5, 1.0001]).reshape(1, 1, 7, 1, 1)
    assert CO.classes(lab).flatten().tolist() == [0, 1, 1, 0, 0, 0, 1]
