"""CPU tests of the region and focal options of the loss (Dice_spvPA(tversky_beta=, focal_tversky_gamma=, batch_dice=, ce_focal_gamma=) and the four flags): the fp64
oracle of tests/region_oracle.py against oracle.vsseg_oracle.dice_spvpa and F.cross_entropy, a known answer, the range checks, the command-line flags and the exported
entry points with their argument checks."""
import argparse
import ctypes

import pytest
import torch

import vs_seg_amd as V
from oracle import vsseg_oracle as O
from tests import ce_oracle as CO
from tests import region_oracle as RO
from tests.helpers import synth_input, synth_label
from vs_seg_amd import _lib as L
from vs_seg_amd import check_region

NAN, INF = float("nan"), float("inf")
BIG = (2, 1, 32, 32, 8)


def _golden(scale=2.0):
    y = synth_label(31, BIG).double()
    lg = (scale * synth_input(32, (2, 2, *BIG[2:]))).double()
    atts = [torch.sigmoid(synth_input(40 + i, s)).double() for i, s in enumerate(CO.ATT_SHAPES)]
    return y, lg, atts


@pytest.mark.parametrize("hard", [True, False])
@pytest.mark.parametrize("att", [True, False])
def test_beta_half_gamma_one_unpooled_is_the_reference_loss(hard, att):
    y, lg, atts = _golden()
    want = O.dice_spvpa(lg, atts, y, supervised_attention=att, hardness_weighting=hard)
    got = RO.region_spvpa(lg, atts, y, supervised_attention=att, hardness_weighting=hard, tversky_beta=0.5, focal_tversky_gamma=1.0, batch_dice=False)
    assert abs(float(got) - float(want)) <= 1e-12
    # and the options are not no-ops on these inputs: every one of them moves the loss
    for kw in (dict(tversky_beta=0.7), dict(focal_tversky_gamma=0.75), dict(batch_dice=True)):
        assert abs(float(RO.region_spvpa(lg, atts, y, supervised_attention=att, hardness_weighting=hard, **kw)) - float(want)) > 1e-6


@pytest.mark.parametrize("w_fg", [1.0, 8.0])
@pytest.mark.parametrize("scale", [2.0, 40.0])
def test_focal_term_at_exponent_zero_is_the_weighted_cross_entropy(scale, w_fg):
    y, lg, _ = _golden(scale)
    want = float(CO.ce_torch(lg, y, w_fg))
    assert abs(float(RO.focal_ce(lg, y, w_fg, 0.0)) - want) <= 1e-12 * max(1.0, abs(want))
    assert abs(float(RO.focal_ce(lg, y, w_fg, 1e-9)) - want) <= 1e-6 * max(1.0, abs(want))  # (gamma_c -> 0)
    assert float(RO.focal_ce(lg, y, w_fg, 2.0)) < want  # q^gamma_c <= 1 bounds the values by the plain term's


@pytest.mark.parametrize("shape", [BIG, (2, 1, 5, 3, 7)])
@pytest.mark.parametrize("scale", [2.0, 40.0])
@pytest.mark.parametrize("w_fg,gamma_c", [(1.0, 2.0), (8.0, 0.5), (4.0, 5.0)])
def test_hand_written_focal_value_and_gradient_agree_with_autograd(shape, scale, w_fg, gamma_c):
    y = synth_label(31, shape).double()
    x = (scale * synth_input(32, (shape[0], 2, *shape[2:]))).double().requires_grad_(True)
    want = RO.focal_ce(x, y, w_fg, gamma_c)
    want.backward()
    got, ggot = RO.focal_ce_by_hand(x.detach(), y, w_fg, gamma_c)
    assert abs(float(got) - float(want.detach())) <= 1e-12 * max(1.0, abs(float(want.detach())))
    assert float((ggot - x.grad).abs().max()) <= 1e-12
    assert torch.isfinite(ggot).all() and torch.isfinite(got)


def _tumour_case():
    """A 4^3 label with a 2^3 tumour, predictions at +-20 logits: half the tumour missed / the whole tumour and as many (8) false positives."""
    y = torch.zeros(1, 1, 4, 4, 4, dtype=torch.float64)
    y[0, 0, 1:3, 1:3, 1:3] = 1
    half, over = y.clone(), y.clone()
    half[0, 0, 1:3, 1:3, 2] = 0
    over[0, 0, 0, 0:2, :] = 1

    def logits(pred):
        x1 = torch.where(pred[:, 0] > 0, 20.0, -20.0).double()
        return torch.stack([-x1, x1], 1)

    return y, logits(half), logits(over)


def test_known_answer_a_missed_tumour_voxel_costs_more_above_beta_half():
    y, half, over = _tumour_case()
    f = lambda x, beta: float(RO.region_spvpa(x, [], y, supervised_attention=False, hardness_weighting=False, tversky_beta=beta))  # noqa: E731
    assert f(half, 0.7) > f(over, 0.7) and f(half, 0.3) < f(over, 0.3)
    for got, want in ((f(half, 0.7), 0.2297), (f(over, 0.7), 0.1392), (f(half, 0.3), 0.1259), (f(over, 0.3), 0.2581)):
        assert abs(got - want) < 5e-5  # (the four digits of the definition's fp64 values)


@pytest.mark.parametrize("pooled", [False, True])
def test_saturated_perfect_prediction_sits_on_the_floor_with_a_zero_gradient(pooled):
    y = torch.zeros(2, 1, 4, 4, 4, dtype=torch.float64)
    y[:, 0, 1:3, 1:3, 1:3] = 1
    x1 = torch.where(y[:, 0] > 0, 200.0, -200.0)
    atts = [torch.nn.functional.max_pool3d(y, 2), y.clone()]  # the label itself at both levels (coarsest first): perfect attention maps too
    loss, glog, gatt = RO.loss_and_grads(torch.stack([-x1, x1], 1), atts, y, supervised_attention=True, hardness_weighting=True, tversky_beta=0.7, focal_tversky_gamma=0.75,
                                         batch_dice=pooled)
    # one term per ratio: the mean over the logits ratios (weight 1 in all) plus 1 / L times each level's mean (1 in all): 2 x 1e-7^0.75
    assert abs(loss - 2.0 * 1e-7 ** 0.75) <= 1e-18
    assert float(glog.abs().max()) == 0.0 and all(float(g.abs().max()) == 0.0 for g in gatt)


BAD = [dict(tversky_beta=0.0), dict(tversky_beta=1.0), dict(tversky_beta=-0.2), dict(tversky_beta=NAN), dict(tversky_beta=INF), dict(tversky_beta="x"),
       dict(focal_tversky_gamma=0.2), dict(focal_tversky_gamma=4.5), dict(focal_tversky_gamma=NAN), dict(focal_tversky_gamma=INF), dict(focal_tversky_gamma=None),
       dict(batch_dice=2), dict(batch_dice="yes"), dict(batch_dice=None),
       dict(ce_weight=1.0, ce_focal_gamma=-1.0), dict(ce_weight=1.0, ce_focal_gamma=5.5), dict(ce_weight=1.0, ce_focal_gamma=NAN), dict(ce_weight=1.0, ce_focal_gamma=INF),
       dict(ce_focal_gamma=2.0), dict(ce_weight=0.0, ce_focal_gamma=2.0),  # a flag that would silently do nothing
       dict(ce_weight=1.0, ce_focal_gamma=2.0, ce_topk=10.0)]  # two different selections of the hard voxels


def test_check_region_accepts_and_rejects():
    assert check_region() == (None, 0.0)
    assert check_region(0.7) == ((0.7, 1.0, False), 0.0)
    assert check_region(None, 0.75) == ((0.5, 0.75, False), 0.0)  # with any region option on, beta defaults to 0.5
    assert check_region(None, 1.0, True) == ((0.5, 1.0, True), 0.0)
    assert check_region(0.5) == ((0.5, 1.0, False), 0.0)  # asked for: the new path at the Dice ratio
    assert check_region(0.3, 4, True, 5, 0.5, 0.0) == ((0.3, 4.0, True), 5.0)
    assert check_region(None, 0.25, False, 0.0, 1.0, 10.0) == ((0.5, 0.25, False), 0.0)  # the region options go with top-k
    for kw in BAD:
        with pytest.raises(ValueError):
            check_region(**kw)
    with pytest.raises(ValueError, match="no effect"):
        check_region(ce_focal_gamma=2.0)
    with pytest.raises(ValueError, match="ce_topk"):
        check_region(ce_weight=1.0, ce_focal_gamma=2.0, ce_topk=10.0)


def test_constructor_takes_the_four_keywords():
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    assert fn.region is None and (fn.tversky_beta, fn.focal_tversky_gamma, fn.batch_dice, fn.ce_focal_gamma) == (None, 1.0, False, 0.0)
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, tversky_beta=0.7, focal_tversky_gamma=0.75, batch_dice=True, ce_weight=0.5, ce_foreground_weight=4, ce_focal_gamma=2)
    assert (fn.tversky_beta, fn.focal_tversky_gamma, fn.batch_dice, fn.ce_focal_gamma) == (0.7, 0.75, True, 2.0) and fn.region == (0.7, 0.75, True)
    assert V.Dice_spvPA(batch_dice=True).tversky_beta == 0.5 and V.Dice_spvPA(focal_tversky_gamma=1.5).tversky_beta == 0.5
    for kw in BAD:
        with pytest.raises(ValueError):
            V.Dice_spvPA(to_onehot_y=True, softmax=True, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        V.Dice_spvPA(tversky_beta=0.7, ce_weight=1.0, ce_focal_gamma=2.0)((torch.zeros(1, 2, 4, 4, 4), []), torch.zeros(1, 1, 4, 4, 4))


def _opts(**kw):
    o = L.LossOpts()
    o.tversky_beta, o.focal_tversky_gamma, o.ce_foreground_weight = 0.5, 1.0, 1.0
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def test_library_exports_the_entry_points_and_checks_the_record_before_any_launch():
    lib = L.lib()
    assert lib.vsseg_version() >= 20 and ctypes.sizeof(L.LossOpts) == 56
    for name in ("vsseg_ce_focal_sums", "vsseg_loss_finalize", "vsseg_loss_pred_bwd", "vsseg_loss_pred_bwd_to"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes
    assert lib.vsseg_ce_focal_sums(None, 2, None, 1, 8, 2.0, None, None) == L.EINVAL and b"vsseg_ce_focal_sums" in lib.vsseg_last_error()
    assert lib.vsseg_ce_focal_sums(16, 3, 16, 1, 8, 2.0, 16, None) == L.EINVAL
    for g in (-0.5, 5.5, NAN, INF):
        assert lib.vsseg_ce_focal_sums(16, 2, 16, 1, 8, g, 16, None) == L.EINVAL and b"ce_focal_gamma" in lib.vsseg_last_error()
    dst = L.Tensor(16, L.F32, 2, 2, 1, 2, 2, 2)
    calls = [("vsseg_loss_finalize", lambda o: lib.vsseg_loss_finalize(16, 16, 1, 0, 16, 8, o, 16, 16, 16, None)),
             ("vsseg_loss_pred_bwd", lambda o: lib.vsseg_loss_pred_bwd(16, 2, 16, 1, 8, 1, 16, 16, o, None, 16, None)),
             ("vsseg_loss_pred_bwd_to", lambda o: lib.vsseg_loss_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, o, None, dst, None))]
    bad = [(dict(region=1, tversky_beta=0.0), b"tversky_beta"), (dict(region=1, tversky_beta=1.0), b"tversky_beta"), (dict(region=1, tversky_beta=NAN), b"tversky_beta"),
           (dict(region=1, focal_tversky_gamma=0.2), b"focal_tversky_gamma"), (dict(region=1, focal_tversky_gamma=4.5), b"focal_tversky_gamma"),
           (dict(region=1, focal_tversky_gamma=NAN), b"focal_tversky_gamma"), (dict(region=2), b"region"), (dict(region=0, batch_dice=1), b"batch_dice"),
           (dict(region=1, batch_dice=3), b"batch_dice"), (dict(reserved=1), b"reserved"), (dict(ce_mode=4), b"ce_mode"), (dict(ce_mode=-1), b"ce_mode"),
           (dict(ce_mode=L.CE_PLAIN, ce_weight=-1.0), b"ce_weight"), (dict(ce_mode=L.CE_FOCAL, ce_weight=NAN), b"ce_weight"), (dict(ce_mode=L.CE_TOPK, ce_weight=1.0, ce_foreground_weight=0.0), b"ce_weight"),
           (dict(ce_mode=L.CE_FOCAL, ce_weight=1.0, ce_foreground_weight=INF), b"ce_weight"), (dict(ce_mode=L.CE_FOCAL, ce_weight=1.0, ce_focal_gamma=5.5), b"ce_focal_gamma"),
           (dict(ce_mode=L.CE_FOCAL, ce_weight=1.0, ce_focal_gamma=-0.1), b"ce_focal_gamma"), (dict(ce_mode=L.CE_FOCAL, ce_weight=1.0, ce_focal_gamma=NAN), b"ce_focal_gamma")]
    for name, call in calls:
        assert call(None) == L.EINVAL and name.encode() in lib.vsseg_last_error()
        for kw, word in bad:
            assert call(_opts(**kw)) == L.EINVAL, (name, kw)
            assert word in lib.vsseg_last_error() and name.encode() in lib.vsseg_last_error(), (name, kw, lib.vsseg_last_error())
    good = _opts(region=1, tversky_beta=0.7, focal_tversky_gamma=0.75, batch_dice=1, ce_mode=L.CE_FOCAL, ce_weight=1.0, ce_focal_gamma=2.0)
    # null pointers and a cross-entropy term without its state, with a good record
    assert lib.vsseg_loss_finalize(None, 16, 1, 0, 16, 8, good, 16, 16, 16, None) == L.EINVAL and b"vsseg_loss_finalize" in lib.vsseg_last_error()
    assert lib.vsseg_loss_finalize(16, None, 1, 2, 16, 8, good, 16, 16, 16, None) == L.EINVAL
    assert lib.vsseg_loss_finalize(16, 16, 1, 0, None, 8, good, 16, 16, 16, None) == L.EINVAL and b"cross-entropy" in lib.vsseg_last_error()
    assert lib.vsseg_loss_finalize(16, 16, 1, 0, 16, 8, good, 16, 16, None, None) == L.EINVAL
    assert lib.vsseg_loss_pred_bwd(16, 2, 16, 1, 8, 1, 16, None, good, None, 16, None) == L.EINVAL and b"vsseg_loss_pred_bwd" in lib.vsseg_last_error()
    assert lib.vsseg_loss_pred_bwd(None, 2, 16, 1, 8, 1, 16, 16, good, None, 16, None) == L.EINVAL
    assert lib.vsseg_loss_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, good, None, L.Tensor(16, L.F32, 3, 4, 1, 2, 2, 2), None) == L.EINVAL and b"2-channel" in lib.vsseg_last_error()
    assert lib.vsseg_loss_pred_bwd_to(16, 2, 16, 1, 8, 1, 16, 16, good, None, L.Tensor(16, L.BF16, 2, 4, 1, 2, 2, 2), None) == L.EINVAL and b"layout" in lib.vsseg_last_error()


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
    assert ap.get_default("tversky_beta") is None and ap.get_default("focal_tversky_gamma") == 1.0 and ap.get_default("batch_dice") is False and ap.get_default("ce_focal_gamma") == 0.0
    for bad in (["--tversky_beta", "0"], ["--tversky_beta", "1"], ["--tversky_beta", "nan"], ["--tversky_beta", "x"], ["--focal_tversky_gamma", "0.1"], ["--focal_tversky_gamma", "5"],
                ["--focal_tversky_gamma", "inf"], ["--ce_focal_gamma", "2"], ["--ce_weight", "0", "--ce_focal_gamma", "2"], ["--ce_weight", "1", "--ce_focal_gamma", "6"],
                ["--ce_weight", "1", "--ce_focal_gamma", "-1"], ["--ce_weight", "1", "--ce_focal_gamma", "nan"], ["--ce_weight", "1", "--ce_topk", "10", "--ce_focal_gamma", "2"],
                ["--batch_dice", "1"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], ["--tversky_beta", "0.7"], ["--focal_tversky_gamma", "0.75"], ["--batch_dice"], ["--ce_weight", "1", "--ce_focal_gamma", "2"],
                 ["--tversky_beta", "0.7", "--focal_tversky_gamma", "0.75", "--batch_dice", "--ce_weight", "0.5", "--ce_foreground_weight", "4", "--ce_focal_gamma", "2"],
                 ["--tversky_beta", "0.3", "--ce_weight", "1", "--ce_topk", "10"]):
        _parse(good)
    assert "rank" in ap.format_help()  # the help text says what batch_dice pools under data parallelism


def test_flags_reach_the_loss_function_and_the_log(monkeypatch):
    """set_and_get_loss_function and log_parameters need no device: build the object past the device check."""
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    for argv, want in (([], (None, 1.0, False, 0.0)), (["--tversky_beta", "0.7"], (0.7, 1.0, False, 0.0)), (["--batch_dice"], (0.5, 1.0, True, 0.0)),
                       (["--focal_tversky_gamma", "0.75", "--ce_weight", "0.5", "--ce_focal_gamma", "2"], (0.5, 0.75, False, 2.0)),
                       (["--ce_weight", "1", "--ce_focal_gamma", "1.5"], (None, 1.0, False, 1.5))):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        assert (p.tversky_beta, p.focal_tversky_gamma, p.batch_dice, p.ce_focal_gamma) == want
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        fn = p.set_and_get_loss_function()
        assert isinstance(fn, V.Dice_spvPA) and (fn.tversky_beta, fn.focal_tversky_gamma, fn.batch_dice, fn.ce_focal_gamma) == want
        p.log_parameters()
        for k in ("tversky_beta", "focal_tversky_gamma", "batch_dice"):
            assert any(ln.split()[:2] == [k, "="] for ln in lines) == (want[0] is not None)
            if want[0] is not None:
                assert any(ln.split() == [k, "=", str(getattr(p, k))] for ln in lines)
        assert any(ln.split() == ["ce_focal_gamma", "=", str(want[3])] for ln in lines) == (want[3] > 0)
