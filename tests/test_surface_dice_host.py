"""CPU tests of the normalised surface Dice: the numpy oracle against scipy's erosion + distance transform, the argument checks of vsseg_surface_metrics (made
before any launch) and of vs_seg_amd.compute_surface_metrics / compute_surface_dice (made before the device check), the column names, the --surface_dice_mm
flag and the header of figures/test_surface_dice.csv."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from tests import surface_dice_oracle as SDO
from vs_seg_amd import compute_surface_dice, compute_surface_metrics, surface_metric_fields

TOL_EXACT, TOL_INEXACT = (0.0, 1.0, 1.5, 2.0, 3.3), (0.0, 0.7, 1.0, 2.0, 3.3)  # where the squared distances are exact in fp64, and where they are not


def _scipy_metrics(pred, gt, spacing, tolerances):
    """[masd, (nsd, precision, recall) per tolerance]: binary_erosion with the default cross and border_value=0, distance_transform_edt(sampling=...)."""
    nd = pytest.importorskip("scipy.ndimage")
    ep, eg = pred & ~nd.binary_erosion(pred, border_value=0), gt & ~nd.binary_erosion(gt, border_value=0)
    n_p, n_g = int(ep.sum()), int(eg.sum())
    if not n_p and not n_g:
        return np.full(1 + 3 * len(tolerances), np.nan)
    if not n_p or not n_g:
        out = [np.inf]
        for _ in tolerances:
            out += [0.0, 0.0 if n_p else np.nan, 0.0 if n_g else np.nan]
        return np.array(out)
    dpg = nd.distance_transform_edt(~eg, sampling=spacing)[ep]
    dgp = nd.distance_transform_edt(~ep, sampling=spacing)[eg]
    out = [(dpg.mean() + dgp.mean()) / 2]
    for t in tolerances:
        w_p, w_g = int((dpg**2 <= t * t).sum()), int((dgp**2 <= t * t).sum())
        out += [(w_p + w_g) / (n_p + n_g), w_p / n_p, w_g / n_g]
    return np.array(out)


@pytest.mark.parametrize("spacing", [None, (0.5, 0.5, 1.5), (0.41, 0.43, 1.5)])
@pytest.mark.parametrize("seed", range(3))
def test_oracle_agrees_with_scipy(seed, spacing):
    rng = np.random.default_rng(40 + seed)
    shape = (24, 20, 9)
    pred, gt = rng.random(shape) < 0.04, rng.random(shape) < 0.03  # sparse, so that the distances spread over the tolerances
    pred[5:12, 4:11, 2:6] = True
    gt[6:14, 5:10, 3:7] = True
    sp = (1.0, 1.0, 1.0) if spacing is None else spacing
    TOL = TOL_EXACT
    if spacing == (0.41, 0.43, 1.5):  # the two fp64 routes round differently: the comparison needs inputs without near-ties (a condition on the inputs)
        TOL = TOL_INEXACT
        assert SDO.near_ties(pred, gt, spacing, TOL, 1e-9) == 0
    got = SDO.surface_metrics(pred, gt, spacing, 95.0, TOL)
    want = _scipy_metrics(pred, gt, sp, TOL)
    assert got.shape == (3 + 3 * len(TOL),)
    np.testing.assert_allclose(got[2], want[0], rtol=1e-12)
    np.testing.assert_array_equal(got[3:], want[1:])  # ratios of equal integer counts
    assert 0.0 < got[3] < got[-3] <= 1.0  # neither all 0 nor all 1
    empty = np.zeros(shape, bool)
    assert np.isnan(SDO.surface_metrics(empty, empty, spacing, 95.0, TOL)).all() and np.isnan(_scipy_metrics(empty, empty, sp, TOL)).all()
    for p, g in ((pred, empty), (empty, gt)):
        a, b = SDO.surface_metrics(p, g, spacing, 95.0, TOL), _scipy_metrics(p, g, sp, TOL)
        assert np.isposinf(a[:3]).all()
        np.testing.assert_array_equal(a[2:], b)


def test_oracle_known_answers():
    shape = (12, 12, 6)
    p, g = np.zeros(shape, bool), np.zeros(shape, bool)
    p[2, 3, 4] = g[5, 7, 4] = True  # offset (3, 4, 0): distance 5 either way
    v = SDO.surface_metrics(p, g, None, 95.0, (4.99, 5.0))
    np.testing.assert_array_equal(v, [5, 5, 5, 0, 0, 0, 1, 1, 1])
    box = np.zeros(shape, bool)
    box[2:9, 3:8, 1:5] = True
    np.testing.assert_array_equal(SDO.surface_metrics(box, box, (0.5, 0.5, 1.5), 95.0, (0.0,)), [0, 0, 0, 1, 1, 1])
    e = np.zeros(shape, bool)
    v = SDO.surface_metrics(e, box, None, 95.0, (1.0,))  # only P empty: precision is over the empty set
    assert np.isposinf(v[:3]).all() and v[3] == 0 and np.isnan(v[4]) and v[5] == 0
    v = SDO.surface_metrics(box, e, None, 95.0, (1.0,))
    assert np.isposinf(v[:3]).all() and v[3] == 0 and v[4] == 0 and np.isnan(v[5])
    assert np.isnan(SDO.surface_metrics(e, e, None, 95.0, (1.0, 2.0))).all() and len(SDO.surface_metrics(e, e, None, 95.0, ())) == 3


def test_surface_metric_fields():
    assert surface_metric_fields(()) == ("hd", "assd", "masd") == surface_metric_fields()
    assert surface_metric_fields((1, 0.5, 2.0, 1e6)) == ("hd", "assd", "masd", "nsd_1mm", "surface_precision_1mm", "surface_recall_1mm", "nsd_0.5mm", "surface_precision_0.5mm",
                                                         "surface_recall_0.5mm", "nsd_2mm", "surface_precision_2mm", "surface_recall_2mm", "nsd_1e+06mm", "surface_precision_1e+06mm",
                                                         "surface_recall_1e+06mm")
    with pytest.raises(ValueError):
        surface_metric_fields((-1.0,))


def test_c_entry_point_rejects_calls_outside_its_domain():
    from vs_seg_amd import _lib as L

    lib = L.lib()
    assert lib.vsseg_version() >= 19
    d = L.i3((4, 4, 4))
    need = lib.vsseg_surface_scratch_bytes(d)
    sp = (ctypes.c_float * 3)(1, 1, 1)
    bad_sp = [(ctypes.c_float * 3)(*v) for v in ((1, 0, 1), (1, -2, 1), (1, 1, float("inf")), (float("nan"), 1, 1))]
    tol = (ctypes.c_float * 8)(0, 0.5, 1, 1.5, 2, 3, 4, 5)
    f1 = lambda v: (ctypes.c_float * 1)(v)  # noqa: E731
    # (fake, aligned device addresses: every call below is rejected before anything is launched)
    # arguments: logits, pitch, label, dims, spacing, percentile, tolerances_mm, ntol, scratch, scratch_bytes, out
    cases = [((8, 2, 16, d, sp, 95.0, tol, -1, 256, need, 16), b"ntol"), ((8, 2, 16, d, sp, 95.0, tol, 9, 256, need, 16), b"ntol"),
             ((8, 2, 16, d, sp, 95.0, None, 1, 256, need, 16), b"tolerances_mm"), ((8, 2, 16, d, sp, 95.0, f1(-0.5), 1, 256, need, 16), b"tolerances_mm[0]"),
             ((8, 2, 16, d, sp, 95.0, f1(float("nan")), 1, 256, need, 16), b"tolerances_mm[0]"), ((8, 2, 16, d, sp, 95.0, f1(float("inf")), 1, 256, need, 16), b"tolerances_mm[0]"),
             ((8, 2, 16, d, sp, 95.0, (ctypes.c_float * 3)(1, 2, -1), 3, 256, need, 16), b"tolerances_mm[2]"),
             ((8, 3, 16, d, sp, 95.0, tol, 8, 256, need, 16), b"pitch"), ((8, 2, 16, L.i3((4, 4, 9000)), sp, 95.0, tol, 8, 256, need, 16), b"dims"),
             ((8, 2, 16, L.i3((0, 4, 4)), sp, 95.0, tol, 8, 256, need, 16), b"dims"), ((8, 2, 16, d, sp, 100.5, tol, 8, 256, need, 16), b"percentile"),
             ((8, 2, 16, d, sp, -1.0, None, 0, 256, need, 16), b"percentile"),  # a NULL tolerance pointer is accepted with ntol = 0: the call gets as far as the percentile
             ((8, 2, 16, d, sp, 95.0, tol, 8, 256, need - 1, 16), b"scratch"), ((8, 2, 16, d, sp, 95.0, None, 0, 256, need - 1, 16), b"scratch"),
             ((None, 2, 16, d, sp, 95.0, tol, 8, 256, need, 16), b"null"), ((8, 2, None, d, sp, 95.0, tol, 8, 256, need, 16), b"null"),
             ((8, 2, 16, d, sp, 95.0, tol, 8, None, need, 16), b"null"), ((8, 2, 16, d, sp, 95.0, tol, 8, 256, need, None), b"null"),
             ((4, 2, 16, d, sp, 95.0, tol, 8, 256, need, 16), b"misaligned"), ((8, 2, 18, d, sp, 95.0, tol, 8, 256, need, 16), b"misaligned"),
             ((8, 2, 16, d, sp, 95.0, tol, 8, 128, need, 16), b"misaligned"), ((8, 2, 16, d, sp, 95.0, tol, 8, 256, need, 18), b"misaligned")]
    cases += [((8, 2, 16, d, b, 95.0, tol, 8, 256, need, 16), b"spacing") for b in bad_sp]
    for args, why in cases:
        assert lib.vsseg_surface_metrics(*args, None) == L.EINVAL, args
        err = lib.vsseg_last_error()
        assert b"vsseg_surface_metrics" in err and why in err, (why, err)
    # the plain entry point still names itself
    assert lib.vsseg_surface_distances(8, 3, 16, d, sp, 95.0, 256, need, 16, None) == L.EINVAL
    assert b"vsseg_surface_distances" in lib.vsseg_last_error() and b"pitch" in lib.vsseg_last_error()


BAD_TOLERANCES = [(-0.5,), (1.0, float("nan")), (float("inf"),), ("a",), 1.0, "1 2", (None,), tuple(range(9))]


@pytest.mark.parametrize("kw", [dict(tolerances=t) for t in BAD_TOLERANCES] + [dict(percentile=-1.0), dict(percentile=100.5), dict(percentile=float("nan")), dict(percentile="high"),
                                                                              dict(spacing=(1.0, 1.0)), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, float("inf"), 1.0)), dict(spacing=3.0)])
def test_bad_arguments_raise_value_error(kw):
    pred, lab = torch.zeros(1, 2, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4)
    with pytest.raises(ValueError):
        compute_surface_metrics(pred, lab, **kw)
    if "percentile" not in kw:
        with pytest.raises(ValueError):
            compute_surface_dice(pred, lab, **kw)


@pytest.mark.parametrize("pred_shape,lab_shape", [((1, 3, 8, 8, 4), (1, 1, 8, 8, 4)), ((1, 2, 8, 8, 4), (1, 1, 8, 8, 5)), ((2, 2, 8, 8, 4), (1, 1, 8, 8, 4)), ((2, 8, 8, 4), (2, 8, 8, 4))])
def test_mismatched_shapes_raise_value_error(pred_shape, lab_shape):
    with pytest.raises(ValueError):
        compute_surface_metrics(torch.zeros(pred_shape), torch.zeros(lab_shape), tolerances=(1.0,))
    with pytest.raises(ValueError):
        compute_surface_dice(torch.zeros(pred_shape), torch.zeros(lab_shape))


def test_cpu_tensors_raise_runtime_error():
    pred, lab = torch.zeros(1, 2, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_surface_metrics(pred, lab, spacing=(0.5, 0.5, 1.5), percentile=None, tolerances=(0, 1, 2, 3, 4, 5, 6, 7))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_surface_metrics(pred, lab)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_surface_dice(pred, lab)


def test_command_line_flag(capsys):
    from vs_seg_amd.params import VSparams

    def parse(argv):
        try:
            return VSparams(argparse.ArgumentParser(), argv)
        except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
            assert "no GPU" in str(e)
            return None

    for bad in (["--surface_dice_mm"], ["--surface_dice_mm", "one"], ["--surface_dice_mm", "-1"], ["--surface_dice_mm", "nan"], ["--surface_dice_mm", "1", "inf"],
                ["--surface_dice_mm", "1", "2", "1.0"], ["--surface_dice_mm"] + [str(i) for i in range(9)]):
        with pytest.raises(SystemExit):
            parse(bad)
        assert "--surface_dice_mm" in capsys.readouterr().err, bad
    for argv, want in (([], ()), (["--surface_dice_mm", "2"], (2.0,)), (["--surface_dice_mm", "2", "0.5", "1", "--surface_metrics"], (0.5, 1.0, 2.0)),
                       (["--surface_dice_mm"] + [str(i) for i in range(8)], tuple(float(i) for i in range(8))), (["--surface_metrics"], ())):
        p = parse(argv)
        if p is not None:
            assert p.surface_dice_mm == want


def test_csv_header():
    from vs_seg_amd.params import surface_dice_csv_header

    assert surface_dice_csv_header((1.0, 2.0)) == "case,dice,masd_mm,nsd_1mm,surface_precision_1mm,surface_recall_1mm,nsd_2mm,surface_precision_2mm,surface_recall_2mm"
    assert surface_dice_csv_header((0.5,)) == "case,dice,masd_mm,nsd_0.5mm,surface_precision_0.5mm,surface_recall_0.5mm"
