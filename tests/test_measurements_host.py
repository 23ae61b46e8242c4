"""CPU tests of the size measurements: the argument checks of the two C entry points (made before any launch) and of vs_seg_amd.compute_measurements
(made before the device check), the numpy oracle's two routines against each other and against known answers, and the --measurements flag."""
import argparse
import ctypes

import numpy as np
import pytest
import torch

from tests import measure_oracle as MO
from vs_seg_amd import MEASUREMENT_FIELDS, compute_measurements


def test_field_names():
    assert MEASUREMENT_FIELDS == MO.FIELDS and len(MEASUREMENT_FIELDS) == 9
    assert MEASUREMENT_FIELDS[0] == "voxels_pred" and MEASUREMENT_FIELDS[-1] == "max_axial_diameter_label_mm"


def test_c_entry_points_reject_calls_outside_their_domain():
    from vs_seg_amd import _lib as L

    lib = L.lib()
    assert lib.vsseg_version() >= 17
    assert lib.vsseg_measure_scratch_bytes(L.i3((512, 512, 120))) > 0
    assert lib.vsseg_measure_scratch_bytes(L.i3((120, 512, 512))) > 0  # 512 x 512 in-plane in any orientation
    for bad in ((0, 8, 8), (8, 8, 0), (4, 513, 512), (4, 8192, 33), (8193, 4, 4)):
        assert lib.vsseg_measure_scratch_bytes(L.i3(bad)) == L.EINVAL, bad
        err = lib.vsseg_last_error()
        assert b"vsseg_measure_scratch_bytes" in err and b"dims" in err
    d = L.i3((4, 4, 4))
    need = lib.vsseg_measure_scratch_bytes(d)
    sp = (ctypes.c_float * 3)(1, 1, 1)
    bad_sp = [(ctypes.c_float * 3)(*v) for v in ((1, 0, 1), (1, -2, 1), (1, 1, float("inf")), (float("nan"), 1, 1))]
    # (fake, aligned device addresses: every call below is rejected before anything is launched)
    # arguments: logits, pitch, label, dims, spacing, scratch, scratch_bytes, out
    cases = [((8, 3, 16, d, sp, 256, need, 32), b"pitch"), ((8, 2, 16, L.i3((4, 4, 9000)), sp, 256, need, 32), b"dims"), ((8, 2, 16, L.i3((0, 4, 4)), sp, 256, need, 32), b"dims"),
             ((8, 2, 16, L.i3((4, 513, 512)), sp, 256, 1 << 40, 32), b"dims"), ((8, 2, 16, d, sp, 256, need - 1, 32), b"scratch"), ((None, 2, 16, d, sp, 256, need, 32), b"null"),
             ((8, 2, 16, d, sp, None, need, 32), b"null"), ((8, 2, 16, d, sp, 256, need, None), b"null"), ((4, 2, 16, d, sp, 256, need, 32), b"misaligned"),
             ((8, 2, 18, d, sp, 256, need, 32), b"misaligned"), ((8, 2, 16, d, sp, 128, need, 32), b"misaligned"), ((8, 2, 16, d, sp, 256, need, 36), b"misaligned"),
             ((8, 2, None, d, sp, 256, need - 1, 32), b"scratch")]  # a NULL label is accepted: the call gets as far as the scratch check
    cases += [((8, 2, 16, d, b, 256, need, 32), b"spacing") for b in bad_sp]
    for args, why in cases:
        assert lib.vsseg_measurements(*args, None) == L.EINVAL, args
        err = lib.vsseg_last_error()
        assert b"vsseg_measurements" in err and why in err, (why, err)


@pytest.mark.parametrize("kw", [dict(spacing=(1.0, 1.0)), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, -2.0, 1.0)), dict(spacing=(1.0, float("inf"), 1.0)), dict(spacing=3.0),
                                dict(spacing=("a", "b", "c"))])
def test_bad_spacing_raises_value_error(kw):
    with pytest.raises(ValueError):
        compute_measurements(torch.zeros(1, 2, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4), **kw)
    with pytest.raises(ValueError):
        compute_measurements(torch.zeros(1, 2, 8, 8, 4), None, **kw)


@pytest.mark.parametrize("pred_shape,lab_shape", [((1, 3, 8, 8, 4), (1, 1, 8, 8, 4)), ((1, 2, 8, 8, 4), (1, 1, 8, 8, 5)), ((2, 2, 8, 8, 4), (1, 1, 8, 8, 4)), ((2, 8, 8, 4), (2, 8, 8, 4)),
                                                  ((1, 3, 8, 8, 4), None), ((2, 8, 8, 4), None)])
def test_mismatched_shapes_raise_value_error(pred_shape, lab_shape):
    with pytest.raises(ValueError):
        compute_measurements(torch.zeros(pred_shape), None if lab_shape is None else torch.zeros(lab_shape))


def test_cpu_tensors_raise_runtime_error():
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_measurements(torch.zeros(1, 2, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4), spacing=(0.5, 0.5, 1.5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        compute_measurements(torch.zeros(1, 2, 8, 8, 4))


@pytest.mark.parametrize("seed", range(12))
def test_oracle_routines_agree_exactly(seed):
    """Brute force over all voxels == brute force over the column extremes (3-D: along z, axial: along y), with == on fp64."""
    rng = np.random.default_rng(100 + seed)
    shape = (int(rng.integers(1, 21)), int(rng.integers(1, 21)), int(rng.integers(1, 10)))
    spacing = None if seed % 3 == 0 else tuple(rng.uniform(0.3, 2.0, 3))
    dp, dg = rng.uniform(0.02, 0.6, 2)
    pred, gt = rng.random(shape) < dp, rng.random(shape) < dg
    a, b = MO.measurements(pred, gt, spacing), MO.measurements_reduced(pred, gt, spacing)
    np.testing.assert_array_equal(a, b)  # (NaN compares equal to NaN here)
    for axis in range(3):  # ... and along any axis for the 3-D diameter
        s = MO._spacing(spacing)
        assert MO.farthest(np.argwhere(MO.column_extremes(pred, axis)), s) == a[5] or (np.isnan(a[5]) and not pred.any())
    np.testing.assert_array_equal(MO.measurements(pred, None, spacing)[[0, 2, 5, 7]], a[[0, 2, 5, 7]])
    assert np.isnan(MO.measurements(pred, None, spacing)[[1, 3, 4, 6, 8]]).all()


def test_oracle_known_answers():
    shape = (20, 18, 9)
    box = np.zeros(shape, bool)
    box[4:11, 3:12, 2:7] = True
    for fn in (MO.measurements, MO.measurements_reduced):
        v = fn(box, box, (0.5, 0.5, 1.5))
        assert v[0] == v[1] == 7 * 9 * 5
        assert v[2] == v[3] == pytest.approx(7 * 9 * 5 * 0.375, rel=1e-12)
        assert v[4] == 0.0
        assert v[5] == v[6] == pytest.approx(np.sqrt(3.0**2 + 4.0**2 + 6.0**2), rel=1e-12)
        assert v[7] == v[8] == pytest.approx(5.0, rel=1e-12)
        two = np.zeros(shape, bool)
        two[2, 3, 4] = two[5, 7, 4] = True  # offset (3, 4, 0)
        assert tuple(fn(two)[[0, 5, 7]]) == (2.0, 5.0, 5.0)
        skew = np.zeros(shape, bool)
        skew[2, 3, 4] = skew[5, 7, 5] = True  # offset (3, 4, 1): no pair shares a slice
        v = fn(skew, two)
        assert v[5] == pytest.approx(np.sqrt(26.0), rel=1e-15) and v[7] == 0.0
        assert v[4] == pytest.approx(0.5, rel=1e-15)  # centres (3.5, 5, 4.5) and (3.5, 5, 4)
        empty, one = np.zeros(shape, bool), np.zeros(shape, bool)
        one[7, 1, 8] = True
        v = fn(empty, one, (0.41, 0.43, 1.5))
        assert v[0] == 0 and v[2] == 0 and np.isnan(v[[4, 5, 7]]).all()
        assert v[1] == 1 and v[3] == pytest.approx(0.41 * 0.43 * 1.5, rel=1e-6) and v[6] == 0.0 and v[8] == 0.0
        assert np.isnan(fn(empty, empty)[4:]).all()


def test_command_line_flag():
    from vs_seg_amd.params import VSparams

    def parse(argv):
        try:
            return VSparams(argparse.ArgumentParser(), argv)
        except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
            assert "no GPU" in str(e)
            return None

    with pytest.raises(SystemExit):
        parse(["--measurements", "yes"])
    for argv, want in (([], False), (["--measurements"], True), (["--measurements", "--keep_largest_component", "--surface_metrics"], True)):
        p = parse(argv)
        if p is not None:
            assert p.measurements is want
