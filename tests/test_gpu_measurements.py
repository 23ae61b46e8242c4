"""-m gpu: vs_seg_amd.compute_measurements (volume, centroid distance, largest 3-D and axial diameter on the device, csrc/measure.hip) against the
numpy oracle, known answers, empty masks, the foreground rules of compute_dice_score, the full 512x512x120 volume, determinism, and VSparams
--measurements end to end.

Tolerances: counts equal; volumes and the centroid distance rtol 1e-9 (a handful of fp64 operations on exact integers); diameters rtol 1e-6 (d^2
carries at most three products and two sums in fp32: off by at most about 6 * 2^-24 = 3.6e-7, d by half of that); diameters at unit spacing and
extents below 2048 equal (every d^2 is an integer below 2^24)."""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import measure_oracle as MO  # noqa: E402
from tests.test_gpu_surface_metrics import _ellipsoids  # noqa: E402
from tests.volume_cases import far_island_case, full_size_outputs, label as _label, logits as _logits, run_inference as _run_inference  # noqa: E402
from vs_seg_amd import MEASUREMENT_FIELDS, compute_measurements  # noqa: E402

COUNTS, EXACT64, DIAMETERS = [0, 1], [2, 3, 4], [5, 6, 7, 8]


def _check(got, want, unit_spacing=False):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape == (len(got), 9)
    print("got ", got.tolist(), "\nwant", want.tolist())
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[:, COUNTS], want[:, COUNTS])
    np.testing.assert_allclose(got[:, EXACT64], want[:, EXACT64], rtol=1e-9, atol=0)
    if unit_spacing:
        np.testing.assert_array_equal(got[:, DIAMETERS], want[:, DIAMETERS])
    else:
        np.testing.assert_allclose(got[:, DIAMETERS], want[:, DIAMETERS], rtol=1e-6, atol=0)


def _measure(pred, gt, spacing=None):
    """compute_measurements of boolean [B,X,Y,Z] masks (gt may be None)."""
    out = compute_measurements(_logits(pred), None if gt is None else _label(gt), spacing)
    assert out.shape == (len(pred), 9) and out.dtype == torch.float64 and out.is_cuda
    return out.cpu().numpy()


def _oracle(pred, gt, spacing=None):
    return [MO.measurements_auto(pred[b], None if gt is None else gt[b], spacing) for b in range(len(pred))]


# (37, 29, 11): 319 columns, two 16 x 16 column tiles along y with a ragged tail in y and z; (64, 48, 16): 768 columns, whole tiles; (150, 7, 5): five
# 32-plane pieces along x merge into one column; (20, 21, 37): three tiles along z, the last one a single plane wide, and equal-z pairs in different y tiles
@pytest.mark.parametrize("shape", [(37, 29, 11), (64, 48, 16), (150, 7, 5), (20, 21, 37)])
@pytest.mark.parametrize("spacing", [None, (0.5, 0.5, 1.5), (0.41, 0.43, 1.5)])
def test_against_oracle_random_ellipsoids(shape, spacing):
    rng = np.random.default_rng(sum(shape) + (0 if spacing is None else round(100 * spacing[1])))
    pred = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 2) for _ in range(2)])
    assert all(p.any() and g.any() for p, g in zip(pred, gt)) and all((p != g).any() for p, g in zip(pred, gt))
    _check(_measure(pred, gt, spacing), _oracle(pred, gt, spacing), spacing is None)


def test_known_answers():
    shape = (20, 18, 9)
    box = np.zeros((1, *shape), bool)
    box[0, 4:11, 3:12, 2:7] = True
    v = _measure(box, box, (0.5, 0.5, 1.5))[0]
    assert v[0] == v[1] == 7 * 9 * 5 and v[4] == 0.0
    np.testing.assert_allclose(v[[2, 3]], 7 * 9 * 5 * 0.375, rtol=1e-9)
    np.testing.assert_allclose(v[[5, 6]], np.sqrt(3.0**2 + 4.0**2 + 6.0**2), rtol=1e-6)
    np.testing.assert_allclose(v[[7, 8]], 5.0, rtol=1e-6)
    two, skew = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    two[0, 2, 3, 4] = two[0, 5, 7, 4] = True  # offset (3, 4, 0): both diameters 5
    skew[0, 2, 3, 4] = skew[0, 5, 7, 5] = True  # offset (3, 4, 1): no pair shares a slice
    v = _measure(two, skew)[0]
    assert (v[5], v[7]) == (5.0, 5.0)  # the 3-D and the axial diameter are equal ...
    assert v[6] == np.sqrt(np.float64(np.float32(26.0))) and v[8] == 0.0  # ... and here the 3-D one is larger
    assert v[4] == 0.5
    _check([v], _oracle(two, skew), True)


def test_farthest_pair_in_two_different_tiles():
    shape = (70, 65, 9)
    m = np.zeros((1, *shape), bool)
    m[0, 0, 0, 0] = m[0, 69, 64, 8] = True
    m[0, 33:37, 30:34, 3:6] = True
    g = np.zeros((1, *shape), bool)
    g[0, 0, 64, 4] = g[0, 69, 0, 4] = True  # the other diagonal, within one slice
    g[0, 30:40, 30:34, 4] = True
    for spacing in (None, (0.41, 0.43, 1.5)):
        got = _measure(m, g, spacing)
        _check(got, _oracle(m, g, spacing), spacing is None)
    assert got[0, 5] > 2 * got[0, 7] and got[0, 6] == got[0, 8]


def test_foreground_on_all_six_faces():
    shape = (21, 19, 18)
    m = np.zeros((1, *shape), bool)
    m[0, 0, 9, 9] = m[0, 20, 9, 9] = m[0, 10, 0, 9] = m[0, 10, 18, 9] = m[0, 10, 9, 0] = m[0, 10, 9, 17] = True
    g = np.zeros((1, *shape), bool)
    g[0, 0], g[0, -1], g[0, :, 0], g[0, :, -1], g[0, :, :, 0], g[0, :, :, -1] = True, True, True, True, True, True
    for spacing in (None, (0.5, 0.5, 1.5)):
        _check(_measure(m, g, spacing), _oracle(m, g, spacing), spacing is None)


def test_every_column_occupied():
    shape = (33, 17, 9)
    full = np.ones((1, *shape), bool)
    for spacing in (None, (0.41, 0.43, 1.5)):
        got = _measure(full, full, spacing)
        _check(got, [MO.measurements_reduced(full[0], full[0], spacing)], spacing is None)
        s = MO._spacing(spacing)
        np.testing.assert_allclose(got[0, [5, 6]], np.sqrt(((np.array(shape) - 1) * s) @ ((np.array(shape) - 1) * s)), rtol=1e-6)  # the body diagonal
        np.testing.assert_allclose(got[0, [7, 8]], np.hypot(32 * s[0], 16 * s[1]), rtol=1e-6)


def test_empty_masks_and_single_voxel():
    shape = (16, 12, 5)
    e, m, one = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    m[0, 3:9, 2:7, 1:4] = True
    one[0, 15, 11, 4] = True
    sp = (0.5, 0.5, 1.5)
    for pred, gt in ((e, m), (m, e), (e, e), (one, m), (m, one), (one, one)):
        _check(_measure(pred, gt, sp), _oracle(pred, gt, sp))
    v = _measure(e, e, sp)[0]
    assert (v[:4] == 0).all() and np.isnan(v[4:]).all()
    v = _measure(one, e, sp)[0]
    assert v[0] == 1 and v[5] == 0.0 and v[7] == 0.0 and np.isnan(v[[4, 6, 8]]).all()


def test_without_a_label():
    shape = (37, 29, 11)
    rng = np.random.default_rng(5)
    pred = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 2) for _ in range(2)])
    sp = (0.41, 0.43, 1.5)
    with_label, without = _measure(pred, gt, sp), _measure(pred, None, sp)
    assert np.isnan(without[:, [1, 3, 4, 6, 8]]).all()
    np.testing.assert_array_equal(without[:, [0, 2, 5, 7]], with_label[:, [0, 2, 5, 7]])
    _check(without, _oracle(pred, None, sp))


def test_foreground_rules_match_compute_dice_score():
    from vs_seg_amd import compute_dice_score

    shape = (12, 10, 6)
    lg = torch.zeros(1, 2, *shape, device="cuda")
    lg[0, 1, 2:5, 2:5, 1:4] = 1.0  # P: a 3x3x3 cube ...
    lg[0, :, 8:10, 6:9, 2:4] = 0.5  # ... tied logits elsewhere, which are class 0 ...
    lg[0, 1, 11, 0:4, 0] = float("nan")  # ... and NaN logits, which are background in either channel
    lg[0, 0, 11, 5:9, 5] = float("nan")
    lab = torch.zeros(1, 1, *shape, device="cuda")
    lab[0, 0, 2:5, 2:5, 1:4] = 1.0  # G = P
    lab[0, 0, 8, 0:3, 0] = 0.999  # not foreground: (int)0.999 == 0
    lab[0, 0, 10, 0:3, 5] = 2.0  # not foreground: (int)2.0 == 2
    v = compute_measurements(lg, lab).cpu().numpy()[0]
    assert v[0] == 27 and v[1] == 27 and v[4] == 0.0
    assert v[5] == v[6] == np.sqrt(12.0) and v[7] == v[8] == np.sqrt(8.0)  # the cube alone
    assert float(compute_dice_score(lg, lab)) == pytest.approx(1.0)  # 2 |P n G| / (|P| + |G|) = 1 with |P n G| <= 27: |P| = |G| = 27
    lab[0, 0, 10, 8, 5] = 1.0  # one more foreground voxel: now G differs from P
    pred = MO.prediction_mask(lg[0].cpu().numpy())  # (a comparison with NaN is false in numpy as well)
    gt = MO.label_mask(lab[0, 0].cpu().numpy())
    assert pred.sum() == 27 and gt.sum() == 28
    got = compute_measurements(lg, lab, (0.5, 0.5, 1.5)).cpu().numpy()
    _check(got, [MO.measurements(pred, gt, (0.5, 0.5, 1.5))])
    assert float(compute_dice_score(lg, lab)) == pytest.approx(2 * 27 / (got[0, 0] + got[0, 1]))


def test_full_size_channels_last_with_far_island():
    """512 x 512 x 120 with the logits in the channels-last view the sliding window returns: a tumour ellipsoid in both masks (shifted in the
    prediction) and one far false-positive island, which sets the prediction's diameter."""
    tumour, island, gt = far_island_case()
    pred = tumour | island
    outputs = full_size_outputs(pred)
    lab = torch.from_numpy(gt.astype(np.float32))[None, None].cuda()
    spacing = (0.41, 0.41, 1.5)
    got = compute_measurements(outputs, lab, spacing).cpu().numpy()
    _check(got, [MO.measurements_reduced(pred, gt, spacing)])
    assert got[0, 5] > 100.0 > got[0, 6]


def test_deterministic_and_batch_equals_single_calls():
    shape = (48, 40, 14)
    rng = np.random.default_rng(7)
    pred = np.stack([_ellipsoids(shape, rng, 4) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    lg, lab = _logits(pred), _label(gt)
    a = compute_measurements(lg, lab, (0.41, 0.43, 1.5))
    b = compute_measurements(lg, lab, (0.41, 0.43, 1.5))
    assert torch.equal(a, b) and not torch.isnan(a).any()
    singles = torch.cat([compute_measurements(lg[i:i + 1], lab[i:i + 1], (0.41, 0.43, 1.5)) for i in range(2)])
    assert torch.equal(a, singles)


PER_CASE = ("volume_pred_mm3", "volume_label_mm3", "volume_error_mm3", "centroid_distance_mm", "max_diameter_pred_mm", "max_diameter_label_mm", "max_axial_diameter_pred_mm",
            "max_axial_diameter_label_mm")
SUMMARY = ("mean_abs_volume_error_mm3", "mean_rel_volume_error", "mean_abs_max_diameter_error_mm", "mean_abs_max_axial_diameter_error_mm")


def test_vsparams_measurements_end_to_end(tmp_path):
    from vs_seg_amd import sliding_window_inference

    p, model, loader, scores, log = _run_inference(tmp_path / "on", ["--measurements"])
    assert scores.shape == (1,)
    assert all(f"{name}[0] = " in log for name in PER_CASE) and all(f"{name} = " in log and "left out)" in log for name in SUMMARY) and "measurements =" in log
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_measurements.csv"))))
    assert len(rows) == 1 and list(rows[0]) == ["case", "dice", *MEASUREMENT_FIELDS, "volume_error_mm3", "volume_rel_error"]
    assert float(rows[0]["dice"]) == pytest.approx(float(scores[0]), abs=1e-6)
    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, model.segmentation_predictor(), mode="gaussian")
        want = compute_measurements(o, data["label"], (0.5, 0.5, 1.5))[0].cpu().numpy()
    got = np.array([float(rows[0][k]) for k in MEASUREMENT_FIELDS])
    np.testing.assert_array_equal(got, want)  # bit for bit (NaN compares equal to NaN here)
    assert want[1] > 0  # the synthetic label is not empty
    assert float(rows[0]["volume_error_mm3"]) == want[2] - want[3]
    assert float(rows[0]["volume_rel_error"]) == abs(want[2] - want[3]) / want[3]

    p1, _, _, _, _ = _run_inference(tmp_path / "klc", ["--measurements", "--keep_largest_component"])
    kept = list(csv.DictReader(open(os.path.join(p1.figures_path, "test_postprocessing.csv"))))
    meas = list(csv.DictReader(open(os.path.join(p1.figures_path, "test_measurements.csv"))))
    assert len(kept) == len(meas) == 1 and float(meas[0]["voxels_pred"]) == int(kept[0]["kept_voxels"])
    assert float(meas[0]["voxels_label"]) == want[1]

    p2, _, _, _, log2 = _run_inference(tmp_path / "off", [])
    assert not os.path.exists(os.path.join(p2.figures_path, "test_measurements.csv"))
    assert not any(w in log2 for w in ("volume_pred", "volume_label", "volume_error", "centroid_distance", "diameter", "measurements ="))  # (the tmp path holds this test's name)
