"""-m gpu: vs_seg_amd.compute_surface_distances (HD / ASSD on the device, csrc/surface.hip) against the brute-force numpy oracle, known answers,
empty masks, the foreground rules of compute_dice_score, the full 512x512x120 volume, determinism, and VSparams --surface_metrics end to end."""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import surface_oracle as SO  # noqa: E402
from tests.volume_cases import far_island_case, full_size_outputs, label as _label, logits as _logits, run_inference  # noqa: E402
from vs_seg_amd import compute_surface_distances  # noqa: E402


def _ellipsoids(shape, rng, k):
    """Union of k random ellipsoids, centres anywhere in (or just outside) the volume; the first one crosses the x = 0 face."""
    g = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    m = np.zeros(shape, bool)
    for i in range(k):
        c = [rng.uniform(-0.1, 1.1) * s for s in shape]
        c[0] = 0.0 if i == 0 else c[0]  # the first one crosses the x = 0 face
        r = [rng.uniform(0.15, 0.45) * s + 0.6 for s in shape]
        m |= sum(((gi - ci) / ri) ** 2 for gi, ci, ri in zip(g, c, r)) <= 1.0
    return m


def _check(got, want):
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape
    same_special = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))
    fin = np.isfinite(want)
    assert (same_special | fin).all() and np.isfinite(got[fin]).all(), (got, want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape", [(37, 29, 11), (64, 48, 16)])
@pytest.mark.parametrize("spacing", [None, (0.5, 0.5, 1.5), (0.41, 0.43, 1.5)])
def test_against_oracle_random_ellipsoids(shape, spacing):
    rng = np.random.default_rng(sum(shape) + (0 if spacing is None else round(100 * spacing[1])))
    pred = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 2) for _ in range(2)])
    assert all(p.any() and g.any() and p[0].any() and g[0].any() for p, g in zip(pred, gt)) and (pred != gt).any()
    lg, lab = _logits(pred), _label(gt)
    for pc in (None, 0, 50, 95, 100):
        got = compute_surface_distances(lg, lab, spacing, pc)
        assert got.shape == (2, 2) and got.dtype == torch.float32 and got.is_cuda
        want = [SO.surface_distances(pred[b], gt[b], spacing, pc) for b in range(2)]
        _check(got.cpu().numpy(), want)


def test_known_answers():
    shape = (20, 18, 9)
    a = np.zeros((1, *shape), bool)
    a[0, 4:11, 3:12, 2:7] = True
    np.testing.assert_array_equal(compute_surface_distances(_logits(a), _label(a)).cpu().numpy(), [[0.0, 0.0]])
    p, g = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    p[0, 2, 3, 4] = True
    g[0, 5, 7, 4] = True  # offset (3, 4, 0): distance 5 either way
    np.testing.assert_allclose(compute_surface_distances(_logits(p), _label(g), None, 95.0).cpu().numpy(), [[5.0, 5.0]], rtol=1e-6)
    outer, inner = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    outer[0, 2:16, 2:16, 1:8] = True
    inner[0, 6:12, 6:12, 3:6] = True
    for spacing in (None, (0.5, 0.5, 1.5)):
        for pc in (None, 50, 95):
            want = SO.surface_distances(outer[0], inner[0], spacing, pc)
            _check(compute_surface_distances(_logits(outer), _label(inner), spacing, pc).cpu().numpy(), [want])


def test_empty_masks():
    shape = (16, 12, 5)
    e, m = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    m[0, 3:9, 2:7, 1:4] = True
    assert np.isnan(compute_surface_distances(_logits(e), _label(e)).cpu().numpy()).all()
    assert np.isposinf(compute_surface_distances(_logits(e), _label(m)).cpu().numpy()).all()  # only P empty
    assert np.isposinf(compute_surface_distances(_logits(m), _label(e)).cpu().numpy()).all()  # only G empty


def test_foreground_rules_match_compute_dice_score():
    from vs_seg_amd import compute_dice_score

    shape = (12, 10, 6)
    lg = torch.zeros(1, 2, *shape, device="cuda")
    lg[0, 1, 2:5, 2:5, 1:4] = 1.0  # P: a 3x3x3 cube ...
    lg[0, :, 8:10, 6:9, 2:4] = 0.5  # ... and tied logits elsewhere, which are class 0
    lab = torch.zeros(1, 1, *shape, device="cuda")
    lab[0, 0, 2:5, 2:5, 1:4] = 1.0  # G = P
    lab[0, 0, 8, 0:3, 0] = 0.999  # not foreground: (int)0.999 == 0
    lab[0, 0, 10, 0:3, 5] = 2.0  # not foreground: (int)2.0 == 2
    np.testing.assert_array_equal(compute_surface_distances(lg, lab).cpu().numpy(), [[0.0, 0.0]])
    assert float(compute_dice_score(lg, lab)) == pytest.approx(1.0)
    lab[0, 0, 10, 8, 5] = 1.0  # one more foreground voxel: now G differs from P
    pred = SO.prediction_mask(lg[0].cpu().numpy())
    gt = SO.label_mask(lab[0, 0].cpu().numpy())
    assert pred.sum() == 27 and gt.sum() == 28
    _check(compute_surface_distances(lg, lab, (0.5, 0.5, 1.5), None).cpu().numpy(), [SO.surface_distances(pred, gt, (0.5, 0.5, 1.5), None)])


def test_full_size_channels_last_with_far_island():
    """512 x 512 x 120 with the logits in the channels-last view the sliding window returns: a tumour ellipsoid in both masks (shifted in the
    prediction) and one far false-positive island; the masks are small, so the brute-force oracle needs no scipy."""
    tumour, island, gt = far_island_case()
    pred = tumour | island
    outputs = full_size_outputs(pred)
    lab = torch.from_numpy(gt.astype(np.float32))[None, None].cuda()
    spacing = (0.41, 0.41, 1.5)
    hd95 = compute_surface_distances(outputs, lab, spacing, 95.0).cpu().numpy()
    _check(hd95, [SO.surface_distances(pred, gt, spacing, 95.0)])
    hd = compute_surface_distances(outputs, lab, spacing, None).cpu().numpy()
    _check(hd, [SO.surface_distances(pred, gt, spacing, None)])
    assert hd[0, 0] > 100.0 > hd95[0, 0]  # the island sets the maximum, not the 95th percentile


def test_deterministic_and_batch_equals_single_calls():
    shape = (48, 40, 14)
    rng = np.random.default_rng(7)
    pred = np.stack([_ellipsoids(shape, rng, 4) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    lg, lab = _logits(pred), _label(gt)
    a = compute_surface_distances(lg, lab, (0.41, 0.43, 1.5), 95.0)
    b = compute_surface_distances(lg, lab, (0.41, 0.43, 1.5), 95.0)
    assert torch.equal(a, b)
    singles = torch.cat([compute_surface_distances(lg[i:i + 1], lab[i:i + 1], (0.41, 0.43, 1.5), 95.0) for i in range(2)])
    assert torch.equal(a, singles)


def test_vsparams_surface_metrics_end_to_end(tmp_path):
    from vs_seg_amd import sliding_window_inference

    p, model, loader, scores, log = run_inference(tmp_path / "on", ["--surface_metrics"])
    assert scores.shape == (1,)
    assert "hd95_mm[0] = " in log and "assd_mm[0] = " in log and "mean_hd95_mm = " in log and "mean_assd_mm = " in log and "surface_metrics =" in log
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_surface_metrics.csv"))))
    assert len(rows) == 1 and list(rows[0]) == ["case", "dice", "hd95_mm", "assd_mm"]
    assert float(rows[0]["dice"]) == pytest.approx(float(scores[0]), abs=1e-6)
    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, model.segmentation_predictor(), mode="gaussian")
        want = compute_surface_distances(o, data["label"], (0.5, 0.5, 1.5), 95.0)[0].cpu().numpy()
    got = np.array([float(rows[0]["hd95_mm"]), float(rows[0]["assd_mm"])])
    np.testing.assert_array_equal(got, want.astype(np.float64))  # (equal_nan: NaN and inf compare equal to themselves)

    p2, _, _, _, log2 = run_inference(tmp_path / "off", [])
    assert not os.path.exists(os.path.join(p2.figures_path, "test_surface_metrics.csv"))
    assert "hd95" not in log2 and "assd" not in log2 and "surface_metrics =" not in log2  # (the tmp path holds this test's name)
