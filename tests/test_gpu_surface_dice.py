"""-m gpu: vs_seg_amd.compute_surface_metrics / compute_surface_dice (normalised surface Dice at mm tolerances from the edge pass and distance transform of the
surface distances, csrc/surface.hip) against the numpy oracle, known answers with exact ties, the empty-mask rules, bit equality with
compute_surface_distances, the full 512x512x120 volume, and VSparams --surface_dice_mm end to end."""
import csv
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import surface_dice_oracle as SDO  # noqa: E402
from tests import surface_oracle as SO  # noqa: E402
from tests.test_gpu_surface_metrics import _check, _ellipsoids  # noqa: E402
from tests.volume_cases import far_island_case, full_size_outputs, label as _label, logits as _logits, run_inference as _run_inference  # noqa: E402
from vs_seg_amd import compute_surface_dice, compute_surface_distances, compute_surface_metrics, surface_metric_fields  # noqa: E402

TOL_EXACT = (0.0, 1.0, 1.5, 2.0, 3.3)  # at spacing None and (0.5, 0.5, 1.5): the fp32 field is exact, so ties are decided exactly
TOL_INEXACT = (0.0, 0.7, 1.0, 2.0, 3.3)  # at spacing (0.41, 0.43, 1.5)


def _check_all(got, want):
    """hd, assd, masd to the 1e-5 of the surface-distance tests; the ratio columns to 1e-6 (one miscounted voxel moves a ratio by >= 1.3e-4 at these sizes)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape
    _check(got[:, :3], want[:, :3])
    r, w = got[:, 3:], want[:, 3:]
    assert (np.isnan(r) == np.isnan(w)).all(), (r, w)
    np.testing.assert_allclose(r[~np.isnan(w)], w[~np.isnan(w)], rtol=1e-6, atol=1e-6)


@functools.lru_cache(maxsize=None)
def _random_case(shape, spacing):
    """The masks of test_gpu_surface_metrics.test_against_oracle_random_ellipsoids (same generator, same seed rule) and their oracle rows."""
    rng = np.random.default_rng(sum(shape) + (0 if spacing is None else round(100 * spacing[1])))
    pred = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 2) for _ in range(2)])
    tol = TOL_INEXACT if spacing == (0.41, 0.43, 1.5) else TOL_EXACT
    want = np.stack([SDO.surface_metrics(pred[b], gt[b], spacing, 95.0, tol) for b in range(2)])
    return pred, gt, tol, want


@pytest.mark.parametrize("shape", [(37, 29, 11), (64, 48, 16)])
@pytest.mark.parametrize("spacing", [None, (0.5, 0.5, 1.5), (0.41, 0.43, 1.5)])
def test_against_oracle_random_ellipsoids(shape, spacing):
    pred, gt, tol, want = _random_case(shape, spacing)
    assert all(p.any() and g.any() for p, g in zip(pred, gt)) and (pred != gt).any()
    for b in range(2):  # conditions on the inputs
        if tol is TOL_EXACT:  # edge voxels whose distance EQUALS tau: the <= rule and the exactness of the field are under test
            assert all(SDO.near_ties(pred[b], gt[b], spacing, (t,), 0.0) > 0 for t in ((1.0, 2.0) if spacing is None else (1.0, 1.5, 2.0)))
        else:  # no fp64 squared distance within a relative 1e-4 of any tau^2: the fp32 field (a few 2^-23 from it) decides every voxel like the oracle
            assert SDO.near_ties(pred[b], gt[b], spacing, tol, 1e-4) == 0
    nsd = want[:, 3::3]
    assert 0.0 <= nsd.min() and 0.1 < nsd.max() < 1.0  # neither all 0 nor all 1
    got = compute_surface_metrics(_logits(pred), _label(gt), spacing, 95.0, tol)
    assert got.shape == (2, 3 + 3 * len(tol)) and got.dtype == torch.float32 and got.is_cuda
    print("got", got.cpu().numpy().tolist(), "want", want.tolist())
    _check_all(got.cpu().numpy(), want)


def test_known_answers():
    shape = (20, 18, 9)
    a = np.zeros((1, *shape), bool)
    a[0, 4:11, 3:12, 2:7] = True
    np.testing.assert_array_equal(compute_surface_metrics(_logits(a), _label(a), None, 95.0, (0.0,)).cpu().numpy(), [[0, 0, 0, 1, 1, 1]])
    p, g = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    p[0, 2, 3, 4] = True
    g[0, 5, 7, 4] = True  # offset (3, 4, 0): distance 5 either way, an exact tie with tau = 5 at unit spacing
    got = compute_surface_metrics(_logits(p), _label(g), None, 95.0, (4.99, 5.0)).cpu().numpy()
    np.testing.assert_array_equal(got[0, 3:], [0, 0, 0, 1, 1, 1])
    assert got[0, 2] == 5.0
    np.testing.assert_array_equal(compute_surface_dice(_logits(p), _label(g), None, (4.99, 5.0)).cpu().numpy(), [[0.0, 1.0]])
    outer, inner = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    outer[0, 2:16, 2:16, 1:8] = True
    inner[0, 6:12, 6:12, 3:6] = True
    tol = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 1e6)
    for spacing in (None, (0.5, 0.5, 1.5)):
        want = SDO.surface_metrics(outer[0], inner[0], spacing, 95.0, tol)
        got = compute_surface_metrics(_logits(outer), _label(inner), spacing, 95.0, tol).cpu().numpy()
        _check_all(got, [want])
        nsd = got[0, 3::3]
        assert (np.diff(nsd) >= 0).all() and nsd[0] == 0.0 and 0.0 < nsd[-2] < 1.0  # non-decreasing in tau
        np.testing.assert_array_equal(got[0, -3:], [1, 1, 1])  # everything is within 1e6 mm


def test_empty_masks():
    shape = (16, 12, 5)
    e, m = np.zeros((1, *shape), bool), np.zeros((1, *shape), bool)
    m[0, 3:9, 2:7, 1:4] = True
    tol = (0.0, 1.0, 1e6)
    both = compute_surface_metrics(_logits(e), _label(e), None, 95.0, tol).cpu().numpy()
    assert both.shape == (1, 12) and np.isnan(both).all()
    only_p_empty = compute_surface_metrics(_logits(e), _label(m), None, 95.0, tol).cpu().numpy()[0]
    only_g_empty = compute_surface_metrics(_logits(m), _label(e), None, 95.0, tol).cpu().numpy()[0]
    for v, empty_col, other_col in ((only_p_empty, 1, 2), (only_g_empty, 2, 1)):  # column 1 of a triple: over E(P), column 2: over E(G)
        assert np.isposinf(v[:3]).all()
        t = v[3:].reshape(3, 3)
        assert (t[:, 0] == 0).all() and np.isnan(t[:, empty_col]).all() and (t[:, other_col] == 0).all()
    for lg, lab, want in ((e, e, np.nan), (e, m, np.inf), (m, e, np.inf)):
        got = compute_surface_metrics(_logits(lg), _label(lab), (0.5, 0.5, 1.5), None, ()).cpu().numpy()
        np.testing.assert_array_equal(got, [[want] * 3])
        assert compute_surface_dice(_logits(lg), _label(lab), None, ()).shape == (1, 0)


def test_shares_the_call_with_the_surface_distances():
    shape = (48, 40, 14)
    rng = np.random.default_rng(7)
    pred = np.stack([_ellipsoids(shape, rng, 4) for _ in range(2)])
    gt = np.stack([_ellipsoids(shape, rng, 3) for _ in range(2)])
    lg, lab, sp = _logits(pred), _label(gt), (0.41, 0.43, 1.5)
    for pc in (None, 0, 50, 95):
        plain = compute_surface_distances(lg, lab, sp, pc)
        for tol in ((), (0.5, 1.0, 2.0, 3.0)):
            assert torch.equal(compute_surface_metrics(lg, lab, sp, pc, tol)[:, :2], plain), (pc, tol)
        assert torch.equal(compute_surface_distances(lg, lab, sp, pc), plain)  # ... and the plain call is not disturbed by the combined one
    a = compute_surface_metrics(lg, lab, sp, 95.0, (0.5, 1.0, 2.0, 3.0))
    assert torch.equal(a, compute_surface_metrics(lg, lab, sp, 95.0, (0.5, 1.0, 2.0, 3.0)))
    assert torch.equal(a, torch.cat([compute_surface_metrics(lg[i:i + 1], lab[i:i + 1], sp, 95.0, (0.5, 1.0, 2.0, 3.0)) for i in range(2)]))
    assert torch.equal(compute_surface_dice(lg, lab, sp, (0.5, 1.0, 2.0, 3.0)), a[:, 3::3])
    assert torch.equal(compute_surface_metrics(lg, lab, sp, 95.0, (1.0, 2.0)), a[:, [0, 1, 2, 6, 7, 8, 9, 10, 11]])
    assert 0.0 < float(a[:, 3].min()) and float(a[:, 3].max()) < float(a[:, 12].min()) <= 1.0
    assert torch.equal(compute_surface_dice(lg, lab, sp), compute_surface_metrics(lg, lab, sp, 95.0, (1.0,))[:, 3:4])  # the default tolerance is 1 mm


def test_full_size_channels_last_with_far_island():
    """The 512 x 512 x 120 case of test_gpu_surface_metrics: a tumour ellipsoid in both masks (shifted in the prediction) and one far false-positive island.  The
    island shows in the surface precision and in masd, and not in the recall."""
    tumour, island, gt = far_island_case()
    pred = tumour | island
    outputs = full_size_outputs(pred)
    lab = torch.from_numpy(gt.astype(np.float32))[None, None].cuda()
    spacing, tol = (0.41, 0.41, 1.5), (0.0, 0.5, 1.0, 2.0, 3.0)
    assert SDO.near_ties(pred, gt, spacing, tol, 1e-4) == 0
    want = SDO.surface_metrics(pred, gt, spacing, 95.0, tol)
    np.testing.assert_allclose(want[3::3], [0.17979, 0.36832, 0.59329, 0.98348, 0.98348], atol=1e-5)  # the oracle's values, recorded with the test
    np.testing.assert_allclose([want[3 + 3 * 3 + 1], want[3 + 3 * 3 + 2], want[2], want[1]], [0.96743, 1.0, 3.40113, 3.43853], atol=1e-5)
    got = compute_surface_metrics(outputs, lab, spacing, 95.0, tol)
    print("got", got.cpu().numpy().tolist(), "want", want.tolist())
    _check_all(got.cpu().numpy(), [want])
    assert torch.equal(got[:, :2], compute_surface_distances(outputs, lab, spacing, 95.0))


def test_vsparams_surface_dice_end_to_end(tmp_path):
    from vs_seg_amd import sliding_window_inference

    p, model, loader, scores, log = _run_inference(tmp_path / "nsd", ["--surface_dice_mm", "2", "1"])
    assert p.surface_dice_mm == (1.0, 2.0) and scores.shape == (1,)
    assert not os.path.exists(os.path.join(p.figures_path, "test_surface_metrics.csv")) and "hd95_mm" not in log and "surface_metrics =" not in log
    for name in ("surface_dice_mm =", "masd_mm[0] = ", "nsd_1mm[0] = ", "surface_precision_2mm[0] = ", "surface_recall_2mm[0] = ", "mean_nsd_2mm = ", "mean_masd_mm = "):
        assert name in log, name
    lines = open(os.path.join(p.figures_path, "test_surface_dice.csv")).read().splitlines()
    assert lines[0] == "case,dice,masd_mm,nsd_1mm,surface_precision_1mm,surface_recall_1mm,nsd_2mm,surface_precision_2mm,surface_recall_2mm" and len(lines) == 2
    row = next(csv.DictReader(lines))
    assert float(row["dice"]) == pytest.approx(float(scores[0]), abs=1e-6)
    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, model.segmentation_predictor(), mode="gaussian")
        same = compute_surface_metrics(o, data["label"], (0.5, 0.5, 1.5), 95.0, (1.0, 2.0))[0].cpu().numpy().astype(np.float64)
        pred, gt = SO.prediction_mask(o[0].cpu().numpy()), SO.label_mask(data["label"][0, 0].cpu().numpy())
    got = np.array([float(row[k]) for k in lines[0].split(",")[2:]])
    np.testing.assert_array_equal(got, same[2:])  # (NaN and inf compare equal to themselves here)
    want = SDO.surface_metrics(pred, gt, (0.5, 0.5, 1.5), 95.0, (1.0, 2.0))  # spacing 0.5 / 1.5: the field is exact, ties included
    _check_all(same[None], want[None])

    alone = _run_inference(tmp_path / "hd", ["--surface_metrics"])
    both = _run_inference(tmp_path / "both", ["--surface_metrics", "--surface_dice_mm", "1", "2"])
    assert not os.path.exists(os.path.join(alone[0].figures_path, "test_surface_dice.csv")) and "nsd" not in alone[4].replace(str(tmp_path), "")
    read = lambda q, name: open(os.path.join(q.figures_path, name), "rb").read()  # noqa: E731
    assert read(both[0], "test_surface_metrics.csv") == read(alone[0], "test_surface_metrics.csv")
    assert read(both[0], "test_surface_dice.csv") == read(p, "test_surface_dice.csv")
    assert [ln.split("        ", 1)[1] for ln in alone[4].splitlines() if "hd95_mm" in ln or "assd_mm" in ln] == [
        ln.split("        ", 1)[1] for ln in both[4].splitlines() if "hd95_mm" in ln or "assd_mm" in ln]
    assert surface_metric_fields((1.0, 2.0))[3:] == tuple(lines[0].split(",")[3:])
