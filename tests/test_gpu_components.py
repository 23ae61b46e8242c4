"""-m gpu: vs_seg_amd.connected_components / keep_largest_component (csrc/components.hip) against the numpy union-find oracle: random masks, known
answers, paths that cross every tile seam, the foreground rules, the full 512x512x120 volume, determinism, and VSparams --keep_largest_component end
to end.  Every comparison is between integers or exact 0.0 / 1.0 values: no tolerance anywhere."""
import csv
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_oracle as CO  # noqa: E402
from tests.test_components_host import CONNECTIVITIES, DENSITIES, SHAPES, random_mask  # noqa: E402
from tests.volume_cases import far_island_case, full_size_outputs as _full_size_outputs, logits as _logits, run_inference as _run_inference  # noqa: E402
from vs_seg_amd import compute_dice_score, compute_surface_distances, connected_components, keep_largest_component  # noqa: E402
from vs_seg_amd.inferers import argmax_segmentation  # noqa: E402


def _check_labels(masks, connectivity):
    """connected_components of the batch `masks` [B,X,Y,Z] equals the oracle, labels and stats."""
    labels, stats = connected_components(_logits(masks), connectivity)
    assert labels.shape == masks.shape and labels.dtype == torch.int32 and labels.is_cuda
    assert stats.shape == (len(masks), 4) and stats.dtype == torch.int64 and stats.is_cuda
    want = [CO.label(m, connectivity) for m in masks]
    np.testing.assert_array_equal(labels.cpu().numpy(), np.stack(want))
    np.testing.assert_array_equal(stats.cpu().numpy(), np.stack([CO.stats(w) for w in want]))
    return stats.cpu().numpy()


def _check_keep(masks, connectivity):
    """keep_largest_component of the batch equals the oracle's one-hot exactly, and leaves its input alone."""
    lg = _logits(masks)
    before = lg.clone()
    out, stats = keep_largest_component(lg, connectivity, return_stats=True)
    assert out.shape == lg.shape and out.dtype == torch.float32 and out.is_cuda
    assert torch.equal(lg, before)
    want = np.stack([CO.one_hot(CO.keep_largest(m, connectivity)) for m in masks])
    np.testing.assert_array_equal(out.cpu().numpy(), want)
    np.testing.assert_array_equal(stats.cpu().numpy(), np.stack([CO.stats(CO.label(m, connectivity)) for m in masks]))
    assert torch.equal(keep_largest_component(lg, connectivity), out)  # without stats: the same tensor
    return out


@pytest.mark.parametrize("shape", SHAPES + [(9, 17, 130)])  # (the last one: every axis straddles the tile and z crosses two seams, as the morphology routes are tested)
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_labels_against_oracle_random_masks(shape, density, connectivity):
    masks = np.stack([random_mask(shape, density), random_mask(shape[::-1], density).transpose(2, 1, 0)])
    _check_labels(masks, connectivity)
    _check_keep(masks, connectivity)


def test_known_answers():
    checker = (np.indices((8, 8, 8)).sum(0) % 2 == 0)[None]
    assert [int(_check_labels(checker, c)[0, 1]) for c in CONNECTIVITIES] == [256, 1, 1]
    m = np.zeros((1, 12, 10, 6), bool)
    m[0, 0, 0, 0] = True
    m[0, 2:4, 2:4, 2:4] = True
    m[0, 7:9, 5:7, 1:3] = True
    keep = np.zeros_like(m)
    keep[0, 2:4, 2:4, 2:4] = True  # the two cubes tie: the first in raster order is kept
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(_check_labels(m, c), [[17, 3, 8, (2 * 10 + 2) * 6 + 2 + 1]])
        np.testing.assert_array_equal(_check_keep(m, c).cpu().numpy(), CO.one_hot(keep[0])[None])


def test_paths_across_every_seam():
    serp = np.zeros((1, 40, 33, 9), bool)  # a one-voxel-wide serpentine: rows along y, joined alternately at y = 32 and y = 0
    for x in range(0, 40, 2):
        serp[0, x, :, 4] = True
        if x + 1 < 40:
            serp[0, x + 1, 32 if (x // 2) % 2 == 0 else 0, 4] = True
    assert serp.sum() == 680
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(_check_labels(serp, c), [[680, 1, 680, 5]])
        np.testing.assert_array_equal(_check_keep(serp, c)[0, 1].cpu().numpy(), serp[0].astype(np.float32))
    i = np.arange(48)
    chain = np.zeros((1, 48, 48, 48), bool)  # contacts at every seam position, whatever the tile size
    chain[0, i, i, i] = True
    assert [int(_check_labels(chain, c)[0, 1]) for c in CONNECTIVITIES] == [48, 48, 1]
    flat = np.zeros((1, 48, 48, 5), bool)
    flat[0, i, i, 2] = True
    assert [int(_check_labels(flat, c)[0, 1]) for c in CONNECTIVITIES] == [48, 1, 1]
    zserp = np.zeros((1, 6, 5, 200), bool)  # the same along z, the axis a wave runs along: rows of 200 joined alternately at z = 199 and z = 0
    for y in range(0, 5, 2):
        zserp[0, 3, y, :] = True
        if y + 1 < 5:
            zserp[0, 3, y + 1, 199 if (y // 2) % 2 == 0 else 0] = True
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(_check_labels(zserp, c), [[602, 1, 602, (3 * 5) * 200 + 1]])


def test_foreground_rules_and_downstream_metrics():
    shape = (12, 10, 6)
    lg = torch.zeros(1, 2, *shape, device="cuda")
    lg[0, 1, 2:5, 2:5, 1:4] = 1.0  # a 3x3x3 cube ...
    lg[0, 1, 9:11, 7:9, 4:6] = 2.0  # ... a 2x2x2 cube ...
    lg[0, :, 8:10, 0:3, 2:4] = 0.5  # ... tied logits, which are background ...
    lg[0, 1, 6, 0:4, 0] = float("nan")  # ... and NaN logits, which are background too
    lg[0, 0, 0, 5:9, 5] = float("nan")
    before = lg.clone()
    labels, stats = connected_components(lg)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[35, 2, 27, (2 * 10 + 2) * 6 + 1 + 1]])
    mask = np.zeros(shape, bool)
    mask[2:5, 2:5, 1:4] = True
    np.testing.assert_array_equal(labels[0].cpu().numpy() == (2 * 10 + 2) * 6 + 1 + 1, mask)
    out = keep_largest_component(lg)
    assert torch.equal(lg.isnan(), before.isnan()) and torch.equal(lg.nan_to_num(7.0), before.nan_to_num(7.0))  # the input is bit-unchanged
    np.testing.assert_array_equal(out.cpu().numpy(), CO.one_hot(mask)[None])
    lab = torch.zeros(1, 1, *shape, device="cuda")
    lab[0, 0, 2:5, 2:5, 1:5] = 1.0
    want = torch.from_numpy(CO.one_hot(mask)[None]).cuda()
    assert torch.equal(compute_dice_score(out, lab), compute_dice_score(want, lab))
    assert float(compute_dice_score(out, lab)) == pytest.approx(2 * 27 / (27 + 36), abs=1e-6)
    assert torch.equal(argmax_segmentation(out), torch.from_numpy(mask.astype(np.uint8))[None].cuda())


def test_empty_prediction():
    lg = torch.zeros(2, 2, 16, 12, 5, device="cuda")
    lg[:, 0] = 1.0
    labels, stats = connected_components(lg)
    assert not labels.any() and not stats.any()
    out, stats = keep_largest_component(lg, return_stats=True)
    assert not stats.any() and torch.equal(out[:, 0], torch.ones_like(out[:, 0])) and not out[:, 1].any()


def test_full_size_channels_last_drops_the_far_island():
    """The tumour + far island of the surface-distance test at 512 x 512 x 120: the island goes, and with it the 100 mm Hausdorff distance."""
    tumour, island, gt = far_island_case()
    assert tumour.sum() == 3213 and island.sum() == 41
    outputs = _full_size_outputs(tumour | island)
    before = outputs.clone()
    filtered, stats = keep_largest_component(outputs, return_stats=True)
    assert torch.equal(outputs, before)
    label = int(np.flatnonzero(tumour.ravel())[0]) + 1
    np.testing.assert_array_equal(stats.cpu().numpy(), [[3254, 2, 3213, label]])
    kept = torch.from_numpy(tumour).cuda()
    assert torch.equal(filtered[0, 1], kept.float()) and torch.equal(filtered[0, 0], 1.0 - kept.float())
    labels, stats2 = connected_components(outputs)
    assert torch.equal(stats2, stats)
    island_label = int(np.flatnonzero(island.ravel())[0]) + 1
    want = torch.from_numpy(np.where(tumour, label, 0) + np.where(island, island_label, 0)).to(torch.int32).cuda()
    assert torch.equal(labels[0], want)
    lab = torch.from_numpy(gt.astype(np.float32))[None, None].cuda()
    spacing = (0.41, 0.41, 1.5)
    clean = compute_surface_distances(_full_size_outputs(tumour), lab, spacing, None)
    assert torch.equal(compute_surface_distances(filtered, lab, spacing, None), clean)
    assert float(clean[0, 0]) < 10.0 < 100.0 < float(compute_surface_distances(outputs, lab, spacing, None)[0, 0])


def test_full_size_all_foreground():
    shape = (512, 512, 120)
    outputs = torch.zeros((1, *shape, 2), device="cuda")
    outputs[..., 1] = 1.0
    outputs = outputs.permute(0, 4, 1, 2, 3)
    n = shape[0] * shape[1] * shape[2]
    for c in CONNECTIVITIES:
        filtered, stats = keep_largest_component(outputs, c, return_stats=True)
        np.testing.assert_array_equal(stats.cpu().numpy(), [[n, 1, n, 1]])
        assert bool((filtered[0, 1] == 1.0).all()) and bool((filtered[0, 0] == 0.0).all())
    labels, stats = connected_components(outputs)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[n, 1, n, 1]])
    assert bool((labels == 1).all())


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_noise_at_half_density(connectivity):
    masks = (np.random.default_rng(5).random((128, 128, 32)) < 0.5)[None]
    _check_labels(masks, connectivity)
    _check_keep(masks, connectivity)


def test_deterministic_batch_equals_single_calls_and_second_stream():
    rng = np.random.default_rng(7)
    masks = rng.random((2, 48, 40, 70)) < 0.22
    lg = _logits(masks)
    for c in CONNECTIVITIES:
        a, sa = keep_largest_component(lg, c, return_stats=True)
        b, sb = keep_largest_component(lg, c, return_stats=True)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        la, _ = connected_components(lg, c)
        lb, _ = connected_components(lg, c)
        assert torch.equal(la, lb)
        singles = [keep_largest_component(lg[i:i + 1], c, return_stats=True) for i in range(2)]
        assert torch.equal(a, torch.cat([s[0] for s in singles])) and torch.equal(sa, torch.cat([s[1] for s in singles]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d, sd = keep_largest_component(lg, c, return_stats=True)
            ld, _ = connected_components(lg, c)
        side.synchronize()
        assert torch.equal(a, d) and torch.equal(sa, sd) and torch.equal(la, ld)


@pytest.mark.parametrize("connectivity", [26, 6])
def test_vsparams_keep_largest_component_end_to_end(tmp_path, connectivity):
    from vs_seg_amd import sliding_window_inference
    from vs_seg_amd.data.nifti import read_nifti

    p, model, loader, scores, log = _run_inference(tmp_path / "on", ["--keep_largest_component", "--surface_metrics", "--component_connectivity", str(connectivity)])
    assert scores.shape == (1,)
    for text in ("dice_score[0] = ", "dice_score_raw[0] = ", "components[0] = ", "removed_voxels[0] = ", "mean_dice_score_raw = ", "keep_largest_component =", "component_connectivity =",
                 "hd95_mm[0] = "):
        assert text in log, text
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))
    assert len(rows) == 1 and list(rows[0]) == ["case", "dice_raw", "dice", "components", "foreground_voxels", "kept_voxels"]
    row = rows[0]
    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, model.segmentation_predictor(), mode="gaussian")
        filtered, stats = keep_largest_component(o, connectivity, return_stats=True)
        assert float(row["dice"]) == float(compute_dice_score(filtered, data["label"])) == float(scores[0])
        assert float(row["dice_raw"]) == float(compute_dice_score(o, data["label"]))
        want_surface = compute_surface_distances(filtered, data["label"], (0.5, 0.5, 1.5), 95.0)[0].cpu().numpy()
    fg, comps, kept, _ = (int(v) for v in stats[0].cpu())
    assert (int(row["foreground_voxels"]), int(row["components"]), int(row["kept_voxels"])) == (fg, comps, kept)
    assert f"components[0] = {comps}" in log and f"removed_voxels[0] = {fg - kept}" in log
    assert fg >= kept
    surf = list(csv.DictReader(open(os.path.join(p.figures_path, "test_surface_metrics.csv"))))[0]  # the surface metrics describe the filtered prediction too
    np.testing.assert_array_equal([float(surf["hd95_mm"]), float(surf["assd_mm"])], want_surface.astype(np.float64))
    assert float(surf["dice"]) == float(row["dice"])
    files = glob.glob(os.path.join(p.results_folder_path, "inferred_segmentations_nifti", "*", "*", "*.nii.gz"))
    assert len(files) == 1
    seg = np.asarray(read_nifti(files[0])[0])
    assert set(np.unique(seg).tolist()) <= {0, 1} and int((seg == 1).sum()) == kept
    assert CO.stats(CO.label(seg == 1, connectivity))[1] <= 1  # (reorienting the volume permutes and flips axes: connectivity is unchanged)

    p2, _, _, scores2, log2 = _run_inference(tmp_path / "off", [])
    assert not os.path.exists(os.path.join(p2.figures_path, "test_postprocessing.csv"))
    for text in ("_raw", "components[", "removed_voxels", "keep_largest_component =", "component_connectivity ="):
        assert text not in log2.replace(str(tmp_path), ""), text  # (the tmp path holds this test's name)
    assert float(scores2[0]) == float(row["dice_raw"])  # without the switch the reported Dice is that of the raw argmax, as before


def test_vsparams_keep_largest_component_removes_scattered_voxels(tmp_path):
    """The same run with a stand-in network that marks the brightest 3 % of the voxels (the tumour and scattered noise, below the percolation density): the
    filter has work to do, and what it leaves is what is scored and exported."""
    from vs_seg_amd import sliding_window_inference
    from vs_seg_amd.data.nifti import read_nifti

    p, model, loader, scores, log = _run_inference(tmp_path / "on", ["--keep_largest_component"], bright_quantile=0.97)
    row = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))[0]
    assert not os.path.exists(os.path.join(p.figures_path, "test_surface_metrics.csv")) and "hd95" not in log
    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, lambda x: model(x)[0], mode="gaussian")
        filtered, stats = keep_largest_component(o, 26, return_stats=True)
        assert float(row["dice"]) == float(compute_dice_score(filtered, data["label"])) == float(scores[0])
        assert float(row["dice_raw"]) == float(compute_dice_score(o, data["label"]))
    mask = CO.prediction_mask(o[0].cpu().numpy())
    np.testing.assert_array_equal(stats[0].cpu().numpy(), CO.stats(CO.label(mask, 26)))
    np.testing.assert_array_equal(filtered[0, 1].cpu().numpy(), CO.keep_largest(mask, 26).astype(np.float32))
    fg, comps, kept, _ = (int(v) for v in stats[0].cpu())
    assert (int(row["foreground_voxels"]), int(row["components"]), int(row["kept_voxels"])) == (fg, comps, kept)
    assert comps > 1 and fg > kept > 0 and f"removed_voxels[0] = {fg - kept}" in log
    assert float(row["dice"]) > float(row["dice_raw"])  # the scattered false positives are gone
    files = glob.glob(os.path.join(p.results_folder_path, "inferred_segmentations_nifti", "*", "*", "*.nii.gz"))
    seg = np.asarray(read_nifti(files[0])[0])
    assert int((seg == 1).sum()) == kept and CO.stats(CO.label(seg == 1, 26))[1] == 1
