"""-m gpu: vs_seg_amd.fill_holes / remove_small_components (csrc/components.hip) against the numpy oracle (tests/morphology_oracle.py): random masks, known
answers, cavities that cross every tile seam, the foreground rules, the full 512x512x120 volume, determinism, and VSparams --fill_holes /
--min_component_mm3 end to end.  Every comparison is between integers or exact 0.0 / 1.0 values: no tolerance anywhere."""
import csv
import functools
import glob
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_oracle as CO  # noqa: E402
from tests import morphology_oracle as MO  # noqa: E402
from tests.test_components_host import random_mask  # noqa: E402
from tests.test_morphology_host import CONNECTIVITIES, FILL_DENSITIES, KNOWN, SHAPES, SMALL_DENSITIES  # noqa: E402
from tests.volume_cases import full_size_ellipsoid as ell, full_size_outputs as _full_size_outputs, logits as _logits, run_inference as _run_inference  # noqa: E402
from vs_seg_amd import (compute_dice_score, compute_surface_distances, connected_components, fill_holes, keep_largest_component, min_component_voxels,  # noqa: E402
                        remove_small_components)
from vs_seg_amd.inferers import argmax_segmentation  # noqa: E402


def _check_fill(masks, connectivity, want=None):
    """fill_holes of the batch `masks` [B,X,Y,Z] equals the oracle's one-hot and statistics exactly (and `want`, when given), and leaves its input alone."""
    lg = _logits(masks)
    before = lg.clone()
    out, stats = fill_holes(lg, connectivity, return_stats=True)
    assert out.shape == lg.shape and out.dtype == torch.float32 and out.is_cuda
    assert stats.shape == (len(masks), 4) and stats.dtype == torch.int64 and stats.is_cuda
    assert torch.equal(lg, before)
    filled = np.stack([MO.fill_holes(m, connectivity) for m in masks])
    if want is not None:
        np.testing.assert_array_equal(filled, want)
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([CO.one_hot(f) for f in filled]))
    np.testing.assert_array_equal(stats.cpu().numpy(), np.stack([MO.fill_stats(m, connectivity) for m in masks]))
    assert torch.equal(fill_holes(lg, connectivity), out)  # without stats: the same tensor
    return stats.cpu().numpy()


def _check_small(masks, min_voxels, connectivity):
    lg = _logits(masks)
    before = lg.clone()
    out, stats = remove_small_components(lg, min_voxels, connectivity, return_stats=True)
    assert out.shape == lg.shape and out.dtype == torch.float32 and out.is_cuda
    assert stats.shape == (len(masks), 4) and stats.dtype == torch.int64 and stats.is_cuda
    assert torch.equal(lg, before)
    np.testing.assert_array_equal(out.cpu().numpy(), np.stack([CO.one_hot(MO.remove_small(m, min_voxels, connectivity)) for m in masks]))
    np.testing.assert_array_equal(stats.cpu().numpy(), np.stack([MO.small_stats(m, min_voxels, connectivity) for m in masks]))
    assert torch.equal(remove_small_components(lg, min_voxels, connectivity), out)
    return stats.cpu().numpy()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", FILL_DENSITIES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_fill_holes_against_oracle_random_masks(shape, density, connectivity):
    masks = np.stack([random_mask(shape, density), random_mask(shape[::-1], density).transpose(2, 1, 0)])
    stats = _check_fill(masks, connectivity)
    if density == 0.9:
        assert stats[0, 2] > 0


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", SMALL_DENSITIES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_remove_small_against_oracle_random_masks(shape, density, connectivity):
    masks = np.stack([random_mask(shape, density), random_mask(shape[::-1], density).transpose(2, 1, 0)])
    stats = {min_voxels: _check_small(masks, min_voxels, connectivity) for min_voxels in (0, 1, 2, 4, 50)}
    if density == 0.05:
        assert (stats[4][:, 3] < stats[4][:, 1]).all()  # the filter has work to do


@pytest.mark.parametrize("name", list(KNOWN))
def test_fill_holes_known_answers(name):
    mask, want = KNOWN[name]
    for c in CONNECTIVITIES:
        _check_fill(mask[None], c, want[c][None])


def test_kernel_in_cavity_comes_out_as_one_component():
    lg = _logits(KNOWN["kernel_in_cavity"][0][None])
    assert int(connected_components(lg, 26)[1][0, 1]) == 2
    assert int(connected_components(fill_holes(lg), 26)[1][0, 1]) == 1


def test_size_filter_known_answers():
    m = np.zeros((1, 12, 10, 6), bool)
    m[0, 0, 0, 0] = True
    m[0, 2:4, 2:4, 2:4] = True
    m[0, 7:9, 5:7, 1:3] = True  # two cubes of 8 voxels: treated alike
    m[0, 10, 1:4, 5] = True
    for c in CONNECTIVITIES:
        want = {0: [20, 4, 20, 4], 1: [20, 4, 20, 4], 3: [20, 4, 19, 3], 4: [20, 4, 16, 2], 8: [20, 4, 16, 2], 9: [20, 4, 0, 0], 2**40: [20, 4, 0, 0]}
        for mv, st in want.items():
            np.testing.assert_array_equal(_check_small(m, mv, c), [st])
    empty = torch.zeros(1, 2, 12, 10, 6, device="cuda")
    empty[:, 0] = 1.0
    out = remove_small_components(_logits(m), 9)
    assert torch.equal(out, empty)  # a threshold above every size: the empty one-hot


def _hollow(shape, lo, hi):
    m = np.zeros(shape, bool)
    m[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    m[lo[0] + 1:hi[0] - 1, lo[1] + 1:hi[1] - 1, lo[2] + 1:hi[2] - 1] = False
    return m


def test_cavities_across_every_seam():
    box = _hollow((20, 24, 140), (2, 3, 50), (15, 21, 80))  # the cavity crosses x = 4, 8, 12, y = 8, 16 and z = 64
    solid = np.zeros_like(box)
    solid[2:15, 3:21, 50:80] = True
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(_check_fill(box[None], c, solid[None]), [[box.sum(), 1, 11 * 16 * 28, solid.sum()]])
    serp = np.zeros((42, 35, 11), bool)  # a solid block with a one-voxel-wide serpentine cavity: rows along y, joined alternately at y = 32 and y = 2
    serp[1:41, 1:34, 1:10] = True
    block = serp.copy()
    for x in range(2, 40, 2):
        serp[x, 2:33, 5] = False
        if x + 1 < 39:
            serp[x + 1, 32 if (x // 2) % 2 == 1 else 2, 5] = False
    carved = int(block.sum() - serp.sum())
    assert carved == 19 * 31 + 18
    zserp = np.zeros((8, 9, 204), bool)  # the same along z, the axis a wave runs along: rows of 200 joined alternately at z = 201 and z = 2
    zserp[1:7, 1:8, 1:203] = True
    zblock = zserp.copy()
    for y in range(2, 7, 2):
        zserp[3, y, 2:202] = False
        if y + 1 < 6:
            zserp[3, y + 1, 201 if (y // 2) % 2 == 1 else 2] = False
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(_check_fill(serp[None], c, block[None]), [[serp.sum(), 1, carved, block.sum()]])
        np.testing.assert_array_equal(_check_fill(zserp[None], c, zblock[None]), [[zserp.sum(), 1, 602, zblock.sum()]])
    # the serpentine with its far end opened to the outside through one voxel: nothing of it is a hole any more
    opened = serp.copy()
    opened[38, 33, 5] = False
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(_check_fill(opened[None], c, opened[None]), [[opened.sum(), 0, 0, opened.sum()]])


@pytest.mark.parametrize("axis,side", [(a, s) for a in range(3) for s in (0, 1)])
def test_cup_open_at_the_face_of_the_bounding_box(axis, side):
    """A cup whose cavity reaches the level of its rim: the cavity lies inside the bounding box of P and its only exit lies exactly one voxel outside that box,
    away from the border of the volume.  It is not a hole; with a lid one voxel thick it is one, and the lid is then a face of the box."""
    shape, lo, hi = (21, 27, 139), [3, 5, 40], [14, 20, 90]  # the cup crosses x, y and z seams
    lid = _hollow(shape, lo, hi)
    cup = lid.copy()
    index = [slice(lo[a] + 1, hi[a] - 1) for a in range(3)]
    index[axis] = hi[axis] - 1 if side else lo[axis]
    cup[tuple(index)] = False  # take the lid off
    solid = np.zeros(shape, bool)
    solid[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    for c in CONNECTIVITIES:
        _check_fill(cup[None], c, cup[None])
        _check_fill(lid[None], c, solid[None])
    # ... and with a far voxel that grows the box by one on that side, the open cavity is still open
    far = cup.copy()
    pos = [1, 1, 1]
    pos[axis] = hi[axis] if side else lo[axis] - 1
    far[tuple(pos)] = True
    _check_fill(far[None], 6, far[None])


def test_foreground_rules_and_downstream_consumers():
    shape = (12, 10, 9)
    lg = torch.zeros(1, 2, *shape, device="cuda")
    lg[0, 1, 2:7, 2:7, 2:7] = 1.0  # a 5 x 5 x 5 cube ...
    lg[0, 1, 3:6, 3:6, 3:6] = 0.0  # ... hollow: the cavity's logits tie, which is background ...
    lg[0, 1, 4, 4, 4] = float("nan")  # ... or are NaN, which is background too
    lg[0, 0, 4, 4, 5] = float("nan")
    lg[0, 1, 10, 8, 1:3] = 3.0  # a 2-voxel island
    lg[0, :, 8:10, 0:3, 2:4] = 0.5  # tied logits outside: background
    before = lg.clone()
    out, stats = fill_holes(lg, return_stats=True)
    assert torch.equal(lg.isnan(), before.isnan()) and torch.equal(lg.nan_to_num(7.0), before.nan_to_num(7.0))  # the input is bit-unchanged
    np.testing.assert_array_equal(stats.cpu().numpy(), [[98 + 2, 1, 27, 125 + 2]])
    want = np.zeros(shape, bool)
    want[2:7, 2:7, 2:7] = True
    want[10, 8, 1:3] = True
    np.testing.assert_array_equal(out.cpu().numpy(), CO.one_hot(want)[None])
    small, sstats = remove_small_components(lg, 3, return_stats=True)
    np.testing.assert_array_equal(sstats.cpu().numpy(), [[100, 2, 98, 1]])
    shell = want.copy()
    shell[3:6, 3:6, 3:6] = False
    shell[10, 8, 1:3] = False
    np.testing.assert_array_equal(small.cpu().numpy(), CO.one_hot(shell)[None])
    # the results are predictions like any other
    lab = torch.zeros(1, 1, *shape, device="cuda")
    lab[0, 0, 2:7, 2:7, 2:7] = 1.0
    want_t = torch.from_numpy(CO.one_hot(want)[None]).cuda()
    assert torch.equal(compute_dice_score(out, lab), compute_dice_score(want_t, lab))
    assert float(compute_dice_score(out, lab)) == pytest.approx(2 * 125 / (127 + 125), abs=1e-6)
    assert float(compute_dice_score(out, lab)) > float(compute_dice_score(lg, lab))  # the hole cost Dice
    assert torch.equal(argmax_segmentation(out), torch.from_numpy(want.astype(np.uint8))[None].cuda())
    assert torch.equal(compute_surface_distances(out, lab, (1.0, 1.0, 1.0), 95.0), compute_surface_distances(want_t, lab, (1.0, 1.0, 1.0), 95.0))
    kept, kstats = keep_largest_component(out, return_stats=True)
    np.testing.assert_array_equal(kstats[0, :3].cpu().numpy(), [127, 2, 125])
    assert torch.equal(kept, remove_small_components(out, 3))
    assert torch.equal(fill_holes(small), keep_largest_component(out))  # the steps compose
    # channels-first storage gives the same result as channels-last
    cl = lg.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)
    assert not cl.is_contiguous() and lg.is_contiguous()
    assert torch.equal(fill_holes(cl), out) and torch.equal(remove_small_components(cl, 3), small)


def test_empty_and_all_foreground_small_volumes():
    lg = torch.zeros(2, 2, 16, 12, 5, device="cuda")
    lg[:, 0] = 1.0
    for out, stats in (fill_holes(lg, return_stats=True), remove_small_components(lg, 0, return_stats=True), remove_small_components(lg, 7, return_stats=True)):
        assert not stats.any() and torch.equal(out[:, 0], torch.ones_like(out[:, 0])) and not out[:, 1].any()
    full = lg.flip(1)
    n = 16 * 12 * 5
    out, stats = fill_holes(full, 26, return_stats=True)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[n, 0, 0, n]] * 2)
    assert torch.equal(out, full)


@functools.lru_cache(maxsize=1)
def _full_size_case():
    """512 x 512 x 120: an ellipsoid with an inner cavity and a 5-voxel island far away, built analytically (the numpy oracle is not run at 31 M voxels)."""
    tumour, cavity = ell((302, 219, 61), (13, 12, 5)), ell((303, 218, 62), (6, 5, 2))
    island = np.zeros(tumour.shape, bool)
    island[40, 470:475, 12] = True
    assert tumour.sum() == 3213 and cavity.sum() == 235 and not (cavity & ~ell((302, 219, 61), (11, 10, 4))).any()  # the cavity lies well inside
    return tumour, cavity, island


def test_full_size_fill_holes_fills_the_cavity_and_keeps_the_island():
    tumour, cavity, island = _full_size_case()
    outputs = _full_size_outputs((tumour & ~cavity) | island)
    before = outputs.clone()
    for c in CONNECTIVITIES:
        filled, stats = fill_holes(outputs, c, return_stats=True)
        np.testing.assert_array_equal(stats.cpu().numpy(), [[3213 - 235 + 5, 1, 235, 3213 + 5]])
        want = torch.from_numpy(tumour | island).cuda().float()
        assert torch.equal(filled[0, 1], want) and torch.equal(filled[0, 0], 1.0 - want)
    assert torch.equal(outputs, before)
    assert filled.permute(0, 2, 3, 4, 1).is_contiguous()  # a channels-last view, as keep_largest_component returns


def test_full_size_remove_small_drops_the_island():
    tumour, cavity, island = _full_size_case()
    outputs = _full_size_outputs((tumour & ~cavity) | island)
    kept, stats = remove_small_components(outputs, 6, return_stats=True)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[3213 - 235 + 5, 2, 3213 - 235, 1]])
    want = torch.from_numpy(tumour & ~cavity).cuda().float()
    assert torch.equal(kept[0, 1], want) and torch.equal(kept[0, 0], 1.0 - want)
    same, stats = remove_small_components(outputs, 5, return_stats=True)  # exactly min_voxels voxels: the island stays
    np.testing.assert_array_equal(stats.cpu().numpy(), [[3213 - 235 + 5, 2, 3213 - 235 + 5, 2]])
    assert int(same[0, 1].sum()) == 3213 - 235 + 5


def test_full_size_all_foreground_and_empty():
    shape = (512, 512, 120)
    n = shape[0] * shape[1] * shape[2]
    outputs = torch.zeros((1, *shape, 2), device="cuda")
    outputs[..., 1] = 1.0
    outputs = outputs.permute(0, 4, 1, 2, 3)
    filled, stats = fill_holes(outputs, return_stats=True)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[n, 0, 0, n]])
    assert bool((filled[0, 1] == 1.0).all()) and bool((filled[0, 0] == 0.0).all())
    kept, stats = remove_small_components(outputs, n, return_stats=True)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[n, 1, n, 1]])
    assert bool((kept[0, 1] == 1.0).all()) and bool((kept[0, 0] == 0.0).all())
    gone, stats = remove_small_components(outputs, n + 1, return_stats=True)
    np.testing.assert_array_equal(stats.cpu().numpy(), [[n, 1, 0, 0]])
    assert not gone[0, 1].any()
    empty = outputs.flip(1)
    for out, stats in (fill_holes(empty, return_stats=True), remove_small_components(empty, 6, return_stats=True)):
        assert not stats.any() and not out[0, 1].any() and bool((out[0, 0] == 1.0).all())


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_noise_at_half_density(connectivity):
    masks = (np.random.default_rng(5).random((96, 64, 80)) < 0.5)[None]
    _check_fill(masks, connectivity)
    _check_small(masks, 5, connectivity)


def test_deterministic_batch_equals_single_calls_and_second_stream():
    rng = np.random.default_rng(7)
    masks = rng.random((2, 48, 40, 70)) < 0.8
    lg = _logits(masks)
    for c in CONNECTIVITIES:
        for fn in (lambda x: fill_holes(x, c, return_stats=True), lambda x: remove_small_components(x, 3, c, return_stats=True)):
            a, sa = fn(lg)
            b, sb = fn(lg)
            assert torch.equal(a, b) and torch.equal(sa, sb)
            singles = [fn(lg[i:i + 1]) for i in range(2)]
            assert torch.equal(a, torch.cat([s[0] for s in singles])) and torch.equal(sa, torch.cat([s[1] for s in singles]))
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                d, sd = fn(lg)
            side.synchronize()
            assert torch.equal(a, d) and torch.equal(sa, sd)
        assert int(fill_holes(lg, c, return_stats=True)[1][:, 2].sum()) > 0


OLD_HEADER = ["case", "dice_raw", "dice", "components", "foreground_voxels", "kept_voxels"]
SPACING = (0.5, 0.5, 1.5)  # of the synthetic cases


def _raw_prediction(p, model, loader):
    from vs_seg_amd import sliding_window_inference

    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, lambda x: model(x)[0], mode="gaussian")
    return data, o, CO.prediction_mask(o[0].cpu().numpy())


def _dice_of(mask, data):
    return float(compute_dice_score(torch.from_numpy(CO.one_hot(mask)[None]).cuda(), data["label"]))


@pytest.mark.parametrize("quantile", [0.6, 0.97])
def test_vsparams_fill_holes_end_to_end(tmp_path, quantile):
    """At the 0.6 quantile the stand-in network marks 40 % of the voxels: a percolating foreground with enclosed background pockets.  At 0.97: the tumour and
    scattered voxels, few holes if any."""
    from vs_seg_amd.data.nifti import read_nifti

    p, model, loader, scores, log = _run_inference(tmp_path, ["--fill_holes", "--hole_connectivity", "26" if quantile > 0.9 else "6"], quantile)
    conn = p.hole_connectivity
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))
    assert len(rows) == 1 and list(rows[0]) == OLD_HEADER + ["holes", "filled_voxels"]
    row = rows[0]
    data, o, mask = _raw_prediction(p, model, loader)
    st = MO.fill_stats(mask, conn)
    final = MO.fill_holes(mask, conn)
    assert (int(row["foreground_voxels"]), int(row["holes"]), int(row["filled_voxels"]), int(row["kept_voxels"])) == tuple(int(v) for v in st)
    assert int(row["components"]) == CO.stats(CO.label(final, 26))[1]  # --fill_holes alone: the components of the filled prediction
    if quantile < 0.9:
        assert st[1] > 0 and st[2] > 0  # there were holes to fill
    assert float(row["dice_raw"]) == float(compute_dice_score(o, data["label"]))
    assert float(row["dice"]) == _dice_of(final, data) == float(scores[0])
    for text in ("fill_holes =", "hole_connectivity =", f"holes[0] = {st[1]}", f"filled_voxels[0] = {st[2]}", "dice_score_raw[0] = ", f"components[0] = {row['components']}"):
        assert text in log, text
    for text in ("removed_voxels", "small_components_removed", "keep_largest_component =", "min_component_mm3 ="):
        assert text not in log.replace(str(tmp_path), ""), text
    files = glob.glob(os.path.join(p.results_folder_path, "inferred_segmentations_nifti", "*", "*", "*.nii.gz"))
    assert len(files) == 1 and int((np.asarray(read_nifti(files[0])[0]) == 1).sum()) == st[3]


def test_vsparams_min_component_mm3_end_to_end(tmp_path):
    p, model, loader, scores, log = _run_inference(tmp_path, ["--min_component_mm3", "1.2"], 0.97)
    min_voxels = min_component_voxels(1.2, SPACING)
    assert min_voxels == 4  # 1.2 mm3 / 0.375 mm3 per voxel = 3.2
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))
    assert len(rows) == 1 and list(rows[0]) == OLD_HEADER + ["small_components", "small_voxels"]
    row = rows[0]
    data, o, mask = _raw_prediction(p, model, loader)
    st = MO.small_stats(mask, min_voxels, 26)
    final = MO.remove_small(mask, min_voxels, 26)
    assert (int(row["foreground_voxels"]), int(row["components"]), int(row["kept_voxels"])) == (st[0], st[1], st[2])
    assert (int(row["small_components"]), int(row["small_voxels"])) == (st[1] - st[3], st[0] - st[2])
    assert st[1] > st[3] > 0 and st[0] > st[2] > 0  # the filter had work to do and left something
    assert float(row["dice"]) == _dice_of(final, data) == float(scores[0]) and float(row["dice"]) > float(row["dice_raw"])
    for text in ("min_component_mm3 =", "component_connectivity =", f"small_components_removed[0] = {st[1] - st[3]}", f"removed_voxels[0] = {st[0] - st[2]}", f"components[0] = {st[1]}"):
        assert text in log, text
    for text in ("filled_voxels", "fill_holes =", "keep_largest_component ="):
        assert text not in log.replace(str(tmp_path), ""), text


def test_vsparams_all_three_steps_in_order(tmp_path):
    from vs_seg_amd.data.nifti import read_nifti

    p, model, loader, scores, log = _run_inference(tmp_path / "all", ["--fill_holes", "--min_component_mm3", "1.2", "--keep_largest_component", "--component_connectivity", "6",
                                                                      "--surface_metrics", "--measurements"], 0.7)
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))
    assert len(rows) == 1 and list(rows[0]) == OLD_HEADER + ["holes", "filled_voxels", "small_components", "small_voxels"]
    row = rows[0]
    data, o, mask = _raw_prediction(p, model, loader)
    fst = MO.fill_stats(mask, 6)
    filled = MO.fill_holes(mask, 6)  # 1. fill holes
    sst = MO.small_stats(filled, 4, 6)
    big = MO.remove_small(filled, 4, 6)  # 2. remove small components, of the filled prediction
    final = CO.keep_largest(big, 6)  # 3. keep the largest of what is left
    assert (int(row["foreground_voxels"]), int(row["holes"]), int(row["filled_voxels"])) == (fst[0], fst[1], fst[2])
    assert (int(row["components"]), int(row["small_components"]), int(row["small_voxels"])) == (sst[1], sst[1] - sst[3], sst[0] - sst[2])
    assert int(row["kept_voxels"]) == final.sum() and fst[2] > 0 and sst[1] > sst[3]
    assert f"removed_voxels[0] = {fst[3] - final.sum()}" in log
    assert float(row["dice"]) == _dice_of(final, data) == float(scores[0])
    final_t = torch.from_numpy(CO.one_hot(final)[None]).cuda()
    surf = list(csv.DictReader(open(os.path.join(p.figures_path, "test_surface_metrics.csv"))))[0]  # the other reports describe the final prediction too
    np.testing.assert_array_equal([float(surf["hd95_mm"]), float(surf["assd_mm"])], compute_surface_distances(final_t, data["label"], SPACING, 95.0)[0].cpu().numpy().astype(np.float64))
    meas = list(csv.DictReader(open(os.path.join(p.figures_path, "test_measurements.csv"))))[0]
    assert float(meas["voxels_pred"]) == final.sum()
    files = glob.glob(os.path.join(p.results_folder_path, "inferred_segmentations_nifti", "*", "*", "*.nii.gz"))
    assert int((np.asarray(read_nifti(files[0])[0]) == 1).sum()) == final.sum()

    p2, _, _, _, log2 = _run_inference(tmp_path / "old", ["--keep_largest_component"], 0.97)  # the old flag alone: the old header and the old lines
    rows2 = list(csv.DictReader(open(os.path.join(p2.figures_path, "test_postprocessing.csv"))))
    assert list(rows2[0]) == OLD_HEADER
    for text in ("holes[", "filled_voxels", "small_components_removed", "small_voxels_removed", "fill_holes =", "hole_connectivity =", "min_component_mm3 ="):
        assert text not in log2.replace(str(tmp_path), ""), text
    assert f"removed_voxels[0] = {int(rows2[0]['foreground_voxels']) - int(rows2[0]['kept_voxels'])}" in log2
