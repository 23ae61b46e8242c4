"""-m gpu: vs_seg_amd.binary_dilate / binary_erode / binary_close / binary_open (csrc/ball.hip) against the fp64 numpy oracle (tests/ball_oracle.py): random masks
at unit, dyadic and non-dyadic spacings, the largest reach, the border rule, known answers, the foreground rules and the consumers of the result, determinism,
the full 512 x 512 x 120 volume, and VSparams --closing_mm / --opening_mm end to end.  Every comparison is between integers or exact 0.0 / 1.0 values: no
tolerance anywhere."""
import csv
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ball_oracle as BO  # noqa: E402
from tests import components_oracle as CO  # noqa: E402
from tests import morphology_oracle as MO  # noqa: E402
from tests.volume_cases import far_island_case, full_size_outputs as _full_size_outputs, logits as _logits, run_inference as _run_inference  # noqa: E402
from vs_seg_amd import (binary_close, binary_dilate, binary_erode, binary_open, compute_dice_score, compute_measurements, keep_largest_component,  # noqa: E402
                        min_component_voxels)

CALLS = {"dilate": binary_dilate, "erode": binary_erode, "close": binary_close, "open": binary_open}
UNIT = (1.0, 1.0, 1.0)


def _one_hot_t(masks):
    return torch.from_numpy(np.stack([CO.one_hot(m) for m in masks]))


def _check(masks, op, spacing, r, want=None):
    """The operation `op` on the batch `masks` [B,X,Y,Z] equals the oracle's one-hot and statistics exactly (and `want`, when given), and leaves its input alone.
    Returns the statistics."""
    lg = _logits(masks)
    before = lg.clone()
    out, stats = CALLS[op](lg, r, spacing, return_stats=True)
    assert out.shape == lg.shape and out.dtype == torch.float32 and out.is_cuda
    assert stats.shape == (len(masks), 4) and stats.dtype == torch.int64 and stats.is_cuda
    assert torch.equal(lg, before)
    results = np.stack([BO.OPS[op](m, spacing, r) for m in masks])
    if want is not None:
        np.testing.assert_array_equal(results, want)
    assert torch.equal(out.cpu(), _one_hot_t(results)), (op, masks.shape, spacing, r, int((out[:, 1].cpu().numpy() != results).sum()))
    assert torch.equal(stats.cpu(), torch.from_numpy(np.stack([BO.stats(m, w) for m, w in zip(masks, results)]))), (op, masks.shape, spacing, r, stats)
    return stats.cpu().numpy()


def _random(shape, density, seed):
    return np.random.default_rng(seed).random(shape) < density


def _two_blobs(density, seed):
    """(70, 40, 33): two blobs in opposite corners, so that the work box spans several tiles along x and y and several lines."""
    m = np.zeros((70, 40, 33), bool)
    m[2:14, 3:12, 1:9] = _random((12, 9, 8), density, seed)
    m[55:69, 27:38, 23:32] = _random((14, 11, 9), density, seed + 1)
    return m


RANDOM_SHAPES = [(24, 20, 12), (37, 29, 19), (1, 17, 9), (16, 1, 1), (2, 2, 2)]


@pytest.mark.parametrize("op", list(CALLS))
@pytest.mark.parametrize("spacing,radii", [(UNIT, (0.0, 1.0, 1.5, 2.0, 3.0)), ((0.5, 0.5, 1.5), (1.5, 2.0)), ((1.0, 1.0, 3.0), (2.0,))])
def test_against_oracle_random_masks(op, spacing, radii):
    """(0.5, 0.5, 1.5) at r = 1.5: the offset dz = 1 is an exact tie and must count; (1, 1, 3) at r = 2: reach 0 along z, nothing spreads across slices."""
    changed = 0
    for density in ((0.02, 0.3) if op in ("dilate", "close") else (0.7, 0.97)):
        for r in radii:
            for shape in RANDOM_SHAPES:
                st = _check(np.stack([_random(shape, density, 1), _random(shape, density, 2)]), op, spacing, r)
                changed += int(st[:, 2:].sum())
            changed += int(_check(_two_blobs(density, 3)[None], op, spacing, r)[:, 2:].sum())
    assert changed > 0 or radii == (0.0,)  # the operation had work to do: an identity implementation cannot pass


@pytest.mark.parametrize("op", list(CALLS))
@pytest.mark.parametrize("r", [2.0, 2.5, 5.0])
def test_non_dyadic_spacing(op, r):
    """(0.41, 0.41, 1.5): the fp32 products are rounded, so an offset within a few 2^-24 of the surface of the ball may fall on either side.  These radii keep every
    offset at least 1e-4 away (1.7e-2, 4.8e-3, 1.9e-3), against fp32 rounding of about 1e-6: the result must equal the fp64 oracle exactly.  (r = 1.5 and 3.0 are
    exact ties along z at this spacing and are left out here.)"""
    spacing = (0.41, 0.41, 1.5)
    assert BO.tie_margin(spacing, r) >= 1e-4
    density = 0.05 if op in ("dilate", "close") else 0.9
    _check(np.stack([_random((37, 29, 19), density, 4), _random((37, 29, 19), density, 5)]), op, spacing, r)
    _check(_two_blobs(density, 6)[None], op, spacing, r)


@pytest.mark.parametrize("op", list(CALLS))
def test_maximum_reach(op):
    spacing, r = (0.25, 1.0, 1.0), 8.0
    assert BO.reach(spacing, r) == [32, 8, 8]
    density = 0.002 if op in ("dilate", "close") else 0.998
    st = _check(np.stack([_random((80, 12, 10), density, 7), _random((80, 12, 10), density, 8)]), op, spacing, r)
    assert st[:, 2:].sum() > 0 and (st[:, 0] > 0).all()
    with pytest.raises(ValueError, match="33 voxels along axis 0"):
        CALLS[op](_logits(np.zeros((1, 80, 12, 10), bool)), 8.25, spacing)


def test_border_rule_empty_and_all_foreground():
    shape = (20, 18, 14)
    blocks = []
    for axis in range(3):
        for side in (0, 1):  # a block on each of the six faces
            m = np.zeros(shape, bool)
            index = [slice(6, 12), slice(5, 11), slice(4, 9)]
            index[axis] = slice(0, 5) if side == 0 else slice(shape[axis] - 5, shape[axis])
            m[tuple(index)] = True
            blocks.append(m)
    corner = np.zeros(shape, bool)
    corner[:6, :5, :4] = True
    blocks.append(corner)
    blocks = np.stack(blocks)
    for r in (1.0, 2.0, 3.0):
        st = _check(blocks, "close", UNIT, r, want=blocks)  # a box is closed already, and the border of the volume takes nothing away
        np.testing.assert_array_equal(st[:, 2:], 0)
        np.testing.assert_array_equal(st[:, 0], st[:, 1])
        _check(blocks, "open", UNIT, r)
        _check(blocks, "erode", UNIT, r)  # ... while an erosion takes the faces inside the volume only
        _check(blocks, "dilate", UNIT, r)
    eroded = _check(corner[None], "erode", UNIT, 1.0)
    np.testing.assert_array_equal(eroded, [[120, 5 * 4 * 3, 0, 120 - 60]])
    full, empty = np.ones((1, 9, 17, 70), bool), np.zeros((1, 9, 17, 70), bool)
    for op in CALLS:
        for spacing, r in ((UNIT, 0.0), (UNIT, 2.0), ((0.5, 0.5, 1.5), 3.0)):
            np.testing.assert_array_equal(_check(full, op, spacing, r, want=full), [[full.size, full.size, 0, 0]])
            np.testing.assert_array_equal(_check(empty, op, spacing, r, want=empty), [[0, 0, 0, 0]])


@pytest.mark.parametrize("r", [1.0, 1.5, 2.0])
def test_closing_bridges_two_slabs_exactly_when_the_oracle_says_so(r):
    bridged = {}
    for gap in range(1, 7):
        m = np.zeros((1, 12, 30, 11), bool)
        m[0, 3:9, 4:12, 2:9] = True
        m[0, 3:9, 12 + gap:22 + gap, 2:9] = True  # two slabs `gap` background voxels apart along y
        _check(m, "close", UNIT, r)
        closed = BO.close(m[0], UNIT, r)
        bridged[gap] = bool(closed[5, 12:12 + gap, 5].all())
        assert bridged[gap] == (CO.stats(CO.label(closed, 6))[1] == 1)
    assert bridged == {gap: gap <= 2 * int(r) for gap in range(1, 7)}  # a gap of g voxels closes when the ball reaches g / 2 voxels from either side


def test_opening_removes_a_spur_and_keeps_the_block():
    m = np.zeros((1, 24, 22, 16), bool)
    m[0, 4:14, 5:15, 3:12] = True
    block = m.copy()
    m[0, 14:22, 9, 7] = True  # a spur one voxel thick along x
    for r in (1.0, 1.5, 2.0):
        st = _check(m, "open", UNIT, r)
        opened = BO.open_(m[0], UNIT, r)
        assert not opened[15:, :, :].any() and st[0, 3] >= 7  # the spur is gone (its first voxel may stay inside the dilated block) ...
        np.testing.assert_array_equal(opened[:14], BO.open_(block[0], UNIT, r)[:14])  # ... and the block keeps the shape the oracle gives it alone
    _check(m, "open", UNIT, 0.0, want=m)


def test_foreground_rules_layouts_and_downstream_consumers():
    shape = (14, 12, 10)
    lg = torch.zeros(1, 2, *shape, device="cuda")
    lg[0, 1, 3:9, 3:9, 2:8] = 1.0  # a 6 x 6 x 6 cube
    lg[0, 1, 5, 5, 4] = 0.0  # one voxel of it ties: background
    lg[0, 1, 6, 6, 5] = float("nan")  # NaN: background
    lg[0, 0, 4, 4, 4] = float("nan")
    lg[0, :, 10:13, 0:3, 2:4] = 0.5  # ties outside: background
    before = lg.clone()
    mask = np.zeros(shape, bool)
    mask[3:9, 3:9, 2:8] = True
    mask[5, 5, 4] = mask[6, 6, 5] = mask[4, 4, 4] = False
    cube = np.zeros(shape, bool)
    cube[3:9, 3:9, 2:8] = True
    closed, stats = binary_close(lg, 1.0, return_stats=True)
    assert torch.equal(lg.isnan(), before.isnan()) and torch.equal(lg.nan_to_num(7.0), before.nan_to_num(7.0))  # the input is bit-unchanged
    np.testing.assert_array_equal(BO.close(mask, UNIT, 1.0), cube)
    assert torch.equal(closed.cpu(), _one_hot_t([cube])) and torch.equal(stats.cpu(), torch.tensor([[213, 216, 3, 0]]))
    assert torch.equal(binary_close(lg, 1.0), closed)  # without stats, and spacing None = 1 mm
    assert torch.equal(binary_close(lg, 1.0, (1.0, 1.0, 1.0)), closed)
    cl = lg.permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)  # channels-last storage gives the same result as channels-first
    assert not cl.is_contiguous() and lg.is_contiguous()
    for fn, op in ((binary_dilate, "dilate"), (binary_erode, "erode"), (binary_close, "close"), (binary_open, "open")):
        a, b = fn(lg, 1.5, (1.0, 0.5, 1.5)), fn(cl, 1.5, (1.0, 0.5, 1.5))
        assert torch.equal(a, b) and a.permute(0, 2, 3, 4, 1).is_contiguous()
        assert torch.equal(a.cpu(), _one_hot_t([BO.OPS[op](mask, (1.0, 0.5, 1.5), 1.5)]))
    # the results are predictions like any other
    lab = torch.from_numpy(cube[None, None].astype(np.float32)).cuda()
    assert float(compute_dice_score(closed, lab)) == 1.0 > float(compute_dice_score(lg, lab))
    kept, kstats = keep_largest_component(binary_dilate(lg, 1.0), return_stats=True)
    dil = BO.dilate(mask, UNIT, 1.0)
    np.testing.assert_array_equal(kstats[0, :3].cpu().numpy(), [dil.sum(), 1, dil.sum()])
    assert torch.equal(kept.cpu(), _one_hot_t([dil]))
    meas = compute_measurements(closed, lab, (0.5, 0.5, 1.5))[0].cpu().numpy()
    assert meas[0] == 216 and meas[1] == 216 and meas[4] == 0.0
    assert torch.equal(binary_close(closed, 1.0), closed)  # the steps compose: a one-hot result is an input like any other
    assert torch.equal(binary_close(closed, 2.0).cpu(), _one_hot_t([BO.close(cube, UNIT, 2.0)]))
    assert torch.equal(binary_open(closed, 1.0).cpu(), _one_hot_t([BO.open_(cube, UNIT, 1.0)])) and not BO.open_(cube, UNIT, 1.0)[3, 3, 2]  # (the cross does not reach a corner)


def test_deterministic_batch_equals_single_calls_and_second_stream():
    masks = np.stack([_random((48, 40, 70), 0.15, 9), _random((48, 40, 70), 0.85, 10)])
    lg = _logits(masks)
    for name, fn in CALLS.items():
        call = lambda x: fn(x, 2.0, (0.5, 0.5, 1.5), return_stats=True)  # noqa: E731
        a, sa = call(lg)
        b, sb = call(lg)
        assert torch.equal(a, b) and torch.equal(sa, sb)
        singles = [call(lg[i:i + 1]) for i in range(2)]
        assert torch.equal(a, torch.cat([s[0] for s in singles])) and torch.equal(sa, torch.cat([s[1] for s in singles]))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            d, sd = call(lg)
        side.synchronize()
        assert torch.equal(a, d) and torch.equal(sa, sd)
        assert int(sa[:, 2:].sum()) > 0, name


def test_full_size_volume_with_a_far_island():
    """512 x 512 x 120 at (0.41, 0.41, 1.5), r = 2 mm: the work box spans the tumour and the island 260 voxels away.  Crops around the two objects (object box grown by
    twice the band) equal the oracle on those crops, and the voxel count of the result equals the sum over the crops: nothing else was set."""
    tumour, island, _ = far_island_case()
    spacing, r = (0.41, 0.41, 1.5), 2.0
    assert BO.tie_margin(spacing, r) >= 1e-4
    pred = tumour | island
    outputs = _full_size_outputs(pred)
    before = outputs.clone()
    grow = [2 * (k + 1) for k in BO.reach(spacing, r)]
    crops = []
    for obj in (tumour, island):
        crops.append(tuple(slice(max(int(i.min()) - g, 0), min(int(i.max()) + g + 1, n)) for i, g, n in zip(np.nonzero(obj), grow, pred.shape)))
        assert all(c.start > 0 and c.stop < n for c, n in zip(crops[-1], pred.shape))  # off the border: a crop sees what the volume sees
    for op, fn in CALLS.items():
        out, stats = fn(outputs, r, spacing, return_stats=True)
        want = [BO.OPS[op](pred[c], spacing, r) for c in crops]
        for c, w in zip(crops, want):
            assert torch.equal(out[0, 1][c].cpu(), torch.from_numpy(w.astype(np.float32))), op
            assert torch.equal(out[0, 0][c].cpu(), torch.from_numpy(1.0 - w.astype(np.float32))), op
        st = np.sum([BO.stats(pred[c], w) for c, w in zip(crops, want)], 0)
        np.testing.assert_array_equal(stats.cpu().numpy(), [st])
        assert int((out[0, 1] == 1.0).sum()) == st[1] and int((out[0, 0] == 1.0).sum()) == pred.size - st[1]  # (integer sums: 31 M ones are beyond fp32)
        assert int((out[0, 1] == 0.0).sum()) == pred.size - st[1] and int((out[0, 0] == 0.0).sum()) == st[1]
        assert out.permute(0, 2, 3, 4, 1).is_contiguous()  # a channels-last view, as keep_largest_component returns
    assert torch.equal(outputs, before)


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


@pytest.mark.parametrize("flag,op,r", [("--closing_mm", "close", 1.5), ("--opening_mm", "open", 1.0)])
def test_vsparams_one_flag_end_to_end(tmp_path, flag, op, r):
    """The stand-in network marks the tumour and 3 % scattered voxels.  Either flag alone switches the post-processing rows, the log lines and the CSV on."""
    p, model, loader, scores, log = _run_inference(tmp_path, [flag, str(r)], 0.97)
    column = "closed_voxels" if op == "close" else "opened_voxels"
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))
    assert len(rows) == 1 and list(rows[0]) == OLD_HEADER + [column]
    row = rows[0]
    data, o, mask = _raw_prediction(p, model, loader)
    final = BO.OPS[op](mask, SPACING, r)
    st = BO.stats(mask, final)
    assert (int(row["foreground_voxels"]), int(row["kept_voxels"]), int(row[column])) == (st[0], st[1], st[2] if op == "close" else st[3])
    assert st[2] + st[3] > 0 and (st[3] if op == "close" else st[2]) == 0  # the step had work to do; closing only adds, opening only removes
    assert int(row["components"]) == CO.stats(CO.label(final, 26))[1]  # no component filter: the components of the final prediction
    assert float(row["dice_raw"]) == float(compute_dice_score(o, data["label"]))
    assert float(row["dice"]) == _dice_of(final, data) == float(scores[0])
    for text in (flag[2:] + " =", f"{column}[0] = {row[column]}", "dice_score_raw[0] = ", f"components[0] = {row['components']}"):
        assert text in log, text
    assert (f"removed_voxels[0] = {st[3]}" in log) == (op == "open")
    for text in ("filled_voxels", "small_components_removed", "keep_largest_component =", "min_component_mm3 =", "fill_holes =", "opened_voxels" if op == "close" else "closed_voxels",
                 "opening_mm =" if op == "close" else "closing_mm ="):
        assert text not in log.replace(str(tmp_path), ""), text


def test_vsparams_all_five_steps_in_order(tmp_path):
    from vs_seg_amd.data.nifti import read_nifti
    import glob

    p, model, loader, scores, log = _run_inference(tmp_path / "all", ["--fill_holes", "--closing_mm", "1.5", "--opening_mm", "1", "--min_component_mm3", "1.2", "--keep_largest_component",
                                                                      "--component_connectivity", "6", "--measurements"], 0.9)
    rows = list(csv.DictReader(open(os.path.join(p.figures_path, "test_postprocessing.csv"))))
    assert len(rows) == 1 and list(rows[0]) == OLD_HEADER + ["holes", "filled_voxels", "small_components", "small_voxels", "closed_voxels", "opened_voxels"]
    row = rows[0]
    data, o, mask = _raw_prediction(p, model, loader)
    fst = MO.fill_stats(mask, 6)
    filled = MO.fill_holes(mask, 6)  # 1. fill holes
    closed = BO.close(filled, SPACING, 1.5)  # 2. closing
    opened = BO.open_(closed, SPACING, 1.0)  # 3. opening
    min_voxels = min_component_voxels(1.2, SPACING)
    sst = MO.small_stats(opened, min_voxels, 6)
    big = MO.remove_small(opened, min_voxels, 6)  # 4. remove small components, of the opened prediction
    final = CO.keep_largest(big, 6)  # 5. keep the largest of what is left
    n_closed, n_opened = int((closed & ~filled).sum()), int((closed & ~opened).sum())
    assert (int(row["foreground_voxels"]), int(row["holes"]), int(row["filled_voxels"])) == (fst[0], fst[1], fst[2])
    assert (int(row["closed_voxels"]), int(row["opened_voxels"])) == (n_closed, n_opened) and n_closed > 0 and n_opened > 0
    assert (int(row["components"]), int(row["small_components"]), int(row["small_voxels"])) == (sst[1], sst[1] - sst[3], sst[0] - sst[2])
    assert int(row["kept_voxels"]) == final.sum() > 0
    assert f"removed_voxels[0] = {fst[3] + n_closed - final.sum()}" in log and f"closed_voxels[0] = {n_closed}" in log and f"opened_voxels[0] = {n_opened}" in log
    assert float(row["dice"]) == _dice_of(final, data) == float(scores[0])
    meas = list(csv.DictReader(open(os.path.join(p.figures_path, "test_measurements.csv"))))[0]  # the other reports describe the final prediction too
    assert float(meas["voxels_pred"]) == final.sum()
    files = glob.glob(os.path.join(p.results_folder_path, "inferred_segmentations_nifti", "*", "*", "*.nii.gz"))
    assert int((np.asarray(read_nifti(files[0])[0]) == 1).sum()) == final.sum()

    p2, _, _, _, log2 = _run_inference(tmp_path / "old", ["--fill_holes", "--keep_largest_component"], 0.97)  # without the new flags: the header and the lines of before
    rows2 = list(csv.DictReader(open(os.path.join(p2.figures_path, "test_postprocessing.csv"))))
    assert list(rows2[0]) == OLD_HEADER + ["holes", "filled_voxels"]
    for text in ("closed_voxels", "opened_voxels", "closing_mm", "opening_mm"):
        assert text not in log2.replace(str(tmp_path), ""), text
    assert f"removed_voxels[0] = {int(rows2[0]['foreground_voxels']) + int(rows2[0]['filled_voxels']) - int(rows2[0]['kept_voxels'])}" in log2
