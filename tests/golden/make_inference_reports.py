"""Recorder of tests/golden/inference_reports.json: what commit e2f522d logs and writes for given per-case values, and what its log_parameters logs.

It runs against THAT commit's method names (VSparams._log_postprocessing / _log_surface_metrics / _log_surface_dice / _log_measurements, which take their rows by
position, and the three Dice lines that its run_inference logs inline, copied into `dice_lines` below); it does not run against a later tree.  Check that commit
out and run `python tests/golden/make_inference_reports.py` from the repository root: no GPU is needed, the four writers and log_parameters are numpy and Python.

Every entry of "reports" holds the argv, the named rows (one value per case), the expected log lines and the expected text of every CSV written; every entry of
"parameters" the argv and the lines of log_parameters.  tests/test_report_host.py feeds the rows through vs_seg_amd/report.py and asserts equality."""
import argparse
import itertools
import json
import os
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vs_seg_amd import params as P  # noqa: E402
from vs_seg_amd.metrics import MEASUREMENT_FIELDS, surface_metric_fields  # noqa: E402

NAN, INF = float("nan"), float("inf")
BASE = ["--data_root", "/data", "--results_folder_name", "t"]
POST_FLAGS = (["--fill_holes"], ["--closing_mm", "1.5"], ["--opening_mm", "1"], ["--min_component_mm3", "1.2"], ["--keep_largest_component"])


def make_params(argv):
    torch.cuda.is_available = lambda: True
    P.DP.init_distributed = lambda: (0, 1, 0)
    p = P.VSparams(argparse.ArgumentParser(), BASE + list(argv))
    lines = []
    p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
    return p, lines


def dice_lines(log, dice_scores):
    for i, v in enumerate(dice_scores):
        log(f"dice_score[{i}] = {v}")
    log(f"all_dice_scores = {dice_scores}")
    log(f"mean_dice_score = {dice_scores.mean()} +- {dice_scores.std()}")


def sdice_names(p):
    return ("masd_mm",) + surface_metric_fields(p.surface_dice_mm)[3:]


def post_rows(p, rng, n):
    """Seeded integer-valued counts; case 0 holds a full 512 x 512 x 120 volume of foreground and 2^24 + 1 kept voxels (an fp32 slip or a float-formatted count shows)."""
    names = ["foreground_voxels", "components", "kept_voxels"] + (["holes", "filled_voxels"] if p.fill_holes else []) + (["small_components", "small_voxels"] if p.min_component_mm3 > 0 else []) + (
        ["closed_voxels"] if p.closing_mm > 0 else []) + (["opened_voxels"] if p.opening_mm > 0 else [])
    rows = {"dice_raw": rng.random(n)}
    rows.update({k: rng.integers(0, 50 if k in ("components", "holes", "small_components") else 200000, n).astype(np.float64) for k in names})
    rows["foreground_voxels"][0], rows["kept_voxels"][0] = 31457280.0, 16777217.0
    return rows


def surface_rows(n, finite):
    """Case 1 is inf (one mask empty) and case 2 NaN (both empty); without `finite` case 0 is inf as well."""
    return {"hd95_mm": np.array([2.8284270763397217 if finite else INF, INF, NAN][:n]), "assd_mm": np.array([0.7320508360862732 if finite else INF, INF, NAN][:n])}


def sdice_rows(p, rng, n, finite):
    rows = {}
    for k in sdice_names(p):
        v = rng.random(n)
        v[1], v[2] = (INF, NAN) if k == "masd_mm" else (0.0, NAN)
        if not finite:
            v[0] = INF if k == "masd_mm" else NAN
        rows[k] = v
    return rows


def measurement_rows(rng, n):
    """Case 1 has an empty label (0 voxels, 0 mm^3: the relative error is NaN) and NaN label diameters and centroid distance; case 2 an empty prediction."""
    rows = {k: rng.random(n) * 40.0 for k in MEASUREMENT_FIELDS}
    rows["voxels_pred"], rows["voxels_label"] = np.array([5120.0, 17.0, 0.0]), np.array([4800.0, 0.0, 4100.0])
    rows["volume_pred_mm3"], rows["volume_label_mm3"] = rows["voxels_pred"] * 0.3515625, rows["voxels_label"] * 0.3515625
    for k in ("centroid_distance_mm", "max_diameter_label_mm", "max_axial_diameter_label_mm"):
        rows[k][1] = NAN
    for k in ("centroid_distance_mm", "max_diameter_pred_mm", "max_axial_diameter_pred_mm"):
        rows[k][2] = NAN
    return rows


def record_report(argv, seed, n=3, finite=True):
    p, lines = make_params(argv)
    rng = np.random.default_rng(seed)
    rows = {"dice": rng.random(n)}
    post = p.fill_holes or p.closing_mm > 0 or p.opening_mm > 0 or p.min_component_mm3 > 0 or p.keep_largest_component
    if post:
        rows.update(post_rows(p, rng, n))
    if p.surface_metrics:
        rows.update(surface_rows(n, finite))
    if p.surface_dice_mm:
        rows.update(sdice_rows(p, rng, n, finite))
    if p.measurements:
        rows.update(measurement_rows(rng, n))
    with tempfile.TemporaryDirectory() as tmp:
        p.figures_path = os.path.join(tmp, "figures")
        dice_lines(p.logger.info, rows["dice"])  # the order of the sections is that of e2f522d's run_inference
        if post:
            extra = [rows[k] for k in ("holes", "filled_voxels", "small_components", "small_voxels", "closed_voxels", "opened_voxels") if k in rows]
            p._log_postprocessing(rows["dice"], rows["dice_raw"], rows["foreground_voxels"], rows["components"], rows["kept_voxels"], *extra)
        if p.surface_metrics:
            p._log_surface_metrics(rows["dice"], rows["hd95_mm"], rows["assd_mm"])
        if p.surface_dice_mm:
            p._log_surface_dice(rows["dice"], np.stack([rows[k] for k in sdice_names(p)]))
        if p.measurements:
            p._log_measurements(rows["dice"], np.stack([rows[k] for k in MEASUREMENT_FIELDS]))
        written = {f: open(os.path.join(p.figures_path, f)).read() for f in sorted(os.listdir(p.figures_path))} if os.path.isdir(p.figures_path) else {}
    return dict(argv=list(argv), rows={k: [float(x) for x in v] for k, v in rows.items()}, log=lines, csv=written)


def record_parameters(argv):
    p, lines = make_params(argv)
    p.log_parameters()
    return dict(argv=list(argv), log=lines)


def main():
    reports = []
    for r in range(1, 6):  # the 31 non-empty subsets of the five post-processing flags
        for subset in itertools.combinations(POST_FLAGS, r):
            reports.append(record_report(sum(subset, []), seed=100 + len(reports)))
    for surf, sdice, meas in itertools.product(([], ["--surface_metrics"]), ([], ["--surface_dice_mm", "2", "1"], ["--surface_dice_mm", "0.5"]), ([], ["--measurements"])):
        reports.append(record_report(surf + sdice + meas, seed=200 + len(reports)))
    reports.append(record_report(["--surface_metrics", "--surface_dice_mm", "2", "1"], seed=300, finite=False))  # every case non-finite: nan +- nan
    everything = sum(POST_FLAGS, []) + ["--surface_metrics", "--surface_dice_mm", "2", "1", "--measurements"]
    reports.append(record_report(everything, seed=301))  # pins the order of the sections

    loss_on = ["--ce_weight", "1", "--ce_foreground_weight", "2", "--tversky_beta", "0.7", "--focal_tversky_gamma", "0.75", "--batch_dice"]
    rest_on = ["--tta_flips", "0", "2", "--tta_average", "probabilities", "--aug_rotate_deg", "10", "--aug_scale", "0.1", "--aug_elastic_mag", "4", "--aug_bias_field", "0.3", "--aug_blur_sigma", "1",
               "--aug_lowres", "0.5", "--aug_thick_slices", "3", "--aug_ghost", "0.5", "--optimizer", "sgd", "--nesterov", "--clip_grad_norm", "12", "--lr_schedule", "poly"]
    groups = [[], ["--surface_metrics"], ["--surface_dice_mm", "2", "1"], ["--measurements"]] + [list(f) for f in POST_FLAGS] + [
        ["--tta_flips", "0"], ["--aug_rotate_deg", "10"], ["--aug_elastic_mag", "4"], ["--aug_bias_field", "0.3"], ["--aug_blur_sigma", "1"], ["--aug_thick_slices", "3"],
        ["--ce_weight", "1"], ["--ce_weight", "1", "--ce_topk", "10"], ["--tversky_beta", "0.7"], ["--ce_weight", "1", "--ce_focal_gamma", "2"],
        ["--optimizer", "sgd"], ["--optimizer", "adamw"], ["--clip_grad_norm", "12"], ["--lr_schedule", "poly"],
        everything + loss_on + ["--ce_topk", "10"] + rest_on, everything + loss_on + ["--ce_focal_gamma", "2"] + rest_on]  # (--ce_topk and --ce_focal_gamma exclude each other)
    out = dict(commit="e2f522d", reports=reports, parameters=[record_parameters(a) for a in groups])
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "inference_reports.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes,", len(reports), "report entries,", len(out["parameters"]), "parameter entries")


if __name__ == "__main__":
    main()
