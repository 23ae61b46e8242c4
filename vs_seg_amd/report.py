"""Inference reports: everything between "a per-case value exists on the device" and "it is in the log and in a CSV" (`VSparams.run_inference`).  `CaseTable` holds one
named fp64 row of per-case values per quantity and `gather` brings it to the host as {name: array}; each report (`postprocessing`, `surface_metrics`, `surface_dice`,
`measurements`) declares, from the flags that are on, its rows, its per-case log lines, its summary lines and its CSV; `emit` walks the declarations.  Nothing here is
read by position.  Host-side only; imports no part of the project."""
from __future__ import annotations

import os
from typing import Callable, Dict, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch


class CaseTable:
    """[len(names), n] fp64 on `device`, zero-initialised: row `name`, column = case.  fp64 holds every value exactly (voxel counts of a full volume are not exact in
    fp32; the fp32 Dice and surface values widen exactly)."""

    def __init__(self, names: Sequence[str], n: int, device):
        self.names = tuple(names)
        self.values = torch.zeros((len(self.names), n), dtype=torch.float64, device=device)

    def set(self, gi: int, names: Sequence[str], values: torch.Tensor):
        """Write `values` (one per name, on the table's device) for case `gi`: one slice assignment, `names` being adjacent rows of the table."""
        r = self.names.index(names[0])
        assert self.names[r:r + len(names)] == tuple(names), f"{tuple(names)} are not adjacent rows of {self.names}"
        self.values[r:r + len(names), gi] = values

    def gather(self, allreduce: Optional[Callable] = None) -> Dict[str, np.ndarray]:
        """{name: float64 array of length n}, views of the one host copy.  `allreduce` (given when the world is larger than 1) sums over the ranks: every case is
        non-zero on one rank only, so the sum adds zeros (NaN / inf + 0 stay NaN / inf)."""
        host = (allreduce(self.values) if allreduce is not None else self.values).cpu().numpy()
        return dict(zip(self.names, host))


class Report(NamedTuple):
    rows: Tuple[str, ...]  # its rows of the table
    lines: Tuple[Tuple[str, str], ...]  # per case, in log order: (label, column)
    summary: Callable  # columns -> summary lines
    csv_name: str
    columns: Tuple[str, ...]  # of the CSV, after "case"
    derive: Callable = lambda v: {}  # columns computed from the rows


COUNTS = frozenset(("components", "foreground_voxels", "kept_voxels", "holes", "filled_voxels", "small_components", "small_voxels", "closed_voxels", "opened_voxels",
                    "removed_voxels"))  # logged and written as integers


def finite_mean(name: str, v: np.ndarray, left_out: str = "non-finite") -> str:
    """"name = mean +- std (k of n cases <left_out>)" over the finite values of `v`."""
    fin = v[np.isfinite(v)]
    m, sd = (fin.mean(), fin.std()) if len(fin) else (float("nan"), float("nan"))
    return f"{name} = {m} +- {sd} ({len(v) - len(fin)} of {len(v)} cases {left_out})"


def _on(flag, *names):
    return names if flag else ()


def postprocessing(fill_holes=False, closing=False, opening=False, min_component=False, keep_largest=False) -> Report:
    """--fill_holes / --closing_mm / --opening_mm / --min_component_mm3 / --keep_largest_component: the raw Dice and the voxel and component counts of the chain."""
    extra = _on(fill_holes, "holes", "filled_voxels") + _on(min_component, "small_components", "small_voxels") + _on(closing, "closed_voxels") + _on(opening, "opened_voxels")
    lines = (("dice_score_raw", "dice_raw"),) + _on(fill_holes, ("holes", "holes"), ("filled_voxels", "filled_voxels")) + _on(closing, ("closed_voxels", "closed_voxels")) + _on(
        opening, ("opened_voxels", "opened_voxels")) + (("components", "components"),) + _on(min_component, ("small_components_removed", "small_components"), ("small_voxels_removed", "small_voxels")) + _on(
            keep_largest or min_component or opening, ("removed_voxels", "removed_voxels"))  # everything taken away after the additions: by the opening and the component filters

    def derive(v):
        return {"removed_voxels": v["foreground_voxels"] + sum(v[k] for k in ("filled_voxels", "closed_voxels") if k in v) - v["kept_voxels"]}

    return Report(("dice_raw", "foreground_voxels", "components", "kept_voxels") + extra, lines, lambda v: [f"mean_dice_score_raw = {v['dice_raw'].mean()} +- {v['dice_raw'].std()}"],
                  "test_postprocessing.csv", ("dice_raw", "dice", "components", "foreground_voxels", "kept_voxels") + extra, derive)


def _distances(rows, csv_name) -> Report:
    return Report(tuple(rows), tuple((k, k) for k in rows), lambda v: [finite_mean(f"mean_{k}", v[k]) for k in rows], csv_name, ("dice",) + tuple(rows))


SURFACE_ROWS = ("hd95_mm", "assd_mm")


def surface_metrics() -> Report:
    """--surface_metrics: HD95 and ASSD per case, mm."""
    return _distances(SURFACE_ROWS, "test_surface_metrics.csv")


def surface_dice(fields: Sequence[str]) -> Report:
    """--surface_dice_mm: `fields` = masd_mm, then nsd, surface precision and surface recall per tolerance."""
    return _distances(fields, "test_surface_dice.csv")


def measurements(fields: Sequence[str]) -> Report:
    """--measurements: `fields` = the nine outputs of compute_measurements; the volume and diameter errors are formed here."""
    def derive(v):
        err = v["volume_pred_mm3"] - v["volume_label_mm3"]
        with np.errstate(divide="ignore", invalid="ignore"):
            rel = np.where(v["voxels_label"] > 0, np.abs(err) / v["volume_label_mm3"], np.nan)  # NaN: the label is empty
        return {"volume_error_mm3": err, "volume_rel_error": rel}

    def summary(v):
        return [finite_mean("mean_abs_volume_error_mm3", np.abs(v["volume_error_mm3"]), "non-finite left out"), finite_mean("mean_rel_volume_error", v["volume_rel_error"], "with an empty label left out")] + [
            finite_mean(f"mean_abs_{d}_error_mm", np.abs(v[f"{d}_pred_mm"] - v[f"{d}_label_mm"]), "with an empty mask left out") for d in ("max_diameter", "max_axial_diameter")]

    logged = ("volume_pred_mm3", "volume_label_mm3", "volume_error_mm3") + tuple(k for k in fields if not k.startswith(("voxels_", "volume_")))
    return Report(tuple(fields), tuple((k, k) for k in logged), summary, "test_measurements.csv", ("dice",) + tuple(fields) + ("volume_error_mm3", "volume_rel_error"), derive)


def postprocessing_csv_header(fill_holes: bool, min_component: bool, closing: bool = False, opening: bool = False) -> str:
    """Columns of figures/test_postprocessing.csv: the six of --keep_largest_component, then those of --fill_holes, --min_component_mm3, --closing_mm and --opening_mm as
    switched on."""
    return csv_header(postprocessing(fill_holes, closing, opening, min_component))


def csv_header(report: Report) -> str:
    return "case," + ",".join(report.columns)


def emit(reports: Sequence[Report], v: Dict[str, np.ndarray], log: Callable, figures_path: Optional[str] = None):
    """Log the Dice section, then the section of every report in turn, and write each report's CSV under `figures_path` (None on every rank but 0)."""
    dice = v["dice"]
    for i, d in enumerate(dice):
        log(f"dice_score[{i}] = {d}")
    log(f"all_dice_scores = {dice}")
    log(f"mean_dice_score = {dice.mean()} +- {dice.std()}")
    if figures_path is not None and reports:
        os.makedirs(figures_path, exist_ok=True)
    for rep in reports:
        v = {**v, **rep.derive(v)}
        for i in range(len(dice)):
            for label, col in rep.lines:
                log(f"{label}[{i}] = {int(v[col][i]) if col in COUNTS else v[col][i]}")
        for line in rep.summary(v):
            log(line)
        if figures_path is not None:
            with open(os.path.join(figures_path, rep.csv_name), "w") as f:
                f.write(csv_header(rep) + "\n")
                for i in range(len(dice)):
                    f.write(",".join([str(i)] + [str(int(v[c][i])) if c in COUNTS else repr(float(v[c][i])) for c in rep.columns]) + "\n")
