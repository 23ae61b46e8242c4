"""CPU tests of the inference reports (vs_seg_amd/report.py) and of VSparams.log_parameters: the log lines and CSV texts recorded from commit e2f522d
(tests/golden/inference_reports.json, written by tests/golden/make_inference_reports.py) come out line for line and byte for byte when the recorded named rows go
through the per-case table and the report declarations, and the table keeps its values exactly, by name, with one host copy."""
import argparse
import json
import os

import numpy as np
import pytest
import torch

from vs_seg_amd import report as R

NAN, INF = float("nan"), float("inf")
BASE = ["--data_root", "/data", "--results_folder_name", "t"]


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "inference_reports.json")) as f:
        return json.load(f)


@pytest.fixture
def make_params(monkeypatch):
    """VSparams past the device check, as tests/test_optim_host.py builds it; its logger collects the lines."""
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))

    def make(argv):
        p = P.VSparams(argparse.ArgumentParser(), BASE + list(argv))
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        return p, lines

    return make


def test_the_fixture_holds_every_case_the_reports_have(recorded):
    reports, argvs = recorded["reports"], [tuple(e["argv"]) for e in recorded["reports"]]
    post = [e for e in reports if not {"--surface_metrics", "--surface_dice_mm", "--measurements"} & set(e["argv"])]
    assert len({a for a in argvs if a and not {"--surface_metrics", "--surface_dice_mm", "--measurements"} & set(a)}) == 31  # every non-empty subset of the five flags
    assert all(e["rows"]["foreground_voxels"][0] == 512 * 512 * 120 and e["rows"]["kept_voxels"][0] == 2**24 + 1 for e in post if e["argv"])
    assert len(set(argvs)) == len(argvs) - 1 and len(recorded["parameters"]) == 25  # (the all-non-finite entry repeats an argv)
    assert any("mean_hd95_mm = nan +- nan (3 of 3 cases non-finite)" in e["log"] for e in reports)
    assert any("test_measurements.csv" in e["csv"] and "test_postprocessing.csv" in e["csv"] and "test_surface_dice.csv" in e["csv"] and "test_surface_metrics.csv" in e["csv"] for e in reports)


def test_reports_log_and_write_what_the_parent_did(recorded, make_params, tmp_path):
    for k, entry in enumerate(recorded["reports"]):
        p, lines = make_params(entry["argv"])
        reports = p._reports()
        rows = {name: np.array(v, dtype=np.float64) for name, v in entry["rows"].items()}
        n = len(rows["dice"])
        table = R.CaseTable(("dice",) + tuple(name for rep in reports for name in rep.rows), n, "cpu")
        assert sorted(table.names) == sorted(rows), entry["argv"]  # the rows the declarations name are the recorded ones
        for gi in range(n):  # one write per case and report, as run_inference makes them
            table.set(gi, ("dice",), torch.tensor([rows["dice"][gi]], dtype=torch.float64))
            for rep in reports:
                table.set(gi, rep.rows, torch.tensor([rows[name][gi] for name in rep.rows], dtype=torch.float64))
        figures = str(tmp_path / str(k) / "figures")
        with np.errstate(all="raise"):  # an empty label gives a NaN relative error without a warning
            R.emit(reports, table.gather(), p.logger.info, figures)
        assert lines == entry["log"], entry["argv"]
        written = {f: open(os.path.join(figures, f), newline="").read() for f in sorted(os.listdir(figures))} if os.path.isdir(figures) else {}
        assert written == entry["csv"], entry["argv"]
        quiet = []
        R.emit(reports, table.gather(), quiet.append, None)  # a rank other than 0 logs the same and writes nothing
        assert quiet == entry["log"] and (not os.path.isdir(figures) or sorted(os.listdir(figures)) == sorted(entry["csv"]))


def test_log_parameters_logs_what_the_parent_did(recorded, make_params):
    for entry in recorded["parameters"]:
        p, lines = make_params(entry["argv"])
        p.log_parameters()
        assert lines == entry["log"], entry["argv"]


def test_csv_headers_come_from_the_declarations():
    from vs_seg_amd.params import postprocessing_csv_header, surface_dice_csv_header

    assert postprocessing_csv_header(True, True, True, True) == R.csv_header(R.postprocessing(True, True, True, True, True))
    assert postprocessing_csv_header(False, False) == "case,dice_raw,dice,components,foreground_voxels,kept_voxels"
    assert surface_dice_csv_header((0.5,)) == "case,dice,masd_mm,nsd_0.5mm,surface_precision_0.5mm,surface_recall_0.5mm"


DICE = 0.1 + 0.7  # 0.7999999999999999: no fp32 value
NAMES = ("dice",) + R.surface_metrics().rows + R.postprocessing(keep_largest=True).rows


def _filled_table(names):
    table = R.CaseTable(names, 4, "cpu")
    table.set(0, ("dice",), torch.tensor([DICE], dtype=torch.float64))
    table.set(0, R.SURFACE_ROWS, torch.tensor([INF, NAN]))  # fp32, as compute_surface_distances returns them
    table.set(0, ("foreground_voxels", "components", "kept_voxels"), torch.tensor([512 * 512 * 120, 3, 2**24 + 1]))  # int64, as the component statistics are
    table.set(2, ("dice",), torch.tensor([np.float32(0.3)]))
    table.set(2, R.SURFACE_ROWS, torch.tensor([-INF, 1.5]))
    return table


def test_table_keeps_values_exactly_and_by_name():
    v = _filled_table(NAMES).gather()
    assert set(v) == set(NAMES) and all(a.dtype == np.float64 and a.shape == (4,) for a in v.values())
    assert float(np.float32(DICE)) != DICE and v["dice"][0] == DICE and v["dice"][2] == float(np.float32(0.3))
    assert v["kept_voxels"][0] == 2**24 + 1 and v["foreground_voxels"][0] == 31457280 and v["components"][0] == 3
    assert v["hd95_mm"][0] == INF and np.isnan(v["assd_mm"][0]) and v["hd95_mm"][2] == -INF and v["assd_mm"][2] == 1.5
    for name, a in v.items():  # a case that was never written is 0
        assert a[1] == 0 and a[3] == 0, name
    assert (v["dice_raw"] == 0).all()
    # the reports registered the other way round: the same values under the same names
    w = _filled_table(("dice",) + R.postprocessing(keep_largest=True).rows + R.surface_metrics().rows).gather()
    assert set(w) == set(v)
    for name in v:
        np.testing.assert_array_equal(w[name], v[name])


def test_table_gather_is_one_host_copy_and_at_most_one_allreduce():
    class Counting(torch.Tensor):
        copies = 0

        def cpu(self, *a, **k):
            Counting.copies += 1
            return super().cpu(*a, **k)

    table = _filled_table(NAMES)
    table.values = table.values.as_subclass(Counting)
    reduced = []
    v = table.gather(lambda t: reduced.append(t.shape) or t)
    assert Counting.copies == 1 and reduced == [(len(NAMES), 4)]
    bases = {id(a.base) for a in v.values()}
    assert len(bases) == 1 and all(a.base is not None for a in v.values())  # views of one array
    assert v["dice"][0] == DICE
    Counting.copies = 0
    table.gather()
    assert Counting.copies == 1


def test_table_rejects_rows_it_does_not_hold_together():
    table = R.CaseTable(NAMES, 2, "cpu")
    with pytest.raises(AssertionError):
        table.set(0, ("hd95_mm", "dice_raw"), torch.zeros(2))  # not adjacent: a slice assignment would write another row
    with pytest.raises(ValueError):
        table.set(0, ("no_such_row",), torch.zeros(1))
    with pytest.raises(RuntimeError):
        table.set(0, R.SURFACE_ROWS, torch.zeros(3))


def test_finite_mean_leaves_out_and_counts():
    assert R.finite_mean("m", np.array([1.0, 3.0, INF, NAN])) == "m = 2.0 +- 1.0 (2 of 4 cases non-finite)"
    assert R.finite_mean("m", np.array([NAN, INF]), "with an empty mask left out") == "m = nan +- nan (2 of 2 cases with an empty mask left out)"
