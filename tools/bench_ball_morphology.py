"""Time vs_seg_amd.binary_dilate / binary_erode / binary_close / binary_open at the test-volume size (512 x 512 x 120, spacing 0.41 x 0.41 x 1.5 mm) with HIP events
after warm-up, in one process: (a) one tumour, (b) the tumour plus one small false-positive island far from it (the work box then spans both), at r = 1, 2 and
5 mm; (c) an empty and (d) an all-foreground prediction at r = 2 mm.  Every group alternates with fill_holes on the same volume, the yardstick: the same 16 B
per voxel of whole-volume traffic (one pass that reads the logits, one that writes the one-hot result).  Prints ms per call, the statistics of each call, the
ratio to fill_holes and, for closing the clean tumour at r = 2 mm, the share of the budget (1 % of the 24 ms sliding-window pass = 240 us).

    python tools/bench_ball_morphology.py [--reps 20] [--radii 1,2,5] [--cases tumour,all_foreground] [--budget_us 240]

Per kernel: rocprofv3 --kernel-trace --stats -- python tools/bench_ball_morphology.py --cases tumour --radii 2 (a run of its own; the kernels are named ball_*).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import binary_close, binary_dilate, binary_erode, binary_open, fill_holes  # noqa: E402

SHAPE = (512, 512, 120)
SPACING = (0.41, 0.41, 1.5)
OPS = {"dilate": binary_dilate, "erode": binary_erode, "close": binary_close, "open": binary_open}


def timed(fn, reps):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def ellipsoid(c, r):
    g = [torch.arange(s, device="cuda", dtype=torch.float32) for s in SHAPE]
    return ((g[0][:, None, None] - c[0]) / r[0]) ** 2 + ((g[1][None, :, None] - c[1]) / r[1]) ** 2 + ((g[2][None, None, :] - c[2]) / r[2]) ** 2 <= 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--radii", type=str, default="1,2,5", help="comma-separated radii in mm for the tumour cases")
    ap.add_argument("--cases", type=str, default="", help="comma-separated subset of the cases (for a kernel trace of one of them); default: all")
    ap.add_argument("--budget_us", type=float, default=240.0, help="the budget that closing the clean tumour at r = 2 mm is held against")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ball_morphology: no GPU visible; nothing is measured without one")
    radii = [float(r) for r in a.radii.split(",")]
    tumour = ellipsoid((302, 219, 61), (13, 12, 5))  # the clean tumour and the far island of tests/volume_cases.far_island_case
    cases = {"tumour": (tumour, radii), "tumour_and_far_island": (tumour | ellipsoid((40, 470, 12), (3, 2, 1.5)), radii),
             "empty": (torch.zeros(SHAPE, dtype=torch.bool, device="cuda"), [2.0]), "all_foreground": (torch.ones(SHAPE, dtype=torch.bool, device="cuda"), [2.0])}
    if a.cases:
        cases = {k: cases[k] for k in a.cases.split(",")}
    res = {"shape": SHAPE, "spacing": SPACING, "reps": a.reps, "budget_us": a.budget_us}
    for name, (pred, rs) in cases.items():
        cl = torch.stack([torch.zeros(SHAPE, device="cuda"), torch.where(pred, 1.0, -1.0)], -1)[None]  # channels-last logits, as the sliding window returns them
        outputs = cl.permute(0, 4, 1, 2, 3)
        for r in rs:
            row = {"fill_holes_ms": round(timed(lambda: fill_holes(outputs), a.reps), 4)}
            for op, fn in OPS.items():  # fill_holes before and after the four: the drift of the yardstick shows beside them
                row[op + "_ms"] = round(timed(lambda: fn(outputs, r, SPACING), a.reps), 4)
                row[op + "_stats"] = [int(v) for v in fn(outputs, r, SPACING, return_stats=True)[1][0].cpu()]
            row["fill_holes_again_ms"] = round(timed(lambda: fill_holes(outputs), a.reps), 4)
            yard = 0.5 * (row["fill_holes_ms"] + row["fill_holes_again_ms"])
            for op in OPS:
                row[op + "_over_fill_holes"] = round(row[op + "_ms"] / yard, 2)
            row["close_share_of_budget"] = round(row["close_ms"] * 1e3 / a.budget_us, 2)
            res[f"{name}@{r:g}mm"] = row
            print(f"{name:22s} r = {r:3g} mm   fill_holes {row['fill_holes_ms']:.4f} / {row['fill_holes_again_ms']:.4f} ms   " +
                  "   ".join(f"{op} {row[op + '_ms']:.4f} ms ({row[op + '_over_fill_holes']:.2f} x)" for op in OPS) +
                  f"   close = {row['close_share_of_budget']:.2f} x the {a.budget_us:g} us budget", flush=True)
        del cl, outputs
    print(json.dumps(res))


if __name__ == "__main__":
    main()
