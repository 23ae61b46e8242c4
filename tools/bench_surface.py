"""Time vs_seg_amd.compute_surface_distances at the test-volume size (512 x 512 x 120, spacing 0.41 x 0.41 x 1.5 mm) with HIP events after warm-up:
a clean tumour prediction, and the same prediction plus one small false-positive island far from the tumour (the edges' bounding box then spans
most of the volume).  Prints ms per call, and the rate of the edge pass (12 B read + 1 B written per voxel) as timed by a call on empty masks.

With --tolerances it also times vs_seg_amd.compute_surface_metrics (the same call plus the normalised surface Dice at these tolerances in mm) against the
plain call: both in this process, in alternating rounds, for the clean, the far-island and the empty case; per case the median over the rounds of each,
their difference, and (plain - empty) / 7 as an upper bound of one histogram launch of the plain call.

    python tools/bench_surface.py [--reps 20] [--tolerances 0.5 1 2 3 [--rounds 5]]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import compute_surface_distances, compute_surface_metrics  # noqa: E402

SHAPE, SPACING = (512, 512, 120), (0.41, 0.41, 1.5)


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


def alternating(plain, combined, reps, rounds):
    """Median ms per call of each of two functions, timed in alternating rounds of `reps` calls."""
    t = [[], []]
    for _ in range(rounds):
        for i, fn in enumerate((plain, combined)):
            t[i].append(timed(fn, reps))
    return [sorted(v)[len(v) // 2] for v in t]


def ellipsoid(c, r):
    g = [torch.arange(s, device="cuda", dtype=torch.float32) for s in SHAPE]
    return ((g[0][:, None, None] - c[0]) / r[0]) ** 2 + ((g[1][None, :, None] - c[1]) / r[1]) ** 2 + ((g[2][None, None, :] - c[2]) / r[2]) ** 2 <= 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tolerances", type=float, nargs="+", default=None, metavar="TAU", help="also time compute_surface_metrics at these tolerances (mm) against the plain call")
    ap.add_argument("--rounds", type=int, default=5, help="alternating rounds of --reps calls each for --tolerances")
    a = ap.parse_args()
    gt = ellipsoid((256, 256, 60), (30, 24, 8))
    clean = ellipsoid((258, 255, 61), (29, 25, 8))
    cases = {"clean": clean, "far_island": clean | ellipsoid((30, 480, 10), (3, 3, 2))}
    lab = gt.float()[None, None].contiguous()
    nvox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    res = {"shape": SHAPE, "spacing": SPACING}
    for name, pred in cases.items():
        cl = torch.stack([torch.zeros(SHAPE, device="cuda"), torch.where(pred, 1.0, -1.0)], -1)[None]  # channels-last logits, as the sliding window returns them
        outputs = cl.permute(0, 4, 1, 2, 3)
        ms = timed(lambda: compute_surface_distances(outputs, lab, SPACING, 95.0), a.reps)
        res[name] = {"ms_per_call": round(ms, 4), "hd95_assd_mm": [round(float(v), 4) for v in compute_surface_distances(outputs, lab, SPACING, 95.0)[0]]}
    # the edge pass: a call whose masks have no edge voxel runs the edge pass over the whole volume, and the later launches exit at once (empty box):
    # its time bounds the edge pass's from above, so the rate below bounds the edge pass's from below (rocprofv3 --kernel-trace gives surf_edge_kernel alone)
    empty, no_label = torch.zeros((1, *SHAPE, 2), device="cuda").permute(0, 4, 1, 2, 3), torch.zeros_like(lab)
    ms_empty = timed(lambda: compute_surface_distances(empty, no_label, SPACING, 95.0), a.reps)
    res["empty_masks"] = {"ms_per_call": round(ms_empty, 4), "edge_pass_gbps_at_least": round(13 * nvox / (ms_empty * 1e-3) / 1e9, 1)}
    if a.tolerances:
        inputs = {name: torch.stack([torch.zeros(SHAPE, device="cuda"), torch.where(pred, 1.0, -1.0)], -1)[None].permute(0, 4, 1, 2, 3) for name, pred in cases.items()}
        labels = {"clean": lab, "far_island": lab, "empty_masks": no_label}
        inputs["empty_masks"] = empty
        comb = {"tolerances_mm": a.tolerances, "rounds": a.rounds}
        for name, outputs in inputs.items():
            plain, both = alternating(lambda: compute_surface_distances(outputs, labels[name], SPACING, 95.0),
                                      lambda: compute_surface_metrics(outputs, labels[name], SPACING, 95.0, a.tolerances), a.reps, a.rounds)
            comb[name] = {"plain_ms": round(plain, 4), "combined_ms": round(both, 4), "increment_ms": round(both - plain, 4)}
            if name != "empty_masks":
                comb[name]["metrics"] = [round(float(v), 5) for v in compute_surface_metrics(outputs, labels[name], SPACING, 95.0, a.tolerances)[0]]
        for name in ("clean", "far_island"):  # 7 of the 14 launches are not the edge pass or a single-workgroup launch: three transforms and four histograms
            comb[name]["hist_launch_ms_at_most"] = round((comb[name]["plain_ms"] - comb["empty_masks"]["plain_ms"]) / 7, 4)
        res["combined"] = comb
    print(json.dumps(res))


if __name__ == "__main__":
    main()
