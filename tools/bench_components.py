"""Time vs_seg_amd.keep_largest_component, remove_small_components and fill_holes at the test-volume size (512 x 512 x 120) with HIP events after warm-up,
in one process: (a) one tumour, (b) the tumour plus one small false-positive island far from it, (c) the tumour with an inner cavity, (d) noise at density
0.5, (e) all foreground.  Beside keep_largest_component, the host route it replaces on the same box: device-to-host copy of the argmax,
scipy.ndimage.label and numpy.bincount on one core (skipped when scipy is absent).  Prints ms per call, the statistics of each case, the multiple of
the traffic floor of the two whole-volume passes of keep_largest_component (8 B read + 4 B + 8 B written per voxel), and the two new calls as multiples
of keep_largest_component on the same volume (the yardstick they are held to for the tumour cases: 1.25).

    python tools/bench_components.py [--reps 20] [--connectivity 26] [--hole_connectivity 6] [--min_voxels 64] [--cases tumour,noise_0.5] [--floor_tbps 3.78]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import fill_holes, keep_largest_component, remove_small_components  # noqa: E402
from vs_seg_amd.inferers import argmax_segmentation  # noqa: E402

SHAPE = (512, 512, 120)


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


def host_route(outputs, connectivity):
    """ms of: argmax on the device (as the export path has it) -> host copy -> scipy label -> bincount -> mask of the largest."""
    try:
        from scipy import ndimage as nd
    except ImportError:
        return None
    st = nd.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    seg = argmax_segmentation(outputs)[0].cpu().numpy()
    lab, n = nd.label(seg, st)
    keep = lab == (np.bincount(lab.ravel())[1:].argmax() + 1) if n else np.zeros(seg.shape, bool)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, int(keep.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--connectivity", type=int, default=26, choices=[6, 18, 26])
    ap.add_argument("--hole_connectivity", type=int, default=6, choices=[6, 18, 26])
    ap.add_argument("--min_voxels", type=int, default=64, help="threshold of remove_small_components (the far island has 41 voxels)")
    ap.add_argument("--cases", type=str, default="", help="comma-separated subset of the cases (for a kernel trace of one of them); default: all")
    ap.add_argument("--floor_tbps", type=float, default=3.78, help="rate of a whole-volume streaming pass (DESIGN.md §3.19: surf_edge_kernel) that the traffic floor is quoted at")
    a = ap.parse_args()
    torch.set_num_threads(1)  # the host route is timed on one core
    tumour = ellipsoid((302, 219, 61), (13, 12, 5))
    gen = torch.Generator(device="cuda").manual_seed(0)
    cases = {"tumour": tumour, "tumour_and_far_island": tumour | ellipsoid((40, 470, 12), (3, 2, 1.5)), "tumour_with_cavity": tumour & ~ellipsoid((303, 218, 62), (6, 5, 2)),
             "noise_0.5": torch.rand(SHAPE, device="cuda", generator=gen) < 0.5, "all_foreground": torch.ones(SHAPE, dtype=torch.bool, device="cuda")}
    if a.cases:
        cases = {k: cases[k] for k in a.cases.split(",")}
    nvox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    floor_ms = 20 * nvox / (a.floor_tbps * 1e12) * 1e3
    res = {"shape": SHAPE, "connectivity": a.connectivity, "hole_connectivity": a.hole_connectivity, "min_voxels": a.min_voxels, "traffic_floor_ms": round(floor_ms, 4),
           "floor_tbps": a.floor_tbps}
    for name, pred in cases.items():
        cl = torch.stack([torch.zeros(SHAPE, device="cuda"), torch.where(pred, 1.0, -1.0)], -1)[None]  # channels-last logits, as the sliding window returns them
        outputs = cl.permute(0, 4, 1, 2, 3)
        reps = a.reps if name.startswith("tumour") else max(1, a.reps // 5)
        ms = timed(lambda: keep_largest_component(outputs, a.connectivity), reps)
        out, stats = keep_largest_component(outputs, a.connectivity, return_stats=True)
        r = {"ms_per_call": round(ms, 4), "times_floor": round(ms / floor_ms, 2), "stats": [int(v) for v in stats[0].cpu()]}
        # the two new calls beside it, alternating with it in the same process; keep_largest_component once more afterwards, to show the drift of the yardstick
        ms_small = timed(lambda: remove_small_components(outputs, a.min_voxels, a.connectivity), reps)
        ms_fill = timed(lambda: fill_holes(outputs, a.hole_connectivity), reps)
        ms_again = timed(lambda: keep_largest_component(outputs, a.connectivity), reps)
        r["keep_largest_again_ms"] = round(ms_again, 4)
        r["remove_small_ms"], r["remove_small_over_keep_largest"] = round(ms_small, 4), round(ms_small / ms, 2)
        r["fill_holes_ms"], r["fill_holes_over_keep_largest"] = round(ms_fill, 4), round(ms_fill / ms, 2)
        r["remove_small_stats"] = [int(v) for v in remove_small_components(outputs, a.min_voxels, a.connectivity, return_stats=True)[1][0].cpu()]
        r["fill_holes_stats"] = [int(v) for v in fill_holes(outputs, a.hole_connectivity, return_stats=True)[1][0].cpu()]
        host = host_route(outputs, a.connectivity)
        if host is not None:
            r["host_scipy_ms"], r["host_over_gpu"] = round(host[0], 1), round(host[0] / ms, 1)
            assert host[1] == r["stats"][2] == int(out[0, 1].sum()), (name, host[1], r["stats"])
        res[name] = r
        del cl, outputs, out
        print(f"{name:24s} keep_largest {r['ms_per_call']:9.4f} ms   remove_small {r['remove_small_ms']:9.4f} ms ({r['remove_small_over_keep_largest']:.2f} x)   "
              f"fill_holes {r['fill_holes_ms']:9.4f} ms ({r['fill_holes_over_keep_largest']:.2f} x)", flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
