"""Time vsseg_measurements (vs_seg_amd.compute_measurements) at the test-volume size (512 x 512 x 120, spacing 0.41 x 0.41 x 1.5 mm) with HIP events after
warm-up, for three predictions against a tumour label: a clean tumour ellipsoid, the same plus one far false-positive island (the (y, z) bounding box
then spans most of the plane), and a noisy prediction with a random half of the voxels foreground (every column occupied: the bad case of the pair
stage).  Beside each: vsseg_hard_dice_counts on the same tensors in the same process, which reads the same 12 B per voxel and is the yardstick of the
streaming pass, and a call on empty masks, whose pair stage exits at once, so that its time bounds init + streaming pass + finalize from above.

    python tools/bench_measurements.py [--reps 20]
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import MEASUREMENT_FIELDS, compute_measurements  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

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


def ellipsoid(c, r):
    g = [torch.arange(s, device="cuda", dtype=torch.float32) for s in SHAPE]
    return ((g[0][:, None, None] - c[0]) / r[0]) ** 2 + ((g[1][None, :, None] - c[1]) / r[1]) ** 2 + ((g[2][None, None, :] - c[2]) / r[2]) ** 2 <= 1.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    lib = L.lib()
    gt = ellipsoid((256, 256, 60), (30, 24, 8))
    clean = ellipsoid((258, 255, 61), (29, 25, 8))
    torch.manual_seed(0)
    cases = {"clean": clean, "far_island": clean | ellipsoid((30, 480, 10), (3, 3, 2)), "noise_half": torch.rand(SHAPE, device="cuda") < 0.5,
             "empty_masks": torch.zeros(SHAPE, dtype=torch.bool, device="cuda")}
    nvox = SHAPE[0] * SHAPE[1] * SHAPE[2]
    stream = torch.cuda.current_stream().cuda_stream
    dims, sp = L.i3(SHAPE), (ctypes.c_float * 3)(*SPACING)
    scratch = torch.empty(int(lib.vsseg_measure_scratch_bytes(dims)), dtype=torch.uint8, device="cuda")
    out, counts = torch.empty(9, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")
    res = {"shape": SHAPE, "spacing": SPACING, "reps": a.reps}
    for name, pred in cases.items():
        lab = (torch.zeros_like(gt) if name == "empty_masks" else gt).float().contiguous()
        cl = torch.stack([torch.zeros(SHAPE, device="cuda"), torch.where(pred, 1.0, -1.0)], -1).contiguous()  # channels-last logits, as the sliding window returns them
        ms = timed(lambda: L.check(lib.vsseg_measurements(cl.data_ptr(), 2, lab.data_ptr(), dims, sp, scratch.data_ptr(), scratch.numel(), out.data_ptr(), stream), "measurements"), a.reps)
        ms_nl = timed(lambda: L.check(lib.vsseg_measurements(cl.data_ptr(), 2, None, dims, sp, scratch.data_ptr(), scratch.numel(), out.data_ptr(), stream), "measurements"), a.reps)
        ms_dice = timed(lambda: L.check(lib.vsseg_hard_dice_counts(cl.data_ptr(), 2, lab.data_ptr(), nvox, counts.data_ptr(), stream), "hard_dice_counts"), a.reps)
        ms_py = timed(lambda: compute_measurements(cl[None].permute(0, 4, 1, 2, 3), lab[None, None], SPACING), a.reps)
        vals = compute_measurements(cl[None].permute(0, 4, 1, 2, 3), lab[None, None], SPACING)[0].tolist()
        res[name] = {"ms_per_call": round(ms, 4), "ms_per_call_without_label": round(ms_nl, 4), "ms_compute_measurements": round(ms_py, 4), "ms_hard_dice_counts": round(ms_dice, 4),
                     "ratio_to_hard_dice_counts": round(ms / ms_dice, 3), "gbps_of_12B_per_voxel": round(12 * nvox / (ms * 1e-3) / 1e9, 1),
                     "values": {k: round(v, 4) for k, v in zip(MEASUREMENT_FIELDS, vals)}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
