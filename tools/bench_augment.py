"""Time the augmenting crops (vsseg_crop_affine, vsseg_crop_field) beside the plain one (vsseg_crop_flip) at the two training shapes, batch 2 of 384 x 384 x 64 and
batch 4 of 384 x 128 x 128, over cached synthetic 512 x 512 x 120 volumes: rotation 15 degrees and scale +-10 % drawn by PatchSampler's own RandomTail, with and without
Gaussian noise; the field launch with the elastic deformation alone (magnitude drawn from [0, 16] voxels, spacing 64 / 64 / 16) and with elastic + bias field (log 0.3) + noise.
The launches alternate in one process (crop, affine, affine + noise, field, field + bias + noise, crop, ...), each timed with its own pair of device events after warm-up.
Prints microseconds per launch (median and mean) and GB/s = (bytes written + source bytes inside the footprint, counted once) / median time.
In the same loop, alternating with them: the appearance launches on the image half of the batch, every sample hit (sigma from [0.75, 1.5], resolution factor from [0.5, 1],
contrast +-25 %, gamma +-30 %): vsseg_patch_filter with blur alone, low resolution alone and both (algorithmic bytes: one read and one write of the image batch), and
vsseg_patch_tone with contrast alone and contrast + gamma (one read for the statistics, one read and one write for the map).

With --acquisition the tool times vsseg_patch_acquisition instead, every family on every sample (slab height 2..4, attenuation up to 0.8, amplitude up to 2): thick slices
alone, ghosting alone, the spike alone and all three (the two kernels and the scratch between them), alternating in the same process with its two yardsticks,
vsseg_patch_filter with low resolution alone and vsseg_patch_tone with contrast + gamma; algorithmic bytes are one read and one write of the image batch per kernel.

    python tools/bench_augment.py [--launches 200] [--warmup 20] [--acquisition]
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402

VOLUME = (512, 512, 120)
SHAPES = [(2, (384, 384, 64)), (4, (384, 128, 128))]
FIELD = dict(elastic_mag=16.0, bias_field=0.3, field_spacing=64)
APPEARANCE = dict(blur_sigma=1.5, lowres=0.5, contrast=0.25, gamma=0.3, appearance_prob=1.0)
ACQUISITION = dict(thick_slices=4, ghost=0.8, spike=2.0, acquisition_prob=1.0)
BUDGET_US = {(2, (384, 384, 64)): 227.0, (4, (384, 128, 128)): 259.0}  # 1 % of the 22.7 / 25.9 ms training step


def acquisition_arm(a, lib, stream):
    """vsseg_patch_acquisition by family beside vsseg_patch_filter (low resolution alone) and vsseg_patch_tone (contrast + gamma) on the same image batch."""
    gen = torch.Generator(device="cuda").manual_seed(0)
    print(f"vsseg_patch_acquisition on {torch.cuda.get_device_name(0)}: {a.launches} launches each after {a.warmup} warm-up, every family on every sample, {ACQUISITION}; "
          f"yardsticks in the same loop: vsseg_patch_filter with low resolution alone and vsseg_patch_tone with contrast + gamma ({APPEARANCE})")
    for B, roi in reversed(SHAPES):
        per = roi[0] * roi[1] * roi[2]
        tail = T.RandomTail(roi, 0.5, 0, **APPEARANCE, **ACQUISITION)
        src, dst, scratch = (torch.randn((B, *roi), device="cuda", generator=gen) for _ in range(3))
        stats, work = torch.empty((B, 4), device="cuda"), torch.empty((B, L.TONE_SHARDS, 3), dtype=torch.float64, device="cuda")
        kinds = ["patch_acquisition thick", "patch_acquisition ghost", "patch_acquisition spike", "patch_acquisition all three", "patch_filter low res", "patch_tone contrast+gamma"]
        kernels = [1, 1, 1, 2, 1, 1.5]  # reads + writes of the image batch, in pairs
        sets = []
        for _ in range(8):
            host = [(L.AcquisitionJob * B)() for _ in range(4)] + [(L.FilterJob * B)(), (L.ToneJob * B)()]
            for b in range(B):
                d = tail.draw_acquisition(roi)
                _, f, con, gam = tail.draw_appearance()
                for k, fields in enumerate((("thick", "thick_offset"), ("ghost_axis", "ghosts", "ghost_alpha"), ("spike_amp", "spike_k", "spike_phase"), tuple(d))):
                    job = dict(T.NEUTRAL_ACQUISITION, **{name: d[name] for name in fields})
                    j = host[k][b]
                    j.thick, j.thick_offset, j.ghost_axis, j.ghosts, j.ghost_alpha = job["thick"], job["thick_offset"], job["ghost_axis"], job["ghosts"], float(job["ghost_alpha"])
                    j.spike_amp, j.spike_k, j.spike_phase = float(job["spike_amp"]), (C.c_int32 * 2)(*job["spike_k"]), float(job["spike_phase"])
                host[4][b].radius, host[4][b].coarse = 0, (C.c_int32 * 2)(*T.coarse_size(roi, f))
                host[5][b].contrast, host[5][b].gamma = con, gam
            sets.append((host, [torch.frombuffer(bytearray(bytes(j)), dtype=torch.uint8).cuda() for j in host]))

        def launch(kind, s):
            host, dev = s
            if kind < 4:
                L.check(lib.vsseg_patch_acquisition(host[kind], dev[kind].data_ptr(), B, src.data_ptr(), dst.data_ptr(), scratch.data_ptr(), L.i3(roi), stream))
            elif kind == 4:
                L.check(lib.vsseg_patch_filter(host[kind], dev[kind].data_ptr(), B, src.data_ptr(), dst.data_ptr(), None, L.i3(roi), stream))
            else:  # in place on the patches the launches before it have just written
                L.check(lib.vsseg_patch_tone(host[kind], dev[kind].data_ptr(), B, dst.data_ptr(), per, stats.data_ptr(), work.data_ptr(), stream))

        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)] for _ in kinds]
        for i in range(a.warmup + a.launches):
            for kind in range(len(kinds)):
                if i >= a.warmup:
                    ev[kind][i - a.warmup][0].record()
                launch(kind, sets[i % len(sets)])
                if i >= a.warmup:
                    ev[kind][i - a.warmup][1].record()
        torch.cuda.synchronize()
        budget = BUDGET_US[(B, roi)]
        print(f"batch {B} of {roi}: {B * per * 4 / 1e6:.1f} MB of image; budget 1 % of the step = {budget:.0f} us")
        for kind, name in enumerate(kinds):
            us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[kind]])
            med, moved = float(np.median(us)), 2 * kernels[kind] * B * per * 4
            print(f"  {name:<28s} median {med:8.1f} us   mean {us.mean():8.1f} us   min {us.min():8.1f} us   {moved / med / 1e3:7.1f} GB/s  ({moved / 1e6:.1f} MB algorithmic)   {100.0 * med / budget:5.1f} % of the budget")


def footprint_voxels(m, roi, sdims):
    """Source voxels inside the axis-aligned box of the eight transformed patch corners (+ one tap), clipped to the volume: what a launch has to read at least once."""
    corners = np.array([[x, y, z, 1.0] for x in (0, roi[0] - 1) for y in (0, roi[1] - 1) for z in (0, roi[2] - 1)])
    s = corners @ m.astype(np.float64).T
    lo, hi = np.floor(s.min(0)), np.floor(s.max(0)) + 1
    n = [max(0.0, min(hi[a], sdims[a] - 1) - max(lo[a], 0) + 1) for a in range(3)]
    return int(n[0] * n[1] * n[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--acquisition", action="store_true", help="time vsseg_patch_acquisition beside its yardsticks instead of the crops and the appearance launches")
    a = ap.parse_args()
    lib, stream = L.lib(), torch.cuda.current_stream().cuda_stream
    if a.acquisition:
        return acquisition_arm(a, lib, stream)
    gen = torch.Generator(device="cuda").manual_seed(0)
    cases = [{"image": torch.randn(VOLUME, device="cuda", generator=gen), "label": (torch.rand(VOLUME, device="cuda", generator=gen) > 0.9).float()} for _ in range(4)]
    print(f"vsseg_crop_flip vs vsseg_crop_affine vs vsseg_crop_field on {torch.cuda.get_device_name(0)}: {a.launches} launches each after {a.warmup} warm-up, volumes {VOLUME}, rotation +-15 deg, scale +-10 %, "
          f"field {FIELD}; vsseg_patch_filter and vsseg_patch_tone with {APPEARANCE}")
    spacing = T.field_launch_spacing(FIELD["field_spacing"])
    for B, roi in SHAPES:
        per = roi[0] * roi[1] * roi[2]
        tail = T.RandomTail(roi, 0.5, 0, rotate_deg=15.0, scale=0.1, **FIELD, **APPEARANCE)
        out = torch.empty((2 * B, *roi), device="cuda")
        filtered, scratch = torch.empty((B, *roi), device="cuda"), torch.empty((B, *roi), device="cuda")  # the filter reads the image half of `out`; the tone maps `filtered`
        stats, work = torch.empty((B, 4), device="cuda"), torch.empty((B, L.TONE_SHARDS, 3), dtype=torch.float64, device="cuda")
        # a fixed set of job lists drawn up front, so that the timed loop holds launches only
        sets = []
        for _ in range(8):
            cj, aj, an, fe, fa = (L.CropJob * (2 * B))(), (L.AffineJob * (2 * B))(), (L.AffineJob * (2 * B))(), (L.FieldJob * (2 * B))(), (L.FieldJob * (2 * B))()
            pb, pl, pbl, tc, tcg = (L.FilterJob * B)(), (L.FilterJob * B)(), (L.FilterJob * B)(), (L.ToneJob * B)(), (L.ToneJob * B)()
            read_c = read_a = 0
            for b in range(B):
                flip, start = tail.draw(VOLUME)
                angle, scale, _, _ = tail.draw_augment()
                mag, blog = tail.draw_field()
                m = T.affine_matrix(roi, start, VOLUME[0], flip, angle, scale)
                sigma, f, con, gam = tail.draw_appearance()
                taps, coarse = T.blur_taps(sigma), T.coarse_size(roi, f)
                for js, w, n in ((pb, taps, roi[:2]), (pl, taps[:0], coarse), (pbl, taps, coarse)):
                    js[b].radius, js[b].taps, js[b].coarse = max(len(w) - 1, 0), (C.c_float * 6)(*w.tolist()), (C.c_int32 * 2)(*n)
                tc[b].contrast, tc[b].gamma, tcg[b].contrast, tcg[b].gamma = con, 1.0, con, gam
                read_c += 2 * per
                read_a += 2 * footprint_voxels(m, roi, VOLUME)
                for k, key in enumerate(("image", "label")):
                    j = cj[b + k * B]
                    j.src, j.sdims, j.origin, j.flip = cases[b][key].data_ptr(), L.i3(VOLUME), L.i3(start), int(flip)
                    for js, std, full in ((aj, 0.0, False), (an, 0.05, False), (fe, 0.0, False), (fa, 0.05, True)):
                        q = js[b + k * B]
                        q.src, q.sdims, q.m, q.interp, q.noise_stream = cases[b][key].data_ptr(), L.i3(VOLUME), (C.c_float * 12)(*m.ravel().tolist()), k, b
                        q.gain, q.bias, q.noise_std = 1.0, 0.0, (std if k == 0 else 0.0)
                        if js is fe or js is fa:
                            q.elastic_mag, q.bias_log = mag, (blog if full and k == 0 else 0.0)
            dev = [torch.frombuffer(bytearray(bytes(j)), dtype=torch.uint8).cuda() for j in (cj, aj, an, fe, fa, pb, pl, pbl, tc, tcg)]
            sets.append(((cj, aj, an, fe, fa, pb, pl, pbl, tc, tcg), dev, read_c, read_a))
        kinds = ["crop_flip", "crop_affine", "crop_affine + noise", "crop_field elastic", "crop_field el+bias+noise",
                 "patch_filter blur", "patch_filter low res", "patch_filter blur+low res", "patch_tone contrast", "patch_tone contrast+gamma"]

        def launch(kind, s):
            host, dev, _, _ = s
            if kind == 0:
                L.check(lib.vsseg_crop_flip(dev[0].data_ptr(), 2 * B, out.data_ptr(), L.i3(roi), stream))
            elif kind < 3:
                L.check(lib.vsseg_crop_affine(host[kind], dev[kind].data_ptr(), 2 * B, out.data_ptr(), L.i3(roi), 12345, stream))
            elif kind < 5:
                L.check(lib.vsseg_crop_field(host[kind], dev[kind].data_ptr(), 2 * B, out.data_ptr(), L.i3(roi), L.i3(spacing), 12345, stream))
            elif kind < 8:
                L.check(lib.vsseg_patch_filter(host[kind], dev[kind].data_ptr(), B, out.data_ptr(), filtered.data_ptr(), scratch.data_ptr(), L.i3(roi), stream))
            else:  # in place on the patches the filter launches before it have just written
                L.check(lib.vsseg_patch_tone(host[kind], dev[kind].data_ptr(), B, filtered.data_ptr(), per, stats.data_ptr(), work.data_ptr(), stream))

        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)] for _ in kinds]
        for i in range(a.warmup + a.launches):
            for kind in range(len(kinds)):
                if i >= a.warmup:
                    ev[kind][i - a.warmup][0].record()
                launch(kind, sets[i % len(sets)])
                if i >= a.warmup:
                    ev[kind][i - a.warmup][1].record()
        torch.cuda.synchronize()
        written = 2 * B * per * 4
        print(f"batch {B} of {roi}: {written / 1e6:.1f} MB written per launch")
        for kind, name in enumerate(kinds):
            us = np.array([e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[kind]])
            med = float(np.median(us))
            if kind >= 5:  # algorithmic bytes over the image half of the batch: filter 1 read + 1 write, tone 2 reads + 1 write
                moved = (2 if kind < 8 else 3) * B * per * 4
                print(f"  {name:<26s} median {med:8.1f} us   mean {us.mean():8.1f} us   min {us.min():8.1f} us   {moved / med / 1e3:7.1f} GB/s  ({moved / 1e6:.1f} MB algorithmic)")
                continue
            read = 4 * np.mean([s[2 if kind == 0 else 3] for s in sets])
            print(f"  {name:<26s} median {med:8.1f} us   mean {us.mean():8.1f} us   min {us.min():8.1f} us   {(written + read) / med / 1e3:7.1f} GB/s  ({read / 1e6:.1f} MB source footprint)")


if __name__ == "__main__":
    main()
