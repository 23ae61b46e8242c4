"""-m gpu: vsseg_patch_filter (in-plane blur, low resolution) and vsseg_patch_tone (contrast, gamma) against the fp64 restatement in tests/appearance_oracle.py, the
PatchSampler path that draws their jobs after the crop launch, and one training epoch of the driver with the five new flags.  Every tolerance is derived in the oracle;
every figure is printed before it is asserted.

powf: no document or header of the device library states its error, so it is measured: test_powf_error_against_fp64 gave max |powf - pow64| = 1.21 ulp on an MI355X
(PO.POW_MEASURED_ULP); the bar of the gamma tolerance, PO.POW_ULP, is 4 x that = 4.84 ulp."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import appearance_oracle as PO  # noqa: E402
from tests import augment_oracle as AO  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402

# the smallest shapes at which the kernels can still go wrong: shorter than 2R + 1 on both in-plane axes (the reflection folds more than once); odd, a multiple of no
# tile; several tiles per axis with z a multiple of the vector width; a single z
SHAPES = [(7, 5, 3), (33, 17, 5), (64, 48, 16), (16, 16, 1)]
# (sigma, f) of the five jobs of one launch: off, two blurs, low resolution alone, both
FIVE = [(0.0, 1.0), (0.5, 1.0), (1.5, 1.0), (0.0, 0.5), (1.0, 0.5)]


def run_filter(src, jobs, scratch="auto"):
    """src [J, *roi] cuda; jobs: (taps or sigma, coarse or f) per job -> (dst [J, *roi] of ONE vsseg_patch_filter launch, the (taps, coarse) it ran)."""
    J, roi = src.shape[0], tuple(src.shape[1:])
    js, ran = (L.FilterJob * J)(), []
    for j, (w, c) in zip(js, jobs):
        w = (PO.taps(w) if w else np.zeros(0, np.float32)) if np.isscalar(w) else np.asarray(w, np.float32)
        c = PO.coarse_size(roi, c) if np.isscalar(c) else tuple(int(a) for a in c)
        j.radius, j.taps, j.coarse = max(len(w) - 1, 0), (C.c_float * 6)(*w.tolist()), (C.c_int32 * 2)(*c)
        ran.append((w, c))
    both = any(len(w) > 1 and c != roi[:2] for w, c in ran)
    sc = torch.empty_like(src) if (scratch == "auto" and both) or scratch is True else None
    jb = torch.frombuffer(bytearray(bytes(js)), dtype=torch.uint8).cuda()
    dst = torch.empty_like(src)
    L.check(L.lib().vsseg_patch_filter(js, jb.data_ptr(), J, src.data_ptr(), dst.data_ptr(), sc.data_ptr() if sc is not None else None, L.i3(roi), torch.cuda.current_stream().cuda_stream), "patch_filter")
    return dst, ran


def run_tone(x, jobs):
    """x [J, n] cuda (left alone); jobs: (contrast, gamma) per job -> (out [J, n], stats [J, 4]) of ONE vsseg_patch_tone launch."""
    J, n = x.shape
    js = (L.ToneJob * J)()
    for j, (c, g) in zip(js, jobs):
        j.contrast, j.gamma = c, g
    jb = torch.frombuffer(bytearray(bytes(js)), dtype=torch.uint8).cuda()
    out, stats, work = x.clone(), torch.empty((J, 4), device="cuda"), torch.empty((J, L.TONE_SHARDS, 3), dtype=torch.float64, device="cuda")
    L.check(L.lib().vsseg_patch_tone(js, jb.data_ptr(), J, out.data_ptr(), n, stats.data_ptr(), work.data_ptr(), torch.cuda.current_stream().cuda_stream), "patch_tone")
    return out, stats


def patches(shape, J, seed=3):
    return np.random.default_rng(seed).standard_normal((J, *shape)).astype(np.float32)


def check_filter(got, v, w, coarse, what):
    want, tol = PO.filter_job(v, w, coarse)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max |device - oracle| {float(err.max()):.3e}, tolerance {float(np.max(tol)):.3e}, worst error / tolerance {float((err / np.maximum(tol, 1e-300)).max()):.3f}; the filter moves the patch by up to {float(np.abs(want - v).max()):.3f}")
    assert np.abs(want - v).max() > 0.05  # the test would notice a missing filter
    assert (err <= tol).all()


# ---- vsseg_patch_filter ----
@pytest.mark.parametrize("roi", SHAPES)
def test_five_jobs_of_one_launch_match_the_oracle_and_touch_only_their_own_patch(roi):
    v = patches(roi, 5)
    src = torch.from_numpy(v).cuda()
    dst, ran = run_filter(src, FIVE)
    again, _ = run_filter(src, FIVE)
    assert torch.equal(dst, again)  # 6. two launches, the same bits
    assert torch.equal(dst[0], src[0])  # the off job is a copy
    got = dst.cpu().numpy()
    assert np.isfinite(got).all()
    for j in range(1, 5):
        check_filter(got[j], v[j], *ran[j], f"roi {roi} job {j} (sigma {FIVE[j][0]}, f {FIVE[j][1]}, coarse {ran[j][1]})")
    # 5. each job alone among sources of 1e30 (the allocator's pools are NaN, so is the fresh scratch): a read outside the job's own patch would show
    for j in range(5):
        alone = torch.full_like(src, 1e30)
        alone[j] = src[j]
        out, _ = run_filter(alone, FIVE)
        assert torch.equal(out[j], dst[j]), (roi, j)


@pytest.mark.parametrize("roi", SHAPES)
def test_low_resolution_factors(roi):
    fs = (0.25, 0.5, 0.77)
    jobs = [(0.0, f) for f in fs] + [(1.0, f) for f in fs]
    v = patches(roi, 6, seed=4)
    dst, ran = run_filter(torch.from_numpy(v).cuda(), jobs)
    got = dst.cpu().numpy()
    for j, (s, f) in enumerate(jobs):
        if ran[j][1] == roi[:2] and not s:
            np.testing.assert_array_equal(got[j], v[j])
        else:
            check_filter(got[j], v[j], *ran[j], f"roi {roi} sigma {s} f {f} coarse {ran[j][1]}")
    # one axis at full size: that axis is not interpolated
    if roi[0] > 1:
        one, ran = run_filter(torch.from_numpy(v[:1]).cuda(), [(0.0, (max(1, roi[0] // 2), roi[1]))])
        check_filter(one.cpu().numpy()[0], v[0], *ran[0], f"roi {roi} coarse {ran[0][1]}")


@pytest.mark.parametrize("roi", [(7, 5, 3), (33, 17, 5)])
@pytest.mark.parametrize("sigma", [0.5, 1.5])
def test_an_impulse_in_a_corner_returns_the_outer_product_of_the_reflected_taps(roi, sigma):
    w = PO.taps(sigma)
    R = len(w) - 1
    v = np.zeros((1, *roi), np.float32)
    v[0, 0, roi[1] - 1, :] = 1.0  # the corner x = 0, y = ry - 1
    got = run_filter(torch.from_numpy(v).cuda(), [(w, roi[:2])])[0].cpu().numpy()[0]
    line = lambda n, at: np.array([sum(float(w[abs(k)]) for k in range(-R, R + 1) if PO.reflect(p + k, n) == at) for p in range(n)])  # noqa: E731
    want = np.outer(line(roi[0], 0), line(roi[1], roi[1] - 1))[:, :, None] * np.ones(roi[2])
    tol = PO.blur_tolerance(v[0], w)
    err = np.abs(got - want)
    print(f"roi {roi} sigma {sigma}: corner value {got[0, -1, 0]:.6f} (w_0 + w_1 squared {float(w[0] + w[1]) ** 2:.6f}), sum {got[:, :, 0].sum():.7f}, max error {float(err.max()):.2e}, tolerance {float(tol.max()):.2e}")
    assert (err <= tol).all() and abs(got[:, :, 0].sum() - 1.0) < 1e-5 and (got >= 0).all()


@pytest.mark.parametrize("roi", SHAPES)
def test_coarse_equal_to_the_roi_gives_the_blurred_patch_bit_exactly(roi):
    v = torch.from_numpy(patches(roi, 3, seed=6)).cuda()
    alone, _ = run_filter(v[:1].contiguous(), [(1.5, roi[:2])])
    beside, _ = run_filter(v, [(1.5, roi[:2]), (1.0, 0.5), (0.0, 0.5)], scratch=True)  # the second launch runs, the scratch is there: job 0 must not notice
    assert torch.equal(beside[0], alone[0])
    assert not torch.equal(beside[0], v[0])


# ---- vsseg_patch_tone ----
def check_stats(stats, x, what):
    mu64 = float(x.astype(np.float64).mean())
    bound = PO.mean_bound(mu64)
    err = abs(float(stats[2]) - float(np.float32(mu64)))
    print(f"{what}: min {stats[0]:.6f} max {stats[1]:.6f} mean {stats[2]:.8f}; |mean - fl32(mean64)| {err:.3e}, bound {bound:.3e}")
    assert stats[0] == x.min() and stats[1] == x.max() and stats[3] == 0.0
    assert err <= bound


@pytest.mark.parametrize("n", PO.TONE_SIZES)
def test_tone_statistics(n):
    rng = np.random.default_rng(n)
    x = (1000.0 + rng.standard_normal((2, n))).astype(np.float32)
    dev = torch.from_numpy(x).cuda()
    out, stats = run_tone(dev, [(0.75, 1.0), (1.0, 0.7)])
    out2, stats2 = run_tone(dev, [(0.75, 1.0), (1.0, 0.7)])
    assert torch.equal(stats, stats2) and torch.equal(out, out2)
    for j in range(2):
        check_stats(stats.cpu().numpy()[j], x[j], f"n {n} job {j} (mean 1000, sd 1)")


@pytest.mark.parametrize("k", range(4))
def test_tone_statistics_of_the_job_volumes(k):
    x = np.ascontiguousarray(AO.job_volume(k)[0], dtype=np.float32).reshape(1, -1)
    out, stats = run_tone(torch.from_numpy(x).cuda(), [(1.25, 1.0)])
    check_stats(stats.cpu().numpy()[0], x[0], f"job volume {k + 1} ({x.shape[1]} voxels)")


def check_tone(got, x, c, g, stats, what):
    want, tol = PO.tone(x, c, g, stats)
    err = np.abs(got.astype(np.float64) - want)
    print(f"{what}: max |device - oracle| {float(err.max()):.3e}, worst error / tolerance {float((err / tol).max()) if np.any(tol) else 0.0:.3f}, largest tolerance {float(np.max(tol)):.3e}; the map moves the values by up to {float(np.abs(want - x).max()):.3f}")
    assert np.isfinite(got).all() and (err <= tol).all()
    return want


@pytest.mark.parametrize("n", PO.TONE_SIZES)
def test_tone_jobs_match_the_oracle(n):
    x = PO.tone_input(n)
    out, stats = run_tone(torch.from_numpy(x).cuda(), PO.TONE_JOBS)
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    for j, (c, g) in enumerate(PO.TONE_JOBS):
        if (c, g) == (1.0, 1.0):
            np.testing.assert_array_equal(out[j], x[j])  # left untouched, bit for bit
            assert (stats[j] == 0.0).all()
            continue
        check_stats(stats[j], x[j], f"n {n} job {j}")
        want = check_tone(out[j], x[j], c, g, stats[j], f"n {n} c {c} gamma {g}")
        assert np.abs(want - x[j]).max() > 0.05
        assert out[j].min() >= stats[j][0] and out[j].max() <= stats[j][1] + 1e-6 * abs(stats[j][1])  # the range is preserved
        if c > 1.0:
            clamped = PO.contrast(x[j], c, stats[j])[2]
            print(f"n {n} c {c}: {int(clamped.sum())} of {n} voxels clamped")
            assert 1 <= clamped.sum() <= n // 2


def test_a_constant_patch_comes_out_unchanged_and_finite():
    x = torch.full((3, 2805), 2.5, device="cuda")
    out, stats = run_tone(x, [(1.25, 1.0), (1.0, 0.7), (0.75, 1.5)])
    assert torch.isfinite(out).all() and torch.equal(out, x)
    assert (stats.cpu().numpy() == np.array([2.5, 2.5, 2.5, 0.0], np.float32)).all()


def test_powf_error_against_fp64():
    """The figure behind PO.POW_ULP.  With min 0 and max 4 and c = 1: a = 0, r = 4, 4 + 1e-7f == 4 in fp32, so base = x / 4 and out = 4 powf(base, gamma), both exact scalings:
    out / 4 is the device library's powf(x / 4, gamma) itself.  Compared with pow in fp64 on the test's own inputs, never with another output of the kernel."""
    assert np.float32(4.0) + np.float32(1e-7) == np.float32(4.0)
    n = 49152
    x = (4.0 * np.random.default_rng(9).random((2, n))).astype(np.float32)
    x[:, 0], x[:, 1] = 0.0, 4.0
    out, stats = run_tone(torch.from_numpy(x).cuda(), [(1.0, 0.7), (1.0, 1.5)])
    out, stats = out.cpu().numpy(), stats.cpu().numpy()
    worst = 0.0
    for j, g in enumerate((0.7, 1.5)):
        assert stats[j][0] == 0.0 and stats[j][1] == 4.0
        ref = (x[j].astype(np.float64) / 4.0) ** float(np.float32(g))
        ulp = np.abs(out[j].astype(np.float64) / 4.0 - ref) / np.spacing(np.maximum(ref, 2.0 ** -126).astype(np.float32)).astype(np.float64)
        print(f"gamma {g}: max |powf - pow64| = {float(ulp.max()):.3f} ulp over {n} bases in [0, 1]")
        worst = max(worst, float(ulp.max()))
    print(f"powf: measured {worst:.3f} ulp; recorded {PO.POW_MEASURED_ULP} ulp, bar {PO.POW_ULP} ulp")
    assert worst <= PO.POW_MEASURED_ULP * 1.25 + 0.25 and worst <= PO.POW_ULP  # the recorded figure still describes the library


# ---- PatchSampler ----
ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)
FIELD_ON = dict(elastic_mag=2.0, bias_field=0.3, field_spacing=8)
APP_ON = dict(blur_sigma=1.5, lowres=0.5, contrast=0.25, gamma=0.3)
MODES = {"plain": {}, "five": ALL_ON, "five+field": dict(ALL_ON, **FIELD_ON)}


@pytest.fixture(scope="module")
def cases():
    return [{"image": torch.from_numpy(np.array(AO.job_volume(k)[0])).cuda(), "label": torch.from_numpy(np.array(AO.job_volume(k)[1])).cuda()} for k in range(4)]


def same_crop_jobs(a, b):
    """The crop launches of two samplers ran the same jobs."""
    assert a.last_draws == b.last_draws and len(a.last_augment) in (len(b.last_augment), len(a.last_draws))
    for x, y in zip(a.last_augment, b.last_augment):
        for k, v in y.items():
            assert np.array_equal(x[k], v), k


@pytest.mark.parametrize("mode", MODES)
def test_patch_sampler_replays_through_the_oracle(cases, mode):
    roi, aug = AO.ROI, MODES[mode]
    s, twin = T.PatchSampler(cases, roi, 0.5, 7, **aug, **APP_ON, appearance_prob=1.0), T.PatchSampler(cases, roi, 0.5, 7, **aug, **APP_ON, appearance_prob=1.0)
    crop = T.PatchSampler(cases, roi, 0.5, 7, **aug)  # the same seed: the crop launch of `s`, relaunched from the same draws (checked below)
    other = T.PatchSampler(cases, roi, 0.5, 8, **aug, **APP_ON, appearance_prob=1.0)
    worst_f = worst_t = 0.0
    for idx in ([0, 1, 2], [3, 2, 0], [1, 3, 3]):
        img, lab = s.sample(idx)
        img2, lab2 = twin.sample(idx)
        assert torch.equal(img, img2) and torch.equal(lab, lab2)  # 11. the same seed, the same bits ...
        assert not torch.equal(other.sample(idx)[0], img)  # ... another seed, another image
        cimg, clab = crop.sample(idx)
        same_crop_jobs(s, crop)
        assert torch.equal(lab, clab)  # the label is the crop's
        assert img.shape == (3, 1, *roi) and s.last_tone_stats.shape == (3, 4)
        # the device's own filter stage on the crop output, job for job as the sampler recorded it; it is deterministic, so this IS what the tone launch read
        filt, ran = run_filter(cimg[:, 0].contiguous(), [(a["blur_taps"], a["coarse"]) for a in s.last_augment])
        v, f, got, stats = cimg[:, 0].cpu().numpy(), filt.cpu().numpy(), img[:, 0].cpu().numpy(), s.last_tone_stats.cpu().numpy()
        for b in range(3):
            a = s.last_augment[b]
            assert 0.75 <= a["blur_sigma"] <= 1.5 and a["blur_taps"].dtype == np.float32 and len(a["blur_taps"]) == PO.radius(a["blur_sigma"]) + 1 and np.array_equal(a["blur_taps"], PO.taps(a["blur_sigma"]))
            assert a["coarse"] == tuple(ran[b][1]) and all(roi[i] // 2 <= a["coarse"][i] <= roi[i] for i in range(2))
            assert a["contrast"].dtype == np.float32 and 0.75 <= a["contrast"] <= 1.25 and a["gamma"].dtype == np.float32 and np.float32(0.7) <= a["gamma"] <= np.float32(1.3)
            want, tol = PO.filter_job(v[b], a["blur_taps"], a["coarse"])
            err = np.abs(f[b] - want)
            worst_f = max(worst_f, float((err / tol).max()))
            assert (err <= tol).all() and np.abs(want - v[b]).max() > 0.05
            check_stats(stats[b], f[b], f"{mode} {idx} sample {b}")
            want, tol = PO.tone(f[b], a["contrast"], a["gamma"], stats[b])
            err = np.abs(got[b] - want)
            worst_t = max(worst_t, float((err / tol).max()))
            assert (err <= tol).all(), (idx, b, float((err / tol).max()))
    print(f"PatchSampler replay ({mode}): worst error / tolerance: filter {worst_f:.3f}, tone {worst_t:.3f}")


@pytest.mark.parametrize("mode", ["plain", "five+field"])
def test_probability_zero_and_zero_ranges_are_the_sampler_of_today(cases, mode):
    roi, aug = AO.ROI, MODES[mode]
    p0 = T.PatchSampler(cases, roi, 0.5, 7, **aug, **APP_ON, appearance_prob=0.0)
    zero = T.PatchSampler(cases, roi, 0.5, 7, **aug, blur_sigma=0.0, lowres=0.0, contrast=0.0, gamma=0.0, appearance_prob=1.0)
    today = T.PatchSampler(cases, roi, 0.5, 7, **aug)
    for idx in ([0, 1, 2], [3, 2, 0, 1]):
        i0, l0 = today.sample(idx)
        for s in (p0, zero):
            i1, l1 = s.sample(idx)
            assert torch.equal(i0, i1) and torch.equal(l0, l1) and s.last_draws == today.last_draws and s.last_tone_stats is None
            assert len(s.last_augment) == len(today.last_augment) and all("blur_sigma" not in a and "gamma" not in a for a in s.last_augment)
            same_crop_jobs(s, today)


def test_at_probability_one_half_some_samples_are_hit_and_the_others_are_the_crop(cases):
    roi = AO.ROI
    s, crop = T.PatchSampler(cases, roi, 0.5, 21, **ALL_ON, **APP_ON, appearance_prob=0.5), T.PatchSampler(cases, roi, 0.5, 21, **ALL_ON)
    hit = missed = 0
    families = np.zeros(4, int)
    for it in range(10):
        idx = [(it + k) % 4 for k in range(4)]
        img, lab = s.sample(idx)
        cimg, clab = crop.sample(idx)
        same_crop_jobs(s, crop)
        assert torch.equal(lab, clab)
        for b, a in enumerate(s.last_augment):
            on = (a["blur_sigma"] != 0.0, a["coarse"] != roi[:2], a["contrast"] != 1.0, a["gamma"] != 1.0)
            families += on
            if any(on):
                hit += 1
                assert not torch.equal(img[b], cimg[b])
            else:
                missed += 1
                assert torch.equal(img[b], cimg[b])
    print(f"P = 0.5 over 40 samples: {hit} hit, {missed} untouched; per family {families}")
    assert hit > 0 and missed > 0 and (families > 5).all() and (families < 35).all()


# ---- the driver ----
def test_training_epoch_with_the_appearance_flags(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 1` with the five new flags, over the synthetic debug cases of tools/make_debug_data.py."""
    import importlib.util

    from vs_seg_amd.params import VSparams

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("make_debug_data", os.path.join(root, "tools", "make_debug_data.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    data = os.path.join(str(tmp_path), "data") + os.sep
    gen.main(["--data_root", data, "--size", "64", "64", "32"])
    monkeypatch.chdir(root)  # --debug reads ./params/split_debug.csv
    argv = ["--debug", "--num_epochs", "1", "--data_root", data, "--compute_dtype", "fp32", "--train_batch_size", "2",
            "--aug_blur_sigma", "1.5", "--aug_lowres", "0.5", "--aug_contrast", "0.25", "--aug_gamma", "0.3", "--aug_appearance_prob", "0.75"]
    p = VSparams(argparse.ArgumentParser(), argv)
    p.create_results_folders()
    p.set_up_logger("training_log.txt")
    p.log_parameters()
    train_files, val_files, _ = p.load_T1_or_T2_data()
    ttf, vtf, _ = p.get_transforms()
    train_loader, val_loader = p.cache_transformed_train_data(train_files, ttf), p.cache_transformed_val_data(val_files, vtf)
    assert train_loader.sampler.appearing and not train_loader.sampler.tail.augmenting and not val_loader.sampler.appearing and not val_loader.sampler.tail.appearing
    model, loss_fn = p.set_and_get_model(), p.set_and_get_loss_function()
    losses, _ = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
    print(f"epoch loss with the appearance families: {losses}")
    assert len(losses) == 1 and np.isfinite(losses[0])
    last = train_loader.sampler.last_augment
    assert len(last) >= 1 and set(last[0]) >= {"blur_sigma", "blur_taps", "coarse", "contrast", "gamma"} and 0.0 <= last[0]["blur_sigma"] <= 1.5
    for h in p.logger.handlers:
        h.flush()
    log = open(os.path.join(p.logs_path, "training_log.txt")).read()
    for k in T.APPEARANCE_KEYS:
        assert "aug_" + k + " =" in log
    assert "epoch 1 average loss" in log
