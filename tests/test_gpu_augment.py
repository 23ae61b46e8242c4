"""-m gpu: vsseg_crop_affine (the resampling gather of the training augmentation) against the fp64 restatement in tests/augment_oracle.py, the PatchSampler path
that draws its jobs, and one training epoch of the driver with the five flags.  Every figure is printed before it is asserted."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import augment_oracle as AO  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402

EPS = 2.0 ** -24
NOISE_TOL = 2e-5  # times noise_std: 6.2831853f * u rounded to fp32 (<= 2.4e-7) times an amplitude <= 5.8, libm errors of a few ulp, margin ~8
SEED = 0x123456789ABC


def run_affine(jobs, roi, seed=0):
    """jobs: dicts (vol: cuda tensor, m, interp, gain, bias, noise_std, stream) -> numpy [njobs, *roi] of one vsseg_crop_affine launch."""
    js = (L.AffineJob * len(jobs))()
    for j, d in zip(js, jobs):
        j.src, j.sdims, j.interp = d["vol"].data_ptr(), L.i3(d["vol"].shape), d.get("interp", 0)
        j.m = (C.c_float * 12)(*np.asarray(d["m"], np.float32).ravel().tolist())
        j.gain, j.bias, j.noise_std, j.noise_stream = d.get("gain", 1.0), d.get("bias", 0.0), d.get("noise_std", 0.0), d.get("stream", 0)
    jb = torch.frombuffer(bytearray(bytes(js)), dtype=torch.uint8).cuda()
    out = torch.empty((len(jobs), *roi), device="cuda")
    L.check(L.lib().vsseg_crop_affine(js, jb.data_ptr(), len(jobs), out.data_ptr(), L.i3(roi), seed, torch.cuda.current_stream().cuda_stream), "crop_affine")
    return out.cpu().numpy()


def mirrored_identity(origin, sdims, mask):
    """[I | origin] with the axes of `mask` mirrored in the matrix: s_a = sdims_a - 1 - (p_a + origin_a)."""
    m = np.concatenate([np.eye(3), np.asarray(origin, np.float64)[:, None]], 1)
    for a in range(3):
        if mask >> a & 1:
            m[a, a], m[a, 3] = -1.0, sdims[a] - 1 - origin[a]
    return m.astype(np.float32)


@pytest.fixture(scope="module")
def small():
    rng = np.random.default_rng(11)
    v = rng.standard_normal((19, 17, 29)).astype(np.float32)
    return v, torch.from_numpy(v).cuda()


@pytest.fixture(scope="module")
def job_results():
    """One launch for the four image jobs, the four label jobs and job 1 with gain and bias (tests 3-5 share it)."""
    vols = [tuple(torch.from_numpy(np.array(a)).cuda() for a in AO.job_volume(k)) for k in range(4)]  # (a copy: the shared references are read-only)
    jobs = [dict(vol=vols[k][0], m=AO.job_matrix(k)) for k in range(4)] + [dict(vol=vols[k][1], m=AO.job_matrix(k), interp=1) for k in range(4)]
    jobs += [dict(vol=vols[0][0], m=AO.job_matrix(0), gain=1.07, bias=-0.2), dict(vol=vols[0][1], m=AO.job_matrix(0), interp=1)]
    out = run_affine(jobs, AO.ROI)
    return dict(image=out[:4], label=out[4:8], gained=out[8], label_again=out[9])


@pytest.mark.parametrize("rz", [24, 22])
def test_identity_matrix_equals_the_plain_crop(small, rz):
    v, dv = small
    roi, origin = (16, 12, rz), (-3, 5, -2)  # three faces hang over; rz = 22: rows that are no multiple of the four voxels a thread owns
    cj = (L.CropJob * 8)()
    for mask in range(8):
        cj[mask].src, cj[mask].sdims, cj[mask].origin, cj[mask].flip = dv.data_ptr(), L.i3(v.shape), L.i3(origin), mask
    cb = torch.frombuffer(bytearray(bytes(cj)), dtype=torch.uint8).cuda()
    want = torch.empty((8, *roi), device="cuda")
    L.check(L.lib().vsseg_crop_flip(cb.data_ptr(), 8, want.data_ptr(), L.i3(roi), torch.cuda.current_stream().cuda_stream))
    want = want.cpu().numpy()
    assert np.abs(want).max() > 1.0 and (want == 0).any()
    for interp in (0, 1):
        got = run_affine([dict(vol=dv, m=mirrored_identity(origin, v.shape, mask), interp=interp) for mask in range(8)], roi)
        np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_half_voxel_shift_is_the_exact_mean_of_two_neighbours(small, axis):
    v, dv = small
    roi, origin = (16, 12, 24), (-3, 5, -2)
    e = np.eye(3, dtype=np.int64)[axis]
    m = np.concatenate([np.eye(3), (np.asarray(origin, np.float64) + 0.5 * e)[:, None]], 1)
    got = run_affine([dict(vol=dv, m=m), dict(vol=dv, m=m, interp=1)], roi)
    a, b = AO.window(v, origin, roi), AO.window(v, tuple(np.asarray(origin) + e), roi)
    np.testing.assert_array_equal(got[0], np.float32(0.5) * a + np.float32(0.5) * b)  # exact products, one rounding
    np.testing.assert_array_equal(got[1], b)  # floorf(s + 0.5f): a half rounds up


@pytest.mark.parametrize("k", range(4))
def test_trilinear_matches_the_oracle(job_results, k):
    s, want, _ = AO.job_reference(k)
    tol = AO.trilinear_tolerance(AO.job_volume(k)[0], s)
    err = float(np.abs(job_results["image"][k] - want).max())
    print(f"job {k + 1}: max |s| {np.abs(s).max():.2f}, max |trilinear - oracle| {err:.3e}, tolerance {tol:.3e}, zero-padded voxels {int((want == 0).sum())}")
    assert np.abs(want).max() > 0.5
    assert err <= tol


@pytest.mark.parametrize("k", range(4))
def test_nearest_matches_the_oracle_outside_the_rounding_band(job_results, k):
    s, _, want = AO.job_reference(k)
    band = AO.rounding_band(s)
    differ = job_results["label"][k] != want
    print(f"job {k + 1}: {int(band.sum())} of {band.size} voxels within {AO.delta(s):.2e} of a rounding boundary, {int(differ.sum())} voxels differ, foreground {int(want.sum())}")
    assert want.sum() > 100
    assert band.sum() <= 1e-3 * band.size
    assert not (differ & ~band).any()


def test_gain_and_bias(job_results):
    s, want, _ = AO.job_reference(0)
    g, b = float(np.float32(1.07)), float(np.float32(-0.2))
    got = job_results["gained"].astype(np.float64)
    # the intensity stage on its own: one fused operation on the value the interpolation gave (bit-identical in every launch)
    plain = job_results["image"][0].astype(np.float64)
    bound = 2.0 * EPS * (np.abs(plain * g) + abs(b))
    err = np.abs(got - (plain * g + b))
    print(f"gain/bias stage: max error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    # and the whole job against the oracle: the interpolation's tolerance scaled by the gain, plus that bound
    tol = AO.trilinear_tolerance(AO.job_volume(0)[0], s) * abs(g) + 2.0 * EPS * (np.abs(want * g) + abs(b))
    err = np.abs(got - (want * g + b))
    print(f"gain/bias job: max error {float(err.max()):.3e}, smallest tolerance {float(tol.min()):.3e}")
    assert (err <= tol).all()
    np.testing.assert_array_equal(job_results["label_again"], job_results["label"][0])  # the label job of the same geometry is unaffected


@pytest.mark.parametrize("roi", [(32, 32, 16), (8, 6, 22)])
def test_noise_matches_the_oracle(small, roi):
    v, dv = small
    std = 0.05
    m = mirrored_identity((0, 0, 0), v.shape, 0)
    jobs = [dict(vol=dv, m=m, gain=0.0, bias=0.0, noise_std=std, stream=st) for st in (0, 1)]
    got = run_affine(jobs, roi, SEED)
    again = run_affine(jobs, roi, SEED)
    np.testing.assert_array_equal(got, again)
    assert np.abs(got[0] - got[1]).max() > std
    for st in (0, 1):
        want = float(np.float32(std)) * AO.normals(roi, st, SEED)
        err = np.abs(got[st] - want)
        i = np.unravel_index(err.argmax(), err.shape)
        print(f"roi {roi} stream {st}: max |noise - oracle| = {float(err.max()) / std:.3e} noise_std at n = {want[i] / std:.3f} (tolerance {NOISE_TOL:.1e}), sample std {got[st].std():.4f}")
        assert err.max() <= NOISE_TOL * std
    assert np.abs(run_affine(jobs[:1], roi, SEED + 1)[0] - got[0]).max() > std  # the seed matters


ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)


def test_patch_sampler_replays_through_the_oracle():
    rng = np.random.default_rng(1)
    cases, host = [], []
    for shape in ((40, 36, 20), (33, 50, 16), (64, 64, 24)):
        v, l = rng.standard_normal(shape).astype(np.float32), (rng.random(shape) > 0.9).astype(np.float32)
        cases.append({"image": torch.from_numpy(v).cuda(), "label": torch.from_numpy(l).cuda()})
        host.append((v, l))
    roi = (32, 32, 16)
    s, twin = T.PatchSampler(cases, roi, flip_prob=0.5, seed=7, **ALL_ON), T.PatchSampler(cases, roi, flip_prob=0.5, seed=7, **ALL_ON)
    plain = T.PatchSampler(cases, roi, flip_prob=0.5, seed=7)
    seeds, worst, differ_total = set(), 0.0, 0
    for idx in ([0, 1, 2], [2, 2, 0, 1], [1]):
        img, lab = s.sample(idx)
        img2, lab2 = twin.sample(idx)
        assert torch.equal(img, img2) and torch.equal(lab, lab2)  # same seed, same bits
        plain.sample(idx)
        assert s.last_draws == plain.last_draws and plain.last_augment == []  # flip and crop draws are the un-augmented ones
        assert img.shape == (len(idx), 1, *roi) and lab.shape == img.shape and len(s.last_augment) == len(idx)
        img, lab = img.cpu().numpy(), lab.cpu().numpy()
        for b, i in enumerate(idx):
            (flip, start), a = s.last_draws[b], s.last_augment[b]
            assert a["m"].dtype == np.float32 and a["m"].shape == (3, 4) and a["noise_stream"] == b and a["noise_std"] == np.float32(0.05)
            assert (a["m"][0, 0] < 0) == flip and abs(float(a["gain"]) - 1.0) <= 0.1 + 1e-6 and abs(float(a["bias"])) <= 0.1 + 1e-6
            seeds.add(a["seed"])
            c = AO.coords(a["m"], roi)
            g, o, std = float(a["gain"]), float(a["bias"]), float(a["noise_std"])
            want = AO.trilinear(host[i][0], c)
            tol = AO.trilinear_tolerance(host[i][0], c) * abs(g) + 2.0 * EPS * (np.abs(want * g) + abs(o)) + NOISE_TOL * std
            err = np.abs(img[b, 0] - (want * g + o + std * AO.normals(roi, b, a["seed"])))
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (idx, b, float((err / tol).max()))
            band, differ = AO.rounding_band(c), lab[b, 0] != AO.nearest(host[i][1], c)
            differ_total += int(differ.sum())
            assert band.sum() <= 1e-3 * band.size and not (differ & ~band).any()
    print(f"PatchSampler replay: worst error / tolerance {worst:.3f}, label voxels that differ inside the rounding band {differ_total}, noise seeds {sorted(seeds)}")
    assert len(seeds) == 3  # one per sample() call
    # every range 0 = the sampler of today, bit for bit
    zero, default = T.PatchSampler(cases, roi, 0.5, 7, 0.0, 0.0, 0.0, 0.0, 0.0), T.PatchSampler(cases, roi, 0.5, 7)
    for idx in ([0, 1, 2], [2, 2, 0, 1]):
        (i0, l0), (i1, l1) = zero.sample(idx), default.sample(idx)
        assert torch.equal(i0, i1) and torch.equal(l0, l1) and zero.last_draws == default.last_draws


def test_training_epoch_with_the_five_flags(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 1` with every augmentation on, over the synthetic debug cases of tools/make_debug_data.py."""
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
            "--aug_rotate_deg", "15", "--aug_scale", "0.1", "--aug_intensity_scale", "0.1", "--aug_intensity_shift", "0.1", "--aug_noise_std", "0.05"]
    p = VSparams(argparse.ArgumentParser(), argv)
    p.create_results_folders()
    p.set_up_logger("training_log.txt")
    p.log_parameters()
    train_files, val_files, _ = p.load_T1_or_T2_data()
    ttf, vtf, _ = p.get_transforms()
    train_loader, val_loader = p.cache_transformed_train_data(train_files, ttf), p.cache_transformed_val_data(val_files, vtf)
    assert train_loader.sampler.tail.augmenting and not val_loader.sampler.tail.augmenting
    model, loss_fn = p.set_and_get_model(), p.set_and_get_loss_function()
    losses, _ = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
    print(f"epoch loss with augmentation: {losses}")
    assert len(losses) == 1 and np.isfinite(losses[0])
    assert len(train_loader.sampler.last_augment) >= 1 and train_loader.sampler.last_augment[0]["noise_std"] == np.float32(0.05)
    for h in p.logger.handlers:
        h.flush()
    log = open(os.path.join(p.logs_path, "training_log.txt")).read()
    for k in T.AUGMENT_KEYS:
        assert "aug_" + k + " =" in log
    assert "epoch 1 average loss" in log
