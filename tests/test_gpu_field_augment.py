"""-m gpu: vsseg_crop_field (elastic deformation and bias field inside the resampling gather) against the fp64 restatement in tests/field_oracle.py, the PatchSampler
path that draws its jobs, and one training epoch of the driver with the three new flags.  Every tolerance is derived in the oracle; every figure is printed before it is asserted."""
import argparse
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import augment_oracle as AO  # noqa: E402
from tests import field_oracle as FO  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402

EPS = 2.0 ** -24
NOISE_TOL = 2e-5  # times noise_std: as derived in tests/test_gpu_augment.py
EXP_REL = 4.0 * 2.0 ** -23  # expf within 4 ulp (the device library documents 1)
SEED = 0x123456789ABC
SPACING, MAG = (8, 8, 2), 2.0  # of the whole-job tests


def _fill(js, jobs):
    for j, d in zip(js, jobs):
        j.src, j.sdims, j.interp = d["vol"].data_ptr(), L.i3(d["vol"].shape), d.get("interp", 0)
        j.m = (C.c_float * 12)(*np.asarray(d["m"], np.float32).ravel().tolist())
        j.gain, j.bias, j.noise_std, j.noise_stream = d.get("gain", 1.0), d.get("bias", 0.0), d.get("noise_std", 0.0), d.get("stream", 0)
    return js


def run_field(jobs, roi, spacing, seed=0, as_tensor=False):
    """jobs: dicts (vol: cuda tensor, m, interp, gain, bias, noise_std, stream, mag, blog) -> [njobs, *roi] of one vsseg_crop_field launch."""
    js = _fill((L.FieldJob * len(jobs))(), jobs)
    for j, d in zip(js, jobs):
        j.elastic_mag, j.bias_log = d.get("mag", 0.0), d.get("blog", 0.0)
    jb = torch.frombuffer(bytearray(bytes(js)), dtype=torch.uint8).cuda()
    out = torch.empty((len(jobs), *roi), device="cuda")
    L.check(L.lib().vsseg_crop_field(js, jb.data_ptr(), len(jobs), out.data_ptr(), L.i3(roi), L.i3(spacing), seed, torch.cuda.current_stream().cuda_stream), "crop_field")
    return out if as_tensor else out.cpu().numpy()


def run_affine(jobs, roi, seed=0, as_tensor=False):
    js = _fill((L.AffineJob * len(jobs))(), jobs)
    jb = torch.frombuffer(bytearray(bytes(js)), dtype=torch.uint8).cuda()
    out = torch.empty((len(jobs), *roi), device="cuda")
    L.check(L.lib().vsseg_crop_affine(js, jb.data_ptr(), len(jobs), out.data_ptr(), L.i3(roi), seed, torch.cuda.current_stream().cuda_stream), "crop_affine")
    return out if as_tensor else out.cpu().numpy()


@pytest.fixture(scope="module")
def vols():
    """(image, label) of the four jobs of the augmentation oracle on the device (a copy: the shared references are read-only)."""
    return [tuple(torch.from_numpy(np.array(a)).cuda() for a in AO.job_volume(k)) for k in range(4)]


def identity(offset):
    return np.concatenate([np.eye(3), np.asarray(offset, np.float64)[:, None]], 1).astype(np.float32)


# ---- 1. zero ranges reproduce vsseg_crop_affine ----
@pytest.mark.parametrize("spacing", [(8, 8, 2), (64, 64, 16)])
def test_zero_ranges_are_bit_identical_to_crop_affine(vols, spacing):
    jobs = [dict(vol=vols[k][0], m=AO.job_matrix(k), gain=1.07, bias=-0.2, noise_std=0.05, stream=k) for k in range(4)] + [dict(vol=vols[k][1], m=AO.job_matrix(k), interp=1, stream=k) for k in range(4)]
    want, got = run_affine(jobs, AO.ROI, SEED, as_tensor=True), run_field(jobs, AO.ROI, spacing, SEED, as_tensor=True)
    assert float(want[:4].std()) > 0.1 and float(want[4:].sum()) > 400
    assert torch.equal(got, want)


# ---- 2. the field itself ----
@pytest.mark.parametrize("roi,spacing", FO.SHAPES)
def test_field_matches_the_oracle(roi, spacing):
    mag = spacing[0] / 4.0  # the largest the entry point accepts
    pad = int(np.ceil(mag)) + 2  # every tap of every deformed coordinate stays inside
    dims = tuple(r + 2 * pad for r in roi)
    idx = np.meshgrid(*[np.arange(d, dtype=np.float32) for d in dims], indexing="ij")  # volumes that hold their own x / y / z index
    vx, vy, vz = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in idx)
    m = identity((pad, pad, pad))
    jobs = [dict(vol=vx, m=m, mag=mag, stream=5), dict(vol=vy, m=m, mag=mag, stream=5), dict(vol=vz, m=m, mag=mag, stream=5, interp=1), dict(vol=vx, m=m, mag=mag, stream=6)]
    got = run_field(jobs, roi, spacing, SEED)
    np.testing.assert_array_equal(got, run_field(jobs, roi, spacing, SEED))  # same stream and seed: the same bits
    other_seed = run_field(jobs[:1], roi, spacing, SEED + 1)[0]
    s = FO.coords(m, roi, spacing, mag, 5, SEED)
    x, y, z = AO.grid(roi)
    cd = FO.coord_delta(s, m, mag, roi)
    for a, (name, und) in enumerate((("d_x", x + pad), ("d_y", y + pad))):
        tol = FO.trilinear_tolerance(idx[a], s, cd)  # the volume is linear along axis a with slope 1: cd[a] + the interpolation's own rounding
        err = float(np.abs((got[a].astype(np.float64) - und) - (s[a] - und)).max())
        print(f"roi {roi} spacing {spacing} mag {mag}: max |{name}| {np.abs(s[a] - und).max():.3f}, max |{name} - oracle| {err:.3e}, tolerance {tol:.3e} (field_delta {FO.field_delta(mag):.3e})")
        assert np.abs(s[a] - und).max() > 0.1 * mag and np.abs(s[a] - und).max() <= mag
        assert err <= tol
    np.testing.assert_array_equal(got[2], z + pad)  # d_z = 0: the nearest lookup returns exactly the undeformed z
    assert np.abs(got[3] - got[0]).max() > 0.05 * mag and np.abs(other_seed - got[0]).max() > 0.05 * mag  # another stream, another seed: another field
    if roi[0] > 1:
        assert (np.diff(got[0], axis=0) > 0.0).all()  # x + d_x strictly increases along x at mag = S / 4: no folding
    assert (np.diff(got[1], axis=1) > 0.0).all()


# ---- 3. whole jobs against the oracle ----
@functools.lru_cache(maxsize=None)
def field_reference(k):
    """(coordinates, trilinear image, nearest label) of job k under the field of stream k, fp64, computed once."""
    img, lab = AO.job_volume(k)
    s = FO.coords(AO.job_matrix(k), AO.ROI, SPACING, MAG, k, SEED)
    return s, AO.trilinear(img, s), AO.nearest(lab, s)


@pytest.fixture(scope="module")
def job_results(vols):
    jobs = [dict(vol=vols[k][0], m=AO.job_matrix(k), mag=MAG, stream=k) for k in range(4)] + [dict(vol=vols[k][1], m=AO.job_matrix(k), mag=MAG, stream=k, interp=1) for k in range(4)]
    out = run_field(jobs, AO.ROI, SPACING, SEED)
    return dict(image=out[:4], label=out[4:])


@pytest.mark.parametrize("k", range(4))
def test_deformed_trilinear_matches_the_oracle(job_results, k):
    s, want, _ = field_reference(k)
    cd = FO.coord_delta(s, AO.job_matrix(k), MAG, AO.ROI)
    tol = FO.trilinear_tolerance(AO.job_volume(k)[0], s, cd)
    err = float(np.abs(job_results["image"][k] - want).max())
    moved = float(np.abs(want - AO.job_reference(k)[1]).max())
    print(f"job {k + 1}: coordinate bound {cd}, max |trilinear - oracle| {err:.3e}, tolerance {tol:.3e}; the field moves the image by up to {moved:.3f}")
    assert moved > 0.5  # the test would notice a missing field
    assert err <= tol


@pytest.mark.parametrize("k", range(4))
def test_deformed_nearest_matches_the_oracle_outside_the_rounding_band(job_results, k):
    s, _, want = field_reference(k)
    band = FO.rounding_band(s, FO.coord_delta(s, AO.job_matrix(k), MAG, AO.ROI))
    differ = job_results["label"][k] != want
    changed = float((want != AO.job_reference(k)[2]).mean())
    print(f"job {k + 1}: {int(band.sum())} of {band.size} voxels in the rounding band, {int(differ.sum())} voxels differ, the field changes {100 * changed:.1f} % of the label voxels")
    assert want.sum() > 100 and changed > 0.02
    assert band.sum() <= 1e-3 * band.size
    assert not (differ & ~band).any()


# ---- 4. bias field ----
@pytest.mark.parametrize("roi,spacing", [FO.SHAPES[0], FO.SHAPES[2]])
def test_bias_field_matches_the_oracle(roi, spacing):
    blog = 0.3
    dims = (roi[0] - 4, roi[1], roi[2])  # the last four x planes of the patch are zero padding
    ones = torch.ones(dims, device="cuda")
    m = identity((0, 0, 0))
    jobs = [dict(vol=ones, m=m, blog=blog, stream=2), dict(vol=ones, m=m, interp=1, stream=2)]
    got = run_field(jobs, roi, spacing, SEED)
    b = float(np.float32(blog)) * FO.fields(roi, spacing, 2, SEED)[2]
    want = np.exp(b)
    inside, rel = got[0][: dims[0]].astype(np.float64), EXP_REL + FO.field_delta(blog)
    err = np.abs(inside / want[: dims[0]] - 1.0)
    print(f"roi {roi} spacing {spacing}: bias in [{inside.min():.4f}, {inside.max():.4f}], max relative error {float(err.max()):.3e}, tolerance {rel:.3e}")
    assert err.max() <= rel
    assert inside.min() >= np.exp(-0.3) and inside.max() <= np.exp(0.3) and inside.max() - inside.min() > 0.05
    assert (got[0][dims[0]:] == 0.0).all()  # zero padding stays exactly 0
    np.testing.assert_array_equal(got[1], run_affine(jobs[1:], roi, SEED)[0])  # the label job of the same launch is unaffected
    assert (got[1][: dims[0]] == 1.0).all()


# ---- 5. PatchSampler ----
ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)
FIELD_ON = dict(elastic_mag=2.0, bias_field=0.3, field_spacing=8)


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(1)
    dev, host = [], []
    for shape in ((40, 36, 20), (33, 50, 16), (64, 64, 24)):
        v, l = rng.standard_normal(shape).astype(np.float32), (rng.random(shape) > 0.9).astype(np.float32)
        dev.append({"image": torch.from_numpy(v).cuda(), "label": torch.from_numpy(l).cuda()})
        host.append((v, l))
    return dev, host


@pytest.mark.parametrize("five", [True, False])
def test_patch_sampler_replays_through_the_oracle(cases, five):
    dev, host = cases
    roi, aug = (32, 32, 16), (ALL_ON if five else {})
    s, twin = T.PatchSampler(dev, roi, flip_prob=0.5, seed=7, **aug, **FIELD_ON), T.PatchSampler(dev, roi, flip_prob=0.5, seed=7, **aug, **FIELD_ON)
    plain = T.PatchSampler(dev, roi, flip_prob=0.5, seed=7, **aug)
    seeds, worst, differ_total = set(), 0.0, 0
    for idx in ([0, 1, 2], [2, 2, 0, 1], [1]):
        img, lab = s.sample(idx)
        img2, lab2 = twin.sample(idx)
        assert torch.equal(img, img2) and torch.equal(lab, lab2)  # same seed, same bits
        plain.sample(idx)
        assert s.last_draws == plain.last_draws  # flip and crop draws are those of a sampler without fields ...
        for a, p in zip(s.last_augment, plain.last_augment):  # ... and so are the five-family draws
            assert (a["m"] == p["m"]).all() and a["gain"] == p["gain"] and a["bias"] == p["bias"] and a["seed"] & 0xFFFFFFFF == p["seed"]
        assert img.shape == (len(idx), 1, *roi) and lab.shape == img.shape and len(s.last_augment) == len(idx)
        img, lab = img.cpu().numpy(), lab.cpu().numpy()
        for b, i in enumerate(idx):
            a = s.last_augment[b]
            assert a["spacing"] == (8, 8, 2) and a["elastic_mag"].dtype == np.float32 and 0.0 <= a["elastic_mag"] <= 2.0 and 0.0 <= a["bias_log"] <= np.float32(0.3) and a["noise_stream"] == b
            seeds.add(a["seed"])
            mag, blog, g, o, std = (float(a[k]) for k in ("elastic_mag", "bias_log", "gain", "bias", "noise_std"))
            c = FO.coords(a["m"], roi, a["spacing"], mag, b, a["seed"])
            cd = FO.coord_delta(c, a["m"], mag, roi)
            t, e = AO.trilinear(host[i][0], c), np.exp(blog * FO.fields(roi, a["spacing"], b, a["seed"])[2])
            want = t * e * g + o + (std * AO.normals(roi, b, a["seed"]) if std else 0.0)
            # the interpolation's tolerance through the two factors; exp and its argument; the product's and the fused gain / bias' roundings; the noise
            tol = FO.trilinear_tolerance(host[i][0], c, cd) * e * abs(g) + np.abs(t * e * g) * (EXP_REL + FO.field_delta(blog) + 2.0 * EPS) + 2.0 * EPS * (np.abs(t * e * g) + abs(o)) + NOISE_TOL * std
            err = np.abs(img[b, 0] - want)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (idx, b, float((err / tol).max()))
            band, differ = FO.rounding_band(c, cd), lab[b, 0] != AO.nearest(host[i][1], c)
            differ_total += int(differ.sum())
            assert band.sum() <= 1e-3 * band.size and not (differ & ~band).any()
    print(f"PatchSampler replay (five flags {five}): worst error / tolerance {worst:.3f}, label voxels that differ inside the rounding band {differ_total}, seeds {sorted(seeds)}")
    assert len(seeds) == 3 and all(sd >> 32 for sd in seeds)  # one per sample() call; the field's half is drawn with noise on or off
    # both field ranges 0 = the sampler of today, bit for bit
    zero, default = T.PatchSampler(dev, roi, 0.5, 7, **aug, elastic_mag=0.0, bias_field=0.0, field_spacing=8), T.PatchSampler(dev, roi, 0.5, 7, **aug)
    for idx in ([0, 1, 2], [2, 2, 0, 1]):
        (i0, l0), (i1, l1) = zero.sample(idx), default.sample(idx)
        assert torch.equal(i0, i1) and torch.equal(l0, l1) and zero.last_draws == default.last_draws
        assert len(zero.last_augment) == len(default.last_augment) and all("elastic_mag" not in a for a in zero.last_augment)


# ---- 6. the driver ----
def test_training_epoch_with_the_field_flags(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 1` with the five flags and the three field flags, over the synthetic debug cases of tools/make_debug_data.py."""
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
            "--aug_rotate_deg", "15", "--aug_scale", "0.1", "--aug_intensity_scale", "0.1", "--aug_intensity_shift", "0.1", "--aug_noise_std", "0.05",
            "--aug_elastic_mag", "4", "--aug_bias_field", "0.3", "--aug_field_spacing", "16"]
    p = VSparams(argparse.ArgumentParser(), argv)
    p.create_results_folders()
    p.set_up_logger("training_log.txt")
    p.log_parameters()
    train_files, val_files, _ = p.load_T1_or_T2_data()
    ttf, vtf, _ = p.get_transforms()
    train_loader, val_loader = p.cache_transformed_train_data(train_files, ttf), p.cache_transformed_val_data(val_files, vtf)
    assert train_loader.sampler.tail.fielding and train_loader.sampler.tail.augmenting and not val_loader.sampler.tail.fielding and not val_loader.sampler.tail.augmenting
    model, loss_fn = p.set_and_get_model(), p.set_and_get_loss_function()
    losses, _ = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
    print(f"epoch loss with the fields: {losses}")
    assert len(losses) == 1 and np.isfinite(losses[0])
    last = train_loader.sampler.last_augment
    assert len(last) >= 1 and last[0]["spacing"] == (16, 16, 4) and 0.0 <= last[0]["elastic_mag"] <= 4.0 and 0.0 <= last[0]["bias_log"] <= np.float32(0.3)
    for h in p.logger.handlers:
        h.flush()
    log = open(os.path.join(p.logs_path, "training_log.txt")).read()
    for k in ("aug_elastic_mag", "aug_bias_field", "aug_field_spacing") + tuple("aug_" + k for k in T.AUGMENT_KEYS):
        assert k + " =" in log
    assert "epoch 1 average loss" in log
