"""-m gpu: vsseg_patch_acquisition (thick slices, ghosting, spike) against the fp64 restatement in tests/acquisition_oracle.py, the PatchSampler path that draws its
jobs after the crop launch, and one training epoch of the driver with the four new flags.  Every tolerance is derived in the oracle; every figure is printed before
it is asserted.

cosf: no document or header of the device library states its error, so it is measured: test_cosf_error_against_fp64 gave max |cosf - cos64| = 1.50 ulp on an MI355X
(QO.COS_MEASURED_ULP); the bar of the spike tolerance, QO.COS_ULP, is 4 x that = 6 ulp."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import acquisition_oracle as QO  # noqa: E402
from tests import augment_oracle as AO  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402


def J(thick=1, thick_offset=0, ghost_axis=0, ghosts=0, ghost_alpha=0.0, spike_amp=0.0, spike_k=(0, 0), spike_phase=0.0):
    return dict(thick=thick, thick_offset=thick_offset, ghost_axis=ghost_axis, ghosts=ghosts, ghost_alpha=np.float32(ghost_alpha), spike_amp=np.float32(spike_amp), spike_k=tuple(spike_k), spike_phase=np.float32(spike_phase))


OFF = J()
# per shape the six jobs of one launch: off, T alone, G along x, G along y, S alone, all three (and what the shape is there for)
SIX = {
    # shorter than any tile; n = 2 and n = 3 along x (one more job; n = 6 = N is the identity up to rounding and has a test of its own)
    (6, 4, 3): [OFF, J(thick=2, thick_offset=1), J(ghosts=2, ghost_alpha=0.5), J(ghost_axis=1, ghosts=2, ghost_alpha=1.0), J(spike_amp=1.5, spike_k=(5, 1), spike_phase=2.0),
                J(thick=3, thick_offset=2, ghosts=3, ghost_alpha=0.7, spike_amp=0.8, spike_k=(1, 3), spike_phase=5.5), J(ghosts=3, ghost_alpha=0.25)],
    # odd; nothing divides 17, so the job along y is the one the sampler would draw: neutral; z no multiple of the vector width; f = 4 with o = 3 leaves slabs of 1 and 4
    (33, 17, 5): [OFF, J(thick=4, thick_offset=3), J(ghosts=3, ghost_alpha=0.6), OFF, J(spike_amp=0.7, spike_k=(32, 16), spike_phase=0.3),
                  J(thick=4, thick_offset=3, ghosts=3, ghost_alpha=1.0, spike_amp=2.0, spike_k=(0, 5), spike_phase=4.0)],
    # several tiles
    (64, 48, 16): [OFF, J(thick=3, thick_offset=2), J(ghosts=8, ghost_alpha=0.8), J(ghost_axis=1, ghosts=6, ghost_alpha=0.4), J(spike_amp=1.0, spike_k=(17, 0), spike_phase=1.0),
                   J(thick=4, thick_offset=1, ghost_axis=1, ghosts=4, ghost_alpha=0.9, spike_amp=0.5, spike_k=(63, 47), spike_phase=6.0)],
    # a single z: f > rz, one slab of one voxel, T is the identity there
    (16, 16, 1): [OFF, J(thick=4, thick_offset=2), J(ghosts=4, ghost_alpha=0.5), J(ghost_axis=1, ghosts=16 // 2, ghost_alpha=0.75), J(spike_amp=1.2, spike_k=(3, 13), spike_phase=3.0),
                  J(thick=2, thick_offset=1, ghosts=2, ghost_alpha=0.3, spike_amp=0.4, spike_k=(8, 8), spike_phase=0.0)],
    # lines of 520 voxels, longer than the 440 rows the ghost kernel holds on chip: the n terms come from memory (scalar along x: rz = 3; vector along y: rz = 4)
    (520, 4, 3): [OFF, J(thick=2), J(ghosts=8, ghost_alpha=0.8), J(ghost_axis=1, ghosts=2, ghost_alpha=0.5), J(spike_amp=1.0, spike_k=(519, 1), spike_phase=1.0),
                  J(thick=3, thick_offset=1, ghosts=4, ghost_alpha=1.0, spike_amp=0.5, spike_k=(7, 0), spike_phase=2.0)],
    (4, 520, 4): [OFF, J(thick=4, thick_offset=2), J(ghosts=2, ghost_alpha=0.8), J(ghost_axis=1, ghosts=8, ghost_alpha=0.5), J(spike_amp=1.0, spike_k=(1, 519), spike_phase=1.0),
                  J(thick=2, thick_offset=1, ghost_axis=1, ghosts=5, ghost_alpha=1.0, spike_amp=0.5, spike_k=(0, 77), spike_phase=2.0)],
}
SHAPES = [(6, 4, 3), (33, 17, 5), (64, 48, 16), (16, 16, 1)]


def run(src, jobs, scratch="auto", fill=None):
    """src [n, *roi] cuda; jobs: dicts with the fields of vsseg_acquisition_job -> dst [n, *roi] of ONE vsseg_patch_acquisition launch."""
    n, roi = src.shape[0], tuple(src.shape[1:])
    js = (L.AcquisitionJob * n)()
    for j, d in zip(js, jobs):
        j.thick, j.thick_offset, j.ghost_axis, j.ghosts, j.ghost_alpha = d["thick"], d["thick_offset"], d["ghost_axis"], d["ghosts"], float(d["ghost_alpha"])
        j.spike_amp, j.spike_k, j.spike_phase = float(d["spike_amp"]), (C.c_int32 * 2)(*d["spike_k"]), float(d["spike_phase"])
    staged = any(d["thick"] != 1 and (d["ghosts"] or d["spike_amp"] != 0.0) for d in jobs)
    sc = (torch.empty_like(src) if fill is None else torch.full_like(src, fill)) if (scratch == "auto" and staged) or scratch is True else None
    jb = torch.frombuffer(bytearray(bytes(js)), dtype=torch.uint8).cuda()
    dst = torch.empty_like(src)
    L.check(L.lib().vsseg_patch_acquisition(js, jb.data_ptr(), n, src.data_ptr(), dst.data_ptr(), sc.data_ptr() if sc is not None else None, L.i3(roi), torch.cuda.current_stream().cuda_stream), "patch_acquisition")
    return dst


def patches(shape, n, seed=3):
    return np.random.default_rng(seed).standard_normal((n, *shape)).astype(np.float32)


def check(got, v, job, what):
    """One job against the oracle; an artefact that does not move the patch by more than the tolerance would let a missing stage pass."""
    want, tol = QO.job(v, **job)
    if not job["ghosts"] and job["spike_amp"] == 0.0 and len(QO.slabs(v.shape[2], job["thick"], job["thick_offset"])) == v.shape[2]:  # thick slices alone, every slab one voxel (a single z): the identity, bit for bit
        print(f"{what}: the identity on this shape")
        np.testing.assert_array_equal(got, v)
        return
    err = np.abs(got.astype(np.float64) - want)
    moved = float(np.abs(want - v).max())
    print(f"{what}: max |device - oracle| {float(err.max()):.3e}, largest tolerance {float(np.max(tol)):.3e}, worst error / tolerance {float((err / tol).max()):.3f}; the artefact moves the patch by up to {moved:.3f}")
    assert np.isfinite(got).all() and moved > 0.01 and moved > 100 * float(np.max(tol))
    assert (err <= tol).all()


def name(job):
    return ", ".join(f"{k} {job[k]}" for k in job if not np.array_equal(job[k], OFF[k])) or "off"


@pytest.mark.parametrize("roi", list(SIX))
def test_six_jobs_of_one_launch_match_the_oracle_and_touch_only_their_own_patch(roi):
    jobs = SIX[roi]
    v = patches(roi, len(jobs))
    src = torch.from_numpy(v).cuda()
    dst = run(src, jobs)
    again = run(src, jobs)
    assert torch.equal(dst, again)  # two launches, the same bits
    got = dst.cpu().numpy()
    for j, job in enumerate(jobs):
        if job is OFF:
            assert torch.equal(dst[j], src[j])  # the off job is a copy
        else:
            check(got[j], v[j], job, f"roi {roi} job {j} ({name(job)})")
    # each job alone among sources and a scratch of 1e30: a read outside the job's own patch would show
    for j in range(len(jobs)):
        alone = torch.full_like(src, 1e30)
        alone[j] = src[j]
        out = run(alone, jobs, fill=1e30)
        assert torch.equal(out[j], dst[j]), (roi, j)


@pytest.mark.parametrize("roi", SHAPES)
def test_every_slab_height_with_every_offset(roi):
    jobs = [J(thick=f, thick_offset=o) for f in (2, 3, 4) for o in range(f)]
    v = patches(roi, len(jobs), seed=4)
    got = run(torch.from_numpy(v).cuda(), jobs, scratch=False).cpu().numpy()  # thick slices alone need no scratch
    for j, job in enumerate(jobs):
        check(got[j], v[j], job, f"roi {roi} f {job['thick']} o {job['thick_offset']}")
    const = run(torch.full((len(jobs), *roi), 1.75, device="cuda"), jobs, scratch=False)
    assert (const == 1.75).all()  # a constant column stays that constant, exactly: 1.75 k is exact for k <= 4


@pytest.mark.parametrize("roi,axis,n", [((6, 4, 3), 0, 3), ((64, 48, 16), 0, 8), ((64, 48, 16), 1, 6), ((16, 16, 1), 1, 2)])
def test_an_impulse_leaves_ghosts_at_multiples_of_the_shift(roi, axis, n):
    N, alpha = roi[axis], np.float32(0.8)
    s, i0 = N // n, 1
    v = np.zeros((1, *roi), np.float32)
    idx = [slice(None)] * 3
    idx[axis] = i0
    v[0][tuple(idx)] = 1.0
    got = run(torch.from_numpy(v).cuda(), [J(ghost_axis=axis, ghosts=n, ghost_alpha=alpha)]).cpu().numpy()[0].astype(np.float64)
    want, tol = QO.ghost(v[0], axis, n, alpha)
    line = np.moveaxis(got, axis, 0)
    expect = np.full(N, float(alpha) / N)  # alpha mu everywhere ...
    expect[(i0 + s * np.arange(n)) % N] -= float(alpha) / n  # ... the copies at i0 + j s with the weight -alpha / n ...
    expect[i0] += 1.0  # ... and the impulse itself
    tl = np.moveaxis(tol, axis, 0)
    err = np.abs(line - expect.reshape(-1, 1, 1))
    means = np.abs(line.mean(axis=0) - 1.0 / N)
    print(f"roi {roi} axis {axis} n {n}: ghosts at {sorted(((i0 + s * np.arange(n)) % N).tolist())}, max error {float(err.max()):.2e} (tolerance {float(tl.max()):.2e}), line means off by {float(means.max()):.2e} (bound {float(tl.mean(axis=0).max()):.2e})")
    assert (err <= tl).all() and float(alpha) / n > 100 * tl.max()
    assert (means <= tl.mean(axis=0)).all()  # the mean of every line is preserved within the mean of the bound


@pytest.mark.parametrize("roi,axis", [((6, 4, 3), 0), ((6, 4, 3), 1), ((16, 16, 1), 0)])
def test_as_many_ghosts_as_voxels_cancel_within_the_bound(roi, axis):
    """n = N: every copy of the line is subtracted with the weight alpha / N and the mean is put back, out = u - alpha (S / N - mu): the identity up to the bound, which
    is why no draw of it can be told from a missing stage and this test asserts the bound alone."""
    v = patches(roi, 2, seed=8)
    jobs = [J(ghost_axis=axis, ghosts=roi[axis], ghost_alpha=a) for a in (0.5, 1.0)]
    got = run(torch.from_numpy(v).cuda(), jobs).cpu().numpy()
    for j, job in enumerate(jobs):
        want, tol = QO.job(v[j], **job)
        err = np.abs(got[j].astype(np.float64) - want)
        print(f"roi {roi} axis {axis} n = N = {roi[axis]} alpha {job['ghost_alpha']}: max |device - oracle| {float(err.max()):.3e}, worst error / tolerance {float((err / tol).max()):.3f}, max |oracle - input| {float(np.abs(want - v[j]).max()):.1e}")
        assert (err <= tol).all() and np.abs(want - v[j]).max() < 1e-14


def test_cosf_error_against_fp64():
    """The figure behind QO.COS_ULP.  On a zero patch with amp = 1 the output is fmaf(1, cosf(theta), 0) = cosf(theta), the device library's cosf itself; rx = 64 and
    ry = 45 are coprime, so k = (1, 1) sends the 2880 voxels of a slice to the 2880 different arguments 2 pi t / 2880 + phase, which the host forms bit for bit
    (QO.spike_theta32).  Compared with cos in fp64 of that fp32 argument, never with another output of the kernel."""
    roi, phases = (64, 45, 4), (0.0, 1.0, 2.5, 4.0, 5.5, 6.2831)
    out = run(torch.zeros((len(phases), *roi), device="cuda"), [J(spike_amp=1.0, spike_k=(1, 1), spike_phase=p) for p in phases]).cpu().numpy()
    assert len(np.unique(QO.spike_t(roi, (1, 1)))) == 64 * 45
    worst, top = 0.0, 0.0
    for j, p in enumerate(phases):
        theta = QO.spike_theta32(roi, (1, 1), p)
        assert (out[j] == out[j][:, :, :1]).all()  # the same wave in every z
        ref = np.cos(theta.astype(np.float64))
        ulp = np.abs(out[j][:, :, 0].astype(np.float64) - ref) / np.spacing(np.maximum(np.abs(ref), 2.0 ** -126).astype(np.float32)).astype(np.float64)
        print(f"phase {p}: arguments in [{float(theta.min()):.4f}, {float(theta.max()):.4f}], max |cosf - cos64| = {float(ulp.max()):.3f} ulp over {theta.size} arguments")
        worst, top = max(worst, float(ulp.max())), max(top, float(theta.max()))
    print(f"cosf: measured {worst:.3f} ulp up to {top:.3f}; recorded {QO.COS_MEASURED_ULP} ulp, bar {QO.COS_ULP} ulp")
    assert top > 12.5  # up to 4 pi
    assert worst <= QO.COS_MEASURED_ULP * 1.25 + 0.25 and worst <= QO.COS_ULP  # the recorded figure still describes the library


# ---- PatchSampler ----
ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)
ACQ_ON = dict(thick_slices=4, ghost=0.8, spike=2.0)


@pytest.fixture(scope="module")
def cases():
    return [{"image": torch.from_numpy(np.array(AO.job_volume(k)[0])).cuda(), "label": torch.from_numpy(np.array(AO.job_volume(k)[1])).cuda()} for k in range(3)]


class CountingLib:
    """The sampler's library with every call counted by name."""

    def __init__(self, lib):
        self._lib, self.calls = lib, {}

    def __getattr__(self, name):
        fn = getattr(self._lib, name)

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*a)

        return counted


@pytest.mark.parametrize("mode", ["plain", "five"])
def test_patch_sampler_replays_through_the_oracle(cases, mode):
    roi, aug = AO.ROI, (ALL_ON if mode == "five" else {})
    s, twin = T.PatchSampler(cases, roi, 0.5, 7, **aug, **ACQ_ON, acquisition_prob=1.0), T.PatchSampler(cases, roi, 0.5, 7, **aug, **ACQ_ON, acquisition_prob=1.0)
    crop = T.PatchSampler(cases, roi, 0.5, 7, **aug)  # the same seed: the crop launch of `s`, relaunched from the same draws (checked below)
    other = T.PatchSampler(cases, roi, 0.5, 8, **aug, **ACQ_ON, acquisition_prob=1.0)
    s.lib = CountingLib(s.lib)
    worst, families = 0.0, np.zeros(3, int)
    for it, idx in enumerate(([0, 1], [2, 0], [1, 2])):
        img, lab = s.sample(idx)
        img2, lab2 = twin.sample(idx)
        assert torch.equal(img, img2) and torch.equal(lab, lab2)  # the same seed, the same bits ...
        assert not torch.equal(other.sample(idx)[0], img)  # ... another seed, another image
        cimg, clab = crop.sample(idx)
        assert s.last_draws == crop.last_draws and torch.equal(lab, clab)  # the label is the crop's
        assert img.shape == (2, 1, *roi) and s.acquisition_launches == it + 1 == s.lib.calls["vsseg_patch_acquisition"]
        v, got = cimg[:, 0].cpu().numpy(), img[:, 0].cpu().numpy()
        for b in range(2):
            a = s.last_augment[b]
            assert set(a) >= set(T.NEUTRAL_ACQUISITION) and (mode == "plain" or "m" in a)
            assert 1 <= a["thick"] <= 4 and a["ghosts"] in (0, 2, 4, 8) and 0.0 <= a["ghost_alpha"] <= np.float32(0.8) and 0.0 <= a["spike_amp"] <= 2.0 and a["ghost_alpha"].dtype == np.float32
            job = {k: a[k] for k in T.NEUTRAL_ACQUISITION}
            families += (a["thick"] != 1, a["ghosts"] != 0, a["spike_amp"] != 0.0)
            want, tol = QO.job(v[b], **job)
            err = np.abs(got[b] - want)
            worst = max(worst, float((err / tol).max()))
            assert (err <= tol).all(), (idx, b, float((err / tol).max()))
            assert np.abs(want - v[b]).max() > 100 * tol.max()
    print(f"PatchSampler replay ({mode}): worst error / tolerance {worst:.3f}; families hit over 6 samples {families}")
    assert (families >= 4).all()  # at probability 1 only a (0, 0) spike or an alpha of 0 is neutral


@pytest.mark.parametrize("mode", ["plain", "five"])
def test_zero_ranges_and_probability_zero_are_the_sampler_of_today(cases, mode):
    roi, aug = AO.ROI, (ALL_ON if mode == "five" else {})
    zero = T.PatchSampler(cases, roi, 0.5, 7, **aug, thick_slices=0, ghost=0.0, spike=0.0, acquisition_prob=1.0)
    p0 = T.PatchSampler(cases, roi, 0.5, 7, **aug, **ACQ_ON, acquisition_prob=0.0)
    today = T.PatchSampler(cases, roi, 0.5, 7, **aug)
    for s in (zero, p0, today):
        s.lib = CountingLib(s.lib)
    for idx in ([0, 1], [2, 1, 0]):
        i0, l0 = today.sample(idx)
        for s in (zero, p0):
            i1, l1 = s.sample(idx)
            assert torch.equal(i0, i1) and torch.equal(l0, l1) and s.last_draws == today.last_draws
            assert len(s.last_augment) == len(today.last_augment) and all("thick" not in a and "ghosts" not in a for a in s.last_augment)
            assert s.acquisition_launches == 0 and s._acquisition_scratch is None and not s.acquiring
            assert s.lib.calls == today.lib.calls and "vsseg_patch_acquisition" not in s.lib.calls  # launch for launch


def test_a_batch_in_which_nothing_is_hit_issues_no_launch(cases):
    roi = AO.ROI
    s, crop = T.PatchSampler(cases, roi, 0.5, 21, **ACQ_ON, acquisition_prob=0.3), T.PatchSampler(cases, roi, 0.5, 21)
    hit = missed = 0
    for it in range(12):
        idx = [it % 3]
        before = s.acquisition_launches
        img, _ = s.sample(idx)
        cimg, _ = crop.sample(idx)
        a = s.last_augment[0]
        if a["thick"] != 1 or a["ghosts"] or a["spike_amp"] != 0.0:
            hit += 1
            assert s.acquisition_launches == before + 1 and not torch.equal(img, cimg)
        else:
            missed += 1
            assert s.acquisition_launches == before and torch.equal(img, cimg)
    print(f"P = 0.3 over 12 batches of one: {hit} with a launch, {missed} without")
    assert hit > 0 and missed > 0


# ---- the driver ----
def test_training_epoch_with_the_acquisition_flags(tmp_path, monkeypatch):
    """`VSparams --debug --num_epochs 1` with the four new flags, over the synthetic debug cases of tools/make_debug_data.py."""
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
            "--aug_thick_slices", "4", "--aug_ghost", "0.8", "--aug_spike", "2.0", "--aug_acquisition_prob", "0.75"]
    p = VSparams(argparse.ArgumentParser(), argv)
    p.create_results_folders()
    p.set_up_logger("training_log.txt")
    p.log_parameters()
    train_files, val_files, _ = p.load_T1_or_T2_data()
    ttf, vtf, _ = p.get_transforms()
    train_loader, val_loader = p.cache_transformed_train_data(train_files, ttf), p.cache_transformed_val_data(val_files, vtf)
    assert train_loader.sampler.acquiring and not train_loader.sampler.appearing and not val_loader.sampler.acquiring and not val_loader.sampler.tail.acquiring
    model, loss_fn = p.set_and_get_model(), p.set_and_get_loss_function()
    losses, _ = p.run_training_algorithm(model, loss_fn, p.set_and_get_optimizer(model), train_loader, val_loader)
    print(f"epoch loss with the acquisition families: {losses}")
    assert len(losses) == 1 and np.isfinite(losses[0])
    last = train_loader.sampler.last_augment
    assert len(last) >= 1 and set(last[0]) >= set(T.NEUTRAL_ACQUISITION) and 1 <= last[0]["thick"] <= 4
    assert train_loader.sampler.acquisition_launches >= 1 and val_loader.sampler.acquisition_launches == 0
    for h in p.logger.handlers:
        h.flush()
    log = open(os.path.join(p.logs_path, "training_log.txt")).read()
    for k in T.ACQUISITION_KEYS:
        assert "aug_" + k + " =" in log
    assert "epoch 1 average loss" in log
