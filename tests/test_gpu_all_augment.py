"""-m gpu: all four augmentation families on at once through PatchSampler, at the ROI of the per-family replay tests, a batch of 2, probability 1.  The result is that of
a twin sampler bit for bit, the launches come in the order crop, acquisition, filter, tone, and every stage is what its family's oracle makes of the stage before it,
fed from `last_augment` and under the tolerance its own test states (tests/test_gpu_field_augment.py, test_gpu_acquisition_augment.py, test_gpu_appearance_augment.py,
whose helpers and settings this test borrows; it has no tolerance of its own)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import acquisition_oracle as QO  # noqa: E402
from tests import appearance_oracle as PO  # noqa: E402
from tests import augment_oracle as AO  # noqa: E402
from tests import field_oracle as FO  # noqa: E402
from tests import test_gpu_acquisition_augment as QT  # noqa: E402
from tests import test_gpu_appearance_augment as PT  # noqa: E402
from tests import test_gpu_field_augment as FT  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402


class OrderLib:
    """Passes every call on and keeps the names in the order they came."""

    def __init__(self, lib):
        self.lib, self.order = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)

        def called(*a):
            self.order.append(name)
            return fn(*a)

        return called


def test_all_four_families_at_once_replay_stage_by_stage():
    rng = np.random.default_rng(1)
    host = [(rng.standard_normal(shape).astype(np.float32), (rng.random(shape) > 0.9).astype(np.float32)) for shape in ((40, 36, 20), (33, 50, 16), (64, 64, 24))]
    dev = [{"image": torch.from_numpy(v).cuda(), "label": torch.from_numpy(l).cuda()} for v, l in host]
    roi, idx = AO.ROI, [0, 2]
    on = dict(FT.ALL_ON, **FT.FIELD_ON, **PT.APP_ON, appearance_prob=1.0, **QT.ACQ_ON, acquisition_prob=1.0)
    s, twin = T.PatchSampler(dev, roi, 0.5, 7, **on), T.PatchSampler(dev, roi, 0.5, 7, **on)
    crop = T.PatchSampler(dev, roi, 0.5, 7, **FT.ALL_ON, **FT.FIELD_ON)  # the same seed: the crop launch of `s`, relaunched from the same draws (checked below)
    s.lib = OrderLib(s.lib)
    img, lab = s.sample(idx)
    img2, lab2 = twin.sample(idx)
    assert torch.equal(img, img2) and torch.equal(lab, lab2)  # the same seed, the same bits
    assert s.lib.order == ["vsseg_crop_field", "vsseg_patch_acquisition", "vsseg_patch_filter", "vsseg_patch_tone"] and s.acquisition_launches == 1
    assert img.shape == (2, 1, *roi) and lab.shape == img.shape and s.last_tone_stats.shape == (2, 4)
    cimg, clab = crop.sample(idx)
    PT.same_crop_jobs(s, crop)
    assert torch.equal(lab, clab)  # the label is the crop's
    # the device's own acquisition and filter stages, job for job as the sampler recorded them; they are deterministic, so these ARE what the next launch read
    acq = QT.run(cimg[:, 0].contiguous(), [{k: a[k] for k in T.NEUTRAL_ACQUISITION} for a in s.last_augment])
    filt, _ = PT.run_filter(acq, [(a["blur_taps"], a["coarse"]) for a in s.last_augment])
    c, q, f, got, stats, labels = cimg[:, 0].cpu().numpy(), acq.cpu().numpy(), filt.cpu().numpy(), img[:, 0].cpu().numpy(), s.last_tone_stats.cpu().numpy(), lab[:, 0].cpu().numpy()
    worst = np.zeros(4)
    for b, i in enumerate(idx):
        a = s.last_augment[b]
        # crop: elastic field, matrix, bias field, gain, bias and noise from the cached volume (the sum of tests/test_gpu_field_augment.py's sampler replay)
        mag, blog, g, o, std = (float(a[k]) for k in ("elastic_mag", "bias_log", "gain", "bias", "noise_std"))
        co = FO.coords(a["m"], roi, a["spacing"], mag, b, a["seed"])
        cd = FO.coord_delta(co, a["m"], mag, roi)
        t, e = AO.trilinear(host[i][0], co), np.exp(blog * FO.fields(roi, a["spacing"], b, a["seed"])[2])
        want = t * e * g + o + std * AO.normals(roi, b, a["seed"])
        tol = FO.trilinear_tolerance(host[i][0], co, cd) * e * abs(g) + np.abs(t * e * g) * (FT.EXP_REL + FO.field_delta(blog) + 2.0 * FT.EPS) + 2.0 * FT.EPS * (np.abs(t * e * g) + abs(o)) + FT.NOISE_TOL * std
        err = [(np.abs(c[b] - want), tol)]
        band, differ = FO.rounding_band(co, cd), labels[b] != AO.nearest(host[i][1], co)
        assert band.sum() <= 1e-3 * band.size and not (differ & ~band).any()
        # acquisition on the crop, filter on the acquisition, tone on the filter
        want, tol = QO.job(c[b], **{k: a[k] for k in T.NEUTRAL_ACQUISITION})
        err.append((np.abs(q[b] - want), tol))
        assert a["thick"] != 1 and np.abs(want - c[b]).max() > 100 * tol.max()  # at probability 1 a slab height of 2..4 is always drawn
        want, tol = PO.filter_job(q[b], a["blur_taps"], a["coarse"])
        err.append((np.abs(f[b] - want), tol))
        assert len(a["blur_taps"]) > 1 and np.abs(want - q[b]).max() > 0.05
        PT.check_stats(stats[b], f[b], f"all four, sample {b}")
        want, tol = PO.tone(f[b], a["contrast"], a["gamma"], stats[b])
        err.append((np.abs(got[b] - want), tol))
        ratio = [float((x / np.maximum(tol, 1e-300)).max()) for x, tol in err]
        worst = np.maximum(worst, ratio)
        print(f"sample {b}: worst error / tolerance: crop {ratio[0]:.3f}, acquisition {ratio[1]:.3f}, filter {ratio[2]:.3f}, tone {ratio[3]:.3f}")
        assert all((x <= tol).all() for x, tol in err), (b, ratio)
    print(f"all four families, batch of 2: worst error / tolerance per stage (crop, acquisition, filter, tone) {worst.round(3).tolist()}")
