"""CPU tests of the appearance augmentation (blur, low resolution, contrast, gamma): the range checks, the RNG layout of RandomTail (a fifth state: nothing else
moves), the host-side derived quantities (taps, coarse sizes), the properties of the oracle in tests/appearance_oracle.py, the command-line flags, and the argument
checks of vsseg_patch_filter / vsseg_patch_tone (made before any launch, so they are the same on a machine without a GPU)."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import appearance_oracle as PO
from vs_seg_amd import _lib as L
from vs_seg_amd.data import transforms as T

ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)
FIELD_ON = dict(elastic_mag=4.0, bias_field=0.3, field_spacing=16)
APP_ON = dict(blur_sigma=1.5, lowres=0.5, contrast=0.25, gamma=0.3, appearance_prob=0.5)
NEUTRAL = (0.0, 1.0, 1.0, 1.0)


def test_check_appearance_augment():
    assert T.APPEARANCE_KEYS == ("blur_sigma", "lowres", "contrast", "gamma", "appearance_prob")
    assert T.check_appearance_augment() == dict(blur_sigma=0.0, lowres=0.0, contrast=0.0, gamma=0.0, appearance_prob=0.25)
    assert T.check_appearance_augment(1.5, 0.25, 0.99, 0.99, 1.0) == dict(blur_sigma=1.5, lowres=0.25, contrast=0.99, gamma=0.99, appearance_prob=1.0)
    assert T.check_appearance_augment(0.01, 0.999, 0.0, 0.0, 0.0)["appearance_prob"] == 0.0
    nan, inf = float("nan"), float("inf")
    for bad in ((1.51, 0, 0, 0), (-0.1, 0, 0, 0), (nan, 0, 0, 0), (inf, 0, 0, 0), (0, 0.24, 0, 0), (0, 1.0, 0, 0), (0, 1.5, 0, 0), (0, -0.5, 0, 0), (0, nan, 0, 0), (0, 0, 1.0, 0), (0, 0, -0.1, 0),
                (0, 0, nan, 0), (0, 0, inf, 0), (0, 0, 0, 1.0), (0, 0, 0, -0.1), (0, 0, 0, nan), (0, 0, 0, 0, -0.01), (0, 0, 0, 0, 1.01), (0, 0, 0, 0, nan), (0, 0, 0, 0, inf)):
        with pytest.raises(ValueError):
            T.check_appearance_augment(*bad)
    with pytest.raises(ValueError):
        T.RandomTail((8, 8, 8), 0.5, 0, blur_sigma=2.0)
    assert T.AUGMENT_KEYS == ("rotate_deg", "scale", "intensity_scale", "intensity_shift", "noise_std") and T.FIELD_KEYS == ("elastic_mag", "bias_field", "field_spacing")  # unchanged


@pytest.mark.parametrize("seed", [0, 7, 123])
@pytest.mark.parametrize("flip_prob", [0.5, None])
@pytest.mark.parametrize("five,field", [(False, False), (True, False), (False, True), (True, True)])
def test_the_fifth_random_state_leaves_the_other_draws_unchanged(seed, flip_prob, five, field):
    roi, aug = (32, 32, 16), dict(ALL_ON if five else {}, **(FIELD_ON if field else {}))
    off, zeros, on = T.RandomTail(roi, flip_prob, seed, **aug), T.RandomTail(roi, flip_prob, seed, **aug, blur_sigma=0.0, lowres=0.0, contrast=0.0, gamma=0.0, appearance_prob=1.0), T.RandomTail(roi, flip_prob, seed, **aug, **APP_ON)
    assert not off.appearing and not zeros.appearing and zeros._appR is None and on.appearing and on.augmenting == five and on.fielding == field
    assert zeros.draw_appearance() == NEUTRAL
    seen = set()
    for shape in [(40, 36, 20), (33, 50, 16), (64, 64, 24), (32, 32, 16)] * 6:
        assert on.draw_noise_seed() == off.draw_noise_seed() and on.draw_field_seed() == off.draw_field_seed()
        assert on.draw(shape) == off.draw(shape)
        if five:
            assert on.draw_augment() == off.draw_augment()
        if field:
            assert on.draw_field() == off.draw_field()
        seen.add(on.draw_appearance())
    assert len(seen) > 12
    # the layout: the appearance state is seeded by the next randint of RandomState(seed) after the flip's, the crop's, the augmentation's and the field's
    R = np.random.RandomState(seed)
    for _ in range((flip_prob is not None) + 1 + five + field):
        R.randint(T.MAX_SEED, dtype="uint32")
    assert T.RandomTail(roi, flip_prob, seed, **aug, **APP_ON)._appR.randint(1 << 30) == np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32")).randint(1 << 30)


def test_a_family_with_range_zero_draws_nothing():
    roi = (8, 8, 8)
    one = T.RandomTail(roi, 0.5, 3, contrast=0.25, appearance_prob=1.0)
    two = T.RandomTail(roi, 0.5, 3, blur_sigma=1.0, contrast=0.25, appearance_prob=1.0)
    only = [one.draw_appearance() for _ in range(4)]
    assert all(d[0] == 0.0 and d[1] == 1.0 and d[3] == 1.0 and d[2] != 1.0 for d in only)
    both = [two.draw_appearance() for _ in range(2)]  # (hit, sigma, hit, c) per sample: the same stream, consumed twice as fast
    R = np.random.RandomState(3)
    for _ in range(2):
        R.randint(T.MAX_SEED, dtype="uint32")
    S = np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32"))
    raw = [(S.random_sample(), S.uniform(0.75, 1.25)) for _ in range(4)]
    assert [d[2] for d in only] == [v for _, v in raw]  # hit and value, hit and value
    assert both[0][0] != 0.0 and both[0][2] != 1.0 and both[0][1] == 1.0 and both[0][3] == 1.0
    # the stream position does not depend on the outcome: with P = 0 nothing is hit, and the state has moved exactly as far
    miss, hit = T.RandomTail(roi, 0.5, 3, **dict(APP_ON, appearance_prob=0.0)), T.RandomTail(roi, 0.5, 3, **dict(APP_ON, appearance_prob=1.0))
    for _ in range(5):
        assert miss.draw_appearance() == NEUTRAL and hit.draw_appearance() != NEUTRAL
    assert miss._appR.randint(1 << 30) == hit._appR.randint(1 << 30)


def test_every_draw_lies_in_its_interval_and_a_miss_is_neutral():
    tail = T.RandomTail((8, 8, 8), 0.5, 11, **APP_ON)
    hits = np.zeros(4, int)
    for _ in range(400):
        s, f, c, g = tail.draw_appearance()
        assert s == 0.0 or 0.75 <= s <= 1.5
        assert f == 1.0 or 0.5 <= f < 1.0
        assert c == 1.0 or 0.75 <= c <= 1.25
        assert g == 1.0 or 0.7 <= g <= 1.3
        hits += (s != 0.0, f != 1.0, c != 1.0, g != 1.0)
    print(f"hits of 400 at P = 0.5: {hits}")
    assert (hits > 150).all() and (hits < 250).all()  # 200 +- 5 standard deviations


@pytest.mark.parametrize("sigma", [0.25, 0.5, 1.0, 1.5])
def test_taps(sigma):
    w = T.blur_taps(sigma)
    assert w.dtype == np.float32 and len(w) == int(np.ceil(3 * sigma)) + 1 <= 6 and PO.radius(sigma) == len(w) - 1
    np.testing.assert_array_equal(w, PO.taps(sigma))
    total = float(w[0]) + 2.0 * float(w[1:].astype(np.float64).sum())
    print(f"sigma {sigma}: R = {len(w) - 1}, taps {w}, w_0 + 2 sum w_k - 1 = {total - 1.0:.2e}")
    assert abs(total - 1.0) <= (2 * len(w) - 1) * 2.0 ** -25  # each of the 2R + 1 taps is rounded once, and is below 1
    assert (np.diff(w) < 0).all() and (w > 0).all()
    np.testing.assert_allclose(w[1] / w[0], np.exp(-1.0 / (2.0 * sigma * sigma)), rtol=2e-7)
    assert len(T.blur_taps(0.0)) == 0


def test_coarse_sizes_and_sample_positions_cover_the_axis():
    assert T.coarse_size((384, 128, 128), 0.5) == (192, 64) and T.coarse_size((7, 5, 3), 0.25) == (2, 1) and T.coarse_size((3, 3, 9), 0.1) == (1, 1)
    assert T.coarse_size((33, 17, 5), 1.0) == (33, 17) and T.coarse_size((33, 17, 5), 0.99) == (33, 17)  # rounds to the roi: off for that sample
    for roi in (1, 5, 7, 16, 33, 64, 384):
        for f in (0.25, 0.4, 0.5, 0.77, 0.999, 1.0):
            n = T.coarse_size((roi, roi, 1), f)[0]
            assert n == PO.coarse_size((roi, roi, 1), f)[0] == max(1, int(np.floor(roi * f + 0.5))) and 1 <= n <= roi
            q = PO.q_index(n, roi)
            assert len(q) == n and q[0] >= 0 and q[-1] < roi and (np.diff(q) >= 1).all()  # strictly increasing inside [0, roi)
            assert q[0] == roi // (2 * n) and abs((q[0] + 0.5) - roi / (2.0 * n)) <= 0.5  # the centre of the first coarse cell
        np.testing.assert_array_equal(PO.q_index(roi, roi), np.arange(roi))


def test_reflection():
    np.testing.assert_array_equal(PO.reflect(np.arange(-7, 10), 3), [0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2, 1, 0, 0, 1, 2, 2])
    np.testing.assert_array_equal(PO.reflect(np.arange(-3, 4), 1), 0)


@pytest.mark.parametrize("shape", [(7, 5, 3), (33, 17, 5), (16, 16, 1)])
@pytest.mark.parametrize("sigma", [0.5, 1.5])
def test_separable_blur_equals_the_direct_sum_over_a_symmetric_pad(shape, sigma):
    rng = np.random.default_rng(5)
    v, w = rng.standard_normal(shape), PO.taps(sigma)
    R = len(w) - 1
    full = np.concatenate([w[:0:-1], w]).astype(np.float64)
    pad = np.pad(v, ((R, R), (R, R), (0, 0)), mode="symmetric")  # numpy repeats the reflection where the roi is shorter than R: the same period 2n
    for a, n in enumerate(shape[:2]):
        np.testing.assert_array_equal(np.take(pad, np.arange(n + 2 * R), axis=a), np.take(np.take(pad, np.arange(R, R + n), axis=a), PO.reflect(np.arange(-R, n + R), n), axis=a))
    direct = np.zeros(shape)
    for a in range(2 * R + 1):
        for b in range(2 * R + 1):
            direct += full[a] * full[b] * pad[a:a + shape[0], b:b + shape[1]]
    err = float(np.abs(PO.blur(v, w) - direct).max())
    print(f"{shape} sigma {sigma}: max |separable - direct| {err:.2e}")
    assert err < 1e-14


def test_blur_of_a_constant_is_that_constant_and_its_tolerance_is_a_few_eps():
    for sigma in (0.25, 0.5, 1.0, 1.5):
        w = PO.taps(sigma)
        c = np.full((7, 5, 3), 3.25)
        total = float(w[0]) + 2.0 * float(w[1:].astype(np.float64).sum())
        assert np.abs(PO.blur(c, w) - 3.25 * total * total).max() < 1e-14 and abs(total * total - 1.0) < 1e-6
        tol = PO.blur_tolerance(c, w)
        assert (tol > 0).all() and tol.max() < 2.1 * (2 * len(w) - 1) * PO.EPS * 3.25 * 1.001


def test_low_resolution_at_full_size_is_the_identity():
    rng = np.random.default_rng(6)
    v = rng.standard_normal((33, 17, 5))
    np.testing.assert_array_equal(PO.lowres(v, (33, 17)), v)
    half = PO.lowres(v, (16, 17))  # one axis only: y is untouched, x is piecewise linear between the samples
    q = PO.q_index(16, 33)
    np.testing.assert_allclose(half[q[3]], v[q[3]], atol=0.3 * np.abs(v).max())  # not exact: output q lies near, not on, coarse sample 3
    assert np.abs(half - v).max() > 0.1
    out, tol = PO.filter_job(v, None, (33, 17))
    assert out is not None and np.array_equal(out, v) and tol == 0.0
    assert PO.lowres(np.full((9, 9, 2), 2.5), (3, 4)).tolist() == np.full((9, 9, 2), 2.5).tolist()  # a constant stays that constant
    ramp = np.arange(64, dtype=np.float64)[:, None, None] * np.ones((1, 4, 1))
    lr = PO.lowres(ramp, (16, 4))  # a ramp is reproduced between the first and the last coarse sample, up to the offset of the sample positions (q + 0.5 = cell centre)
    assert np.abs(lr[2:-2] - ramp[2:-2]).max() <= 0.5 + 1e-12 and lr.min() == PO.q_index(16, 64)[0] and lr.max() == PO.q_index(16, 64)[-1]


def test_tone_oracle_properties():
    rng = np.random.default_rng(7)
    x = rng.standard_normal(4096).astype(np.float32)
    stats = (x.min(), x.max(), np.float32(x.astype(np.float64).mean()), 0.0)
    y, tol, clamped = PO.contrast(x, 1.25, stats)
    frac = clamped.mean()
    print(f"c = 1.25 on a standard normal: {int(clamped.sum())} of {x.size} voxels clamped")
    assert clamped.sum() >= 1 and frac <= 0.5 and y.min() == x.min() and y.max() == x.max()  # the range is preserved
    y, _, clamped = PO.contrast(x, 0.75, stats)
    assert not clamped.any() and y.min() > x.min() and y.max() < x.max()
    out, tol = PO.tone(x, 1.0, 1.0, stats)
    assert np.array_equal(out, x) and not tol.any()
    for g in (0.7, 1.5):
        out, tol = PO.tone(x, 1.0, g, stats)
        assert abs(out.min() - x.min()) < 1e-6 and abs(out.max() - x.max()) < 1e-5 and np.isfinite(tol).all() and tol.max() < 1e-4  # gamma keeps the range
        assert ((out > x) if g < 1 else (out < x))[(x > x.min()) & (x < x.max())].all()
    for n in PO.TONE_SIZES:  # the inputs of the GPU test: the reference alone says that c = 1.25 clamps at least one voxel and at most half of them
        xs = PO.tone_input(n)
        for x, (c, g) in zip(xs, PO.TONE_JOBS):
            clamped = PO.contrast(x, c, (x.min(), x.max(), np.float32(x.astype(np.float64).mean()), 0.0))[2]
            assert (1 <= clamped.sum() <= n // 2) if c > 1.0 else not clamped.any()
    const = np.full(64, 2.5, np.float32)
    out, tol = PO.tone(const, 1.25, 0.7, (2.5, 2.5, 2.5, 0.0))
    assert (out == 2.5).all() and np.isfinite(tol).all()
    assert PO.mean_bound(1000.0) == 2.0 ** -14 and PO.POW_ULP >= 2.0


def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


FLAGS = ["--aug_rotate_deg", "15", "--aug_scale", "0.1", "--aug_intensity_scale", "0.1", "--aug_intensity_shift", "0.1", "--aug_noise_std", "0.05"]
APP_FLAGS = ["--aug_blur_sigma", "1.5", "--aug_lowres", "0.5", "--aug_contrast", "0.25", "--aug_gamma", "0.3", "--aug_appearance_prob", "0.5"]


def test_command_line_flags_default_to_off_and_reject_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    assert [ap.get_default("aug_" + k) for k in T.APPEARANCE_KEYS] == [0.0, 0.0, 0.0, 0.0, 0.25]
    for bad in (["--aug_blur_sigma", "1.6"], ["--aug_blur_sigma", "-1"], ["--aug_blur_sigma", "nan"], ["--aug_lowres", "0.2"], ["--aug_lowres", "1"], ["--aug_lowres", "inf"], ["--aug_contrast", "1"],
                ["--aug_contrast", "-0.5"], ["--aug_gamma", "1.0"], ["--aug_gamma", "nan"], ["--aug_appearance_prob", "1.5"], ["--aug_appearance_prob", "-0.1"], ["--aug_gamma", "x"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], APP_FLAGS, ["--aug_blur_sigma", "1.5"], ["--aug_lowres", "0.25"], ["--aug_contrast", "0.99"], ["--aug_gamma", "0.5", "--aug_appearance_prob", "1"], ["--aug_appearance_prob", "0"]):
        p = _parse(good)
        if p is not None:
            assert p.aug_blur_sigma == (1.5 if "--aug_blur_sigma" in good else 0.0)


def test_flags_reach_the_training_chain_only(monkeypatch):
    """get_transforms needs no device: build the object past the device check."""
    import torch
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    keys = tuple("aug_" + k for k in T.APPEARANCE_KEYS)
    for argv, five, on in (([], False, False), (APP_FLAGS, False, True), (FLAGS + APP_FLAGS, True, True), (FLAGS, True, False), (["--aug_appearance_prob", "0.9"], False, False)):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        train, val, test = p.get_transforms()
        text = lambda tf: " ".join(tf["chain"])  # noqa: E731
        for k in keys[:4]:
            assert (k in text(train)) == on
            assert k not in text(val) and k not in text(test)
        assert "appearance_augment" not in val and "appearance_augment" not in test
        assert train["appearance_augment"] == p.appearance_augment and set(train["appearance_augment"]) == set(T.APPEARANCE_KEYS)
        if on:
            assert train["appearance_augment"] == APP_ON
            assert text(train).index("aug_blur_sigma") < text(train).index("aug_lowres") < text(train).index("aug_contrast") < text(train).index("aug_gamma")  # the order they are applied in
        assert set(train["augment"]) == set(T.AUGMENT_KEYS) and set(train["field_augment"]) == set(T.FIELD_KEYS)
        tail = T.RandomTail(train["roi"], train["flip_prob"], 0, **train["augment"], **train["field_augment"], **train["appearance_augment"])
        assert tail.appearing == on and tail.augmenting == five and not tail.fielding
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        p.log_parameters()
        for k in keys:
            assert any(k in ln for ln in lines) == on
    p = P.VSparams(argparse.ArgumentParser(), ["--aug_gamma", "0.2"])  # one family alone
    assert "aug_gamma" in " ".join(p.get_transforms()[0]["chain"]) and "aug_blur_sigma" not in " ".join(p.get_transforms()[0]["chain"])


def _fake_pointer():
    mem = ctypes.create_string_buffer(512)
    return mem, (ctypes.addressof(mem) + 15) & ~15


def test_patch_filter_rejects_bad_arguments_before_the_launch():
    """Fake device addresses: every call below is refused before anything is launched, the job records are read from the host copy."""
    lib = L.lib()
    assert lib.vsseg_version() >= 13 and ctypes.sizeof(L.FilterJob) == 36
    mem, ptr = _fake_pointer()
    roi = (8, 6, 4)
    w = T.blur_taps(1.0)

    def jobs(n=2, **kw):
        js = (L.FilterJob * n)()
        for i in range(n):
            js[i].radius, js[i].taps, js[i].coarse = len(w) - 1, (ctypes.c_float * 6)(*w.tolist()), (ctypes.c_int32 * 2)(8, 6)
        for k, v in kw.items():  # the LAST job is the bad one: every record is checked
            if k.startswith("w") and k[1:].isdigit():
                js[n - 1].taps[int(k[1:])] = v
            else:
                setattr(js[n - 1], k, v)
        return js

    def refused(why, js=None, dev=ptr, n=2, src=ptr, dst=ptr + 64, scratch=ptr + 128, r=roi):
        rc = lib.vsseg_patch_filter(js if js is not None else jobs(n if n > 0 else 1), dev, n, src, dst, scratch, L.i3(r) if r is not None else None, None)
        err = lib.vsseg_last_error()
        assert rc == L.EINVAL and b"vsseg_patch_filter" in err and why in err, (why, rc, err)

    refused(b"null", js=ctypes.POINTER(L.FilterJob)())
    refused(b"null", dev=None)
    refused(b"null", src=None)
    refused(b"null", dst=None)
    refused(b"null", r=None)
    refused(b"src == dst", dst=ptr)
    refused(b"njobs", n=0)
    refused(b"njobs", n=-3)
    for r in ((0, 6, 4), (8, -1, 4), (8, 6, 0)):
        refused(b"roi", r=r)
    refused(b"misaligned", dst=ptr + 68)
    refused(b"misaligned", src=ptr + 4)
    for radius in (-1, 6, 100):
        refused(b"radius", js=jobs(radius=radius))
    for bad in (float("nan"), float("inf"), -float("inf")):
        for k in ("w0", "w2", "w3"):
            refused(b"non-finite taps", js=jobs(**{k: bad}))
    refused(b"not normalised", js=jobs(w0=float(w[0]) + 3e-5))
    refused(b"not normalised", js=jobs(w3=float(w[3]) - 2e-5))
    refused(b"not normalised", js=jobs(radius=2))  # the taps of radius 3, cut short
    for coarse in ((0, 6), (9, 6), (8, 0), (8, 7), (-2, 3)):
        refused(b"coarse", js=jobs(coarse=(ctypes.c_int32 * 2)(*coarse)))
    refused(b"scratch must not be null", js=jobs(coarse=(ctypes.c_int32 * 2)(4, 3)), scratch=None)  # blur and low resolution in one job


def test_patch_tone_rejects_bad_arguments_before_the_launch():
    lib = L.lib()
    assert ctypes.sizeof(L.ToneJob) == 8 and L.TONE_SHARDS == 128
    mem, ptr = _fake_pointer()

    def jobs(n=2, **kw):
        js = (L.ToneJob * n)()
        for i in range(n):
            js[i].contrast, js[i].gamma = 1.25, 0.7
        for k, v in kw.items():
            setattr(js[n - 1], k, v)
        return js

    def refused(why, js=None, dev=ptr, n=2, x=ptr, count=100, stats=ptr + 64, work=ptr + 128):
        rc = lib.vsseg_patch_tone(js if js is not None else jobs(n if n > 0 else 1), dev, n, x, count, stats, work, None)
        err = lib.vsseg_last_error()
        assert rc == L.EINVAL and b"vsseg_patch_tone" in err and why in err, (why, rc, err)

    refused(b"null", js=ctypes.POINTER(L.ToneJob)())
    for k in ("dev", "x", "stats", "work"):
        refused(b"null", **{k: None})
    refused(b"njobs", n=0)
    refused(b"njobs", n=-1)
    refused(b"n = 0", count=0)
    refused(b"n = -5", count=-5)
    for field in ("contrast", "gamma"):
        for bad in (float("nan"), float("inf"), -float("inf"), 0.0, -0.5, 2.0, 3.0):
            refused(field.encode(), js=jobs(**{field: bad}))
