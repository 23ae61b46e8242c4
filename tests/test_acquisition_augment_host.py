"""CPU tests of the acquisition augmentation (thick slices, ghosting, spike): the image-space forms of the contract against their k-space definitions through numpy.fft,
the properties of the thick-slice stage, the range checks, the RNG layout of RandomTail (a sixth state: nothing else moves), the command-line flags, and the argument
checks of vsseg_patch_acquisition (made before any launch, so they are the same on a machine without a GPU)."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import acquisition_oracle as QO
from vs_seg_amd import _lib as L
from vs_seg_amd.data import transforms as T

ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)
FIELD_ON = dict(elastic_mag=4.0, bias_field=0.3, field_spacing=16)
APP_ON = dict(blur_sigma=1.5, lowres=0.5, contrast=0.25, gamma=0.3, appearance_prob=0.5)
ACQ_ON = dict(thick_slices=4, ghost=0.8, spike=2.0, acquisition_prob=0.5)


def same_job(a, b):
    return set(a) == set(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ---- the image-space forms are the k-space definitions ----
@pytest.mark.parametrize("N,n", [(6, 2), (6, 3), (24, 8), (33, 3)])
@pytest.mark.parametrize("axis", [0, 1])
def test_ghosting_in_image_space_is_the_scaled_kspace_lines(N, n, axis):
    rng = np.random.default_rng(N * 10 + n)
    shape = (N, 5, 3) if axis == 0 else (5, N, 3)
    u = rng.standard_normal(shape)
    for alpha in (0.25, 1.0):
        got, tol = QO.ghost(u, axis, n, alpha)
        want = QO.ghost_kspace(u, axis, n, alpha)
        err = float(np.abs(got - want).max())
        print(f"N {N} n {n} axis {axis} alpha {alpha}: max |image space - k-space| {err:.2e}; the ghosts move the patch by up to {float(np.abs(got - u).max()):.3f}")
        assert err < 1e-13 and np.abs(got - u).max() > 0.01
        np.testing.assert_allclose(got.mean(axis=axis), u.mean(axis=axis), atol=1e-14)  # the mean of every line is preserved
        assert (tol > 0).all() and tol.max() < 64 * QO.EPS * np.abs(u).max()
    const = np.full(shape, 2.5)
    got, tol = QO.ghost(const, axis, n, 0.7)
    assert np.abs(got - 2.5).max() < 1e-14 and tol.max() < 32 * QO.EPS * 2.5  # a constant line stays, and the bound stays a few eps of it
    with pytest.raises(AssertionError):
        QO.ghost(u, axis, 4 if N % 4 else 5, 0.5)  # n must divide N


@pytest.mark.parametrize("k", [(1, 0), (0, 3), (5, 7), (6, 0), (6, 5), (11, 9)])
def test_spike_in_image_space_is_the_pair_of_kspace_points(k):
    rng = np.random.default_rng(sum(k))
    w = rng.standard_normal((12, 10, 2))
    for amp, phase in ((1.5, 0.0), (0.3, 2.0), (2.0, 6.0)):
        got, tol = QO.spike(w, amp, k, phase)
        want = QO.spike_kspace(w, float(np.float32(amp)), k, float(np.float32(phase)))
        err = float(np.abs(got - want).max())
        print(f"k {k} amp {amp} phase {phase}: max |image space - k-space| {err:.2e}")
        assert err < 1e-13 and np.abs(got - w).max() > 0.1 * amp
        assert np.array_equal(got[:, :, 0] - w[:, :, 0], got[:, :, 1] - w[:, :, 1]) or np.allclose(got[:, :, 0] - w[:, :, 0], got[:, :, 1] - w[:, :, 1], atol=1e-15)  # the same wave in every z slice
        assert (tol > 0).all() and tol.max() < (64 + 2 * QO.COS_ULP) * QO.EPS * (amp + np.abs(w).max())
    t = QO.spike_t((12, 10), k)
    assert t.min() >= 0 and t.max() < 120 and t[0, 0] == 0
    x, y = np.arange(12)[:, None], np.arange(10)[None, :]
    np.testing.assert_array_equal(t, (k[0] * x * 10 + k[1] * y * 12) % 120)  # the reduced phase is the plain one modulo rx ry


def test_device_argument_of_the_cosine_is_reproduced_exactly():
    th = QO.spike_theta32((12, 10), (5, 7), 0.0)
    t = QO.spike_t((12, 10), (5, 7))
    want = (np.float64(QO.TWO_PI_F) * (t.astype(np.float32) / np.float32(120)).astype(np.float64)).astype(np.float32)  # phase 0: one rounding of an exact fp64 product
    np.testing.assert_array_equal(th, want)
    th = QO.spike_theta32((12, 10), (5, 7), 3.0)
    assert th.dtype == np.float32 and np.abs(th.astype(np.float64) - (2 * np.pi * t / 120.0 + 3.0)).max() < 8 * QO.EPS * 4 * np.pi


# ---- thick slices ----
def test_thick_slices_properties():
    rng = np.random.default_rng(1)
    v = rng.standard_normal((3, 2, 13))
    out, tol = QO.thick(v, 1, 0)
    assert out is not None and np.array_equal(out, v) and not np.any(tol)  # f = 1 is the identity
    for f in (2, 3, 4, 8):
        for o in range(f):
            const, tol = QO.thick(np.full((2, 2, 13), 1.75), f, o)
            assert np.abs(const - 1.75).max() < 1e-15 and tol.max() < 4 * f * QO.EPS * 1.75  # a constant column stays constant
            out, tol = QO.thick(v, f, o)
            sl = QO.slabs(13, f, o)
            assert sl[0][0] == 0 and sl[-1][1] == 12 and all(b[0] == a[1] + 1 for a, b in zip(sl, sl[1:])) and all(1 <= hi - lo + 1 <= f for lo, hi in sl)
            assert sl[0][1] - sl[0][0] + 1 == (f - o if f - o <= 13 else 13)  # the first slab is short by the offset
            for lo, hi in sl:  # at a slab centre that is a voxel the output is the slab mean: the column sum over the slab is kept
                if (lo + hi) % 2 == 0:
                    np.testing.assert_allclose(out[:, :, (lo + hi) // 2] * (hi - lo + 1), v[:, :, lo:hi + 1].sum(axis=2), atol=1e-13)
            # before the first and behind the last centre the end slab's mean is held
            np.testing.assert_allclose(out[:, :, 0], v[:, :, sl[0][0]:sl[0][1] + 1].mean(axis=2), atol=1e-14)
            np.testing.assert_allclose(out[:, :, 12], v[:, :, sl[-1][0]:sl[-1][1] + 1].mean(axis=2), atol=1e-14)
            assert out.min() >= v.min() - 1e-12 and out.max() <= v.max() + 1e-12 and (tol > 0).all()
            assert np.abs(out - v).max() > 0.1
    # ragged first and last slabs: rz = 5, f = 4, o = 3 leaves slabs of 1 and 4; rz = 6, f = 4, o = 1 slabs of 3 and 3
    assert QO.slabs(5, 4, 3) == [(0, 0), (1, 4)] and QO.slabs(6, 4, 1) == [(0, 2), (3, 5)] and QO.slabs(1, 4, 3) == [(0, 0)] and QO.slabs(3, 8, 0) == [(0, 2)]
    a, b, phi = QO.thick_weights(5, 4, 3)
    assert a.tolist() == [0, 0, 0, 1, 1] and b.tolist() == [1, 1, 1, 1, 1] and np.allclose(phi, [0.0, 0.4, 0.8, 0.0, 0.0])  # centres 0 and 2.5
    one, _ = QO.thick(v[:, :, :3], 8, 0)  # one slab: every z gets the column mean
    np.testing.assert_allclose(one, np.broadcast_to(v[:, :, :3].mean(axis=2, keepdims=True), one.shape), atol=1e-15)
    ramp = np.arange(16, dtype=np.float64)[None, None, :] * np.ones((1, 1, 1))
    lin, _ = QO.thick(ramp, 4, 0)  # a ramp is reproduced between the first and the last slab centre
    np.testing.assert_allclose(lin[0, 0, 2:14], ramp[0, 0, 2:14], atol=1e-13)


def test_job_chains_the_stages_in_order():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((6, 4, 5))
    out, tol = QO.job(v, **QO.NEUTRAL)
    assert np.array_equal(out, v) and not np.any(tol)
    full = dict(thick=2, thick_offset=1, ghost_axis=0, ghosts=3, ghost_alpha=0.5, spike_amp=0.7, spike_k=(2, 1), spike_phase=1.0)
    out, tol = QO.job(v, **full)
    t, _ = QO.thick(v, 2, 1)
    g, _ = QO.ghost(t, 0, 3, 0.5)
    s, _ = QO.spike(g, 0.7, (2, 1), 1.0)
    assert np.array_equal(out, s) and (tol > 0).all() and tol.max() < 1e-5
    # T acts along z and G in-plane, both linear: exchanged they give the same values up to rounding, which is why the contract fixes the order
    other, _ = QO.spike(QO.thick(QO.ghost(v, 0, 3, 0.5)[0], 2, 1)[0], 0.7, (2, 1), 1.0)
    assert np.abs(other - out).max() < 1e-14 and np.abs(out - v).max() > 0.5


# ---- ranges and draws ----
def test_check_acquisition_augment():
    assert T.ACQUISITION_KEYS == ("thick_slices", "ghost", "spike", "acquisition_prob")
    assert T.check_acquisition_augment() == dict(thick_slices=0, ghost=0.0, spike=0.0, acquisition_prob=0.25)
    assert T.check_acquisition_augment(4, 1.0, 10.0, 1.0) == dict(thick_slices=4, ghost=1.0, spike=10.0, acquisition_prob=1.0)
    assert T.check_acquisition_augment(2.0, 0.0, 0.0, 0.0)["thick_slices"] == 2 and isinstance(T.check_acquisition_augment(3)["thick_slices"], int)
    nan, inf = float("nan"), float("inf")
    for bad in ((1,), (5,), (2.5,), (-2,), (nan,), (inf,), (0, 1.01), (0, -0.1), (0, nan), (0, inf), (0, 0, -1.0), (0, 0, nan), (0, 0, inf), (0, 0, 0, -0.01), (0, 0, 0, 1.01), (0, 0, 0, nan)):
        with pytest.raises(ValueError):
            T.check_acquisition_augment(*bad)
    with pytest.raises(ValueError):
        T.RandomTail((8, 8, 8), 0.5, 0, thick_slices=7)
    assert T.APPEARANCE_KEYS == ("blur_sigma", "lowres", "contrast", "gamma", "appearance_prob")  # unchanged


@pytest.mark.parametrize("seed", [0, 7, 123])
@pytest.mark.parametrize("flip_prob", [0.5, None])
@pytest.mark.parametrize("five,field,app", [(False, False, False), (True, False, True), (False, True, False), (True, True, True), (False, False, True)])
def test_the_sixth_random_state_leaves_the_other_draws_unchanged(seed, flip_prob, five, field, app):
    roi, aug = (32, 24, 16), dict(ALL_ON if five else {}, **(FIELD_ON if field else {}), **(APP_ON if app else {}))
    off, zeros, on = T.RandomTail(roi, flip_prob, seed, **aug), T.RandomTail(roi, flip_prob, seed, **aug, thick_slices=0, ghost=0.0, spike=0.0, acquisition_prob=1.0), T.RandomTail(roi, flip_prob, seed, **aug, **ACQ_ON)
    assert not off.acquiring and not zeros.acquiring and zeros._acqR is None and on.acquiring and on.augmenting == five and on.fielding == field and on.appearing == app
    assert same_job(zeros.draw_acquisition(roi), T.NEUTRAL_ACQUISITION)
    seen = set()
    for shape in [(40, 36, 20), (33, 50, 16), (64, 64, 24), (32, 32, 16)] * 6:
        assert on.draw_noise_seed() == off.draw_noise_seed() and on.draw_field_seed() == off.draw_field_seed()
        assert on.draw(shape) == off.draw(shape)
        if five:
            assert on.draw_augment() == off.draw_augment()
        if field:
            assert on.draw_field() == off.draw_field()
        if app:
            assert on.draw_appearance() == off.draw_appearance()
        seen.add(repr(on.draw_acquisition(roi)))
    assert len(seen) > 12
    # the layout: the acquisition state is seeded by the next randint of RandomState(seed) after the flip's, the crop's, the augmentation's, the field's and the appearance's
    R = np.random.RandomState(seed)
    for _ in range((flip_prob is not None) + 1 + five + field + app):
        R.randint(T.MAX_SEED, dtype="uint32")
    assert T.RandomTail(roi, flip_prob, seed, **aug, **ACQ_ON)._acqR.randint(1 << 30) == np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32")).randint(1 << 30)


def test_a_family_with_range_zero_draws_nothing():
    roi = (24, 16, 8)
    one = T.RandomTail(roi, 0.5, 3, spike=1.0, acquisition_prob=1.0)
    only = [one.draw_acquisition(roi) for _ in range(4)]
    assert all(d["thick"] == 1 and d["ghosts"] == 0 for d in only)
    R = np.random.RandomState(3)
    for _ in range(2):
        R.randint(T.MAX_SEED, dtype="uint32")
    S = np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32"))
    raw = [(S.random_sample(), np.float32(S.uniform(0.0, 1.0)), int(S.randint(0, 24)), int(S.randint(0, 16)), np.float32(S.uniform(0.0, 2.0 * np.pi))) for _ in range(4)]
    for d, (_, amp, kx, ky, phase) in zip(only, raw):  # hit, amp, kx, ky, phase: five numbers per sample and nothing else
        assert (kx, ky) == (0, 0) or (d["spike_amp"] == amp and d["spike_k"] == (kx, ky) and d["spike_phase"] == phase)
    three = T.RandomTail(roi, 0.5, 3, **dict(ACQ_ON, acquisition_prob=1.0))
    d = three.draw_acquisition(roi)  # thick first: hit, f, o from the same stream
    S = np.random.RandomState(np.random.RandomState(3).randint(T.MAX_SEED, size=3, dtype="uint32")[2])
    S.random_sample()
    f, o = int(S.randint(2, 5)), int(S.randint(0, 12))
    assert (d["thick"], d["thick_offset"]) == (f, o % f)
    # the stream position does not depend on the outcome: with P = 0 nothing is hit, and the state has moved exactly as far
    miss, hit = T.RandomTail(roi, 0.5, 3, **dict(ACQ_ON, acquisition_prob=0.0)), T.RandomTail(roi, 0.5, 3, **dict(ACQ_ON, acquisition_prob=1.0))
    for _ in range(5):
        assert same_job(miss.draw_acquisition(roi), T.NEUTRAL_ACQUISITION) and not same_job(hit.draw_acquisition(roi), T.NEUTRAL_ACQUISITION)
    assert miss._acqR.randint(1 << 30) == hit._acqR.randint(1 << 30)


def test_every_draw_lies_in_its_interval_and_n_divides_the_axis():
    roi = (24, 18, 8)  # x: 2 3 4 6 8 divide 24; y: 2 3 6 divide 18
    tail = T.RandomTail(roi, 0.5, 11, **ACQ_ON)
    hits, counts = np.zeros(3, int), {0: set(), 1: set()}
    for _ in range(400):
        d = tail.draw_acquisition(roi)
        assert set(d) == set(T.NEUTRAL_ACQUISITION)
        assert d["thick"] == 1 and d["thick_offset"] == 0 or (2 <= d["thick"] <= 4 and 0 <= d["thick_offset"] < d["thick"])
        assert d["ghost_axis"] in (0, 1) and (d["ghosts"] == 0 and d["ghost_alpha"] == 0.0 or (d["ghosts"] in T.GHOST_COUNTS and roi[d["ghost_axis"]] % d["ghosts"] == 0 and 0.0 < d["ghost_alpha"] <= np.float32(0.8)))
        assert d["ghost_alpha"].dtype == np.float32 and d["spike_amp"].dtype == np.float32 and d["spike_phase"].dtype == np.float32
        assert d["spike_amp"] == 0.0 and d["spike_k"] == (0, 0) or (0.0 < d["spike_amp"] <= 2.0 and 0 <= d["spike_k"][0] < 24 and 0 <= d["spike_k"][1] < 18 and d["spike_k"] != (0, 0) and 0.0 <= d["spike_phase"] <= np.float32(2 * np.pi))
        hits += (d["thick"] != 1, d["ghosts"] != 0, d["spike_amp"] != 0.0)
        if d["ghosts"]:
            counts[d["ghost_axis"]].add(d["ghosts"])
    print(f"hits of 400 at P = 0.5: {hits}; ghost counts drawn along x {sorted(counts[0])}, along y {sorted(counts[1])}")
    assert (hits > 150).all() and (hits < 250).all()  # 200 +- 5 standard deviations
    assert counts[0] == {2, 3, 4, 6, 8} and counts[1] == {2, 3, 6}


def test_an_axis_without_a_candidate_yields_a_neutral_ghost():
    roi = (17, 17, 5)  # 17 is prime: none of 2, 3, 4, 6, 8 divides it
    tail, twin = T.RandomTail(roi, 0.5, 5, ghost=1.0, acquisition_prob=1.0), T.RandomTail((24, 24, 5), 0.5, 5, ghost=1.0, acquisition_prob=1.0)
    for _ in range(20):
        assert same_job(tail.draw_acquisition(roi), T.NEUTRAL_ACQUISITION)
        assert twin.draw_acquisition((24, 24, 5))["ghosts"] != 0
    assert tail._acqR.randint(1 << 30) == twin._acqR.randint(1 << 30)  # and still draws its four numbers
    mixed = T.RandomTail((33, 17, 5), 0.5, 5, ghost=1.0, acquisition_prob=1.0)  # along x 3 divides 33, along y nothing divides 17
    jobs = [mixed.draw_acquisition((33, 17, 5)) for _ in range(40)]
    assert {(d["ghost_axis"], d["ghosts"]) for d in jobs} == {(0, 3), (0, 0)}


# ---- the command line ----
def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


FLAGS = ["--aug_rotate_deg", "15", "--aug_blur_sigma", "1.5", "--aug_appearance_prob", "0.5"]
ACQ_FLAGS = ["--aug_thick_slices", "4", "--aug_ghost", "0.8", "--aug_spike", "2.0", "--aug_acquisition_prob", "0.5"]


def test_command_line_flags_default_to_off_and_reject_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    assert [ap.get_default("aug_" + k) for k in T.ACQUISITION_KEYS] == [0, 0.0, 0.0, 0.25]
    for bad in (["--aug_thick_slices", "1"], ["--aug_thick_slices", "5"], ["--aug_thick_slices", "2.5"], ["--aug_thick_slices", "-3"], ["--aug_thick_slices", "nan"], ["--aug_ghost", "1.1"], ["--aug_ghost", "-0.5"],
                ["--aug_ghost", "inf"], ["--aug_spike", "-1"], ["--aug_spike", "nan"], ["--aug_acquisition_prob", "1.5"], ["--aug_acquisition_prob", "-0.1"], ["--aug_spike", "x"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], ACQ_FLAGS, ["--aug_thick_slices", "2"], ["--aug_ghost", "1"], ["--aug_spike", "0.5", "--aug_acquisition_prob", "1"], ["--aug_acquisition_prob", "0"]):
        p = _parse(good)
        if p is not None:
            assert p.aug_thick_slices == (4 if good is ACQ_FLAGS else 2 if "--aug_thick_slices" in good else 0)


def test_flags_reach_the_training_chain_only(monkeypatch):
    """get_transforms needs no device: build the object past the device check."""
    import torch
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    keys = tuple("aug_" + k for k in T.ACQUISITION_KEYS)
    for argv, others, on in (([], False, False), (ACQ_FLAGS, False, True), (FLAGS + ACQ_FLAGS, True, True), (FLAGS, True, False), (["--aug_acquisition_prob", "0.9"], False, False)):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        train, val, test = p.get_transforms()
        text = lambda tf: " ".join(tf["chain"])  # noqa: E731
        for k in keys[:3]:
            assert (k in text(train)) == on
            assert k not in text(val) and k not in text(test)
        assert "acquisition_augment" not in val and "acquisition_augment" not in test
        assert train["acquisition_augment"] == p.acquisition_augment and set(train["acquisition_augment"]) == set(T.ACQUISITION_KEYS)
        if on:
            assert train["acquisition_augment"] == ACQ_ON
            assert text(train).index("RandSpatialCrop") < text(train).index("aug_thick_slices") < text(train).index("aug_ghost") < text(train).index("aug_spike")  # the order they are applied in
            if others:
                assert text(train).index("aug_rotate_deg") < text(train).index("aug_thick_slices") and text(train).index("aug_spike") < text(train).index("aug_blur_sigma")  # after the crop launch, before the appearance
        tail = T.RandomTail(train["roi"], train["flip_prob"], 0, **train["augment"], **train["field_augment"], **train["appearance_augment"], **train["acquisition_augment"])
        assert tail.acquiring == on and tail.augmenting == others and tail.appearing == others and not tail.fielding
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        p.log_parameters()
        for k in keys:
            assert any(k in ln for ln in lines) == on
    p = P.VSparams(argparse.ArgumentParser(), ["--aug_ghost", "0.2"])  # one family alone
    assert "aug_ghost" in " ".join(p.get_transforms()[0]["chain"]) and "aug_spike" not in " ".join(p.get_transforms()[0]["chain"])


# ---- the entry point ----
def _fake_pointer():
    mem = ctypes.create_string_buffer(512)
    return mem, (ctypes.addressof(mem) + 15) & ~15


def test_patch_acquisition_rejects_bad_arguments_before_the_launch():
    """Fake device addresses: every call below is refused before anything is launched, the job records are read from the host copy."""
    lib = L.lib()
    assert "vsseg_patch_acquisition" in L.SYMBOLS and lib.vsseg_version() >= 21 and ctypes.sizeof(L.AcquisitionJob) == 36
    mem, ptr = _fake_pointer()
    roi = (8, 6, 4)

    def jobs(n=2, **kw):
        js = (L.AcquisitionJob * n)()
        for i in range(n):
            js[i].thick, js[i].thick_offset, js[i].ghost_axis, js[i].ghosts, js[i].ghost_alpha = 2, 1, 0, 4, 0.5
            js[i].spike_amp, js[i].spike_k, js[i].spike_phase = 1.0, (ctypes.c_int32 * 2)(3, 2), 1.0
        for k, v in kw.items():  # the LAST job is the bad one: every record is checked
            setattr(js[n - 1], k, v)
        return js

    def refused(why, js=None, dev=ptr, n=2, src=ptr, dst=ptr + 64, scratch=ptr + 128, r=roi):
        rc = lib.vsseg_patch_acquisition(js if js is not None else jobs(n if n > 0 else 1), dev, n, src, dst, scratch, L.i3(r) if r is not None else None, None)
        err = lib.vsseg_last_error()
        assert rc == L.EINVAL and b"vsseg_patch_acquisition" in err and why in err, (why, rc, err)

    nan, inf = float("nan"), float("inf")
    k2 = lambda a, b: (ctypes.c_int32 * 2)(a, b)  # noqa: E731
    refused(b"null", js=ctypes.POINTER(L.AcquisitionJob)())
    refused(b"null", dev=None)
    refused(b"null", src=None)
    refused(b"null", dst=None)
    refused(b"null", r=None)
    refused(b"src == dst", dst=ptr)
    refused(b"njobs", n=0)
    refused(b"njobs", n=-3)
    for r in ((0, 6, 4), (8, -1, 4), (8, 6, 0), (65536, 6, 4), (8, 6, 70000)):
        refused(b"roi", r=r)
    refused(b"misaligned", dst=ptr + 68)
    refused(b"misaligned", src=ptr + 4)
    refused(b"misaligned", scratch=ptr + 136)
    for thick in (0, -1, 9, 100):
        refused(b"thick =", js=jobs(thick=thick))
    for off in (-1, 2, 7):
        refused(b"thick_offset", js=jobs(thick_offset=off))
    for axis in (-1, 2):
        refused(b"ghost_axis", js=jobs(ghost_axis=axis))
    for n in (1, -2, 3, 5, 16):  # below 2, or no divisor of roi_x = 8
        refused(b"ghosts", js=jobs(ghosts=n))
    refused(b"ghosts", js=jobs(ghost_axis=1, ghosts=4))  # 4 divides roi_x = 8 but not roi_y = 6
    for alpha in (nan, inf, -inf, 0.0, -0.5, 1.5):
        refused(b"ghost_alpha", js=jobs(ghost_alpha=alpha))
    for amp in (nan, inf, -inf):
        refused(b"spike_amp", js=jobs(spike_amp=amp))
    for phase in (nan, inf, -inf):
        refused(b"spike_phase", js=jobs(spike_phase=phase))
    for k in ((-1, 2), (8, 2), (3, -1), (3, 6)):
        refused(b"spike_k", js=jobs(spike_k=k2(*k)))
    refused(b"(0, 0)", js=jobs(spike_k=k2(0, 0)))
    refused(b"scratch must not be null", scratch=None)  # thick slices and a later stage in one job
    # what is off is not checked: with a ghost count of 0 any alpha and with an amplitude of 0 any k pass, and the complaint is about the field behind them
    refused(b"spike_phase", js=jobs(ghosts=0, ghost_alpha=7.0, spike_amp=0.0, spike_k=k2(99, -4), spike_phase=nan))
