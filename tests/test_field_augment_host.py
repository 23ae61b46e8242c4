"""CPU tests of the B-spline field augmentation (elastic deformation, bias field): the properties of the field the oracle restates (partition of unity, |d| <= mag,
no folding at mag = S / 4), the range checks, the RNG layout of RandomTail (a fourth state: nothing else moves), the command-line flags, and the argument checks of
vsseg_crop_field (made before any launch, so they are the same on a machine without a GPU)."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import field_oracle as FO
from vs_seg_amd import _lib as L
from vs_seg_amd.data import transforms as T

ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)
FIELD_ON = dict(elastic_mag=4.0, bias_field=0.3, field_spacing=16)
SEED = 0x123456789ABC


@pytest.mark.parametrize("roi,spacing", FO.SHAPES)
def test_field_is_a_partition_of_unity_and_bounded_by_its_controls(roi, spacing):
    n = FO.lattice_shape(roi, spacing)
    assert n == tuple((r - 1) // s + 4 for r, s in zip(roi, spacing))
    one = FO.field(np.ones((1, *n)), roi, spacing)
    assert one.shape == (1, *roi) and np.abs(one - 1.0).max() < 1e-14  # F(1) = 1
    w = FO.bspline_weights(np.linspace(0.0, 1.0, 33)[:-1])
    assert (w >= 0.0).all() and np.abs(w.sum(0) - 1.0).max() < 1e-15
    c = FO.control(roi, spacing, 3, SEED)
    assert c.shape == (3, *n) and c.min() >= -1.0 and c.max() < 1.0 and c.std() > 0.4
    F = FO.fields(roi, spacing, 3, SEED)
    assert np.abs(F).max() <= 1.0  # a convex combination of the controls: |d| <= mag
    mag = spacing[0] / 4.0
    s = FO.coords(np.concatenate([np.eye(3), np.zeros((3, 1))], 1), roi, spacing, mag, 3, SEED)
    x, y, z = np.meshgrid(*[np.arange(r, dtype=np.float64) for r in roi], indexing="ij")
    assert np.abs(s[0] - x).max() <= mag and np.abs(s[1] - y).max() <= mag and (s[2] == z).all()  # and d_z = 0
    assert np.abs(s[0] - x).max() > 0.0
    # another stream or seed is another lattice
    assert np.abs(c - FO.control(roi, spacing, 4, SEED)).max() > 0.5 and np.abs(c - FO.control(roi, spacing, 3, SEED + 1)).max() > 0.5


@pytest.mark.parametrize("roi,spacing", FO.SHAPES)
def test_deformation_does_not_fold_at_a_quarter_of_the_spacing(roi, spacing):
    mag = spacing[0] / 4.0
    worst = 1.0
    for stream in range(4):
        F = FO.fields(roi, spacing, stream, SEED)
        worst = min(worst, FO.jacobian_min(mag * F[0], mag * F[1]))
    print(f"roi {roi} spacing {spacing}: smallest discrete in-plane Jacobian at mag = S / 4: {worst:.3f}")
    assert worst > 0.0
    # the worst lattice there is: alternating controls.  Every partial stays below 2 mag / S, the determinant above 1 - 4 mag / S = 0
    n = FO.lattice_shape(roi, spacing)
    i, j, _ = np.meshgrid(*[np.arange(a) for a in n], indexing="ij")
    alt = np.stack([(-1.0) ** i, (-1.0) ** j]) + 0.0 * i
    F = FO.field(alt, roi, spacing)
    assert np.abs(np.diff(mag * F[0], axis=0)).max() < 2.0 * mag / spacing[0] + 1e-12 and FO.jacobian_min(mag * F[0], mag * F[1]) > 0.0


def test_field_delta_is_a_small_multiple_of_the_fp32_epsilon():
    assert FO.field_delta(1.0) == 96.0 * 2.0 ** -24 and FO.field_delta(16.0) == 16.0 * FO.field_delta(1.0) and FO.field_delta(0.0) == 0.0
    m = np.array([[0.8, -0.6, 0.0, 3.0], [0.6, 0.8, 0.0, 2.0], [0.0, 0.0, 1.0, 1.0]], np.float32)
    s = FO.coords(m, (32, 32, 16), (8, 8, 2), 2.0, 0, SEED)
    from tests import augment_oracle as AO

    cd = FO.coord_delta(s, m, 2.0, (32, 32, 16))
    assert cd[2] == AO.delta(s) and (cd[:2] > AO.delta(s)).all() and (cd[:2] < AO.delta(s) + 1.5 * (FO.field_delta(2.0) + 2.0 ** -19)).all()
    assert (FO.coord_delta(s, m, 0.0, (32, 32, 16)) == AO.delta(s)).all()


def test_check_field_augment():
    assert T.FIELD_KEYS == ("elastic_mag", "bias_field", "field_spacing")
    assert T.check_field_augment() == dict(elastic_mag=0.0, bias_field=0.0, field_spacing=64)
    assert T.check_field_augment(16.0, 0.3, 64) == dict(elastic_mag=16.0, bias_field=0.3, field_spacing=64)  # S / 4 is accepted ...
    assert T.check_field_augment(0.25, 0.0, 1)["field_spacing"] == 1
    for bad in ((16.000001, 0.0, 64), (np.nextafter(4.0, 5.0), 0.0, 16), (-1.0, 0.0, 64), (0.0, -0.1, 64), (float("nan"), 0.0, 64), (0.0, float("inf"), 64), (1.0, 0.0, 0), (0.0, 0.0, -8),
                (0.0, 0.0, 7.5), (0.0, 0.0, float("nan"))):  # ... anything above it is refused
        with pytest.raises(ValueError):
            T.check_field_augment(*bad)
    with pytest.raises(ValueError):
        T.RandomTail((8, 8, 8), 0.5, 0, elastic_mag=5.0, field_spacing=16)
    assert T.field_launch_spacing(64) == (64, 64, 16) and T.field_launch_spacing(8) == (8, 8, 2) and T.field_launch_spacing(12) == (12, 12, 3) and T.field_launch_spacing(16) == (16, 16, 4)
    assert T.field_launch_spacing(1) == (1, 1, 1)
    assert T.AUGMENT_KEYS == ("rotate_deg", "scale", "intensity_scale", "intensity_shift", "noise_std")  # unchanged


@pytest.mark.parametrize("seed", [0, 7, 123])
@pytest.mark.parametrize("flip_prob", [0.5, None])
@pytest.mark.parametrize("five", [False, True])
def test_the_fourth_random_state_leaves_the_other_draws_unchanged(seed, flip_prob, five):
    roi, aug = (32, 32, 16), (ALL_ON if five else {})
    off, zeros, on = T.RandomTail(roi, flip_prob, seed, **aug), T.RandomTail(roi, flip_prob, seed, **aug, elastic_mag=0.0, bias_field=0.0, field_spacing=16), T.RandomTail(roi, flip_prob, seed, **aug, **FIELD_ON)
    assert not off.fielding and not zeros.fielding and zeros._fieldR is None and on.fielding and on.augmenting == five
    assert zeros.draw_field_seed() == 0 and zeros.draw_field() == (0.0, 0.0)
    seen, seeds = set(), set()
    for shape in [(40, 36, 20), (33, 50, 16), (64, 64, 24), (32, 32, 16)] * 6:
        assert on.draw_noise_seed() == off.draw_noise_seed()
        seeds.add(on.draw_field_seed())
        assert on.draw(shape) == off.draw(shape)
        if five:
            assert on.draw_augment() == off.draw_augment()
        a, b = on.draw_field()
        assert 0.0 <= a <= 4.0 and 0.0 <= b <= 0.3
        seen.add((a, b))
    assert len(seen) == 24 and len(seeds) == 24
    # the layout: the field state is seeded by the next randint of RandomState(seed) after the flip's, the crop's and the augmentation's
    R = np.random.RandomState(seed)
    for _ in range((flip_prob is not None) + 1 + five):
        R.randint(T.MAX_SEED, dtype="uint32")
    assert T.RandomTail(roi, flip_prob, seed, **aug, **FIELD_ON)._fieldR.randint(1 << 30) == np.random.RandomState(R.randint(T.MAX_SEED, dtype="uint32")).randint(1 << 30)


def test_a_field_family_with_range_zero_draws_nothing():
    e = T.RandomTail((8, 8, 8), 0.5, 3, elastic_mag=2.0, field_spacing=8)
    both = T.RandomTail((8, 8, 8), 0.5, 3, elastic_mag=2.0, bias_field=0.3, field_spacing=8)
    only = [e.draw_field() for _ in range(4)]
    assert all(b == 0.0 and 0.0 <= a <= 2.0 for a, b in only)
    two = [both.draw_field() for _ in range(2)]  # a, beta, a, beta: the same stream, consumed twice as fast
    assert [two[0][0], two[1][0]] == [only[0][0], only[2][0]] and two[0][1] != 0.0
    b = T.RandomTail((8, 8, 8), 0.5, 3, bias_field=0.3)
    assert all(a == 0.0 and 0.0 < beta <= 0.3 for a, beta in (b.draw_field() for _ in range(4)))


def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


FLAGS = ["--aug_rotate_deg", "15", "--aug_scale", "0.1", "--aug_intensity_scale", "0.1", "--aug_intensity_shift", "0.1", "--aug_noise_std", "0.05"]
FIELD_FLAGS = ["--aug_elastic_mag", "4", "--aug_bias_field", "0.3", "--aug_field_spacing", "16"]


def test_command_line_flags_default_to_off_and_reject_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    assert ap.get_default("aug_elastic_mag") == 0.0 and ap.get_default("aug_bias_field") == 0.0 and ap.get_default("aug_field_spacing") == 64
    assert "half" in next(a.help for a in ap._actions if a.dest == "aug_elastic_mag")  # the peak displacement is about half of VOX
    for bad in (["--aug_elastic_mag", "-1"], ["--aug_elastic_mag", "16.5"], ["--aug_elastic_mag", "4.01", "--aug_field_spacing", "16"], ["--aug_elastic_mag", "nan"], ["--aug_bias_field", "-0.1"],
                ["--aug_bias_field", "inf"], ["--aug_field_spacing", "0"], ["--aug_field_spacing", "-4"], ["--aug_field_spacing", "7.5"], ["--aug_bias_field", "x"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], FIELD_FLAGS, ["--aug_elastic_mag", "16"], ["--aug_elastic_mag", "4", "--aug_field_spacing", "16"], ["--aug_bias_field", "0.5"]):
        p = _parse(good)
        if p is not None:
            assert p.aug_elastic_mag == (float(good[1]) if good[:1] == ["--aug_elastic_mag"] else 0.0)


def test_flags_reach_the_training_chain_only(monkeypatch):
    """get_transforms needs no device: build the object past the device check."""
    import torch
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    for argv, five, on in (([], False, False), (FIELD_FLAGS, False, True), (FLAGS + FIELD_FLAGS, True, True), (FLAGS, True, False)):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        train, val, test = p.get_transforms()
        text = lambda tf: " ".join(tf["chain"])  # noqa: E731
        for k in ("aug_elastic_mag", "aug_field_spacing", "aug_bias_field"):
            assert (k in text(train)) == on
            assert k not in text(val) and k not in text(test)
        assert "field_augment" not in val and "field_augment" not in test and "augment" not in val
        assert train["field_augment"] == (FIELD_ON if on else dict(elastic_mag=0.0, bias_field=0.0, field_spacing=64))
        assert train["augment"] == (ALL_ON if five else dict.fromkeys(T.AUGMENT_KEYS, 0.0)) and set(train["augment"]) == set(T.AUGMENT_KEYS)  # exactly its five keys
        tail = T.RandomTail(train["roi"], train["flip_prob"], 0, **train["augment"], **train["field_augment"])
        assert tail.fielding == on and tail.augmenting == five
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        p.log_parameters()
        for k in ("aug_elastic_mag", "aug_bias_field", "aug_field_spacing"):
            assert any(k in ln for ln in lines) == on
    p = P.VSparams(argparse.ArgumentParser(), ["--aug_bias_field", "0.2"])  # one family alone
    assert "aug_bias_field" in " ".join(p.get_transforms()[0]["chain"]) and "aug_elastic_mag" not in " ".join(p.get_transforms()[0]["chain"])


def test_crop_field_rejects_bad_arguments_before_the_launch():
    """Fake device addresses: every call below is refused before anything is launched, the job records are read from the host copy."""
    lib = L.lib()
    assert lib.vsseg_version() >= 12
    assert ctypes.sizeof(L.FieldJob) == ctypes.sizeof(L.AffineJob) + 8 and [f[0] for f in L.FieldJob._fields_[:-2]] == [f[0] for f in L.AffineJob._fields_]
    mem = ctypes.create_string_buffer(256)
    ptr = (ctypes.addressof(mem) + 15) & ~15
    roi, spacing = (8, 6, 4), (8, 8, 2)

    def jobs(n=2, mag=2.0, **kw):
        js = (L.FieldJob * n)()
        for i in range(n):
            js[i].src, js[i].sdims, js[i].interp, js[i].m = ptr, L.i3((9, 9, 9)), i & 1, (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
            js[i].gain, js[i].bias, js[i].noise_std, js[i].noise_stream, js[i].elastic_mag, js[i].bias_log = 1.0, 0.0, 0.0, i, mag, 0.3
        for k, v in kw.items():  # the LAST job is the bad one: every record is checked
            if k.startswith("m") and k[1:].isdigit():
                js[n - 1].m[int(k[1:])] = v
            else:
                setattr(js[n - 1], k, v)
        return js

    def refused(why, js=None, dev=ptr, n=2, dst=ptr, r=roi, sp=spacing):
        rc = lib.vsseg_crop_field(js if js is not None else jobs(n if n > 0 else 1), dev, n, dst, L.i3(r), L.i3(sp) if sp is not None else None, 0, None)
        err = lib.vsseg_last_error()
        assert rc == L.EINVAL and b"vsseg_crop_field" in err and why in err, (why, rc, err)

    # everything vsseg_crop_affine checks
    refused(b"null", js=ctypes.POINTER(L.FieldJob)())
    refused(b"null", dev=None)
    refused(b"null", dst=None)
    refused(b"null", sp=None)
    refused(b"null", js=jobs(src=None))
    refused(b"njobs", n=0)
    refused(b"njobs", n=-3)
    for r in ((0, 6, 4), (8, -1, 4), (8, 6, 0)):
        refused(b"roi", r=r)
    refused(b"sdims", js=jobs(sdims=L.i3((9, 0, 9))))
    refused(b"misaligned", dst=ptr + 4)
    for interp in (2, -1):
        refused(b"interp", js=jobs(interp=interp))
    for bad in (float("nan"), float("inf"), -float("inf")):
        for field in ("m0", "m7", "m11", "gain", "bias", "noise_std"):
            refused(b"non-finite", js=jobs(**{field: bad}))
        # and the field's own
        for field in ("elastic_mag", "bias_log"):
            refused(b"negative or non-finite", js=jobs(**{field: bad}))
    for sp in ((0, 8, 2), (8, -8, 2), (8, 8, 0)):
        refused(b"spacing", sp=sp)
    refused(b"negative or non-finite", js=jobs(elastic_mag=-0.5))
    refused(b"negative or non-finite", js=jobs(bias_log=-0.5))
    refused(b"above min(spacing_x, spacing_y) / 4", js=jobs(elastic_mag=float(np.nextafter(np.float32(2.0), np.float32(3.0)))))
    refused(b"above min(spacing_x, spacing_y) / 4", js=jobs(elastic_mag=2.0), sp=(8, 7, 2))
    refused(b"above min(spacing_x, spacing_y) / 4", js=jobs(elastic_mag=2.0), sp=(4, 8, 2))
    # a lattice plane beyond the 1024 nodes the kernel holds: (roi_y - 1) / 1 + 4 = 36 by (roi_z - 1) / 1 + 4 = 35
    refused(b"cannot hold", js=jobs(mag=0.25), r=(8, 33, 32), sp=(1, 1, 1))
