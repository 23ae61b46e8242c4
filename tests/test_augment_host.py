"""CPU tests of the training augmentation: the oracle's Philox against Random123's published known answers, the RNG layout of RandomTail (flip and crop draws do not
move when augmentation is switched on), the fp32 matrix PatchSampler hands to the kernel, the command-line flags, and the argument checks of vsseg_crop_affine (made
before any launch, so they are the same on a machine without a GPU)."""
import argparse
import ctypes

import numpy as np
import pytest

from tests import augment_oracle as AO
from vs_seg_amd import _lib as L
from vs_seg_amd.data import transforms as T

ALL_ON = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.1, intensity_shift=0.1, noise_std=0.05)


def _words(r):
    return [int(np.asarray(w).reshape(-1)[0]) for w in r]


def test_oracle_philox_reproduces_the_published_known_answers():
    """Random123 kat_vectors, philox4x32 with 10 rounds: the generator of csrc/common.h."""
    assert _words(AO.philox4x32_10((0, 0, 0, 0), (0, 0))) == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    f = 0xFFFFFFFF
    assert _words(AO.philox4x32_10((f, f, f, f), (f, f))) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]
    assert _words(AO.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]
    # vectorised counters give what single counters give
    g = np.arange(5, dtype=np.uint64)
    r = AO.philox4x32_10((g, 0 * g, 3, 0), (0x9ABC, 0x1234))
    for i in range(5):
        assert [int(w[i]) for w in r] == _words(AO.philox4x32_10((i, 0, 3, 0), (0x9ABC, 0x1234)))


def test_oracle_normals_look_normal_and_depend_on_stream_and_seed():
    n = AO.normals((32, 32, 16), 0, 0x123456789ABC)
    assert abs(n.mean()) < 0.03 and abs(n.std() - 1.0) < 0.03 and np.abs(n).max() < 5.9
    assert np.abs(n - AO.normals((32, 32, 16), 1, 0x123456789ABC)).max() > 1.0
    assert np.abs(n - AO.normals((32, 32, 16), 0, 0x123456789ABD)).max() > 1.0
    # a patch whose size is no multiple of four takes the first voxels of the same groups
    np.testing.assert_array_equal(AO.normals((1, 1, 22), 0, 5).ravel(), AO.normals((1, 1, 24), 0, 5).ravel()[:22])


@pytest.mark.parametrize("seed", [0, 7, 123])
@pytest.mark.parametrize("flip_prob", [0.5, None])
def test_flip_and_crop_draws_do_not_depend_on_augmentation(seed, flip_prob):
    roi = (32, 32, 16)
    plain, zeros, on = T.RandomTail(roi, flip_prob, seed), T.RandomTail(roi, flip_prob, seed, 0.0, 0.0, 0.0, 0.0, 0.0), T.RandomTail(roi, flip_prob, seed, **ALL_ON)
    assert not plain.augmenting and not zeros.augmenting and zeros._augR is None and on.augmenting
    seen = set()
    for shape in [(40, 36, 20), (33, 50, 16), (64, 64, 24), (32, 32, 16)] * 6:
        want = plain.draw(shape)
        assert zeros.draw(shape) == want and on.draw(shape) == want
        on.draw_noise_seed()
        angle, scale, gain, bias = on.draw_augment()
        assert abs(angle) <= np.deg2rad(15.0) and abs(scale - 1.0) <= 0.1 and abs(gain - 1.0) <= 0.1 and abs(bias) <= 0.1
        seen.add((angle, scale, gain, bias))
    assert len(seen) == 24
    # today's layout: the transform seeds are the first randint draws of RandomState(seed), in chain order
    R = np.random.RandomState(seed)
    first = R.randint(T.MAX_SEED, dtype="uint32")
    ref = T.RandomTail(roi, flip_prob, seed)
    crop_seed = R.randint(T.MAX_SEED, dtype="uint32") if flip_prob is not None else first
    assert ref._cropR.randint(1 << 30) == np.random.RandomState(crop_seed).randint(1 << 30)


def test_a_family_with_range_zero_draws_nothing():
    a = T.RandomTail((8, 8, 8), 0.5, 3, rotate_deg=10.0)
    b = T.RandomTail((8, 8, 8), 0.5, 3, rotate_deg=10.0, intensity_shift=0.2)
    angles = [a.draw_augment() for _ in range(4)]
    assert all(s == 1.0 and g == 1.0 and o == 0.0 for _, s, g, o in angles) and a.draw_noise_seed() == 0
    both = [b.draw_augment() for _ in range(2)]  # angle, bias, angle, bias: the same stream, consumed twice as fast
    assert [both[0][0], both[1][0]] == [angles[0][0], angles[2][0]] and both[0][3] != 0.0
    for bad in (dict(rotate_deg=-1.0), dict(rotate_deg=181.0), dict(scale=1.0), dict(intensity_scale=1.5), dict(noise_std=-0.1), dict(intensity_shift=float("nan"))):
        with pytest.raises(ValueError):
            T.RandomTail((8, 8, 8), 0.5, 0, **bad)


def test_matrix_is_an_exact_translation_when_every_range_is_zero():
    roi = (32, 32, 16)
    for start in ((0, 0, 0), (3, -2, 1), (400, 300, 90), (-4, 9, -3)):
        m = T.affine_matrix(roi, start, 512, False)
        assert m.dtype == np.float32 and m.shape == (3, 4)
        np.testing.assert_array_equal(m, np.concatenate([np.eye(3), np.asarray(start, np.float64)[:, None]], 1))
        mm = T.affine_matrix(roi, start, 512, True)
        want = np.concatenate([np.diag([-1.0, 1.0, 1.0]), np.array([512 - 1 - start[0], start[1], start[2]], np.float64)[:, None]], 1)
        np.testing.assert_array_equal(mm, want)
        assert not (np.signbit(m) & (m == 0)).any() and not (np.signbit(mm) & (mm == 0)).any()  # no negative zeros


@pytest.mark.parametrize("roi,start,sx,flip,angle,scale", [((32, 32, 16), (3, -2, 1), 40, False, 0.3, 1.1), ((32, 32, 16), (-4, 9, -3), 33, True, -0.26, 0.9),
                                                            ((384, 384, 64), (100, 77, 31), 512, True, 0.2617, 1.1), ((8, 6, 22), (0, 0, 5), 19, False, 3.1, 0.91)])
def test_matrix_rotates_and_scales_about_the_centre_of_the_crop_window(roi, start, sx, flip, angle, scale):
    m = T.affine_matrix(roi, start, sx, flip, angle, scale).astype(np.float64)
    c_roi = (np.asarray(roi, np.float64) - 1.0) / 2.0
    c_src = np.asarray(start, np.float64) + c_roi
    if flip:
        c_src[0] = sx - 1 - c_src[0]
    eps = 2.0 ** -24
    mag = np.abs(m[:, :3]) @ c_roi + np.abs(m[:, 3])  # every entry is within half an fp32 ulp of its fp64 value
    assert (np.abs(m[:, :3] @ c_roi + m[:, 3] - c_src) <= 2 * eps * mag).all()
    R = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]]) / scale
    if flip:
        R[0] = -R[0]
    assert (np.abs(m[:2, :2] - R) <= eps * np.abs(R)).all()
    np.testing.assert_array_equal(m[2], [0.0, 0.0, 1.0, start[2]])
    np.testing.assert_array_equal(m[:2, 2], [0.0, 0.0])


def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


FLAGS = ["--aug_rotate_deg", "15", "--aug_scale", "0.1", "--aug_intensity_scale", "0.1", "--aug_intensity_shift", "0.1", "--aug_noise_std", "0.05"]


def test_command_line_flags_default_to_off_and_reject_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    for k in T.AUGMENT_KEYS:
        assert ap.get_default("aug_" + k) == 0.0
    for bad in (["--aug_rotate_deg", "-1"], ["--aug_rotate_deg", "180.5"], ["--aug_scale", "-0.1"], ["--aug_scale", "1"], ["--aug_intensity_scale", "1.0"],
                ["--aug_intensity_scale", "-0.2"], ["--aug_intensity_shift", "-0.1"], ["--aug_noise_std", "-1e-3"], ["--aug_noise_std", "nan"], ["--aug_scale", "x"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], FLAGS, ["--aug_rotate_deg", "180"], ["--aug_scale", "0.99"]):
        p = _parse(good)
        if p is not None:
            assert p.aug_rotate_deg == (float(good[1]) if good[:1] == ["--aug_rotate_deg"] else 0.0)


def test_flags_reach_the_training_chain_only(monkeypatch):
    """get_transforms needs no device: build the object past the device check."""
    import torch
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    for argv, on in (([], False), (FLAGS, True)):
        p = P.VSparams(argparse.ArgumentParser(), argv)
        train, val, test = p.get_transforms()
        text = lambda tf: " ".join(tf["chain"])  # noqa: E731
        for k in T.AUGMENT_KEYS:
            assert ("aug_" + k in text(train)) == on
            assert "aug_" + k not in text(val) and "aug_" + k not in text(test)
        assert "augment" not in val and "augment" not in test
        assert train["augment"] == (ALL_ON if on else dict.fromkeys(T.AUGMENT_KEYS, 0.0))
        assert T.RandomTail(train["roi"], train["flip_prob"], 0, **train["augment"]).augmenting == on
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        p.log_parameters()
        assert any("aug_noise_std" in ln for ln in lines) == on


def test_crop_affine_rejects_bad_arguments_before_the_launch():
    """Fake device addresses: every call below is refused before anything is launched, the job records are read from the host copy."""
    lib = L.lib()
    assert lib.vsseg_version() >= 11
    mem = ctypes.create_string_buffer(256)
    ptr = (ctypes.addressof(mem) + 15) & ~15
    roi = (8, 6, 4)

    def jobs(n=2, **kw):
        js = (L.AffineJob * n)()
        for i in range(n):
            js[i].src, js[i].sdims, js[i].interp, js[i].m = ptr, L.i3((9, 9, 9)), i & 1, (ctypes.c_float * 12)(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)
            js[i].gain, js[i].bias, js[i].noise_std, js[i].noise_stream = 1.0, 0.0, 0.0, i
        for k, v in kw.items():  # the LAST job is the bad one: every record is checked
            if k.startswith("m"):
                js[n - 1].m[int(k[1:])] = v
            else:
                setattr(js[n - 1], k, v)
        return js

    def refused(why, js=None, dev=ptr, n=2, dst=ptr, r=roi):
        rc = lib.vsseg_crop_affine(js if js is not None else jobs(n if n > 0 else 1), dev, n, dst, L.i3(r), 0, None)
        err = lib.vsseg_last_error()
        assert rc == L.EINVAL and b"vsseg_crop_affine" in err and why in err, (why, rc, err)

    refused(b"null", js=ctypes.POINTER(L.AffineJob)())
    refused(b"null", dev=None)
    refused(b"null", dst=None)
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
