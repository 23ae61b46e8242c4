"""CPU tests of the ball morphology: the numpy oracle (tests/ball_oracle.py) against scipy.ndimage and against the properties of the four operations, a numpy
restatement of the route the kernels take (banded, separable, fp32, confined to the work box) against the oracle, the ABI, the argument checks of
vs_seg_amd.binary_dilate / binary_erode / binary_close / binary_open (made before the device check) and of the C entry point (made before any launch), and the
flags."""
import argparse
import re

import numpy as np
import pytest
import torch

from tests import ball_oracle as BO
from vs_seg_amd import binary_close, binary_dilate, binary_erode, binary_open

SHAPES = [(24, 20, 12), (37, 29, 19), (1, 17, 9), (2, 2, 2)]
SPACINGS = [(1.0, 1.0, 1.0), (0.5, 0.5, 1.5), (1.0, 1.0, 3.0)]
RADII = [1.0, 1.5, 2.0, 3.0]
CALLS = [binary_dilate, binary_erode, binary_close, binary_open]


def random_mask(shape, density, seed=0):
    return np.random.default_rng(sum(shape) + round(100 * density) + seed).random(shape) < density


# ---------------------------------------------------------------- the oracle
def test_the_ball_is_what_the_definition_says():
    assert BO.ball_offsets((1, 1, 1), 0) == [(0, 0, 0)]
    assert sorted(BO.ball_offsets((1, 1, 1), 1)) == sorted([(0, 0, 0), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)])  # a tie belongs
    assert len(BO.ball_offsets((1, 1, 1), 0.999)) == 1 and len(BO.ball_offsets((1, 1, 1), 1.5)) == 19 and len(BO.ball_offsets((1, 1, 1), 2)) == 33
    assert BO.reach((0.5, 0.5, 1.5), 1.5) == [3, 3, 1] and (0, 0, 1) in BO.ball_offsets((0.5, 0.5, 1.5), 1.5)  # the exact tie at dz = 1 counts
    assert BO.reach((1, 1, 3), 2) == [2, 2, 0] and all(d[2] == 0 for d in BO.ball_offsets((1, 1, 3), 2))
    assert BO.reach((0.41, 0.41, 1.5), 13.0) == [31, 31, 8] and BO.reach((0.25, 1, 1), 8) == [32, 8, 8]
    assert BO.ball_array((0.5, 0.5, 1.5), 2).shape == (9, 9, 3)
    for r, want in ((2.0, 1.7e-2), (2.5, 4.8e-3), (5.0, 1.9e-3)):
        assert BO.tie_margin((0.41, 0.41, 1.5), r) == pytest.approx(want, rel=0.05)
    assert BO.tie_margin((0.41, 0.41, 1.5), 1.5) == 0 and BO.tie_margin((0.41, 0.41, 1.5), 3.0) == 0  # exact ties along z


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_oracle_agrees_with_scipy(shape, spacing):
    nd = pytest.importorskip("scipy.ndimage")
    for density in (0.05, 0.3, 0.7, 0.95):
        mask = random_mask(shape, density)
        for r in RADII:
            st = BO.ball_array(spacing, r)
            dil = nd.binary_dilation(mask, st, border_value=0)
            ero = nd.binary_erosion(mask, st, border_value=1)
            np.testing.assert_array_equal(BO.dilate(mask, spacing, r), dil)
            np.testing.assert_array_equal(BO.erode(mask, spacing, r), ero)
            np.testing.assert_array_equal(BO.close(mask, spacing, r), nd.binary_erosion(dil, st, border_value=1))
            np.testing.assert_array_equal(BO.open_(mask, spacing, r), nd.binary_dilation(ero, st, border_value=0))


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_oracle_agrees_with_the_distance_transform(shape, spacing):
    """dilate(M) = {distance to M <= r}, erode(M) = {distance to the background of the volume > r}, with scipy's exact Euclidean transform at the same sampling.
    Unit and dyadic spacings: the squared distances are exact in fp64, so `<=` decides ties as the ball does."""
    nd = pytest.importorskip("scipy.ndimage")
    for density in (0.1, 0.9):
        mask = random_mask(shape, density, seed=1)
        for r in RADII:
            if mask.any():
                d = nd.distance_transform_edt(~mask, sampling=spacing)
                np.testing.assert_array_equal(BO.dilate(mask, spacing, r), d * d <= r * r + 1e-9)
            else:
                assert not BO.dilate(mask, spacing, r).any()
            if not mask.all():
                d = nd.distance_transform_edt(mask, sampling=spacing)
                np.testing.assert_array_equal(BO.erode(mask, spacing, r), d * d > r * r + 1e-9)
            else:
                assert BO.erode(mask, spacing, r).all()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("spacing", SPACINGS)
def test_oracle_properties(shape, spacing):
    for density in (0.1, 0.5, 0.9):
        mask = random_mask(shape, density, seed=2)
        for r in RADII:
            closed, opened = BO.close(mask, spacing, r), BO.open_(mask, spacing, r)
            assert not (mask & ~closed).any() and not (opened & ~mask).any()  # close contains M contains open, also at the border of the volume
            np.testing.assert_array_equal(BO.close(closed, spacing, r), closed)  # idempotent
            np.testing.assert_array_equal(BO.open_(opened, spacing, r), opened)
            np.testing.assert_array_equal(BO.erode(mask, spacing, r), ~BO.dilate(~mask, spacing, r))  # duality inside the volume
            assert not (mask & ~BO.dilate(mask, spacing, r)).any() and not (BO.erode(mask, spacing, r) & ~mask).any()
    for op in BO.OPS.values():
        for r in [0.0] + RADII:
            assert not op(np.zeros(shape, bool), spacing, r).any() and op(np.ones(shape, bool), spacing, r).all()
        np.testing.assert_array_equal(op(mask, spacing, 0.0), mask)
    np.testing.assert_array_equal(BO.stats(mask, closed), [mask.sum(), closed.sum(), closed.sum() - mask.sum(), 0])
    np.testing.assert_array_equal(BO.stats(mask, opened), [mask.sum(), opened.sum(), 0, mask.sum() - opened.sum()])


# ---------------------------------------------------------------- the route of the kernels, restated in numpy
def _fmaf(a, c):
    """fl32(a * a + c) for fp32 arrays: the product of two fp32 values is exact in fp64, and the fp64 sum of it and an fp32 value is rounded once more to fp32."""
    return (np.asarray(a, np.float64) ** 2 + np.asarray(c, np.float64)).astype(np.float32)


def _banded_min(g, axis, s, h, first):
    """out[i] = min over |d| <= h, i + d inside the array, of fl32((s d)^2 + g[i + d]) (first: fl32((s d)^2) where g[i + d] == 0, the z step)."""
    out = np.full(g.shape, np.inf, np.float32)
    n = g.shape[axis]
    for d in range(-h, h + 1):
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[axis], dst[axis] = slice(max(0, d), n + min(0, d)), slice(max(0, -d), n - max(0, d))
        if src[axis].stop <= src[axis].start:
            continue
        a = np.float32(s) * np.float32(d)
        cand = np.where(g[tuple(src)] == 0, np.float32(a * a), np.float32(np.inf)) if first else _fmaf(a, g[tuple(src)])
        out[tuple(dst)] = np.minimum(out[tuple(dst)], cand)
    return out


def _stage(mask, box, erode, spacing, h, t2):
    """One stage of csrc/ball.hip.  Features: inside the work box, the voxels of the mask (dilation) or its background (erosion); inside the volume but outside the
    box, nothing (dilation) or everything (erosion); the result is formed inside the box only."""
    feat = np.full(mask.shape, erode)
    feat[box] = mask[box] != erode
    g = np.where(feat, np.float32(0), np.float32(np.inf))
    g = _banded_min(g, 2, spacing[2], h[2], True)
    g = _banded_min(g, 1, spacing[1], h[1], False)
    g = _banded_min(g, 0, spacing[0], h[0], False)
    out = np.zeros(mask.shape, bool)
    out[box] = ((g <= t2) != erode)[box]
    return out


def kernel_route(mask, spacing, r, op):
    if not mask.any():
        return np.zeros(mask.shape, bool)
    s32 = np.asarray(spacing, np.float32)
    h = [k + 1 for k in BO.reach(spacing, r)]
    t2 = np.float32(float(r) * float(r))
    box = tuple(slice(max(int(i.min()) - k, 0), min(int(i.max()) + k, n - 1) + 1) for i, k, n in zip(np.nonzero(mask), h, mask.shape))
    first = op in ("erode", "open")
    out = _stage(mask, box, first, s32, h, t2)
    if op in ("close", "open"):
        out = _stage(out, box, not first, s32, h, t2)
    return out


@pytest.mark.parametrize("op", list(BO.OPS))
@pytest.mark.parametrize("spacing,radii", [((1.0, 1.0, 1.0), (0.0, 1.0, 1.5, 2.0, 3.0)), ((0.5, 0.5, 1.5), (1.5, 2.0)), ((1.0, 1.0, 3.0), (2.0,)), ((0.41, 0.41, 1.5), (2.0, 2.5))])
def test_kernel_route_equals_the_definition(op, spacing, radii):
    for shape in SHAPES:
        for density in ((0.02, 0.3) if op in ("dilate", "close") else (0.7, 0.97)):
            mask = random_mask(shape, density, seed=3)
            inner = np.zeros_like(mask)  # the mask cut to a box inside the volume: the work box then has faces off the border
            cut = tuple(slice(n // 4, max(n // 4 + 1, 3 * n // 4)) for n in shape)
            inner[cut] = mask[cut]
            for m in (mask, inner):
                for r in radii:
                    np.testing.assert_array_equal(kernel_route(m, spacing, r, op), BO.OPS[op](m, spacing, r), err_msg=f"{op} {shape} {density} {spacing} {r}")


# ---------------------------------------------------------------- the ABI
def test_abi_version_and_symbols():
    from vs_seg_amd import _lib as L

    lib = L.lib()
    assert lib.vsseg_version() >= 22
    for name in ("vsseg_ball_scratch_bytes", "vsseg_ball_morphology"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes
    assert (L.OP_DILATE, L.OP_ERODE, L.OP_CLOSE, L.OP_OPEN) == (0, 1, 2, 3)
    header = open("include/vsseg_hip.h").read()
    header = re.sub(r"static inline[^{]*\{.*?\n\}", "", header, flags=re.S)
    declared = set(re.findall(r"\b(vsseg_[a-z0-9_]+)\s*\(", header))
    assert {"vsseg_ball_scratch_bytes", "vsseg_ball_morphology"} <= declared
    for name in declared:  # every header-declared name is bound
        assert name in L.SYMBOLS and getattr(lib, name) is not None, name
    assert len(L.SYMBOLS) == len(set(L.SYMBOLS)) == 89


def test_scratch_bytes():
    from vs_seg_amd import _lib as L

    lib = L.lib()
    small, big = lib.vsseg_ball_scratch_bytes(L.i3((4, 4, 4))), lib.vsseg_ball_scratch_bytes(L.i3((512, 512, 120)))
    assert 0 < small < 4096 and small % 256 == 0
    n = 512 * 512 * 120
    assert 6 * n <= big <= 6 * n + 4096 and big % 256 == 0  # a record, one fp32 field and two byte masks
    for bad in ((0, 4, 4), (4, 4, 8193), (2048, 2048, 512)):
        assert lib.vsseg_ball_scratch_bytes(L.i3(bad)) == L.EINVAL
        assert b"vsseg_ball_scratch_bytes" in lib.vsseg_last_error() and b"dims" in lib.vsseg_last_error()


def test_c_entry_point_rejects_calls_outside_its_domain():
    import ctypes

    from vs_seg_amd import _lib as L
    from vs_seg_amd._volume import float3

    lib = L.lib()
    d = L.i3((4, 4, 4))
    need = lib.vsseg_ball_scratch_bytes(d)
    sp = float3((0.5, 0.5, 1.5))
    # (fake, aligned device addresses: every call below is rejected before anything is launched)
    # arguments: logits, pitch, dims, spacing, op, radius_mm, scratch, scratch_bytes, out, stats
    good = (8, 2, d, sp, 2, 2.0, 256, need, 16, 32)

    def bad(why, *message, **change):
        names = ("logits", "pitch", "dims", "spacing", "op", "radius_mm", "scratch", "scratch_bytes", "out", "stats")
        args = [change.get(n, v) for n, v in zip(names, good)]
        assert lib.vsseg_ball_morphology(*args, None) == L.EINVAL, (why, change)
        err = lib.vsseg_last_error()
        assert b"vsseg_ball_morphology" in err and why in err and all(m in err for m in message), (why, message, err)

    bad(b"null", logits=None)
    bad(b"null", spacing=None)
    bad(b"null", scratch=None)
    bad(b"null", out=None)
    bad(b"misaligned", logits=4)
    bad(b"misaligned", out=20)
    bad(b"misaligned", stats=36)
    bad(b"misaligned", scratch=128)
    bad(b"pitch", b"3", pitch=3)
    bad(b"pitch", b"1", pitch=1)
    bad(b"dims", dims=L.i3((0, 4, 4)))
    bad(b"dims", dims=L.i3((4, 4, 9000)))
    bad(b"dims", dims=L.i3((2048, 2048, 512)), scratch_bytes=1 << 40)
    bad(b"spacing[1]", b"-1", spacing=float3((1.0, -1.0, 1.0)))
    bad(b"spacing[0]", b"0", spacing=float3((0.0, 1.0, 1.0)))
    bad(b"spacing[2]", b"nan", spacing=float3((1.0, 1.0, float("nan"))))
    bad(b"spacing[2]", b"inf", spacing=float3((1.0, 1.0, float("inf"))))
    bad(b"op", b"4", op=4)
    bad(b"op", b"-1", op=-1)
    bad(b"radius_mm", b"-0.5", radius_mm=-0.5)
    bad(b"radius_mm", b"nan", radius_mm=float("nan"))
    bad(b"radius_mm", b"inf", radius_mm=float("inf"))
    bad(b"reaches 33 voxels along axis 0", b"16.5", radius_mm=16.5)  # 16.5 / 0.5
    bad(b"reaches 33 voxels along axis 2", b"33", radius_mm=33.0, spacing=float3((2.0, 2.0, 1.0)))
    bad(b"scratch", str(need - 1).encode(), scratch_bytes=need - 1)
    bad(b"scratch", scratch_bytes=0, stats=None)
    assert ctypes.sizeof(sp) == 12


# ---------------------------------------------------------------- the Python functions: argument checks before the device check
@pytest.mark.parametrize("fn", CALLS)
def test_bad_arguments_raise_value_error(fn):
    good = torch.zeros(1, 2, 8, 8, 4)
    for bad in (torch.zeros(2, 8, 8, 4), torch.zeros(1, 2, 8, 8), torch.zeros(1, 3, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4), "mask"):
        with pytest.raises(ValueError, match="outputs"):
            fn(bad, 1.0)
    for bad in (True, -1.0, float("nan"), float("inf"), None, "2", [2.0]):
        with pytest.raises(ValueError, match="radius_mm"):
            fn(good, bad)
    for bad in ((1.0, 1.0), (1.0, 1.0, 0.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0), "abc", 1.0):
        with pytest.raises(ValueError, match="spacing"):
            fn(good, 1.0, bad)
    with pytest.raises(ValueError, match="33 voxels along axis 1"):
        fn(good, 33.0, (2.0, 1.0, 2.0))
    with pytest.raises(ValueError, match="axis 0"):
        fn(good, 13.6, (0.41, 0.41, 1.5))  # 13.6 / 0.41 = 33.2


@pytest.mark.parametrize("fn", CALLS)
def test_cpu_tensors_raise_runtime_error(fn):
    with pytest.raises(RuntimeError, match="runs on an MI355X only"):
        fn(torch.zeros(1, 2, 8, 8, 4), 1.0)
    with pytest.raises(RuntimeError, match="vs_seg_amd." + fn.__name__):
        fn(torch.zeros(1, 2, 8, 8, 4), 32, spacing=np.asarray((1.0, 1.0, 1.5)), return_stats=True)  # a reach of exactly 32 is in the domain


def test_signatures_and_exports():
    import inspect

    import vs_seg_amd

    for fn in CALLS:
        assert list(inspect.signature(fn).parameters) == ["outputs", "radius_mm", "spacing", "return_stats"]
        assert inspect.signature(fn).parameters["spacing"].default is None and inspect.signature(fn).parameters["return_stats"].default is False
        assert getattr(vs_seg_amd, fn.__name__) is fn and fn.__name__ in vs_seg_amd.__all__ and fn.__doc__


# ---------------------------------------------------------------- flags
def test_command_line_flags():
    from vs_seg_amd.params import VSparams

    def parse(argv):
        try:
            return VSparams(argparse.ArgumentParser(), argv)
        except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
            assert "no GPU" in str(e)
            return None

    for bad in (["--closing_mm", "-1"], ["--closing_mm", "nan"], ["--closing_mm", "inf"], ["--closing_mm", "wide"], ["--closing_mm"], ["--opening_mm", "-0.5"], ["--opening_mm", "nan"],
                ["--opening_mm"]):
        with pytest.raises(SystemExit):
            parse(bad)
    for argv, want in (([], (0.0, 0.0)), (["--closing_mm", "2"], (2.0, 0.0)), (["--opening_mm", "1.5"], (0.0, 1.5)), (["--closing_mm", "0"], (0.0, 0.0)),
                       (["--closing_mm", "2", "--opening_mm", "1", "--fill_holes", "--min_component_mm3", "10", "--keep_largest_component", "--measurements"], (2.0, 1.0))):
        p = parse(argv)
        if p is not None:
            assert (p.closing_mm, p.opening_mm) == want


def test_csv_header_for_each_flag_combination():
    from vs_seg_amd.params import postprocessing_csv_header

    old = "case,dice_raw,dice,components,foreground_voxels,kept_voxels"
    olds = {(False, False): old, (True, False): old + ",holes,filled_voxels", (False, True): old + ",small_components,small_voxels",
            (True, True): old + ",holes,filled_voxels,small_components,small_voxels"}
    for (fill, small), want in olds.items():
        assert postprocessing_csv_header(fill, small) == want  # the two-argument calls return what they returned
        assert postprocessing_csv_header(fill, small, closing=False, opening=False) == want
        assert postprocessing_csv_header(fill, small, closing=True) == want + ",closed_voxels"
        assert postprocessing_csv_header(fill, small, opening=True) == want + ",opened_voxels"
        assert postprocessing_csv_header(fill, small, closing=True, opening=True) == want + ",closed_voxels,opened_voxels"
        assert postprocessing_csv_header(fill, small, True, True) == want + ",closed_voxels,opened_voxels"
