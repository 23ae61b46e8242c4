"""CPU tests of the hole filling and the size filter: the numpy oracle (tests/morphology_oracle.py) against scipy.ndimage and known answers, the argument checks
of vs_seg_amd.fill_holes / remove_small_components (made before the device check) and of the two C entry points (made before any launch), and the flags."""
import argparse
import math

import numpy as np
import pytest
import torch

from tests import components_oracle as CO
from tests import morphology_oracle as MO
from tests.test_components_host import random_mask
from vs_seg_amd import fill_holes, min_component_voxels, remove_small_components

SHAPES = [(37, 29, 11), (64, 48, 16), (9, 17, 130)]  # every axis straddles the 4 x 8 x 64 tile somewhere; Z = 130 crosses two z seams
FILL_DENSITIES = [0.2, 0.35, 0.6, 0.8, 0.9]
SMALL_DENSITIES = [0.05, 0.2]
CONNECTIVITIES = [6, 18, 26]
RANK = {6: 1, 18: 2, 26: 3}


# ---------------------------------------------------------------- known answers: name -> (mask, {connectivity: expected filled mask})
def _shell(shape=(14, 13, 12)):
    m = np.zeros(shape, bool)
    m[3:10, 3:10, 3:9] = True
    m[4:9, 4:9, 4:8] = False  # the cavity: 5 x 5 x 4 = 100 voxels
    return m


def _solid(shape=(14, 13, 12)):
    m = np.zeros(shape, bool)
    m[3:10, 3:10, 3:9] = True
    return m


def known_answers():
    """name -> (mask, expected result per connectivity).  Shared with the GPU tests."""
    same = lambda want: {c: want for c in CONNECTIVITIES}  # noqa: E731
    cases = {"hollow_box": (_shell(), same(_solid()))}
    tunnel = _shell()
    tunnel[9, 6, 6] = False  # a one-voxel straight tunnel through the wall: open at every connectivity
    cases["straight_tunnel"] = (tunnel, same(tunnel))
    gap = _shell()
    gap[9, 9, 7] = False  # an edge voxel of the shell: it touches the cavity's voxel (8, 8, 7) by a diagonal step only
    closed = _solid()
    closed[9, 9, 7] = False
    cases["diagonal_gap"] = (gap, {6: closed, 18: gap, 26: gap})
    kernel = _shell()
    kernel[6, 6, 5:7] = True  # a separate kernel inside the cavity
    cases["kernel_in_cavity"] = (kernel, same(_solid()))
    cut = np.zeros((14, 13, 12), bool)
    cut[0:6, 3:10, 3:9] = True
    cut[0:5, 4:9, 4:8] = False  # the cavity reaches the face x = 0 of the volume
    cases["cut_by_a_face"] = (cut, same(cut))
    ring = np.zeros((14, 13, 12), bool)
    ring[4:9, 4:9, 5] = True
    ring[5:8, 5:8, 5] = False
    cases["ring"] = (ring, same(ring))
    cases["empty"] = (np.zeros((7, 9, 5), bool), same(np.zeros((7, 9, 5), bool)))
    cases["all_foreground"] = (np.ones((7, 9, 5), bool), same(np.ones((7, 9, 5), bool)))
    flat = np.zeros((9, 9, 1), bool)
    flat[2:7, 2:7, 0] = True
    flat[3:6, 3:6, 0] = False  # enclosed in the plane, but every voxel of an extent of 1 lies on the border
    cases["extent_one"] = (flat, same(flat))
    thin = np.ones((9, 2, 9), bool)
    thin[4, :, 4] = False
    cases["extent_two"] = (thin, same(thin))
    return cases


KNOWN = known_answers()


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", FILL_DENSITIES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_fill_oracle_agrees_with_scipy(shape, density, connectivity):
    nd = pytest.importorskip("scipy.ndimage")
    mask = random_mask(shape, density)
    st = nd.generate_binary_structure(3, RANK[connectivity])
    want = nd.binary_fill_holes(mask, st)
    got = MO.fill_holes(mask, connectivity)
    np.testing.assert_array_equal(got, want)
    stats = MO.fill_stats(mask, connectivity)
    assert stats[0] == mask.sum() and stats[2] == (want & ~mask).sum() and stats[3] == want.sum()
    assert stats[1] == nd.label(want & ~mask, st)[1]  # the holes are whole components of the complement: labelling them alone counts them
    if density == 0.9:
        assert stats[2] > 0 and stats[1] > 0  # the random masks have holes to fill: an identity implementation cannot pass


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", SMALL_DENSITIES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_size_filter_oracle_agrees_with_scipy(shape, density, connectivity):
    nd = pytest.importorskip("scipy.ndimage")
    mask = random_mask(shape, density)
    lab, n = nd.label(mask, nd.generate_binary_structure(3, RANK[connectivity]))
    counts = np.bincount(lab.ravel())
    for min_voxels in (0, 1, 2, 4, 50):
        ok = counts >= min_voxels
        ok[0] = False
        np.testing.assert_array_equal(MO.remove_small(mask, min_voxels, connectivity), ok[lab])
        np.testing.assert_array_equal(MO.small_stats(mask, min_voxels, connectivity), [mask.sum(), n, counts[1:][ok[1:]].sum(), ok.sum()])
    if density == 0.05:
        st = MO.small_stats(mask, 4, connectivity)
        assert st[3] < st[1] and st[2] < st[0]  # min_voxels = 4 removes at least one component


@pytest.mark.parametrize("name", list(KNOWN))
def test_fill_oracle_known_answers(name):
    mask, want = KNOWN[name]
    for c in CONNECTIVITIES:
        np.testing.assert_array_equal(MO.fill_holes(mask, c), want[c], err_msg=f"{name} at {c}")
        st = MO.fill_stats(mask, c)
        assert st[0] == mask.sum() and st[2] == (want[c] & ~mask).sum() and st[3] == want[c].sum()


def test_fill_oracle_known_counts():
    np.testing.assert_array_equal(MO.fill_stats(KNOWN["hollow_box"][0], 6), [7 * 7 * 6 - 100, 1, 100, 7 * 7 * 6])
    np.testing.assert_array_equal(MO.fill_stats(KNOWN["diagonal_gap"][0], 6), [7 * 7 * 6 - 101, 1, 100, 7 * 7 * 6 - 1])
    np.testing.assert_array_equal(MO.fill_stats(KNOWN["diagonal_gap"][0], 26), [7 * 7 * 6 - 101, 0, 0, 7 * 7 * 6 - 101])
    kernel = KNOWN["kernel_in_cavity"][0]
    np.testing.assert_array_equal(MO.fill_stats(kernel, 6), [7 * 7 * 6 - 98, 1, 98, 7 * 7 * 6])
    assert CO.stats(CO.label(kernel, 26))[1] == 2 and CO.stats(CO.label(MO.fill_holes(kernel, 6), 26))[1] == 1  # shell + kernel come out as one solid
    two = _shell((14, 13, 24))
    two[3:10, 3:10, 13:19] = True
    two[5:8, 5:8, 14:18] = False  # a second shell with a 3 x 3 x 4 cavity
    np.testing.assert_array_equal(MO.fill_stats(two, 6), [2 * 7 * 7 * 6 - 136, 2, 136, 2 * 7 * 7 * 6])
    with pytest.raises(ValueError):
        MO.fill_holes(two, 8)


def test_size_filter_known_answers():
    m = np.zeros((12, 10, 6), bool)
    m[0, 0, 0] = True  # 1 voxel
    m[2:4, 2:4, 2:4] = True  # 8 voxels
    m[7:9, 5:7, 1:3] = True  # 8 voxels: equal-sized components are treated alike
    m[10, 1:4, 5] = True  # 3 voxels
    cubes = np.zeros_like(m)
    cubes[2:4, 2:4, 2:4] = cubes[7:9, 5:7, 1:3] = True
    for c in CONNECTIVITIES:
        for mv in (0, 1):  # the identity
            np.testing.assert_array_equal(MO.remove_small(m, mv, c), m)
            np.testing.assert_array_equal(MO.small_stats(m, mv, c), [20, 4, 20, 4])
        np.testing.assert_array_equal(MO.remove_small(m, 3, c), m & ~(np.arange(12)[:, None, None] == 0))  # a component of exactly min_voxels voxels stays
        np.testing.assert_array_equal(MO.small_stats(m, 3, c), [20, 4, 19, 3])
        np.testing.assert_array_equal(MO.remove_small(m, 4, c), cubes)  # ... and min_voxels + 1 removes it
        np.testing.assert_array_equal(MO.small_stats(m, 4, c), [20, 4, 16, 2])
        np.testing.assert_array_equal(MO.remove_small(m, 8, c), cubes)
        assert not MO.remove_small(m, 9, c).any()  # both cubes go together; a threshold above every size leaves nothing
        np.testing.assert_array_equal(MO.small_stats(m, 9, c), [20, 4, 0, 0])
        np.testing.assert_array_equal(CO.one_hot(MO.remove_small(m, 2**40, c)), CO.one_hot(np.zeros_like(m)))
    assert not MO.remove_small(np.zeros((4, 4, 4), bool), 0).any()
    np.testing.assert_array_equal(MO.small_stats(np.zeros((4, 4, 4), bool), 3), [0, 0, 0, 0])


def _fill_inside_box(mask, connectivity):
    """What the kernels do (csrc/components.hip): label the complement inside the bounding box of the mask only; the components without a voxel on a face of the BOX are the holes."""
    if not mask.any():
        return mask.copy()
    box = tuple(slice(int(i.min()), int(i.max()) + 1) for i in np.nonzero(mask))
    out = mask.copy()
    out[box] = MO.fill_holes(mask[box], connectivity)  # (the oracle takes the faces of the array it is given: here the box)
    return out


@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_box_restricted_route_equals_the_definition(connectivity):
    for name, (mask, want) in KNOWN.items():
        np.testing.assert_array_equal(_fill_inside_box(mask, connectivity), want[connectivity], err_msg=name)
    rng = np.random.default_rng(connectivity)
    for shape in SHAPES[:2]:
        for density in (0.6, 0.9):
            mask = random_mask(shape, density)
            lo, hi = [int(rng.integers(0, s // 2)) for s in shape], [int(rng.integers(s // 2 + 1, s + 1)) for s in shape]
            inner = np.zeros_like(mask)  # the mask cut to a box inside the volume: its own box has faces off the border
            inner[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = mask[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]
            for m in (mask, inner):
                np.testing.assert_array_equal(_fill_inside_box(m, connectivity), MO.fill_holes(m, connectivity))


# ---------------------------------------------------------------- the Python functions: argument checks before the device check
def _call(fn, x, **kw):
    return fn(x, 4, **kw) if fn is remove_small_components else fn(x, **kw)


@pytest.mark.parametrize("fn", [fill_holes, remove_small_components])
def test_bad_arguments_raise_value_error(fn):
    good = torch.zeros(1, 2, 8, 8, 4)
    for bad in (torch.zeros(2, 8, 8, 4), torch.zeros(1, 2, 8, 8), torch.zeros(1, 3, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4)):
        with pytest.raises(ValueError):
            _call(fn, bad)
    for conn in (4, 27, "full", 26.0, None, True):
        with pytest.raises(ValueError):
            _call(fn, good, connectivity=conn)


def test_bad_min_voxels_raises_value_error():
    for bad in (-1, 2.5, None, "3", True, 2**63):
        with pytest.raises(ValueError, match="min_voxels"):
            remove_small_components(torch.zeros(1, 2, 8, 8, 4), bad)


@pytest.mark.parametrize("fn", [fill_holes, remove_small_components])
def test_cpu_tensors_raise_runtime_error(fn):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(fn, torch.zeros(1, 2, 8, 8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _call(fn, torch.zeros(1, 2, 8, 8, 4), connectivity=18, return_stats=True)


def test_defaults():
    import inspect

    assert inspect.signature(fill_holes).parameters["connectivity"].default == 6
    assert inspect.signature(remove_small_components).parameters["connectivity"].default == 26
    assert inspect.signature(remove_small_components).parameters["min_voxels"].default is inspect.Parameter.empty


def test_c_entry_points_reject_calls_outside_their_domain():
    from vs_seg_amd import _lib as L

    lib = L.lib()
    assert lib.vsseg_version() >= 18
    for name in ("vsseg_fill_holes", "vsseg_remove_small_components"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes
    d = L.i3((4, 4, 4))
    need = lib.vsseg_components_scratch_bytes(d)  # the new entry points use the scratch of the old ones
    assert need > 0
    # (fake, aligned device addresses: every call below is rejected before anything is launched)
    # arguments: logits, pitch, dims, connectivity, scratch, scratch_bytes, out, stats
    cases = [((8, 3, d, 26, 256, need, 16, 32), b"pitch"), ((8, 1, d, 26, 256, need, 16, 32), b"pitch"), ((8, 2, L.i3((4, 4, 9000)), 26, 256, need, 16, 32), b"dims"),
             ((8, 2, L.i3((0, 4, 4)), 26, 256, need, 16, 32), b"dims"), ((8, 2, L.i3((2048, 2048, 512)), 26, 256, 1 << 40, 16, 32), b"dims"), ((8, 2, d, 4, 256, need, 16, 32), b"connectivity"),
             ((8, 2, d, 27, 256, need, 16, 32), b"connectivity"), ((8, 2, d, 26, 256, need - 1, 16, 32), b"scratch"), ((8, 2, d, 6, 256, 0, 16, None), b"scratch"),
             ((None, 2, d, 26, 256, need, 16, 32), b"null"), ((8, 2, d, 26, None, need, 16, 32), b"null"), ((8, 2, d, 26, 256, need, None, 32), b"null"),
             ((4, 2, d, 26, 256, need, 16, 32), b"misaligned"), ((8, 2, d, 26, 128, need, 16, 32), b"misaligned"), ((8, 2, d, 26, 256, need, 20, 32), b"misaligned"),
             ((8, 2, d, 26, 256, need, 16, 36), b"misaligned")]
    for name, extra in (("vsseg_fill_holes", ()), ("vsseg_remove_small_components", (4,))):
        fn = getattr(lib, name)
        for args, why in cases:
            assert fn(*args[:4], *extra, *args[4:], None) == L.EINVAL, (name, args)
            err = lib.vsseg_last_error()
            assert name.encode() in err and why in err, (name, why, err)
    for bad in (-1, -(2**62)):
        assert lib.vsseg_remove_small_components(8, 2, d, 26, bad, 256, need, 16, 32, None) == L.EINVAL
        assert b"vsseg_remove_small_components" in lib.vsseg_last_error() and b"min_voxels" in lib.vsseg_last_error()


# ---------------------------------------------------------------- flags
def test_command_line_flags():
    from vs_seg_amd.params import VSparams

    def parse(argv):
        try:
            return VSparams(argparse.ArgumentParser(), argv)
        except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
            assert "no GPU" in str(e)
            return None

    for bad in (["--fill_holes", "yes"], ["--hole_connectivity", "8"], ["--hole_connectivity", "six"], ["--min_component_mm3", "-1"], ["--min_component_mm3", "nan"],
                ["--min_component_mm3", "inf"], ["--min_component_mm3", "big"], ["--min_component_mm3"]):
        with pytest.raises(SystemExit):
            parse(bad)
    for argv, want in (([], (False, 6, 0.0)), (["--fill_holes"], (True, 6, 0.0)), (["--fill_holes", "--hole_connectivity", "26"], (True, 26, 0.0)),
                       (["--min_component_mm3", "12.5", "--component_connectivity", "6"], (False, 6, 12.5)),
                       (["--fill_holes", "--min_component_mm3", "0", "--keep_largest_component", "--measurements", "--surface_metrics"], (True, 6, 0.0))):
        p = parse(argv)
        if p is not None:
            assert (p.fill_holes, p.hole_connectivity, p.min_component_mm3) == want


def test_min_voxels_formula():
    spacing = (0.41, 0.41, 1.5)
    voxel = float(np.float32(0.41)) * float(np.float32(0.41)) * float(np.float32(1.5))  # fp64 product of the fp32 spacing, as vsseg_measurements forms it
    assert voxel != 0.41 * 0.41 * 1.5 and voxel == pytest.approx(0.25215, rel=1e-6)
    assert min_component_voxels(0.0, spacing) == 0
    assert min_component_voxels(10.0, spacing) == math.ceil(10.0 / voxel) == 40
    assert min_component_voxels(1e-9, spacing) == 1
    assert min_component_voxels(3 * voxel, spacing) == 3 and min_component_voxels(np.nextafter(3 * voxel, np.inf), spacing) == 4
    assert min_component_voxels(100, (1.0, 1.0, 1.0)) == 100 and isinstance(min_component_voxels(100, (1.0, 1.0, 1.0)), int)
    assert min_component_voxels(10.0, np.asarray(spacing)) == 40
    for bad in (-1.0, float("nan"), float("inf"), None, "3"):
        with pytest.raises(ValueError):
            min_component_voxels(bad, spacing)
    for bad in ((1.0, 0.0, 1.0), (1.0, -1.0, 1.0), (1.0, float("nan"), 1.0)):
        with pytest.raises(ValueError):
            min_component_voxels(1.0, bad)


def test_csv_header_for_each_flag_combination():
    from vs_seg_amd.params import postprocessing_csv_header

    old = "case,dice_raw,dice,components,foreground_voxels,kept_voxels"
    assert postprocessing_csv_header(False, False) == old
    assert postprocessing_csv_header(True, False) == old + ",holes,filled_voxels"
    assert postprocessing_csv_header(False, True) == old + ",small_components,small_voxels"
    assert postprocessing_csv_header(True, True) == old + ",holes,filled_voxels,small_components,small_voxels"
