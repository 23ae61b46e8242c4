"""CPU tests of the connected-component post-processing: the numpy oracle against scipy.ndimage.label and known answers, and the argument checks of
vs_seg_amd.connected_components / keep_largest_component (made before the device check) and of the three C entry points (made before any launch)."""
import numpy as np
import pytest
import torch

from tests import components_oracle as CO
from vs_seg_amd import connected_components, keep_largest_component

SHAPES = [(37, 29, 11), (64, 48, 16)]
DENSITIES = [0.05, 0.2, 0.35, 0.6]
CONNECTIVITIES = [6, 18, 26]


def random_mask(shape, density):
    return np.random.default_rng(sum(shape) + round(100 * density)).random(shape) < density


def n_components(mask, connectivity):
    return int(CO.stats(CO.label(mask, connectivity))[1])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("density", DENSITIES)
@pytest.mark.parametrize("connectivity", CONNECTIVITIES)
def test_oracle_agrees_with_scipy(shape, density, connectivity):
    nd = pytest.importorskip("scipy.ndimage")
    mask = random_mask(shape, density)
    got = CO.label(mask, connectivity)
    assert got.dtype == np.int32 and got.shape == mask.shape
    lab, n = nd.label(mask, nd.generate_binary_structure(3, {6: 1, 18: 2, 26: 3}[connectivity]))
    first = nd.minimum(np.arange(mask.size).reshape(shape), lab, np.arange(1, n + 1))  # smallest linear index per scipy label
    want = np.concatenate([[0], np.asarray(first, np.int64) + 1])[lab]
    np.testing.assert_array_equal(got, want)
    st = CO.stats(got)
    counts = np.bincount(lab.ravel())[1:]
    assert st[0] == mask.sum() and st[1] == n and st[2] == counts.max()
    assert st[3] == min(int(first[i]) + 1 for i in np.flatnonzero(counts == counts.max()))  # ties: the component met first in raster order


def test_oracle_known_answers():
    checker = np.indices((8, 8, 8)).sum(0) % 2 == 0
    assert [n_components(checker, c) for c in CONNECTIVITIES] == [256, 1, 1]
    i = np.arange(48)
    chain = np.zeros((48, 48, 48), bool)
    chain[i, i, i] = True
    assert [n_components(chain, c) for c in CONNECTIVITIES] == [48, 48, 1]
    flat = np.zeros((48, 48, 5), bool)
    flat[i, i, 2] = True
    assert [n_components(flat, c) for c in CONNECTIVITIES] == [48, 1, 1]
    m = np.zeros((12, 10, 6), bool)
    m[0, 0, 0] = True
    m[2:4, 2:4, 2:4] = True
    m[7:9, 5:7, 1:3] = True
    for c in CONNECTIVITIES:
        lab = CO.label(m, c)
        first = (2 * 10 + 2) * 6 + 2 + 1  # the label of the cube at (2, 2, 2): the two cubes tie, the first in raster order is kept
        np.testing.assert_array_equal(CO.stats(lab), [17, 3, 8, first])
        keep = np.zeros_like(m)
        keep[2:4, 2:4, 2:4] = True
        np.testing.assert_array_equal(CO.keep_largest(m, c), keep)
    empty = np.zeros((5, 4, 3), bool)
    np.testing.assert_array_equal(CO.stats(CO.label(empty)), [0, 0, 0, 0])
    assert not CO.keep_largest(empty).any()
    with pytest.raises(ValueError):
        CO.label(m, 8)


@pytest.mark.parametrize("fn", [connected_components, keep_largest_component])
def test_bad_arguments_raise_value_error(fn):
    good = torch.zeros(1, 2, 8, 8, 4)
    for bad in (torch.zeros(2, 8, 8, 4), torch.zeros(1, 2, 8, 8), torch.zeros(1, 3, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4)):
        with pytest.raises(ValueError):
            fn(bad)
    for conn in (4, 27, "full", 26.0, None):
        with pytest.raises(ValueError):
            fn(good, connectivity=conn)


@pytest.mark.parametrize("fn", [connected_components, keep_largest_component])
def test_cpu_tensors_raise_runtime_error(fn):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(torch.zeros(1, 2, 8, 8, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fn(torch.zeros(1, 2, 8, 8, 4), connectivity=6)


def test_c_entry_points_reject_calls_outside_their_domain():
    from vs_seg_amd import _lib as L

    lib = L.lib()
    assert lib.vsseg_version() >= 9
    assert lib.vsseg_components_scratch_bytes(L.i3((512, 512, 120))) >= 4 * 512 * 512 * 120
    for dims in ((0, 8, 8), (8, 8, 8193), (2048, 2048, 512)):  # the last one holds 2^31 voxels: more than int32 labels can name
        assert lib.vsseg_components_scratch_bytes(L.i3(dims)) == L.EINVAL
        assert b"vsseg_components_scratch_bytes" in lib.vsseg_last_error() and b"dims" in lib.vsseg_last_error()
    d = L.i3((4, 4, 4))
    need = lib.vsseg_components_scratch_bytes(d)
    assert need > 0
    # (fake, aligned device addresses: every call below is rejected before anything is launched)
    # arguments: logits, pitch, dims, connectivity, scratch, scratch_bytes, labels / out, stats
    cases = [((8, 3, d, 26, 256, need, 16, 32), b"pitch"), ((8, 2, L.i3((4, 4, 9000)), 26, 256, need, 16, 32), b"dims"), ((8, 2, L.i3((0, 4, 4)), 26, 256, need, 16, 32), b"dims"),
             ((8, 2, L.i3((2048, 2048, 512)), 26, 256, 1 << 40, 16, 32), b"dims"), ((8, 2, d, 4, 256, need, 16, 32), b"connectivity"), ((8, 2, d, 27, 256, need, 16, 32), b"connectivity"),
             ((8, 2, d, 26, 256, need - 1, 16, 32), b"scratch"), ((None, 2, d, 26, 256, need, 16, 32), b"null"), ((8, 2, d, 26, None, need, 16, 32), b"null"),
             ((8, 2, d, 26, 256, need, None, 32), b"null"), ((4, 2, d, 26, 256, need, 16, 32), b"misaligned"), ((8, 2, d, 26, 128, need, 16, 32), b"misaligned"),
             ((8, 2, d, 26, 256, need, 16, 36), b"misaligned")]
    for name in ("vsseg_components_label", "vsseg_keep_largest_component"):
        fn = getattr(lib, name)
        for args, why in cases:
            assert fn(*args, None) == L.EINVAL, (name, args)
            err = lib.vsseg_last_error()
            assert name.encode() in err and why in err, (name, why, err)
    assert lib.vsseg_components_label(8, 2, d, 26, 256, need, 18, 32, None) == L.EINVAL and b"misaligned" in lib.vsseg_last_error()  # labels: 4 B
    assert lib.vsseg_keep_largest_component(8, 2, d, 26, 256, need, 20, 32, None) == L.EINVAL and b"misaligned" in lib.vsseg_last_error()  # out: 8 B
    assert lib.vsseg_components_label(8, 2, d, 26, 256, need, 16, None, None) == L.EINVAL and b"null" in lib.vsseg_last_error()  # stats are not optional here
