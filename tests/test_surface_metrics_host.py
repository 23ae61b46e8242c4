"""CPU tests of the surface-distance metrics: voxel_spacing, argument checks (made before the device check), and the numpy oracle against
scipy's edge + distance-transform pipeline."""
import numpy as np
import pytest
import torch

from tests import surface_oracle as SO
from vs_seg_amd import compute_surface_distances, voxel_spacing


def test_voxel_spacing_is_the_column_norms():
    assert voxel_spacing(np.diag([-0.5, -0.5, 1.5, 1.0])) == pytest.approx((0.5, 0.5, 1.5))
    c, s = np.cos(0.3), np.sin(0.3)
    rot = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]])
    aff = np.eye(4)
    aff[:3, :3] = rot @ np.diag([0.41, 0.43, 1.5])
    aff[:3, 3] = [10.0, -4.0, 2.0]
    assert voxel_spacing(aff) == pytest.approx(tuple(np.linalg.norm(aff[:3, :3], axis=0)))
    assert voxel_spacing(aff) == pytest.approx((0.41, 0.43, 1.5))
    with pytest.raises(ValueError):
        voxel_spacing(np.eye(3))


@pytest.mark.parametrize("kw", [dict(percentile=-1.0), dict(percentile=100.5), dict(percentile=float("nan")), dict(percentile="high"),
                                dict(spacing=(1.0, 1.0)), dict(spacing=(1.0, 0.0, 1.0)), dict(spacing=(1.0, -2.0, 1.0)), dict(spacing=(1.0, float("inf"), 1.0)), dict(spacing=3.0)])
def test_bad_arguments_raise_value_error(kw):
    pred, lab = torch.zeros(1, 2, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4)
    with pytest.raises(ValueError):
        compute_surface_distances(pred, lab, **kw)


@pytest.mark.parametrize("pred_shape,lab_shape", [((1, 3, 8, 8, 4), (1, 1, 8, 8, 4)), ((1, 2, 8, 8, 4), (1, 1, 8, 8, 5)), ((2, 2, 8, 8, 4), (1, 1, 8, 8, 4)), ((2, 8, 8, 4), (2, 8, 8, 4))])
def test_mismatched_shapes_raise_value_error(pred_shape, lab_shape):
    with pytest.raises(ValueError):
        compute_surface_distances(torch.zeros(pred_shape), torch.zeros(lab_shape))


def test_cpu_tensors_raise_runtime_error():
    with pytest.raises(RuntimeError):
        compute_surface_distances(torch.zeros(1, 2, 8, 8, 4), torch.zeros(1, 1, 8, 8, 4), spacing=(0.5, 0.5, 1.5), percentile=None)


def _scipy_metrics(pred, gt, spacing, percentile):
    nd = pytest.importorskip("scipy.ndimage")
    st = nd.generate_binary_structure(3, 1)
    ep = nd.binary_erosion(pred, st, border_value=0) ^ pred
    eg = nd.binary_erosion(gt, st, border_value=0) ^ gt
    if not ep.any() and not eg.any():
        return float("nan"), float("nan")
    if not ep.any() or not eg.any():
        return float("inf"), float("inf")
    dpg = nd.distance_transform_edt(~eg, sampling=spacing)[ep]
    dgp = nd.distance_transform_edt(~ep, sampling=spacing)[eg]
    pct = (lambda d: d.max()) if percentile is None else (lambda d: np.percentile(d, percentile))
    return max(pct(dpg), pct(dgp)), (dpg.sum() + dgp.sum()) / (len(dpg) + len(dgp))


@pytest.mark.parametrize("seed", range(4))
def test_oracle_agrees_with_scipy(seed):
    pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    shape = (int(rng.integers(5, 20)), int(rng.integers(5, 20)), int(rng.integers(1, 9)))
    spacing = (1.0, 1.0, 1.0) if seed == 0 else tuple(rng.uniform(0.3, 2.0, 3))
    pred, gt = rng.random(shape) < 0.3, rng.random(shape) < 0.2
    for pc in (None, 0, 50, 95, 100):
        np.testing.assert_allclose(SO.surface_distances(pred, gt, spacing, pc), _scipy_metrics(pred, gt, spacing, pc), rtol=1e-12, atol=1e-12)
    empty = np.zeros(shape, bool)
    assert np.isnan(SO.surface_distances(empty, empty)).all() and np.isnan(_scipy_metrics(empty, empty, spacing, 95)).all()
    assert SO.surface_distances(pred, empty) == (float("inf"), float("inf")) == _scipy_metrics(pred, empty, spacing, 95)
    assert SO.surface_distances(empty, gt) == (float("inf"), float("inf")) == _scipy_metrics(empty, gt, spacing, 95)


def test_oracle_edges_of_a_single_slice_are_3d():
    m = np.zeros((6, 6, 1), bool)
    m[1:5, 1:5, 0] = True
    assert (SO.edges(m) == m).all()  # one slice thick: every voxel touches the background in z


def test_c_entry_point_rejects_calls_outside_its_domain():
    import ctypes

    from vs_seg_amd import _lib as L

    lib = L.lib()
    assert lib.vsseg_surface_scratch_bytes(L.i3((512, 512, 120))) >= 512 * 512 * 120 * 9
    assert lib.vsseg_surface_scratch_bytes(L.i3((0, 8, 8))) == L.EINVAL and b"vsseg_surface_scratch_bytes" in lib.vsseg_last_error()
    need = lib.vsseg_surface_scratch_bytes(L.i3((4, 4, 4)))
    sp, bad_sp = (ctypes.c_float * 3)(1, 1, 1), (ctypes.c_float * 3)(1, 0, 1)
    # (fake, aligned device addresses: every call below is rejected before anything is launched)
    for args, why in [((8, 3, 16, L.i3((4, 4, 4)), sp, 95.0, 256, need, 16), b"pitch"), ((8, 2, 16, L.i3((4, 4, 9000)), sp, 95.0, 256, need, 16), b"dims"),
                      ((8, 2, 16, L.i3((4, 4, 4)), bad_sp, 95.0, 256, need, 16), b"spacing"), ((8, 2, 16, L.i3((4, 4, 4)), sp, 100.5, 256, need, 16), b"percentile"),
                      ((8, 2, 16, L.i3((4, 4, 4)), sp, 95.0, 256, need - 1, 16), b"scratch"), ((None, 2, 16, L.i3((4, 4, 4)), sp, 95.0, 256, need, 16), b"null"),
                      ((4, 2, 16, L.i3((4, 4, 4)), sp, 95.0, 256, need, 16), b"misaligned")]:
        assert lib.vsseg_surface_distances(*args, None) == L.EINVAL
        assert why in lib.vsseg_last_error()
