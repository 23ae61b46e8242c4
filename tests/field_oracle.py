"""numpy fp64 restatement of `vsseg_crop_field` (include/vsseg_hip.h) on top of tests/augment_oracle.py: the Philox lattice (u in fp32 as the ABI defines it, everything
else in fp64), the cubic B-spline field F, the deformed coordinates and the bias field, and the DERIVED bounds on what fp32 may do to them.  Test infrastructure only."""
import numpy as np

from tests import augment_oracle as AO

EPS = 2.0 ** -24  # fp32: a correctly rounded operation is within EPS * |result| of the exact one
MASK = AO.MASK


def lattice_shape(roi, spacing):
    return tuple((int(r) - 1) // int(s) + 4 for r, s in zip(roi, spacing))


def control(roi, spacing, stream, seed):
    """The control values (c_x, c_y, c_b) of every lattice node, fp64 [3, n_x, n_y, n_z], each in [-1, 1)."""
    n = lattice_shape(roi, spacing)
    ids = np.arange(int(np.prod(n)), dtype=np.uint64)  # (i * n_y + j) * n_z + k is the C order of [n_x, n_y, n_z]
    r = AO.philox4x32_10((ids & MASK, ids >> np.uint64(32), stream, 1), (seed & 0xFFFFFFFF, seed >> 32))
    u = [(((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24)).astype(np.float64) for w in r[:3]]
    return np.stack([(2.0 * v - 1.0).reshape(n) for v in u])


def bspline_weights(f):
    """The four uniform cubic B-spline weights at the fraction f (any shape) -> [4, ...]."""
    f = np.asarray(f, np.float64)
    return np.stack([(1.0 - f) ** 3 / 6.0, (3.0 * f ** 3 - 6.0 * f ** 2 + 4.0) / 6.0, (-3.0 * f ** 3 + 3.0 * f ** 2 + 3.0 * f + 1.0) / 6.0, f ** 3 / 6.0])


def axis_matrix(r, s, n):
    """[r, n]: row p holds the weights of p on the nodes p // s .. p // s + 3."""
    p = np.arange(r)
    w = bspline_weights((p % s) / float(s))
    W = np.zeros((r, n))
    for a in range(4):
        W[p, p // s + a] = w[a]
    return W


def field(c, roi, spacing):
    """F(c) at every voxel of the patch: c [..., n_x, n_y, n_z] -> [..., *roi], the tensor-product sum over 4 x 4 x 4 nodes."""
    n = c.shape[-3:]
    Wx, Wy, Wz = (axis_matrix(int(roi[a]), int(spacing[a]), n[a]) for a in range(3))
    return np.einsum("xi,yj,zk,...ijk->...xyz", Wx, Wy, Wz, c, optimize=True)


def fields(roi, spacing, stream, seed):
    """(F(c_x), F(c_y), F(c_b)) of a job, fp64 [3, *roi], each within [-1, 1]."""
    return field(control(roi, spacing, stream, seed), roi, spacing)


def coords(m, roi, spacing, elastic_mag, stream, seed):
    """fp64 source coordinates [3, *roi]: the fp32 matrix applied to (x + d_x, y + d_y, z), d = elastic_mag (at its fp32 value) * F."""
    m = np.asarray(m, np.float32).astype(np.float64).reshape(3, 4)
    x, y, z = AO.grid(roi)
    if elastic_mag != 0.0:
        F = fields(roi, spacing, stream, seed)
        x, y = x + float(np.float32(elastic_mag)) * F[0], y + float(np.float32(elastic_mag)) * F[1]
    return np.stack([m[i, 0] * x + m[i, 1] * y + m[i, 2] * z + m[i, 3] for i in range(3)])


def apply(vol, m, roi, spacing, interp=0, gain=1.0, bias=0.0, noise_std=0.0, stream=0, seed=0, elastic_mag=0.0, bias_log=0.0):
    """One job of vsseg_crop_field in fp64 (the scalars of the job are taken at their fp32 values)."""
    s = coords(m, roi, spacing, elastic_mag, stream, seed)
    v = AO.trilinear(vol, s) if interp == 0 else AO.nearest(vol, s)
    if bias_log != 0.0:
        v = v * np.exp(float(np.float32(bias_log)) * fields(roi, spacing, stream, seed)[2])
    v = v * float(np.float32(gain)) + float(np.float32(bias))
    if noise_std != 0.0:
        v = v + float(np.float32(noise_std)) * AO.normals(roi, stream, seed)
    return v


def field_delta(mag):
    """Bound on |fp32 field - fp64 field| for d = mag * F (or b = bias_log * F), from the operation count of ANY evaluation that forms the three weight vectors in
    fp32 and reduces axis by axis with one rounding per accumulated term; nothing here is measured.
      weights   f = (p mod S) / S is one division (EPS), and |B'| <= 2/3: 0.7 EPS.  B0 = ((g*g)*g)/6 with g = 1 - f and B3 = ((f*f)*f)/6: four roundings of values <= 1/6
                and the rounded 1/6: < 1 EPS.  B1 = (3f^3 - 6f^2 + 4)/6 and B2 = (-3f^3 + 3f^2 + 3f + 1)/6 by Horner: three roundings of intermediates <= 6, carried
                through factors f <= 1, give <= 16 EPS on a numerator <= 4, then the division by six: <= 4.1 EPS.  Every weight is within dw = 6 EPS (absolute).
      products  F = sum over 64 nodes of wx wy wz c with |c| <= 1 and each axis' weights summing to 1: the weight errors move F by at most
                (4 dw) * 1 * 1 per axis, 12 dw = 72 EPS in all.
      sums      four accumulated terms per axis, each rounding within EPS of a partial sum <= 1, weighted by the other axes' weights (sum 1): 4 EPS per axis, 12 EPS.
      control   c = fmaf(2, u, -1): one rounding, 1 EPS.   scale: mag * F, one rounding: 1 EPS.
    72 + 12 + 1 + 1 = 86 EPS; the second-order terms are below one more.  Rounded up to 96 EPS, times mag."""
    return 96.0 * EPS * float(mag)


def coord_delta(s, m, elastic_mag, roi):
    """Per axis, the bound on |fp32 coordinate - fp64 coordinate| of a field job: AO.delta(s) for the three fused operations, plus what the row of the matrix makes of
    the error of its in-plane inputs x' = x + d_x and y' = y + d_y: field_delta(elastic_mag) and the rounding of the sum itself, half an ulp of a value <= roi - 1 + mag."""
    if elastic_mag == 0.0:
        return np.full(3, AO.delta(s))
    m = np.asarray(m, np.float32).astype(np.float64).reshape(3, 4)
    e_in = field_delta(elastic_mag) + 0.5 * float(np.spacing(np.float32(max(roi[0], roi[1]) - 1 + elastic_mag)))
    return AO.delta(s) + e_in * (np.abs(m[:, 0]) + np.abs(m[:, 1]))


def trilinear_tolerance(vol, s, cd):
    """AO.trilinear_tolerance with the per-axis coordinate bound `cd`."""
    return float(np.dot(cd, AO.lipschitz(vol))) + 8.0 * EPS * float(np.abs(vol).max())


def rounding_band(s, cd):
    """AO.rounding_band with the per-axis coordinate bound `cd`: the only voxels whose nearest lookup may differ in fp32."""
    t = s + 0.5
    return (np.abs(t - np.round(t)) < np.asarray(cd).reshape(3, 1, 1, 1)).any(0)


def jacobian_min(dx, dy):
    """Smallest discrete in-plane Jacobian determinant of p -> p + d (forward differences along x and y)."""
    ax, ay = 1.0 + np.diff(dx, axis=0)[:, :-1], np.diff(dx, axis=1)[:-1]
    bx, by = np.diff(dy, axis=0)[:, :-1], 1.0 + np.diff(dy, axis=1)[:-1]
    return float((ax * by - ay * bx).min())


# ---- the lattice shapes of the tests, the smallest at which the indexing can go wrong: roi, spacing, why ----
SHAPES = [((32, 32, 16), (8, 8, 2)),      # several cells per workgroup
          ((32, 32, 16), (12, 12, 3)),    # roi not a multiple of the spacing
          ((40, 24, 10), (16, 16, 4)),    # rz % 4 != 0 tail
          ((8, 6, 22), (64, 64, 16))]     # one cell, patch smaller than the spacing
