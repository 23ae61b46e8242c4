"""numpy-only restatement of the size measurements (vs_seg_amd.compute_measurements) in fp64: voxel counts, volumes, the distance between the
centres of mass, and the largest distance between two voxel centres of a mask in 3-D and within one axial (equal z) slice, by brute force over
every pair of foreground voxels.  The spacing is rounded to fp32 first, as the kernel receives it.

`measurements_reduced` first reduces a mask to the extremes of its columns (with the other two index differences fixed, a pair whose extent
along the column can grow is not the farthest) and then runs the same brute force: along z for the 3-D diameter and along y for the axial one,
where the kernel reduces along x, so the two do not share the shortcut."""
import numpy as np

from tests.surface_oracle import label_mask, prediction_mask  # noqa: F401  (the foreground rules)

FIELDS = ("voxels_pred", "voxels_label", "volume_pred_mm3", "volume_label_mm3", "centroid_distance_mm", "max_diameter_pred_mm", "max_diameter_label_mm",
          "max_axial_diameter_pred_mm", "max_axial_diameter_label_mm")
BRUTE_FORCE_LIMIT = 3000  # voxels: brute force takes a quarter of a second at 2 000 voxels and six seconds at 11 000


def _spacing(spacing):
    s = np.ones(3, np.float32) if spacing is None else np.asarray(spacing, dtype=np.float32)
    assert s.shape == (3,)
    return s.astype(np.float64)


def farthest(idx, s, chunk=256):
    """Largest distance between two of the points idx [n,3] (integer indices) scaled by s; NaN without points."""
    if len(idx) == 0:
        return float("nan")
    p = idx.astype(np.float64) * s
    best = 0.0
    for i in range(0, len(p), chunk):  # every unordered pair once: a chunk against itself and everything after it
        d2 = np.subtract.outer(p[i:i + chunk, 0], p[i:, 0]) ** 2
        for a in (1, 2):
            t = np.subtract.outer(p[i:i + chunk, a], p[i:, a])
            t *= t
            d2 += t
        best = max(best, float(d2.max()))
    return float(np.sqrt(best))


def farthest_axial(idx, s):
    """The same over pairs with equal z."""
    if len(idx) == 0:
        return float("nan")
    return max(farthest(idx[idx[:, 2] == z], s) for z in np.unique(idx[:, 2]))


def column_extremes(mask, axis):
    """The mask reduced to the first and the last foreground voxel of every column along `axis`."""
    m = np.moveaxis(np.asarray(mask, bool), axis, -1)
    n = m.shape[-1]
    any_ = m.any(-1)
    first = np.where(any_, m.argmax(-1), -1)
    last = np.where(any_, n - 1 - m[..., ::-1].argmax(-1), -1)
    out = np.zeros_like(m)
    a, b = np.nonzero(any_)
    out[a, b, first[a, b]] = True
    out[a, b, last[a, b]] = True
    return np.moveaxis(out, -1, axis)


def _measure(pred, label, spacing, reduce):
    s = _spacing(spacing)
    voxel = (s[0] * s[1]) * s[2]
    out = np.full(9, np.nan)
    cen = [None, None]
    for m, mask in enumerate((pred, label)):
        if mask is None:
            continue
        mask = np.asarray(mask, bool)
        assert mask.ndim == 3
        idx = np.argwhere(mask)
        out[m] = len(idx)
        out[2 + m] = len(idx) * voxel
        if len(idx):
            cen[m] = idx.sum(0).astype(np.float64) / len(idx)
            out[5 + m] = farthest(np.argwhere(column_extremes(mask, 2)) if reduce else idx, s)
            out[7 + m] = farthest_axial(np.argwhere(column_extremes(mask, 1)) if reduce else idx, s)
    if cen[0] is not None and cen[1] is not None:
        out[4] = float(np.sqrt((((cen[0] - cen[1]) * s) ** 2).sum()))
    return out


def measurements(pred, label=None, spacing=None):
    """The nine values (FIELDS) of two boolean [X,Y,Z] masks (label may be None) by brute force over all foreground voxels."""
    return _measure(pred, label, spacing, False)


def measurements_reduced(pred, label=None, spacing=None):
    """The same with every mask reduced to its column extremes first: for masks beyond BRUTE_FORCE_LIMIT voxels."""
    return _measure(pred, label, spacing, True)


def measurements_auto(pred, label=None, spacing=None):
    big = max(int(np.count_nonzero(pred)), 0 if label is None else int(np.count_nonzero(label))) > BRUTE_FORCE_LIMIT
    return (measurements_reduced if big else measurements)(pred, label, spacing)
