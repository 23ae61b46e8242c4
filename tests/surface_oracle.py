"""numpy-only restatement of the surface-distance metrics (vs_seg_amd.compute_surface_distances): edges by 6-connected erosion of the
zero-padded mask, directed distances by brute force over every pair of edge voxels, numpy.percentile, and the empty-mask rules."""
import numpy as np


def edges(mask):
    """M AND NOT erode(M), 6-connected cross, voxels outside the volume background (always 3-D)."""
    m = np.pad(np.asarray(mask, dtype=bool), 1)
    c = m[1:-1, 1:-1, 1:-1]
    inner = c & m[:-2, 1:-1, 1:-1] & m[2:, 1:-1, 1:-1] & m[1:-1, :-2, 1:-1] & m[1:-1, 2:, 1:-1] & m[1:-1, 1:-1, :-2] & m[1:-1, 1:-1, 2:]
    return c & ~inner


def directed(src, dst, spacing=None, chunk=2048):
    """For every voxel of `src` (an [n,3] index array) the Euclidean distance in mm to the nearest voxel of `dst`."""
    s = np.ones(3) if spacing is None else np.asarray(spacing, dtype=np.float64)
    a, b = src.astype(np.float64) * s, dst.astype(np.float64) * s
    out = np.empty(len(a))
    for i in range(0, len(a), chunk):
        d2 = ((a[i:i + chunk, None, :] - b[None, :, :]) ** 2).sum(-1)
        out[i:i + chunk] = np.sqrt(d2.min(1))
    return out


def surface_distances(pred, gt, spacing=None, percentile=95.0):
    """(hd, assd) of two boolean [X,Y,Z] masks; percentile None = the maximum."""
    ep, eg = np.argwhere(edges(pred)), np.argwhere(edges(gt))
    if len(ep) == 0 and len(eg) == 0:
        return float("nan"), float("nan")
    if len(ep) == 0 or len(eg) == 0:
        return float("inf"), float("inf")
    dpg, dgp = directed(ep, eg, spacing), directed(eg, ep, spacing)
    pct = (lambda d: d.max()) if percentile is None else (lambda d: np.percentile(d, percentile))
    return float(max(pct(dpg), pct(dgp))), float((dpg.sum() + dgp.sum()) / (len(dpg) + len(dgp)))


def prediction_mask(logits):
    """argmax over the two class channels of [2,X,Y,Z] logits, ties -> class 0."""
    return logits[1] > logits[0]


def label_mask(label):
    """(int)label == 1 (truncation towards zero), as the hard Dice reads the label."""
    return np.trunc(label) == 1
