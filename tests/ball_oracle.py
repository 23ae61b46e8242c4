"""numpy oracle (fp64) of vs_seg_amd.binary_dilate / binary_erode / binary_close / binary_open: the ball as an explicit set of voxel offsets, dilation and
erosion by shifting the padded mask over those offsets.

The ball of radius r mm at the voxel spacing s: the integer offsets d with (sx dx)^2 + (sy dy)^2 + (sz dz)^2 <= r^2, a tie included; s is rounded to fp32 first,
as the library receives it, and everything after that is fp64.  dilate(M): the voxels of the volume with a voxel of M at a ball offset (nothing outside the
volume).  erode(M): the voxels of M with no background voxel OF THE VOLUME at a ball offset (positions outside the volume are ignored).  close = erode(dilate),
open = dilate(erode)."""
import itertools
import math

import numpy as np


def _spacing64(spacing):
    return [float(np.float32(s)) for s in spacing]


def reach(spacing, r):
    """floor(r / s_a) per axis: the largest |d_a| of a ball offset."""
    return [int(math.floor(float(r) / s)) for s in _spacing64(spacing)]


def ball_offsets(spacing, r):
    """The offsets (dx, dy, dz) of the ball, as a list of tuples."""
    s = _spacing64(spacing)
    r2 = float(r) * float(r)
    ranges = [range(-k, k + 1) for k in reach(spacing, r)]
    return [d for d in itertools.product(*ranges) if (s[0] * d[0]) ** 2 + (s[1] * d[1]) ** 2 + (s[2] * d[2]) ** 2 <= r2]


def ball_array(spacing, r):
    """The ball as a boolean structuring element for scipy.ndimage (odd extents, centred)."""
    k = reach(spacing, r)
    st = np.zeros([2 * a + 1 for a in k], bool)
    for d in ball_offsets(spacing, r):
        st[d[0] + k[0], d[1] + k[1], d[2] + k[2]] = True
    return st


def tie_margin(spacing, r):
    """The smallest |d^2 - r^2| / r^2 over the offsets with |d_a| <= reach_a + 1: how far the nearest offset is from the surface of the ball, to be compared with
    the fp32 rounding of the library's squared lengths (a few 2^-24).  0: an offset lies exactly on the surface (exact in fp32 too where the products are: unit
    and dyadic spacings).  r = 0: inf."""
    if r == 0:
        return math.inf
    s = _spacing64(spacing)
    r2 = float(r) * float(r)
    return min(abs((s[0] * d[0]) ** 2 + (s[1] * d[1]) ** 2 + (s[2] * d[2]) ** 2 - r2) / r2 for d in itertools.product(*[range(0, k + 2) for k in reach(spacing, r)]))


def _any_at_offsets(mask, offsets, outside):
    """out[v] = any(mask[v + d] for d in offsets), with `outside` standing for the positions beyond the array."""
    mask = np.asarray(mask, bool)
    k = [max([abs(d[a]) for d in offsets] + [0]) for a in range(3)]
    padded = np.pad(mask, [(a, a) for a in k], constant_values=outside)
    out = np.zeros(mask.shape, bool)
    X, Y, Z = mask.shape
    for d in offsets:
        out |= padded[k[0] + d[0]:k[0] + d[0] + X, k[1] + d[1]:k[1] + d[1] + Y, k[2] + d[2]:k[2] + d[2] + Z]
    return out


def dilate(mask, spacing, r):
    return _any_at_offsets(mask, ball_offsets(spacing, r), False)


def erode(mask, spacing, r):
    return ~_any_at_offsets(~np.asarray(mask, bool), ball_offsets(spacing, r), False)  # a background voxel of the volume at a ball offset (the ball is symmetric)


def close(mask, spacing, r):
    return erode(dilate(mask, spacing, r), spacing, r)


def open_(mask, spacing, r):
    return dilate(erode(mask, spacing, r), spacing, r)


OPS = {"dilate": dilate, "erode": erode, "close": close, "open": open_}


def stats(mask, result):
    """[|P|, |result|, |result \\ P|, |P \\ result|]"""
    mask, result = np.asarray(mask, bool), np.asarray(result, bool)
    return np.array([mask.sum(), result.sum(), (result & ~mask).sum(), (mask & ~result).sum()], np.int64)
