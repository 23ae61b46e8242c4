"""numpy-only restatement of vs_seg_amd.compute_surface_metrics on top of tests/surface_oracle.py: the edges and the brute-force directed distances of that
module in fp64, the mean of the two directed means, and per tolerance the counts of edge voxels with d * d <= tau * tau (a tie counts), with MONAI's rules
for empty masks."""
import numpy as np

from tests import surface_oracle as SO


def directed_pair(pred, gt, spacing=None):
    """(d(P->G), d(G->P)) in fp64 for two boolean [X,Y,Z] masks; an array is empty when its own edge set is, and +inf when only the other one is."""
    ep, eg = np.argwhere(SO.edges(pred)), np.argwhere(SO.edges(gt))
    dpg = SO.directed(ep, eg, spacing) if len(ep) and len(eg) else np.full(len(ep), np.inf)
    dgp = SO.directed(eg, ep, spacing) if len(ep) and len(eg) else np.full(len(eg), np.inf)
    return dpg, dgp


def surface_metrics(pred, gt, spacing=None, percentile=95.0, tolerances=()):
    """The 3 + 3T columns [hd, assd, masd, (nsd, surface precision, surface recall) per tolerance] as a fp64 array."""
    dpg, dgp = directed_pair(pred, gt, spacing)
    n_p, n_g = len(dpg), len(dgp)
    out = list(SO.surface_distances(pred, gt, spacing, percentile))
    if n_p == 0 and n_g == 0:
        return np.full(3 + 3 * len(tolerances), np.nan)
    out.append((dpg.mean() + dgp.mean()) / 2 if n_p and n_g else np.inf)
    for tau in tolerances:
        tau = float(tau)
        w_p, w_g = int((dpg * dpg <= tau * tau).sum()), int((dgp * dgp <= tau * tau).sum())  # (+inf never counts)
        out += [(w_p + w_g) / (n_p + n_g), w_p / n_p if n_p else np.nan, w_g / n_g if n_g else np.nan]
    return np.array(out, dtype=np.float64)


def near_ties(pred, gt, spacing, tolerances, rel=1e-4):
    """Number of edge voxels whose squared fp64 distance lies within a relative `rel` of some tau^2 (tau > 0)."""
    dpg, dgp = directed_pair(pred, gt, spacing)
    d2 = np.concatenate([dpg, dgp]) ** 2
    d2 = d2[np.isfinite(d2)]
    return int(sum((np.abs(d2 - float(t) ** 2) <= rel * float(t) ** 2).sum() for t in tolerances if float(t) > 0))
