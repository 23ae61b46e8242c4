"""numpy oracle of vs_seg_amd.connected_components / keep_largest_component: union-find over the foreground voxels of a 3-D mask.

Connectivity 6 / 18 / 26: two voxels are neighbours when their index offset d has every |d_a| <= 1 and |dx| + |dy| + |dz| <= 1 / 2 / 3; outside the
volume is background.  Canonical label: 1 + the smallest linear index (x * Y + y) * Z + z of the component, background 0."""
import itertools

import numpy as np


def prediction_mask(logits):
    """Foreground of [2,X,Y,Z] logits: channel 1 strictly above channel 0 (ties and NaN are background)."""
    return np.asarray(logits[1] > logits[0])


def offsets(connectivity):
    """The neighbour offsets that follow (0, 0, 0) in raster order: each unordered pair of neighbours once."""
    if connectivity not in (6, 18, 26):
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    reach = {6: 1, 18: 2, 26: 3}[connectivity]
    return [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0) and sum(abs(a) for a in d) <= reach]


def label(mask, connectivity=26):
    """int32 labels of the boolean mask [X,Y,Z]."""
    mask = np.asarray(mask, bool)
    assert mask.ndim == 3
    idx = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    a, b = [], []
    for d in offsets(connectivity):
        src = tuple(slice(max(0, -o), s - max(0, o)) for o, s in zip(d, mask.shape))
        dst = tuple(slice(max(0, o), s - max(0, -o)) for o, s in zip(d, mask.shape))
        both = mask[src] & mask[dst]
        a.append(idx[src][both])
        b.append(idx[dst][both])
    a, b = np.concatenate(a), np.concatenate(b)
    parent = np.arange(mask.size, dtype=np.int64)  # parent[i] <= i throughout; a root has parent[i] == i
    while True:
        ra, rb = parent[a], parent[b]  # roots: the forest is flat here
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        if (lo == hi).all():
            break
        np.minimum.at(parent, hi, lo)  # hang the larger root below the smallest root it touches
        while True:  # flatten
            pp = parent[parent]
            if (pp == parent).all():
                break
            parent = pp
    return np.where(mask, parent.reshape(mask.shape) + 1, 0).astype(np.int32)


def largest(labels):
    """Label of the component with the most voxels, ties to the smallest label; 0 when there is no foreground."""
    fg = labels[labels > 0]
    if fg.size == 0:
        return 0
    values, counts = np.unique(fg, return_counts=True)  # ascending labels: argmax takes the first of equal counts
    return int(values[counts.argmax()])


def stats(labels):
    """[foreground voxels, number of components, voxels of the largest, its label]."""
    k = largest(labels)
    return np.array([int((labels > 0).sum()), len(np.unique(labels[labels > 0])), int((labels == k).sum()) if k else 0, k], np.int64)


def keep_largest(mask, connectivity=26):
    """Boolean mask of the largest component of `mask` (all False when `mask` is empty)."""
    lab = label(mask, connectivity)
    k = largest(lab)
    return (lab == k) if k else np.zeros(lab.shape, bool)


def one_hot(mask):
    """fp32 [2,X,Y,Z]: channel 1 = mask, channel 0 = 1 - mask."""
    m = np.asarray(mask, np.float32)
    return np.stack([1.0 - m, m])
