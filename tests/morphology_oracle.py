"""numpy oracle of vs_seg_amd.fill_holes / remove_small_components, built on tests/components_oracle.label.

Fill holes: label the complement of the mask at the connectivity of the BACKGROUND, collect the labels met on the six faces of the volume (a border voxel
has an index equal to 0 or to dim - 1), and add every other voxel of the complement to the mask.  Remove small: keep the components of the mask (at the
connectivity of the foreground) with at least min_voxels voxels; strictly smaller ones go."""
import numpy as np

from tests import components_oracle as CO


def holes(mask, connectivity=6):
    """Boolean mask H: the voxels of the components of ~mask that hold no border voxel of the volume."""
    mask = np.asarray(mask, bool)
    lab = CO.label(~mask, connectivity)
    faces = [lab[0], lab[-1], lab[:, 0], lab[:, -1], lab[:, :, 0], lab[:, :, -1]]
    outside = np.unique(np.concatenate([f.ravel() for f in faces]))
    return (lab > 0) & ~np.isin(lab, outside)


def fill_holes(mask, connectivity=6):
    """The mask with its holes filled."""
    return np.asarray(mask, bool) | holes(mask, connectivity)


def fill_stats(mask, connectivity=6):
    """[|P|, number of holes, |H|, |P| + |H|]."""
    mask = np.asarray(mask, bool)
    h = holes(mask, connectivity)
    lab = CO.label(~mask, connectivity)
    return np.array([int(mask.sum()), len(np.unique(lab[h])), int(h.sum()), int(mask.sum()) + int(h.sum())], np.int64)


def remove_small(mask, min_voxels, connectivity=26):
    """The components of the mask with at least min_voxels voxels."""
    lab = CO.label(mask, connectivity)
    values, counts = np.unique(lab[lab > 0], return_counts=True)
    return np.isin(lab, values[counts >= min_voxels]) & (lab > 0)


def small_stats(mask, min_voxels, connectivity=26):
    """[|P|, number of components of P, kept voxels, kept components]."""
    lab = CO.label(mask, connectivity)
    counts = np.unique(lab[lab > 0], return_counts=True)[1]
    keep = counts >= min_voxels
    return np.array([int(counts.sum()), len(counts), int(counts[keep].sum()), int(keep.sum())], np.int64)
