"""`VSparams` — the reference's experiment driver (ref:params/VSparams.py) over the MI355X hot path.

Same command line, same public methods, same protocol as the reference class, so `VS_train.py` / `VS_inference.py` read
like the reference's scripts.  What is different underneath:

* data: no MONAI / nibabel / DataLoader workers — `vs_seg_amd.data` reads NIfTI, re-orients to RAS, normalises on the GPU,
  keeps every case cached in HBM and crops/flips whole batches with one HIP launch (the "loaders" returned by
  `cache_transformed_*_data` are light iterables over that cache yielding the reference's `{"image", "label"}` dicts);
* step: model / loss / optimizer are the HIP-backed objects; epoch sums stay on the device, the host reads them once per
  epoch (the reference calls `.item()` every step, ref:params/VSparams.py:463);
* validation (N1): eval forward + loss + hard Dice accumulated on the device, one read per validation pass.  The
  reference's loop adds every case twice (ref:params/VSparams.py:490-496): the mean Dice is unaffected, the logged
  validation loss is twice the mean — reproduced, because `best_metric`/logs are part of the observable behaviour;
* export (N3): argmax on the GPU, written as NIfTI in the label's original orientation and affine.

Not carried over (SURVEY §2 out-of-scope rows): TensorBoard writer, matplotlib figures.
"""
from __future__ import annotations

import csv
import logging
import os
from time import perf_counter, strftime
from typing import Dict, Iterator, List, Optional, Sequence

import numpy as np
import torch

from . import SGD, Adam, AdamW, Dice_spvPA, UNet2d5_spvPA, check_ce, check_ce_topk, check_optimizer, check_region, compute_dice_score, poly_lr, sliding_window_inference
from .optim import DEFAULT_WEIGHT_DECAY, LR_SCHEDULES, OPTIMIZERS
from .inferers import argmax_segmentation, tta_masks
from .metrics import MEASUREMENT_FIELDS, check_tolerances, compute_measurements, compute_surface_distances, compute_surface_metrics, surface_metric_fields, voxel_spacing
from .postprocess import binary_close, binary_open, check_radius_mm, connected_components, fill_holes, keep_largest_component, min_component_voxels, remove_small_components
from . import parallel as DP
from . import report as R
from .report import postprocessing_csv_header  # noqa: F401  (part of this module's interface)
from .data import nifti
from .data.transforms import DEFAULTS, FAMILIES, Augmentation, PatchSampler, epoch_batches, load_case

HP = dict(
    channels=(16, 32, 48, 64, 80, 96),
    strides=((2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (2, 2, 2)),
    kernel_sizes=((3, 3, 1), (3, 3, 1), (3, 3, 3), (3, 3, 3), (3, 3, 3), (3, 3, 3)),
    sample_kernel_sizes=((3, 3, 1), (3, 3, 1), (3, 3, 3), (3, 3, 3), (3, 3, 3)),
)


def surface_dice_rows(tolerances) -> tuple:
    """The rows of --surface_dice_mm: masd_mm, then nsd, surface precision and surface recall per tolerance (the columns of compute_surface_metrics after hd and assd)."""
    return ("masd_mm",) + surface_metric_fields(tolerances)[3:]


def surface_dice_csv_header(tolerances) -> str:
    """Columns of figures/test_surface_dice.csv: case, dice, masd_mm, then nsd, surface precision and surface recall per tolerance of --surface_dice_mm."""
    return R.csv_header(R.surface_dice(surface_dice_rows(tolerances)))


def _fill_step(p, outputs, spacing):
    outputs, st = fill_holes(outputs, p.hole_connectivity, return_stats=True)
    return outputs, dict(foreground_voxels=st[0, 0], holes=st[0, 1], filled_voxels=st[0, 2], kept_voxels=st[0, 3])


def _closing_step(p, outputs, spacing):
    outputs, st = binary_close(outputs, p.closing_mm, spacing, return_stats=True)
    return outputs, dict(foreground_voxels=st[0, 0], kept_voxels=st[0, 1], closed_voxels=st[0, 2])  # closing only adds


def _opening_step(p, outputs, spacing):
    outputs, st = binary_open(outputs, p.opening_mm, spacing, return_stats=True)
    return outputs, dict(foreground_voxels=st[0, 0], kept_voxels=st[0, 1], opened_voxels=st[0, 3])  # opening only removes


def _small_step(p, outputs, spacing):
    outputs, st = remove_small_components(outputs, min_component_voxels(p.min_component_mm3, spacing), p.component_connectivity, return_stats=True)
    return outputs, dict(foreground_voxels=st[0, 0], components=st[0, 1], kept_voxels=st[0, 2], small_components=st[0, 1] - st[0, 3], small_voxels=st[0, 0] - st[0, 2])


def _largest_step(p, outputs, spacing):
    outputs, st = keep_largest_component(outputs, p.component_connectivity, return_stats=True)
    return outputs, dict(foreground_voxels=st[0, 0], components=st[0, 1], kept_voxels=st[0, 2])


# the post-processing chain in the order it runs, under the flag names of report.postprocessing (closing before the component filters, so that they see the bridged
# prediction).  A step maps (params, one-hot prediction, spacing) to the new prediction and its statistics by name: what it was given, what it left, what it did
POST_STEPS = dict(fill_holes=_fill_step, closing=_closing_step, opening=_opening_step, min_component=_small_step, keep_largest=_largest_step)


# the --aug_<argument> flags: argument -> (type, metavar, help).  Their order, their defaults and the family each belongs to are those of data.transforms.FAMILIES
AUG_FLAGS = dict(
    rotate_deg=(float, "DEG", "training augmentation: rotate every training patch about the z axis by an angle drawn from [-DEG, DEG] (0: off)"),
    scale=(float, "FRAC", "training augmentation: zoom every training patch in-plane by a factor drawn from [1 - FRAC, 1 + FRAC] (0: off)"),
    intensity_scale=(float, "FRAC", "training augmentation: multiply the image of every training patch by a gain drawn from [1 - FRAC, 1 + FRAC] (0: off)"),
    intensity_shift=(float, "STD", "training augmentation: add a bias drawn from [-STD, STD] to the image of every training patch, in standard deviations of the normalised image (0: off)"),
    noise_std=(float, "STD", "training augmentation: add Gaussian noise of this standard deviation to the image of every training patch (0: off)"),
    elastic_mag=(float, "VOX", "training augmentation: deform every training patch in-plane by a smooth random B-spline field whose control points move by at most a length drawn from [0, VOX] voxels; the peak displacement of the field is typically about half of it; at most aug_field_spacing / 4 (0: off)"),
    bias_field=(float, "LOG", "training augmentation: multiply the image of every training patch by exp of a smooth random B-spline field whose amplitude is drawn from [0, LOG] (the MR bias field; 0: off)"),
    field_spacing=(int, "VOX", "in-plane control-point spacing of the two B-spline fields in voxels (64: about 26 mm; along z a quarter of it)"),
    blur_sigma=(float, "VOX", "training augmentation: blur the image of a training patch in-plane with a Gaussian whose sigma is drawn from [VOX / 2, VOX] in-plane voxels; at most 1.5 (0: off)"),
    lowres=(float, "FRAC", "training augmentation: simulate a low-resolution acquisition of the image of a training patch: sample it in-plane at a resolution factor drawn from [FRAC, 1] and interpolate back; in [0.25, 1) (0: off)"),
    contrast=(float, "FRAC", "training augmentation: scale the image of a training patch about its mean by a factor drawn from [1 - FRAC, 1 + FRAC], clipped to the range it had (0: off)"),
    gamma=(float, "FRAC", "training augmentation: apply a gamma curve over the value range of the image of a training patch, with an exponent drawn from [1 - FRAC, 1 + FRAC] (0: off)"),
    appearance_prob=(float, "P", "probability with which each of the blur, low-resolution, contrast and gamma augmentations is applied to a training sample, independently of the others"),
    thick_slices=(float, "F", "training augmentation: simulate a thick-slice acquisition of the image of a training patch: average slabs of 2 to F voxels along z (drawn per sample, at a random offset) and interpolate linearly back between the slab centres; an integer in 2..4 (0: off)"),
    ghost=(float, "A", "training augmentation: add phase-encode ghosts to the image of a training patch: 2 to 8 shifted copies along x or y, as left by attenuating every n-th k-space line by a factor drawn from [0, A]; in [0, 1] (0: off)"),
    spike=(float, "S", "training augmentation: add a k-space spike to the image of a training patch: a plane wave in-plane at a random frequency and phase with an amplitude drawn from [0, S], in standard deviations of the normalised image (the herringbone artefact; 0: off)"),
    acquisition_prob=(float, "P", "probability with which each of the thick-slice, ghosting and spike augmentations is applied to a training sample, independently of the others"),
)

# the augmentation steps of the training chain description: (the arguments of which a non-zero one switches the step on, its text over all arguments), in the order the
# launches apply them: the deformation acts in patch space, the matrix after it; the bias field multiplies the interpolated value before the gain
AUG_CHAIN = (
    (("elastic_mag",), "RandElastic(aug_elastic_mag={elastic_mag}, aug_field_spacing={field_spacing}, in-plane, cubic B-spline)"),
    (("rotate_deg", "scale"), "RandAffine(aug_rotate_deg={rotate_deg}, aug_scale={scale}, axis=z, about the crop centre)"),
    (("bias_field",), "RandBiasField(aug_bias_field={bias_field}, aug_field_spacing={field_spacing})"),
    (("intensity_scale",), "RandScaleIntensity(aug_intensity_scale={intensity_scale})"),
    (("intensity_shift",), "RandShiftIntensity(aug_intensity_shift={intensity_shift})"),
    (("noise_std",), "RandGaussianNoise(aug_noise_std={noise_std})"),
    (("thick_slices",), "RandThickSlices(aug_thick_slices={thick_slices}, along z, p={acquisition_prob})"),
    (("ghost",), "RandGhosting(aug_ghost={ghost}, in-plane, p={acquisition_prob})"),
    (("spike",), "RandSpike(aug_spike={spike}, in-plane, p={acquisition_prob})"),
    (("blur_sigma",), "RandGaussianBlur(aug_blur_sigma={blur_sigma}, in-plane, p={appearance_prob})"),
    (("lowres",), "RandLowResolution(aug_lowres={lowres}, in-plane, p={appearance_prob})"),
    (("contrast",), "RandContrast(aug_contrast={contrast}, preserve_range, p={appearance_prob})"),
    (("gamma",), "RandGamma(aug_gamma={gamma}, p={appearance_prob})"),
)


class CachedLoader:
    """Iterable over GPU-cached cases with the random tail of the transform chain applied per epoch.

    Yields the reference DataLoader's batch dicts: {"image": [B,1,X,Y,Z], "label": [B,1,X,Y,Z]} fp32 device tensors (+ the
    meta dicts of the cases for batch_size 1 loaders).  `len()` = number of cases, `batch_size` as in torch's DataLoader —
    the reference's first-epoch log line divides one by the other (ref:params/VSparams.py:466)."""

    def __init__(self, cases: List[Dict], roi: Optional[Sequence[int]], batch_size: int, shuffle: bool, flip_prob: Optional[float], seed: int = 0, pad: Optional[bool] = None, **families):
        # families: the arguments of the augmentation families as dicts under the keys of a transform description (augment, field_augment, ...; None or absent: off)
        augmentation = Augmentation.of(**{k: v for fam in FAMILIES for k, v in (families.pop(fam.key, None) or {}).items()})
        if families:
            raise TypeError(f"CachedLoader got an unexpected keyword argument '{next(iter(families))}'")
        self.cases, self.batch_size, self.shuffle = cases, batch_size, shuffle
        # equal step counts on every rank (wrap-around padding) only where every step issues a collective: the shuffled training loader.
        # Validation / test loaders give rank r exactly shard_indices(n, r, world) — a padded case would be counted twice in their sums
        self.pad = shuffle if pad is None else pad
        self.rank, self.world = DP.get_rank(), DP.world_size()
        # every rank shuffles with the SAME stream (the shards must partition one permutation) but draws its own flips / crops
        self.sampler = PatchSampler(cases, roi, flip_prob, seed + 7919 * self.rank, augmentation) if roi is not None else None
        self._order = np.random.RandomState(seed)

    def __len__(self):
        return len(self.cases)

    def __iter__(self) -> Iterator[Dict]:
        for idx in epoch_batches(len(self.cases), self.batch_size, self.shuffle, self._order, self.rank, self.world, pad=self.pad):
            if self.sampler is not None:
                img, lab = self.sampler.sample(idx)
            else:  # test chain: whole volumes, no crop (ref:params/VSparams.py:238-245)
                assert len(idx) == 1
                img, lab = self.cases[idx[0]]["image"][None, None], self.cases[idx[0]]["label"][None, None]
            batch = {"image": img, "label": lab}
            if len(idx) == 1:
                batch["image_meta_dict"], batch["label_meta_dict"] = self.cases[idx[0]]["image_meta"], self.cases[idx[0]]["label_meta"]
            yield batch


class VSparams:
    def __init__(self, parser, argv=None):
        parser.add_argument("--debug", dest="debug", action="store_true", help="activate debugging mode")
        parser.set_defaults(debug=False)
        parser.add_argument("--split", type=str, default="./params/split_TCIA.csv", help="path to CSV file that defines training, validation and test datasets")
        parser.add_argument("--dataset", type=str, default="T1", help='(string) use "T1" or "T2" to select dataset')
        parser.add_argument("--train_batch_size", type=int, default=1, help="batch size of the forward pass")
        parser.add_argument("--initial_learning_rate", type=float, default=1e-4, help="learning rate at first epoch")
        parser.add_argument("--no_attention", dest="attention", action="store_false", help="disables the attention module in the network and the attention map weighting in the loss function")
        parser.set_defaults(attention=True)
        parser.add_argument("--no_hardness", dest="hardness", action="store_false", help="disables the hardness weighting in the loss function")
        parser.set_defaults(hardness=True)
        parser.add_argument("--results_folder_name", type=str, default="temp" + strftime("%Y%m%d%H%M%S"), help="name of results folder")
        # additions of this implementation (defaults reproduce the reference)
        parser.add_argument("--data_root", type=str, default="./data/VS_defaced/", help="data set root (the reference hard-codes this path)")
        parser.add_argument("--compute_dtype", type=str, default="bf16", choices=["bf16", "fp32"], help="bf16 MFMA (benchmark) or exact-fp32 MFMA (parity)")
        parser.add_argument("--num_epochs", type=int, default=None)
        parser.add_argument("--closing_mm", type=float, default=0.0, metavar="R", help="run_inference closes each predicted segmentation with a ball of R mm (dilation, then erosion, with the voxel spacing of the case; on the GPU, after --fill_holes and before --opening_mm, --min_component_mm3 and --keep_largest_component, so that fragments less than about 2 R apart are bridged before the component filters see them) and adds closed_voxels to figures/test_postprocessing.csv (0: off; the ball may reach 32 voxels per axis)")
        parser.add_argument("--opening_mm", type=float, default=0.0, metavar="R", help="run_inference opens each predicted segmentation with a ball of R mm (erosion, then dilation: spurs and islands thinner than the ball go; on the GPU, after --closing_mm and before --min_component_mm3 and --keep_largest_component) and adds opened_voxels to figures/test_postprocessing.csv (0: off)")
        parser.add_argument("--surface_metrics", action="store_true", help="run_inference also reports HD95 and ASSD per test case (mm, on the GPU) and writes figures/test_surface_metrics.csv")
        parser.add_argument("--surface_dice_mm", type=float, nargs="+", default=None, metavar="TAU", help="run_inference also reports per test case the normalised surface Dice (the share of the two boundaries within TAU mm of the other one), the surface precision and recall at each of 1 to 8 distinct tolerances and the mean of the two directed mean surface distances (on the GPU, from the one edge pass and distance transform that also serve --surface_metrics), and writes figures/test_surface_dice.csv")
        parser.add_argument("--keep_largest_component", action="store_true", help="run_inference keeps only the largest connected component of each predicted segmentation (on the GPU) before the Dice, the surface metrics and the NIfTI export, and writes figures/test_postprocessing.csv")
        parser.add_argument("--measurements", action="store_true", help="run_inference also reports per test case the volume (mm^3), the largest 3-D diameter and the largest diameter within an axial slice (mm) of the predicted and of the manual segmentation and the distance between their centres of mass (on the GPU), and writes figures/test_measurements.csv")
        parser.add_argument("--component_connectivity", type=int, default=26, choices=[6, 18, 26], help="voxel connectivity of --keep_largest_component and --min_component_mm3 (26: MONAI's KeepLargestConnectedComponent)")
        parser.add_argument("--fill_holes", action="store_true", help="run_inference fills the holes of each predicted segmentation (background enclosed by foreground, e.g. the missed fluid of a cystic tumour; on the GPU, before --min_component_mm3 and --keep_largest_component) and adds holes,filled_voxels to figures/test_postprocessing.csv (MONAI's FillHoles)")
        parser.add_argument("--hole_connectivity", type=int, default=6, choices=[6, 18, 26], help="voxel connectivity of the BACKGROUND for --fill_holes (6: scipy.ndimage.binary_fill_holes, the dual of a 26-connected foreground; 26: MONAI's FillHoles)")
        parser.add_argument("--min_component_mm3", type=float, default=0.0, metavar="V", help="run_inference drops every connected component of a predicted segmentation that is smaller than V cubic millimetres (ceil(V / voxel volume) voxels per case; on the GPU, at --component_connectivity) and adds small_components,small_voxels to figures/test_postprocessing.csv (MONAI's RemoveSmallObjects; 0: off)")
        parser.add_argument("--tta_flips", type=int, nargs="*", choices=[0, 1, 2], default=None, metavar="AXIS", help="run_inference predicts every case on mirrored copies as well (spatial axes 0 1 2 = X Y Z: one pass per subset of the given axes) and averages the un-mirrored predictions; training mirrors axis 0")
        parser.add_argument("--tta_average", type=str, default="logits", choices=["logits", "probabilities"], help="what --tta_flips averages: the blended logits, or their softmax over the classes (nnU-Net)")
        for k, default in DEFAULTS.items():
            kind, metavar, text = AUG_FLAGS[k]
            parser.add_argument("--aug_" + k, type=kind, default=default, metavar=metavar, help=text)
        parser.add_argument("--ce_weight", type=float, default=0.0, metavar="LAMBDA", help="training loss: add LAMBDA times the voxel-wise cross-entropy of the final logits to the Dice loss (the Dice + CE loss of nnU-Net, MONAI's DiceCELoss; 0: off, the reference's loss)")
        parser.add_argument("--ce_foreground_weight", type=float, default=1.0, metavar="W", help="class weight of the foreground voxels in the cross-entropy term, the background's being 1 (needs --ce_weight > 0)")
        parser.add_argument("--ce_topk", type=float, default=0.0, metavar="PCT", help="training loss: average the cross-entropy term over the hardest PCT percent of the voxels of the batch only, selected on the GPU, and divide by their number K, not by the class-weight sum (the Dice + TopK loss of nnU-Net, DC_and_topk_loss: --ce_weight 1 --ce_topk 10; in (0, 100], needs --ce_weight > 0; 0: off, the mean over every voxel)")
        parser.add_argument("--tversky_beta", type=float, default=None, metavar="BETA", help="training loss: replace every Dice ratio by the Tversky index (2I + eps) / (2 (1 - BETA) P + 2 BETA G + eps): BETA weights the missed tumour voxels, 1 - BETA the false positives (mirrored for the background class); in (0, 1), above 0.5 a missed voxel costs more, 0.5 is the Dice ratio (Salehi 2017, MONAI's TverskyLoss; default: off, 0.5 where --focal_tversky_gamma or --batch_dice is given)")
        parser.add_argument("--focal_tversky_gamma", type=float, default=1.0, metavar="GAMMA", help="training loss: raise every region term 1 - T to the power GAMMA, floored at 1e-7 (the focal Tversky loss of Abraham 2019 is GAMMA = 0.75); in [0.25, 4] (1: off)")
        parser.add_argument("--batch_dice", action="store_true", help="training loss: form one region ratio per class and per attention level over the pooled sums of the batch instead of one per sample, so that a sample without tumour has no ratio of its own (nnU-Net's batch_dice); under data parallelism the pool is the samples of the rank's own batch, nothing is exchanged between ranks")
        parser.add_argument("--ce_focal_gamma", type=float, default=0.0, metavar="GAMMA", help="training loss: weight every voxel of the cross-entropy term by (1 - p_y)^GAMMA (the focal loss of MONAI's DiceFocalLoss; with --tversky_beta and --focal_tversky_gamma the Unified Focal family); in (0, 5], needs --ce_weight > 0, not together with --ce_topk; 0: off")
        parser.add_argument("--optimizer", type=str, default="adam", choices=list(OPTIMIZERS), help="adam: the reference's Adam with coupled weight decay; adamw: decoupled weight decay (torch.optim.AdamW); sgd: SGD with --momentum / --nesterov (nnU-Net: --optimizer sgd --nesterov --weight_decay 3e-5 --clip_grad_norm 12 --lr_schedule poly --initial_learning_rate 1e-2)")
        parser.add_argument("--momentum", type=float, default=None, metavar="MU", help="momentum of --optimizer sgd, in [0, 1) (default 0.99; sgd only)")
        parser.add_argument("--nesterov", action="store_true", help="Nesterov momentum (--optimizer sgd only)")
        parser.add_argument("--weight_decay", type=float, default=DEFAULT_WEIGHT_DECAY, metavar="WD", help="weight decay of the optimizer (1e-7: the reference's)")
        parser.add_argument("--clip_grad_norm", type=float, default=0.0, metavar="NORM", help="clip the L2 norm of the whole gradient to NORM inside the optimizer step, on the GPU (torch.nn.utils.clip_grad_norm_; a step whose norm is NaN / Inf is skipped; 0: off)")
        parser.add_argument("--lr_schedule", type=str, default="halving", choices=list(LR_SCHEDULES), help="halving: the reference's division by 2 every 100 epochs; poly: lr = initial_learning_rate * (1 - epoch / num_epochs) ** poly_power, set at the start of every epoch")
        parser.add_argument("--poly_power", type=float, default=None, metavar="P", help="exponent of --lr_schedule poly (default 0.9)")
        args = parser.parse_args(argv)
        try:
            tta_masks(args.tta_flips, args.tta_average)
            opt = check_optimizer(args.optimizer, args.momentum, args.nesterov, args.weight_decay, args.clip_grad_norm, args.lr_schedule, args.poly_power)
            ce_weight, ce_foreground_weight = check_ce(args.ce_weight, args.ce_foreground_weight)
            ce_topk = check_ce_topk(args.ce_topk, ce_weight)
            region, ce_focal_gamma = check_region(args.tversky_beta, args.focal_tversky_gamma, args.batch_dice, args.ce_focal_gamma, ce_weight, ce_topk)
            augmentation = Augmentation.of(**{k: getattr(args, "aug_" + k) for k in AUG_FLAGS})
            min_component_voxels(args.min_component_mm3, (1.0, 1.0, 1.0))  # a finite value >= 0
            check_radius_mm(args.closing_mm, what="--closing_mm")  # (the reach depends on the spacing of the case: checked per case)
            check_radius_mm(args.opening_mm, what="--opening_mm")
            surface_dice_mm = tuple(sorted(check_tolerances(args.surface_dice_mm or (), "--surface_dice_mm", distinct=True)))
        except ValueError as e:
            parser.error(str(e))

        self.debug, self.dataset, self.data_root = args.debug, args.dataset, args.data_root
        self.split_csv = "./params/split_debug.csv" if self.debug else args.split
        self.pad_crop_shape = [128, 128, 32] if self.debug else [384, 384, 64]
        self.pad_crop_shape_test = list(self.pad_crop_shape)
        self.num_workers = 4  # kept for the log; there are no loader workers (the cache lives in HBM)
        self.torch_device_arg = "cuda:0"
        self.train_batch_size = args.train_batch_size
        self.initial_learning_rate = args.initial_learning_rate
        self.epochs_with_const_lr = 3 if self.debug else 100
        self.lr_divisor = 2.0
        self.weight_decay = opt["weight_decay"]
        self.optimizer, self.momentum, self.nesterov, self.clip_grad_norm = opt["optimizer"], opt["momentum"], opt["nesterov"], opt["clip_grad_norm"]
        self.lr_schedule, self.poly_power = opt["lr_schedule"], opt["poly_power"]
        self.num_epochs = args.num_epochs or (10 if self.debug else 300)
        self.val_interval = 2
        self.model = "UNet2d5_spvPA"
        self.sliding_window_inferer_roi_size = [128, 128, 32] if self.debug else [384, 384, 64]
        self.attention, self.hardness = args.attention, args.hardness
        self.export_inferred_segmentations = True
        self.compute_dtype = args.compute_dtype
        self.surface_metrics = args.surface_metrics
        self.surface_dice_mm = surface_dice_mm  # () = off
        self.measurements = args.measurements
        self.keep_largest_component, self.component_connectivity = args.keep_largest_component, args.component_connectivity
        self.fill_holes, self.hole_connectivity, self.min_component_mm3 = args.fill_holes, args.hole_connectivity, float(args.min_component_mm3)
        self.closing_mm, self.opening_mm = float(args.closing_mm), float(args.opening_mm)
        self.tta_flips, self.tta_average = tuple(args.tta_flips or ()), args.tta_average
        for k, v in augmentation.flat().items():  # aug_rotate_deg ... aug_acquisition_prob, as validated
            setattr(self, "aug_" + k, v)
        self.ce_weight, self.ce_foreground_weight, self.ce_topk = ce_weight, ce_foreground_weight, ce_topk
        self.tversky_beta, self.focal_tversky_gamma, self.batch_dice = region if region is not None else (None, 1.0, False)  # (None: the reference's Dice ratio per sample)
        self.ce_focal_gamma = ce_focal_gamma
        self.results_folder_path = os.path.join(self.data_root, "results", "debug" if self.debug else args.results_folder_name)
        self.logs_path = os.path.join(self.results_folder_path, "logs")
        self.model_path = os.path.join(self.results_folder_path, "model")
        self.figures_path = os.path.join(self.results_folder_path, "figures")
        rank, world, local = DP.init_distributed()
        self.rank, self.world = rank, world
        if not torch.cuda.is_available():
            raise RuntimeError("vs_seg_amd.VSparams: no GPU visible — this implementation has no CPU path (the reference falls back to whatever torch.device('cuda:0') does)")
        self.device = torch.device("cuda", local)
        self.logger = logging.getLogger()

    # ------------------------------------------------------------------ housekeeping
    def create_results_folders(self):
        for p in (self.logs_path, self.model_path, self.figures_path):
            os.makedirs(p, exist_ok=True)

    def set_up_logger(self, log_file_name):
        os.makedirs(self.logs_path, exist_ok=True)
        self.logger = logging.getLogger()
        fmt = logging.Formatter("%(asctime)s %(levelname)s        %(message)s")
        for h in (logging.FileHandler(os.path.join(self.logs_path, log_file_name), mode="w"), logging.StreamHandler()):
            h.setFormatter(fmt)
            self.logger.addHandler(h)
        self.logger.setLevel(logging.INFO if self.rank == 0 else logging.WARNING)
        self.logger.info("Created " + log_file_name)
        return self.logger

    def log_parameters(self):
        log = self.logger.info
        log("-" * 10)
        log("Parameters: ")
        logged = [  # (parameter names, logged when), in log order: an addition of this implementation is logged only where it is switched on
            (("dataset", "data_root", "split_csv", "pad_crop_shape", "pad_crop_shape_test", "num_workers", "torch_device_arg", "train_batch_size", "initial_learning_rate",
              "epochs_with_const_lr", "lr_divisor", "weight_decay", "num_epochs", "val_interval", "model", "sliding_window_inferer_roi_size", "attention", "hardness",
              "results_folder_path", "export_inferred_segmentations", "compute_dtype"), True),
            (("surface_metrics",), self.surface_metrics),
            (("surface_dice_mm",), self.surface_dice_mm),
            (("measurements",), self.measurements),
            (("fill_holes", "hole_connectivity"), self.fill_holes),
            (("closing_mm",), self.closing_mm > 0),
            (("opening_mm",), self.opening_mm > 0),
            (("min_component_mm3",), self.min_component_mm3 > 0),
            (("keep_largest_component",), self.keep_largest_component),
            (("component_connectivity",), self.keep_largest_component or self.min_component_mm3 > 0),
            (("tta_flips", "tta_average"), self.tta_flips),
            *((tuple("aug_" + k for k in fam.defaults), any(getattr(self, "aug_" + k) for k in fam.ranges)) for fam in FAMILIES),  # a family is logged when one of its ranges is non-zero
            (("ce_weight", "ce_foreground_weight"), self.ce_weight > 0),
            (("ce_topk",), self.ce_topk > 0),
            (("tversky_beta", "focal_tversky_gamma", "batch_dice"), self.tversky_beta is not None),
            (("ce_focal_gamma",), self.ce_focal_gamma > 0),
            (("optimizer",), self.optimizer != "adam"),
            (("momentum", "nesterov"), self.optimizer == "sgd"),
            (("clip_grad_norm",), self.clip_grad_norm > 0),
            (("lr_schedule", "poly_power"), self.lr_schedule == "poly"),
        ]
        for names, on in logged:
            for k in names if on else ():
                log("{:<34s} {}".format(k + " =", getattr(self, k)))
        log("-" * 10)

    # ------------------------------------------------------------------ data
    def load_T1_or_T2_data(self):
        names = {"T1": ("vs_gk_t1_refT1.nii.gz", "vs_gk_seg_refT1.nii.gz"), "T2": ("vs_gk_t2_refT2.nii.gz", "vs_gk_seg_refT2.nii.gz")}[self.dataset]
        sets: Dict[str, list] = {"training": [], "validation": [], "test": []}
        with open(self.split_csv) as f:
            for row in csv.reader(f):
                if len(row) >= 2 and row[1] in sets:
                    d = os.path.join(self.data_root, "input_data", row[0])
                    sets[row[1]].append({"image": os.path.join(d, names[0]), "label": os.path.join(d, names[1])})
        for fd in sets["training"] + sets["validation"] + sets["test"]:
            for k in ("image", "label"):
                assert os.path.isfile(fd[k]), f" {fd[k]} is not a file"
        self.logger.info("Number of images in training set   = {}".format(len(sets["training"])))
        self.logger.info("Number of images in validation set = {}".format(len(sets["validation"])))
        self.logger.info("Number of images in test set       = {}".format(len(sets["test"])))
        return sets["training"], sets["validation"], sets["test"]

    def get_transforms(self):
        """The three chains as plain descriptions; `cache_transformed_*_data` executes them (deterministic head cached in
        HBM, random tail per batch).  The augmentation flags reach the training chain only: the arguments of every family of FAMILIES as a dict under its key
        (`augment`, `field_augment`, `appearance_augment`, `acquisition_augment`; these dicts are also properties of that name, defined below the class)."""
        head = ["LoadNifti", "AddChannel", "Orientation(RAS)", "NormalizeIntensity(image)"]
        families = {fam.key: getattr(self, fam.key) for fam in FAMILIES}
        flat = {k: v for d in families.values() for k, v in d.items()}
        aug = [text.format(**flat) for keys, text in AUG_CHAIN if any(flat[k] for k in keys)]
        train = dict(chain=head + [f"SpatialPad({self.pad_crop_shape})", "RandFlip(p=0.5, axis=0)", f"RandSpatialCrop({self.pad_crop_shape})"] + aug, pad=self.pad_crop_shape, roi=self.pad_crop_shape, flip_prob=0.5, **families)
        val = dict(chain=head + [f"SpatialPad({self.pad_crop_shape})", f"RandSpatialCrop({self.pad_crop_shape})"], pad=self.pad_crop_shape, roi=self.pad_crop_shape, flip_prob=None)
        test = dict(chain=head, pad=None, roi=None, flip_prob=None)
        return train, val, test

    @staticmethod
    def get_center_of_mass_slice(label):
        """Index of the z slice closest to the label's centre of mass (uniform weights for an empty label)."""
        lab = np.asarray(label.detach().cpu() if torch.is_tensor(label) else label, dtype=np.float64)
        n = lab.shape[2]
        masses = np.array([lab[:, :, z].sum() for z in range(n)])
        w = masses / sum(masses) if sum(masses) != 0 else np.ones(n) / n
        # left-to-right Python sum, as the reference accumulates it: for an empty 10-slice label that is 4.500000000000001 -> 5
        return int(sum(w * np.arange(n)).round())

    def check_transforms_on_first_validation_image_and_label(self, val_files, val_transforms):
        """ref:params/VSparams.py:266-297 (called at ref:VS_train.py:36): run the validation chain on the first validation case and
        log what came out.  The PNG of the centre-of-mass slice is out of scope; the slice index is still logged."""
        logger = self.logger
        case = load_case(val_files[0], val_transforms["pad"], self.device)
        sampler = PatchSampler([case], val_transforms["roi"], val_transforms["flip_prob"], seed=0)
        img, lab = sampler.sample([0])
        check_data = {"image": img, "label": lab, "image_meta_dict": case["image_meta"], "label_meta_dict": case["label_meta"]}
        image, label = check_data["image"][0][0], check_data["label"][0][0]
        logger.info("-" * 10)
        logger.info("Check the transforms on the first validation set image and label")
        logger.info("Length of check_data = {}".format(len(check_data)))
        logger.info("check_data['image'].shape = {}".format(check_data["image"].shape))
        logger.info("Validation image shape = {}".format(image.shape))
        logger.info("Validation label shape = {}".format(label.shape))
        slice_idx = self.get_center_of_mass_slice(label)
        logger.info("-" * 10)
        logger.info("image shape: {}, label shape: {}, slice = {}".format(image.shape, label.shape, slice_idx))
        return check_data

    def _cache(self, files, tf, batch_size, shuffle, what):
        self.logger.info(f"Caching {what} data set...")
        cases = [load_case(fd, tf["pad"], self.device) for fd in files]
        return CachedLoader(cases, tf["roi"], batch_size, shuffle, tf["flip_prob"], seed=0, **{fam.key: tf.get(fam.key) for fam in FAMILIES})  # the crop/flip stream is decorrelated per rank inside CachedLoader

    def cache_transformed_train_data(self, train_files, train_transforms):
        return self._cache(train_files, train_transforms, self.train_batch_size, True, "training")

    def cache_transformed_val_data(self, val_files, val_transforms):
        return self._cache(val_files, val_transforms, 1, False, "validation")

    def cache_transformed_test_data(self, test_files, test_transforms):
        return self._cache(test_files, test_transforms, 1, False, "test")

    # ------------------------------------------------------------------ model / loss / optimizer
    def set_and_get_model(self):
        self.logger.info("Setting up the model type...")
        if self.model != "UNet2d5_spvPA":
            raise Exception("Model not defined.")
        return UNet2d5_spvPA(dimensions=3, in_channels=1, out_channels=2, num_res_units=2, norm="batch", dropout=0.1, attention_module=self.attention,
                             compute_dtype=self.compute_dtype, **HP).to(self.device)

    def set_and_get_loss_function(self):
        self.logger.info("Setting up the loss function...")
        return Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=self.attention, hardness_weighting=self.hardness, ce_weight=self.ce_weight, ce_foreground_weight=self.ce_foreground_weight, ce_topk=self.ce_topk,
                          tversky_beta=self.tversky_beta, focal_tversky_gamma=self.focal_tversky_gamma, batch_dice=self.batch_dice, ce_focal_gamma=self.ce_focal_gamma)

    def set_and_get_optimizer(self, model):
        self.logger.info("Setting up the optimizer...")
        clip = self.clip_grad_norm if self.clip_grad_norm > 0 else None
        if self.optimizer == "sgd":
            return SGD(model.parameters(), lr=self.initial_learning_rate, momentum=self.momentum, weight_decay=self.weight_decay, nesterov=self.nesterov, max_grad_norm=clip)
        if self.optimizer == "adamw":
            return AdamW(model.parameters(), lr=self.initial_learning_rate, weight_decay=self.weight_decay, max_grad_norm=clip)
        return Adam(model.parameters(), lr=self.initial_learning_rate, weight_decay=self.weight_decay, max_grad_norm=clip)

    def compute_dice_score(self, predicted_probabilities, label):
        return compute_dice_score(predicted_probabilities, label)  # [1,1] tensor, as the reference's

    # ------------------------------------------------------------------ training (ref:params/VSparams.py:409-528)
    def run_training_algorithm(self, model, loss_function, optimizer, train_loader, val_loader):
        logger = self.logger
        logger.info("Running the training loop...")
        trainer = DP.DataParallelTrainer(model, loss_function, optimizer)
        best_metric, best_metric_epoch = -1, -1
        epoch_loss_values, metric_values = [], []
        start = perf_counter()
        for epoch in range(self.num_epochs):
            logger.info("-" * 10)
            logger.info("Epoch {}/{}".format(epoch + 1, self.num_epochs))
            if epoch == self.val_interval:
                el = perf_counter() - start
                logger.info("Average duration of first {0:.0f} epochs = {1:.2f} s. Expected total training time = {2:.2f} h".format(self.val_interval, el / self.val_interval, el * self.num_epochs / self.val_interval / 3600))
            if self.lr_schedule == "poly":
                for group in optimizer.param_groups:
                    group["lr"] = poly_lr(self.initial_learning_rate, epoch, self.num_epochs, self.poly_power)
                    logger.info("Polynomial learning rate schedule: lr = {}".format(group["lr"]))
            model.train()
            step, losses = 0, []
            for batch in train_loader:
                step += 1
                losses.append(trainer.step(batch["image"], batch["label"], sync=False))  # device scalar, no host read
            lv = torch.stack(losses).double().cpu() if losses else torch.zeros(0)
            if epoch == 0:
                denom = len(train_loader) // train_loader.batch_size  # the reference's denominator (ref:params/VSparams.py:466)
                for i, v in enumerate(lv.tolist()):
                    logger.info("{}/{}, train_loss: {:.4f}".format(i + 1, denom, v))
            if self.clip_grad_norm > 0 and hasattr(optimizer, "grad_norm_stats"):  # one more host read, beside the epoch's own
                gn = optimizer.grad_norm_stats(reset=True)
                logger.info("epoch {} gradient norm: mean {:.4f} max {:.4f}, clipped {}/{} steps at {}, skipped {} (NaN / Inf norm)".format(
                    epoch + 1, gn["mean_norm"], gn["max_norm"], gn["clipped"], gn["steps"], self.clip_grad_norm, gn["skipped"]))
            epoch_loss = float(lv.sum()) / max(step, 1)
            if not np.isfinite(epoch_loss):
                # the fixed-point accumulators (BatchNorm statistics, backward sums, Dice sums) flag an out-of-range or non-finite partial sum and every kernel that decodes
                # them returns NaN from then on (include/vsseg_hip.h): name that cause once and clear the flag, so that a later epoch is not poisoned by it
                from ._lib import fx_status

                if fx_status(reset=True):
                    logger.error("epoch {}: a fixed-point partial sum left its range or was NaN / Inf (diverging activations or gradients, or a loss scale beyond 256): "
                                 "the statistics / loss of the affected steps are NaN; the flag was reset".format(epoch + 1))
            epoch_loss_values.append(epoch_loss)
            logger.info("epoch {} average loss: {:.4f}".format(epoch + 1, epoch_loss))

            if (epoch + 1) % self.val_interval == 0:
                metric, epoch_loss_val = self.validate(model, loss_function, val_loader)
                metric_values.append(metric)
                logger.info("validation loss (reference accounting: twice the mean): {:.4f}".format(epoch_loss_val))
                if metric > best_metric:
                    best_metric, best_metric_epoch = metric, epoch + 1
                    if self.rank == 0:
                        torch.save(model.state_dict(), os.path.join(self.model_path, "best_metric_model.pth"))
                    logger.info("saved new best metric model")
                logger.info("current epoch {} current mean dice: {:.4f} best mean dice: {:.4f} at epoch {}".format(epoch + 1, metric, best_metric, best_metric_epoch))

            if self.lr_schedule == "halving" and (epoch + 1) % self.epochs_with_const_lr == 0:
                for group in optimizer.param_groups:
                    group["lr"] = group["lr"] / self.lr_divisor
                    logger.info("Dividing learning rate by {}. New learning rate is: lr = {}".format(self.lr_divisor, group["lr"]))

        logger.info("Train completed, best_metric: {:.4f}  at epoch: {}".format(best_metric, best_metric_epoch))
        if self.rank == 0:
            torch.save(model.state_dict(), os.path.join(self.model_path, "last_epoch_model.pth"))
        logger.info(f'Saved model of the last epoch at: {os.path.join(self.model_path, "last_epoch_model.pth")}')
        return epoch_loss_values, metric_values

    def validate(self, model, loss_function, val_loader):
        """N1: one validation pass without per-case host reads.  Returns (mean Dice, validation loss in the reference's
        accounting).  Multi-GPU: cases are sharded by the loader, sums are all-reduced."""
        DP.broadcast_buffers(model)  # data parallel: every rank validates (and rank 0 saves) rank 0's BatchNorm running statistics
        model.eval()
        dice_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        loss_sum = torch.zeros((), dtype=torch.float64, device=self.device)
        count = steps = 0
        with torch.no_grad():
            for batch in val_loader:
                steps += 1
                outputs = model(batch["image"])
                dice = self.compute_dice_score(outputs[0], batch["label"])
                loss = loss_function(outputs, batch["label"])
                # the reference adds every case twice (ref:params/VSparams.py:490-496)
                count += 2 * len(dice)
                dice_sum += 2.0 * dice.sum().double()
                loss_sum += 2.0 * loss.double()
        t = torch.stack([dice_sum, loss_sum, torch.tensor(float(count), dtype=torch.float64, device=self.device), torch.tensor(float(steps), dtype=torch.float64, device=self.device)])
        t = DP.allreduce_sum(t)
        d, l, c, s = t.tolist()  # the only host read of the pass
        return d / max(c, 1.0), l / max(s, 1.0)

    def plot_loss_curve_and_mean_dice(self, epoch_loss_values, metric_values):
        """Figures are out of scope; the curves are written as CSV next to where the reference puts its PNG."""
        os.makedirs(self.figures_path, exist_ok=True)
        with open(os.path.join(self.figures_path, "epoch_average_loss_and_val_mean_dice.csv"), "w") as f:
            f.write("epoch,average_loss,val_mean_dice\n")
            for i, v in enumerate(epoch_loss_values):
                m = metric_values[(i + 1) // self.val_interval - 1] if (i + 1) % self.val_interval == 0 and (i + 1) // self.val_interval <= len(metric_values) else ""
                f.write(f"{i + 1},{v},{m}\n")

    # ------------------------------------------------------------------ inference (ref:params/VSparams.py:546-625)
    def load_trained_state_of_model(self, model):
        from .checkpoint import load_checkpoint

        load_checkpoint(model, os.path.join(self.model_path, "best_metric_model.pth"))
        return model

    @property
    def _post_flags(self) -> Dict[str, bool]:
        """Which steps of the post-processing chain are on, under the names of POST_STEPS and report.postprocessing."""
        return dict(fill_holes=self.fill_holes, closing=self.closing_mm > 0, opening=self.opening_mm > 0, min_component=self.min_component_mm3 > 0, keep_largest=self.keep_largest_component)

    def _reports(self) -> List[R.Report]:
        """The reports that are switched on, in the order of their sections in the log."""
        return ([R.postprocessing(**self._post_flags)] if any(self._post_flags.values()) else []) + ([R.surface_metrics()] if self.surface_metrics else []) + (
            [R.surface_dice(surface_dice_rows(self.surface_dice_mm))] if self.surface_dice_mm else []) + ([R.measurements(MEASUREMENT_FIELDS)] if self.measurements else [])

    def run_inference(self, model, data_loader):
        logger = self.logger
        logger.info("Running inference...")
        model.eval()
        n = len(data_loader)
        reports = self._reports()
        table = R.CaseTable(("dice",) + tuple(k for rep in reports for k in rep.rows), n, self.device)
        post_rows = R.postprocessing(**self._post_flags).rows[1:] if any(self._post_flags.values()) else ()  # after dice_raw: the statistics of the chain
        predictor = model.segmentation_predictor() if hasattr(model, "segmentation_predictor") else (lambda *a, **k: model(*a, **k)[0])  # model_segmentation, ref:params/VSparams.py:560
        mine = DP.shard_indices(n)  # the unpadded, unshuffled test loader yields exactly these cases, in this order
        with torch.no_grad():
            for i, data in enumerate(data_loader):
                assert i < len(mine), "the test loader yielded more cases than this rank's shard (a padded loader would double-count them)"
                logger.info("starting image {}".format(mine[i]))
                outputs = sliding_window_inference(inputs=data["image"], roi_size=self.sliding_window_inferer_roi_size, sw_batch_size=1, predictor=predictor, mode="gaussian",
                                                   tta_flips=self.tta_flips, tta_average=self.tta_average)
                gi, label, spacing = mine[i], data["label"], voxel_spacing(data["label_meta_dict"]["affine"])
                if post_rows:  # everything below describes the filtered prediction; the raw Dice is kept beside it
                    table.set(gi, ("dice_raw",), self.compute_dice_score(outputs, label).reshape(1))
                    outputs, stats = self._postprocess(outputs, spacing)
                    table.set(gi, post_rows, torch.stack([stats[k] for k in post_rows]))
                table.set(gi, ("dice",), self.compute_dice_score(outputs, label).reshape(1))
                if self.surface_dice_mm:  # one call: its first two columns are the bits compute_surface_distances returns
                    sm = compute_surface_metrics(outputs, label, spacing, 95.0, self.surface_dice_mm)[0]
                    table.set(gi, surface_dice_rows(self.surface_dice_mm), sm[2:])
                    if self.surface_metrics:
                        table.set(gi, R.SURFACE_ROWS, sm[:2])
                elif self.surface_metrics:
                    table.set(gi, R.SURFACE_ROWS, compute_surface_distances(outputs, label, spacing, 95.0)[0])
                if self.measurements:
                    table.set(gi, MEASUREMENT_FIELDS, compute_measurements(outputs, label, spacing)[0])
                if self.export_inferred_segmentations:
                    self.export_segmentation(outputs, data["label_meta_dict"])
        values = table.gather(DP.allreduce_sum if self.world > 1 else None)  # one all-reduce, one host read
        R.emit(reports, values, logger.info, self.figures_path if self.rank == 0 else None)
        return values["dice"]

    def _postprocess(self, outputs, spacing):
        """The steps of POST_STEPS that are switched on, each on the output of the previous one.  Returns the final one-hot prediction and the statistics of the case by name,
        on the device: foreground_voxels of the raw prediction, components of the input of the first component filter (without one: of the final prediction), kept_voxels of
        the final prediction, and what each step filled, closed, opened or removed."""
        stats = {}
        for name, step in POST_STEPS.items():
            if self._post_flags[name]:
                outputs, st = step(self, outputs, spacing)
                stats = {**st, **stats, "kept_voxels": st["kept_voxels"]}  # a name belongs to the first step that reports it (foreground_voxels, components); kept_voxels to the last
        if "components" not in stats:  # no component filter: --fill_holes, --closing_mm, --opening_mm alone or together
            stats["components"] = connected_components(outputs, self.component_connectivity)[1][0, 1]
        return outputs, stats

    def export_segmentation(self, outputs, label_meta):
        """N3: argmax → uint8 NIfTI in the label's original orientation / affine, under
        results/inferred_segmentations_nifti/<case folder>/ like MONAI's NiftiSaver(output_postfix='')."""
        seg = argmax_segmentation(outputs)[0].cpu().numpy()  # vsseg_argmax2: ties -> class 0, like torch.argmax
        seg = nifti.from_ras(seg, label_meta["ornt"])
        src = label_meta["filename_or_obj"]
        folder = os.path.basename(os.path.dirname(src))
        out_dir = os.path.join(self.results_folder_path, "inferred_segmentations_nifti", folder, os.path.basename(src).split(".")[0])
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, os.path.basename(src).split(".")[0] + ".nii.gz")
        nifti.write_nifti(path, seg, label_meta["original_affine"], dtype=np.uint8)
        self.logger.info(f"export to nifti... {path}")
        return path


for _fam in FAMILIES:  # VSparams.augment, .field_augment, .appearance_augment, .acquisition_augment
    setattr(VSparams, _fam.key, property(lambda self, fam=_fam: {k: getattr(self, "aug_" + k) for k in fam.defaults}))  # under PatchSampler's argument names (every range 0: off)

