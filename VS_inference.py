#!/usr/bin/env python
"""Sliding-window inference on the test set — the reference's VS_inference.py (ref:VS_inference.py) on the MI355X hot path.

    python VS_inference.py --results_folder_name run1 [--dataset T2] [--no_attention] [--debug]

`--surface_metrics` also reports HD95 and ASSD (mm) per test case, computed on the GPU, and writes figures/test_surface_metrics.csv.
`--surface_dice_mm TAU [TAU ...]` also reports the normalised surface Dice, the surface precision and recall at each tolerance (mm) and the mean of the two
directed mean surface distances per test case, from the same GPU call, and writes figures/test_surface_dice.csv.
`--keep_largest_component [--component_connectivity 26]` keeps only the largest connected component of each predicted segmentation (on the GPU) before
the Dice, the surface metrics and the NIfTI export; the raw Dice and the component counts go to the log and figures/test_postprocessing.csv.
`--fill_holes [--hole_connectivity 6]` fills the holes of each predicted segmentation and `--min_component_mm3 V` drops its connected components below
V cubic millimetres (both on the GPU, in this order, before --keep_largest_component); their counts are added to the same log and CSV.
`--closing_mm R` / `--opening_mm R` close / open each predicted segmentation with a ball of R mm at the voxel spacing of the case (on the GPU, after
--fill_holes and before --min_component_mm3, closing first): fragments a millimetre apart are bridged before the component filters see them, spurs
thinner than the ball go before the measurements are taken; closed_voxels / opened_voxels are added to the same log and CSV.
`--measurements` also reports per test case the volume (mm^3), the largest 3-D diameter and the largest diameter within an axial slice (mm) of the
predicted and of the manual segmentation and the distance between their centres of mass, computed on the GPU (after --keep_largest_component and
--tta_flips, when given), the volume and diameter errors over the cases, and writes figures/test_measurements.csv.
"""
import argparse
import random

import numpy as np
import torch

from vs_seg_amd.params import VSparams

parser = argparse.ArgumentParser(description="Run inference with the trained model")
p = VSparams(parser)
logger = p.set_up_logger("test_log.txt")
p.log_parameters()
train_files, val_files, test_files = p.load_T1_or_T2_data()
train_transforms, val_transforms, test_transforms = p.get_transforms()
random.seed(0)
np.random.seed(0)
torch.manual_seed(0)
test_loader = p.cache_transformed_test_data(test_files, test_transforms)
model = p.set_and_get_model()
model = p.load_trained_state_of_model(model)
p.run_inference(model, test_loader)
