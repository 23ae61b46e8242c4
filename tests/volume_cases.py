"""Inputs that the GPU tests of the whole-volume analysis calls share (components, morphology, measurements, surface metrics, surface Dice): logits with a given
argmax, labels, the full-size channels-last case with its far island, a stand-in threshold network and one VSparams inference run on synthetic cases."""
import argparse
import functools
import os

import numpy as np
import torch


def logits(pred):
    """[B,2,X,Y,Z] logits whose argmax is `pred` [B,X,Y,Z], with random magnitudes."""
    rng = np.random.default_rng(11)
    a = rng.standard_normal(pred.shape).astype(np.float32)
    b = a + np.where(pred, 1.0, -1.0).astype(np.float32) * rng.uniform(0.01, 2.0, pred.shape).astype(np.float32)
    return torch.from_numpy(np.stack([a, b], 1)).cuda()


def label(gt):
    return torch.from_numpy(gt[:, None].astype(np.float32)).cuda()


FULL_SIZE = (512, 512, 120)


def full_size_ellipsoid(c, r):
    g = np.ogrid[: FULL_SIZE[0], : FULL_SIZE[1], : FULL_SIZE[2]]
    return ((g[0] - c[0]) / r[0]) ** 2 + ((g[1] - c[1]) / r[1]) ** 2 + ((g[2] - c[2]) / r[2]) ** 2 <= 1.0


def full_size_outputs(pred):
    cl = torch.full((1, *pred.shape, 2), -1.0, device="cuda")
    cl[0, ..., 1] = torch.where(torch.from_numpy(pred).cuda(), 1.0, -2.0)
    return cl.permute(0, 4, 1, 2, 3)  # [1,2,X,Y,Z] view of channels-last storage, as sliding_window_inference returns it


@functools.lru_cache(maxsize=1)
def far_island_case():
    """(tumour, island, gt) at 512 x 512 x 120: a tumour ellipsoid in the prediction, shifted against the one of the label `gt`, and one far false-positive island.
    The arrays are shared between the tests: read them only."""
    tumour, island, gt = full_size_ellipsoid((302, 219, 61), (13, 12, 5)), full_size_ellipsoid((40, 470, 12), (3, 2, 1.5)), full_size_ellipsoid((300, 220, 60), (14, 11, 5))
    return tumour, island, gt


class BrightVoxels:
    """A stand-in network: class 1 where the image is brighter than `threshold`, so that the prediction is the bright tumour plus scattered noise voxels."""

    def __init__(self, threshold):
        self.threshold = threshold

    def eval(self):
        return self

    def __call__(self, x):
        return (torch.cat([torch.zeros_like(x), x - self.threshold], 1),)


def run_inference(tmp_path, flags, bright_quantile=None):
    """(params, model, test loader, scores, log text) of one VSparams test run with `flags` on four synthetic cases; `bright_quantile`: with the stand-in network
    that marks the voxels above that quantile of the first image instead of the seeded UNet."""
    from tests.test_gpu_data import _write_cases
    from vs_seg_amd.params import VSparams

    root = str(tmp_path)
    split = _write_cases(root, 4, np.random.default_rng(3))
    argv = ["--split", split, "--data_root", root, "--results_folder_name", "t", "--compute_dtype", "fp32"] + list(flags)
    p = VSparams(argparse.ArgumentParser(), argv)
    p.sliding_window_inferer_roi_size = [64, 64, 16]
    p.create_results_folders()
    logger = p.set_up_logger("test_log.txt")
    p.log_parameters()
    _, _, test_files = p.load_T1_or_T2_data()
    _, _, stf = p.get_transforms()
    test_loader = p.cache_transformed_test_data(test_files, stf)
    torch.manual_seed(0)
    if bright_quantile is None:
        model = p.set_and_get_model()
        model.eval()
    else:
        model = BrightVoxels(float(next(iter(test_loader))["image"].flatten().quantile(bright_quantile)))
    scores = p.run_inference(model, test_loader)
    for h in list(logger.handlers):
        logger.removeHandler(h)
        h.close()
    return p, model, test_loader, scores, open(os.path.join(p.logs_path, "test_log.txt")).read()
