"""-m gpu: the post-processing chain of VSparams (POST_STEPS, `_postprocess`) on a 64 x 64 x 16 stand-in case: for subsets of the five steps the statistics it
returns BY NAME, and the final prediction, equal what the numpy oracles give step by step (tests/morphology_oracle.py, tests/ball_oracle.py,
tests/components_oracle.py).  Integers and exact 0.0 / 1.0 values only: no tolerance."""
import argparse

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import ball_oracle as BO  # noqa: E402
from tests import components_oracle as CO  # noqa: E402
from tests import morphology_oracle as MO  # noqa: E402
from tests.volume_cases import run_inference  # noqa: E402

SPACING = (0.5, 0.5, 1.5)  # of the synthetic cases
ARGV = dict(fill_holes=["--fill_holes"], closing=["--closing_mm", "1.5"], opening=["--opening_mm", "1"], min_component=["--min_component_mm3", "1.2"], keep_largest=["--keep_largest_component"])


@pytest.fixture(scope="module")
def raw(tmp_path_factory):
    """(argv head, raw prediction [1,2,X,Y,Z] on the device, its mask, spacing) of the first case: the tumour and 10 % scattered voxels.  Read only."""
    from vs_seg_amd import sliding_window_inference
    from vs_seg_amd.metrics import voxel_spacing

    p, model, loader, _, _ = run_inference(tmp_path_factory.mktemp("chain"), [], 0.9)
    with torch.no_grad():
        data = next(iter(loader))
        o = sliding_window_inference(data["image"], p.sliding_window_inferer_roi_size, 1, lambda x: model(x)[0], mode="gaussian")
    spacing = voxel_spacing(data["label_meta_dict"]["affine"])
    np.testing.assert_allclose(spacing, SPACING, rtol=1e-6)
    return ["--data_root", p.data_root, "--results_folder_name", "t"], o, CO.prediction_mask(o[0].cpu().numpy()), spacing


def _oracle_chain(mask, on, min_voxels):
    """(final mask, statistics by name) of the steps `on` in the order fill holes, closing, opening, remove small, keep largest."""
    want, cur = {"foreground_voxels": int(mask.sum())}, mask  # of the raw prediction, whichever step runs first
    if "fill_holes" in on:
        st = MO.fill_stats(cur, 6)
        want.update(holes=int(st[1]), filled_voxels=int(st[2]))
        cur = MO.fill_holes(cur, 6)
    if "closing" in on:
        new = BO.close(cur, SPACING, 1.5)
        want["closed_voxels"], cur = int((new & ~cur).sum()), new
    if "opening" in on:
        new = BO.open_(cur, SPACING, 1.0)
        want["opened_voxels"], cur = int((cur & ~new).sum()), new
    if "min_component" in on:  # the first component filter: `components` is that of its input
        st = MO.small_stats(cur, min_voxels, 6)
        want.update(components=int(st[1]), small_components=int(st[1] - st[3]), small_voxels=int(st[0] - st[2]))
        cur = MO.remove_small(cur, min_voxels, 6)
    if "keep_largest" in on:
        want.setdefault("components", int(CO.stats(CO.label(cur, 6))[1]))
        cur = CO.keep_largest(cur, 6)
    want.setdefault("components", int(CO.stats(CO.label(cur, 6))[1]))  # no component filter: of the final prediction
    want["kept_voxels"] = int(cur.sum())
    return cur, want


@pytest.mark.parametrize("on", [("closing",), ("fill_holes", "opening"), ("min_component",), tuple(ARGV)], ids="+".join)
def test_chain_statistics_by_name_equal_the_oracles(raw, on):
    from vs_seg_amd import min_component_voxels
    from vs_seg_amd import report as R
    from vs_seg_amd.params import VSparams

    head, o, mask, spacing = raw
    p = VSparams(argparse.ArgumentParser(), head + ["--component_connectivity", "6"] + sum((ARGV[k] for k in on), []))
    assert p._post_flags == {k: k in on for k in ARGV}
    before = o.clone()
    out, stats = p._postprocess(o, spacing)
    assert torch.equal(o, before)
    final, want = _oracle_chain(mask, on, min_component_voxels(1.2, SPACING))
    assert set(stats) == set(want) == set(R.postprocessing(**p._post_flags).rows[1:])  # what the report declares, no more
    assert all(torch.is_tensor(v) and v.is_cuda and v.shape == () for v in stats.values())  # nothing was read on the host
    assert {k: int(v) for k, v in stats.items()} == want
    assert want["foreground_voxels"] == int(mask.sum()) > want["components"] > 0 and (final != mask).any()  # the steps had work to do
    assert torch.equal(out.cpu(), torch.from_numpy(CO.one_hot(final)[None]))
