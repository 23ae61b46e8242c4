"""-m gpu: test-time mirror augmentation of sliding-window inference (`tta_flips`): the three-axis mirror of the crop kernel, the mirrored passes against the
composition that defines them (tests/tta_oracle.py) — bit for bit through vs_seg_amd's own sliding_window_inference and `torch.flip`, and at the blend tolerance
against the CPU oracle — the schedule, the probability average, the real network, the window-sharded path and the command line."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vs_seg_amd as V  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd import parallel as DP  # noqa: E402
from vs_seg_amd.inferers import window_geometry  # noqa: E402
from tests import tta_oracle as TO  # noqa: E402

BLEND_TOL = 2e-6  # test_gpu_ops.py::test_sliding_window_blend_matches_oracle


def test_crop_mirrors_every_subset_of_the_axes():
    lib = L.lib()
    dims, roi = (9, 7, 5), (12, 6, 4)  # the pad total along x is 3: odd
    v = np.random.default_rng(4).standard_normal(dims).astype(np.float32)
    src = torch.from_numpy(v).cuda()
    cases = [(mask, origin) for mask in range(8) for origin in ((-1, 0, 0), (-2, 1, 1))]
    jobs = (L.CropJob * (len(cases) + 1))()
    for j, (mask, origin) in zip(jobs, cases):
        j.src, j.sdims, j.origin, j.flip = src.data_ptr(), L.i3(dims), L.i3(origin), mask
    jobs[len(cases)].src, jobs[len(cases)].sdims, jobs[len(cases)].origin, jobs[len(cases)].flip_x = src.data_ptr(), L.i3(dims), L.i3((-1, 0, 0)), 1  # as the training sampler sets it
    assert jobs[len(cases)].flip == 1 and jobs[1].flip_x == 0 and jobs[2].flip_x == 1
    jb = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).cuda()
    out = torch.full((len(jobs), *roi), 7.0, device="cuda")
    L.check(lib.vsseg_crop_flip(jb.data_ptr(), len(jobs), out.data_ptr(), L.i3(roi), torch.cuda.current_stream().cuda_stream))
    got = out.cpu().numpy()

    def want(mask, origin):
        m = np.flip(v, [a for a in range(3) if mask >> a & 1])  # the mirror acts on the volume, before the zero padding
        big = np.pad(m, [(8, 8)] * 3)
        return big[tuple(slice(8 + o, 8 + o + r) for o, r in zip(origin, roi))]

    for i, (mask, origin) in enumerate(cases):
        np.testing.assert_array_equal(got[i], want(mask, origin), err_msg=f"mask {mask} origin {origin}")
    np.testing.assert_array_equal(got[-1], np.pad(v[::-1], ((1, 2), (0, 0), (0, 0)))[:, :6, :4])  # flip_x = 1: what the x-only kernel produced


@pytest.fixture(scope="module")
def blend_inputs():
    return [TO.volume(c).cuda() for c in range(len(TO.CASES))]


@pytest.mark.parametrize("case", range(len(TO.CASES)))
@pytest.mark.parametrize("flips", TO.FLIPS)
def test_mirrored_passes_equal_the_hand_made_composition(blend_inputs, case, flips):
    vol, roi, ov, mode = TO.CASES[case]
    x = blend_inputs[case]
    pred = TO.position_dependent_predictor(roi, "cuda")
    got = V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=flips)
    assert tuple(got.shape) == (TO.BATCH, 2, *vol)
    assert torch.equal(got, TO.composed_tta(x, roi, 1, pred, ov, mode, flips))
    want = TO.oracle_case(case, flips)
    err = float((got.cpu() - want).abs().max())
    print(f"case {case} flips {flips}: max |gpu - oracle| {err:.3e}")
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=BLEND_TOL, rtol=BLEND_TOL)


@pytest.mark.parametrize("case", range(len(TO.CASES)))
def test_result_does_not_depend_on_the_schedule(blend_inputs, case):
    vol, roi, ov, mode = TO.CASES[case]
    x = blend_inputs[case]
    pred = TO.position_dependent_predictor(roi, "cuda")
    plain = V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode)
    assert torch.equal(V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=()), plain)
    assert torch.equal(V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=None), plain)
    for flips in ((0,), (1, 2)):
        base = V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=flips, concurrent_groups=1)
        assert not torch.equal(base, plain)
        assert torch.equal(V.sliding_window_inference(x, roi, 3, pred, overlap=ov, mode=mode, tta_flips=flips, concurrent_groups=1), base)
        assert torch.equal(V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=flips, concurrent_groups=2), base)
        assert torch.equal(V.sliding_window_inference(x, roi, 3, pred, overlap=ov, mode=mode, tta_flips=flips, concurrent_groups=2), base)


@pytest.mark.parametrize("swb,lanes", [(1, 1), (3, 1), (3, 2)])
def test_predictor_sees_pass_order_then_reference_window_order(blend_inputs, swb, lanes):
    vol, roi, ov, mode = TO.CASES[0]
    x = blend_inputs[0]
    flips = (0, 2)
    _, _, pad_before, _, starts = window_geometry(vol, roi, ov)
    seen = []

    def pred(w):
        seen.append(w[:, 0, 0, 0, 0].clone())  # the first voxel of every window of the group
        return torch.cat([w, -w], 1)

    V.sliding_window_inference(x, roi, swb, pred, overlap=ov, mode=mode, tta_flips=flips, concurrent_groups=lanes)
    n_windows = TO.BATCH * len(starts)
    assert len(seen) == 4 * math.ceil(n_windows / swb)  # groups never straddle two passes
    want = []
    for dims in TO.pass_dims(flips):
        padded = torch.nn.functional.pad(torch.flip(x, dims), [p for a in (2, 1, 0) for p in (pad_before[a], max(roi[a] - vol[a], 0) - pad_before[a])])
        want += [padded[b, 0, s[0], s[1], s[2]] for b in range(TO.BATCH) for s in starts]
    assert torch.equal(torch.cat(seen), torch.stack(want))


@pytest.mark.parametrize("flips", [(0,), (0, 1, 2)])
def test_probability_average(blend_inputs, flips):
    """tta_average="probabilities": the mean over the passes of the softmax of each pass's normalised logits.  Reference: float64 softmax of the per-pass GPU logits.
    atol 1e-6 is about 8 fp32 ulp at 1.0, twice the error bound of roughly 4 ulp (expf 1-2 ulp, a correctly rounded divide, a two-term sum)."""
    vol, roi, ov, mode = TO.CASES[0]
    x = blend_inputs[0]
    pred = TO.position_dependent_predictor(roi, "cuda")
    got = V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=flips, tta_average="probabilities")
    per_pass = TO.passes(lambda v: V.sliding_window_inference(v, roi, 1, pred, overlap=ov, mode=mode), x, flips)
    want = torch.stack([torch.softmax(r.double(), 1) for r in per_pass]).mean(0)
    err = float((got.double() - want).abs().max())
    print(f"flips {flips}: max |probability - float64 reference| {err:.3e}")
    assert err <= 1e-6
    assert float((got.double().sum(1) - 1.0).abs().max()) <= 1e-6
    assert not torch.equal(got, V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, tta_flips=flips))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_network_with_mirrored_passes_equals_the_composition(dt):
    from tests.helpers import synth_input
    from tests.test_gpu_network import make_model

    seed = 57
    m = make_model(True, dt, seed).eval()
    vol, roi = (70, 36, 5), (32, 32, 8)  # x starts 0,16,32,38: not symmetric; z pad 3, pad_before 1; 8 windows
    assert len(window_geometry(vol, roi, 0.5)[4]) == 8
    x = synth_input(seed, (1, 1, *vol)).cuda()
    sp = m.segmentation_predictor()
    with torch.no_grad():
        for flips in ((0,), (0, 2)):
            want = TO.composed_tta(x, roi, 1, lambda w: m(w)[0], 0.5, "gaussian", flips)
            assert torch.equal(V.sliding_window_inference(x, roi, 1, lambda w: m(w)[0], overlap=0.5, mode="gaussian", tta_flips=flips), want)
            assert torch.equal(V.sliding_window_inference(x, roi, 1, sp, overlap=0.5, mode="gaussian", tta_flips=flips, concurrent_groups=2), want)
            assert torch.isfinite(want).all()


def test_sharded_inference_with_mirrored_passes_equals_the_single_process_result(blend_inputs):
    vol, roi, ov, mode = TO.CASES[0]
    x = blend_inputs[0]
    pred = TO.position_dependent_predictor(roi, "cuda")
    assert DP.world_size() == 1
    for kw in (dict(tta_flips=(0, 1)), dict(tta_flips=(0, 1), tta_average="probabilities"), dict()):
        assert torch.equal(DP.sharded_sliding_window_inference(x, roi, pred, overlap=ov, mode=mode, **kw), V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode, **kw)), kw


def test_vsparams_tta_flips_end_to_end(tmp_path):
    from tests.volume_cases import run_inference as _run_inference

    p, model, loader, scores, log = _run_inference(tmp_path / "on", ["--tta_flips", "0"])
    assert scores.shape == (1,) and "tta_flips =" in log and "tta_average =" in log
    with torch.no_grad():
        data = next(iter(loader))
        roi = p.sliding_window_inferer_roi_size
        tta = V.sliding_window_inference(data["image"], roi, 1, model.segmentation_predictor(), mode="gaussian", tta_flips=(0,))
        plain = V.sliding_window_inference(data["image"], roi, 1, model.segmentation_predictor(), mode="gaussian")
        assert float(scores[0]) == float(V.compute_dice_score(tta, data["label"]))
        assert f"dice_score[0] = {float(scores[0])}" in log
    p2, _, _, scores2, log2 = _run_inference(tmp_path / "off", [])
    assert "tta_" not in log2.replace(str(tmp_path), "")
    assert float(scores2[0]) == float(V.compute_dice_score(plain, data["label"]))
