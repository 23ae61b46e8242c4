"""CPU tests of test-time mirror augmentation: the argument checks of `sliding_window_inference(..., tta_flips=, tta_average=)` are made before the device check,
the pass order, the command-line flags, and the sanity of the oracle composition the GPU tests compare against (tests/tta_oracle.py)."""
import argparse
import ctypes

import pytest
import torch

import vs_seg_amd as V
from vs_seg_amd import _lib as L
from vs_seg_amd.inferers import tta_masks
from vs_seg_amd import parallel as DP
from tests import tta_oracle as TO


def _pred(w):
    return torch.cat([w, -w], 1)


@pytest.mark.parametrize("kw", [dict(tta_flips=(3,)), dict(tta_flips=(-1,)), dict(tta_flips=(0, 1, 0)), dict(tta_flips=(0,), tta_average="mean"), dict(tta_average="probabilities"),
                                dict(tta_flips=(), tta_average="probabilities")])
def test_bad_tta_arguments_are_value_errors_before_the_device_check(kw):
    x = torch.zeros(1, 1, 8, 8, 8)
    with pytest.raises(ValueError):
        V.sliding_window_inference(x, (8, 8, 8), 1, _pred, **kw)
    with pytest.raises(ValueError):
        DP.sharded_sliding_window_inference(x, (8, 8, 8), _pred, **kw)


@pytest.mark.parametrize("kw", [dict(), dict(tta_flips=None), dict(tta_flips=()), dict(tta_flips=(0,)), dict(tta_flips=(0, 2), tta_average="probabilities")])
def test_cpu_tensors_are_still_rejected(kw):
    with pytest.raises(RuntimeError, match="MI355X only"):
        V.sliding_window_inference(torch.zeros(1, 1, 8, 8, 8), (8, 8, 8), 1, _pred, **kw)


def test_pass_order_is_the_bit_mask_order_with_the_identity_first():
    assert tta_masks(None) == tta_masks(()) == [0]
    assert tta_masks((0,)) == [0, 1] and tta_masks((2,)) == [0, 4]
    assert tta_masks((1, 2)) == [0, 2, 4, 6] and tta_masks((2, 1)) == [0, 4, 2, 6]  # bit i of the pass number selects tta_flips[i]
    assert tta_masks((0, 1, 2)) == list(range(8))
    for flips in TO.FLIPS:  # the oracle numbers its passes the same way (dims of [B,C,X,Y,Z])
        assert [sum(1 << (d - 2) for d in dims) for dims in TO.pass_dims(flips)] == tta_masks(flips)


def test_command_line_flags():
    from vs_seg_amd.params import VSparams

    def parse(argv):
        try:
            return VSparams(argparse.ArgumentParser(), argv)
        except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
            assert "no GPU" in str(e)
            return None

    for bad in (["--tta_flips", "3"], ["--tta_flips", "0", "0"], ["--tta_average", "probabilities"], ["--tta_flips", "0", "--tta_average", "mean"]):
        with pytest.raises(SystemExit):
            parse(bad)
    for good in ([], ["--tta_flips"], ["--tta_flips", "0"], ["--tta_flips", "0", "2", "--tta_average", "probabilities"]):
        p = parse(good)
        if p is not None:
            assert p.tta_flips == tuple(int(a) for a in good[1:] if a.isdigit())


@pytest.mark.parametrize("flips", TO.FLIPS)
def test_oracle_leaves_a_voxelwise_predictor_unchanged(flips):
    """A predictor that maps every voxel on its own commutes with mirroring, and the blend is a weighted mean of equal values: every pass gives the plain result."""
    vol, roi, ov, mode = TO.CASES[0]
    x = TO.volume(0)
    pred = lambda w: torch.cat([w * 2.0 + 1.0, torch.tanh(w) - 0.5], 1)  # noqa: E731
    plain = TO.O.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode=mode)
    for r in TO.passes(lambda v: TO.O.sliding_window_inference(v, roi, 1, pred, overlap=ov, mode=mode), x, flips):
        torch.testing.assert_close(r, plain, atol=2e-6, rtol=2e-6)
    torch.testing.assert_close(TO.oracle_tta(x, roi, 1, pred, ov, mode, flips), plain, atol=2e-6, rtol=2e-6)


@pytest.mark.parametrize("case", range(len(TO.CASES)))
@pytest.mark.parametrize("flips", TO.FLIPS)
def test_oracle_tta_differs_from_the_plain_result_for_the_position_dependent_predictor(case, flips):
    """What the GPU tests compare against is far from the un-augmented volume, so an implementation that ignored tta_flips cannot pass them."""
    vol, roi, ov, mode = TO.CASES[case]
    plain = TO.O.sliding_window_inference(TO.volume(case), roi, 1, TO.position_dependent_predictor(roi), overlap=ov, mode=mode)
    want = TO.oracle_case(case, flips)
    assert want.shape == plain.shape == (TO.BATCH, 2, *vol)
    assert float((want - plain).abs().max()) > 1.0


def test_finalize_rejects_bad_arguments_before_the_launch():
    """vsseg_swi_finalize_mirrored checks its arguments before it touches the device, so the refusals are the same on a machine without one (the pointers are never followed)."""
    lib = L.lib()
    assert lib.vsseg_version() >= 10
    mem = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(mem)

    def call(pdims=(4, 4, 4), pad=(1, 0, 0), dims=(3, 4, 4), c=2, mirror=1, scale=1.0, out=ptr):
        return lib.vsseg_swi_finalize_mirrored(out, ptr, L.i3(pdims), L.i3(pad), L.i3(dims), c, mirror, 0, 1, scale, ptr, None)

    for bad in (dict(mirror=8), dict(mirror=-1), dict(c=0), dict(out=None), dict(scale=0.0), dict(scale=float("nan")), dict(pad=(2, 0, 0)), dict(pad=(-1, 0, 0)), dict(dims=(3, 0, 4))):
        assert call(**bad) == L.EINVAL and b"vsseg_swi_finalize_mirrored" in lib.vsseg_last_error(), bad
