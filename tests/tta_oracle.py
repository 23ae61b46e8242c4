"""Test-time mirror augmentation of sliding-window inference (`sliding_window_inference(..., tta_flips=...)`) restated as the composition it is defined by:
result = (sum over the passes m of unflip_m(SWI(flip_m(inputs)))) * (1/M), an fp32 sum in pass order — with `torch.flip` around any plain sliding-window
function: the CPU oracle's (`oracle_tta`) or vs_seg_amd's own on GPU tensors (`composed_tta`).  Also the geometry cases and the predictor the TTA tests share."""
import functools

import torch

from oracle import vsseg_oracle as O

# volume, roi, overlap, mode — what each exercises:
CASES = [
    ((41, 36, 21), (16, 16, 32), 0.5, "gaussian"),  # x starts 0,8,16,24,25 and y starts 0,8,16,20 are not mirror-symmetric; z pad 11, pad_before 5
    ((20, 21, 45), (16, 32, 16), 0.5, "gaussian"),  # y pad 11; z starts 0,8,16,24,29
    ((20, 20, 20), (16, 16, 8), 0.25, "constant"),  # constant importance map
]
FLIPS = [(0,), (2,), (1, 2), (0, 1, 2)]
BATCH = 2


def pass_dims(tta_flips):
    """Per pass, in pass order, the dims of [B,C,X,Y,Z] it mirrors: bit i of the pass number selects tta_flips[i]; pass 0 is the identity."""
    return [[2 + a for i, a in enumerate(tta_flips) if m >> i & 1] for m in range(1 << len(tta_flips))]


def passes(swi, inputs, tta_flips):
    """unflip_m(swi(flip_m(inputs))) for every pass m."""
    return [torch.flip(swi(torch.flip(inputs, d)), d) for d in pass_dims(tta_flips)]


def compose(swi, inputs, tta_flips, average="logits"):
    rs = passes(swi, inputs, tta_flips)
    if average == "probabilities":
        rs = [torch.softmax(r, 1) for r in rs]
    acc = rs[0]
    for r in rs[1:]:
        acc = acc + r
    return acc * (1.0 / len(rs))


def oracle_tta(inputs, roi, sw_batch_size, predictor, overlap, mode, tta_flips, average="logits"):
    return compose(lambda x: O.sliding_window_inference(x, roi, sw_batch_size, predictor, overlap=overlap, mode=mode), inputs, tta_flips, average)


def composed_tta(inputs, roi, sw_batch_size, predictor, overlap, mode, tta_flips, average="logits", **kw):
    import vs_seg_amd as V

    return compose(lambda x: V.sliding_window_inference(x, roi, sw_batch_size, predictor, overlap=overlap, mode=mode, **kw), inputs, tta_flips, average)


def volume(case):
    vol = CASES[case][0]
    return torch.randn((BATCH, 1, *vol), generator=torch.Generator().manual_seed(70 + case))


def position_dependent_predictor(roi, device="cpu"):
    """Neither voxel-wise (it shifts along x and weights by the position in the window) nor mirror-equivariant: a pass that blended, padded or un-mirrored in the wrong
    frame gives another volume."""
    R = torch.randn((1, 1, *roi), generator=torch.Generator().manual_seed(9)).to(device)

    def pred(w):
        return torch.cat([w * R + torch.roll(w, 1, dims=2), torch.tanh(w) * R.flip(3) - 0.5], 1)

    return pred


@functools.lru_cache(maxsize=None)
def oracle_case(case, tta_flips):
    """The CPU oracle's result for CASES[case] (computed once; do not modify)."""
    _, roi, ov, mode = CASES[case]
    return oracle_tta(volume(case), roi, 1, position_dependent_predictor(roi), ov, mode, tta_flips)
