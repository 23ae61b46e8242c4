"""-m gpu: per-kernel parity of the HIP path (through the C ABI) against the CPU oracle / torch fp32-fp64 definitions.

Tolerances: fp32 path = exact-fp32 MFMA, differences are summation-order only (<= 1e-4 relative to the output scale,
well inside the 1e-3 bar of BASELINE.json's north_star).  bf16 path = bf16 operands, fp32 accumulate: inputs are
pre-rounded to bf16 on both sides so the only difference left is the output rounding, and the comparison holds the kernels to it: every
element of a bf16 output lies between the bf16 roundings of ref -+ 2e-5 max|ref| (tests/rounding.py; the 2e-5 is the fp32 path's bar, the
accumulators are fp32 in both).  Where a kernel rounds an intermediate tensor to bf16 by design, the reference is built from that stored
tensor (never from a rounding of its own), so no slack is left for a second rounding.
"""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import vsseg_oracle as O  # noqa: E402
from tests import gpu_harness as H  # noqa: E402
from tests.helpers import load, synth_input, synth_label  # noqa: E402
from tests.rounding import assert_one_rounding  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd import planner as P  # noqa: E402

CONVS = [
    # kernel, stride, cin, cout, dims
    ((3, 3, 1), (1, 1, 1), 16, 16, (16, 16, 8)),
    ((3, 3, 3), (1, 1, 1), 32, 48, (8, 8, 8)),
    ((1, 1, 1), (1, 1, 1), 32, 16, (8, 8, 8)),
    ((3, 3, 1), (2, 2, 1), 16, 16, (16, 16, 4)),
    ((3, 3, 3), (2, 2, 2), 48, 48, (8, 8, 8)),
    ((3, 3, 3), (1, 1, 1), 40, 1, (4, 4, 8)),
    ((3, 3, 1), (1, 1, 1), 32, 2, (8, 8, 4)),
    ((3, 3, 3), (1, 1, 1), 160, 80, (6, 2, 8)),
    ((3, 3, 3), (1, 1, 1), 96, 96, (3, 1, 4)),  # bottleneck-sized, ragged tiles
]


def _round(x, dt):
    return x.to(H.DT[dt]).to(torch.float32) if dt == "bf16" else x


def _tol(dt, ref):
    scale = float(ref.abs().max()) + 1e-12
    return (2e-5 if dt == "fp32" else 1.2e-2) * scale


def _check(dt, got, ref, what=""):
    """An output (float image, NCDHW) against its fp64 definition: fp32 within the accumulator bar of `_tol`, bf16 within ONE correct rounding of it."""
    if dt == "bf16":
        assert_one_rounding(got, ref, what=what)
    else:
        np.testing.assert_allclose(got.numpy(), ref.detach().float().numpy(), atol=_tol(dt, ref), err_msg=what)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k,s,cin,cout,dims", CONVS)
def test_conv_forward_and_dgrad(k, s, cin, cout, dims, dt):
    torch.manual_seed(1)
    pad = P.same_pad(k)
    x = _round(torch.randn(2, cin, *dims), dt).requires_grad_(True)
    w = _round(torch.randn(cout, cin, *k) / (cin * np.prod(k)) ** 0.5, dt)
    b = torch.randn(cout)
    y = F.conv3d(x.double(), w.double(), b.double(), stride=s, padding=pad)
    out = torch.zeros(2, *y.shape[2:], cout, dtype=H.DT[dt], device="cuda")
    bias = b.cuda()
    H.run_lattice_op("conv_fwd", w, H.to_cl(x, H.DT[dt], P.round_up(cin, 8)), out, s, bias=bias.data_ptr())
    _check(dt, H.from_cl(out), y.detach(), "conv_fwd")
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    dx = torch.zeros(2, *dims, cin, dtype=H.DT[dt], device="cuda")
    H.run_lattice_op("conv_dgrad", w, H.to_cl(gy, H.DT[dt], P.round_up(cout, 8)), dx, s)
    _check(dt, H.from_cl(dx), x.grad, "conv_dgrad")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k,s,cin,cout,dims", [((3, 3, 1), (2, 2, 1), 32, 16, (8, 8, 4)), ((3, 3, 3), (2, 2, 2), 96, 80, (3, 1, 4)), ((3, 3, 3), (2, 2, 2), 48, 32, (6, 4, 4))])
def test_conv_transpose_forward_and_dgrad(k, s, cin, cout, dims, dt):
    torch.manual_seed(2)
    pad = P.same_pad(k)
    opad = tuple(ss + 2 * p - (kk - 1) - 1 for ss, p, kk in zip(s, pad, k))
    x = _round(torch.randn(2, cin, *dims), dt).requires_grad_(True)
    w = _round(torch.randn(cin, cout, *k) / (cin * np.prod(k) / 4) ** 0.5, dt)
    y = F.conv_transpose3d(x.double(), w.double(), stride=s, padding=pad, output_padding=opad)
    out = torch.zeros(2, *y.shape[2:], cout, dtype=H.DT[dt], device="cuda")
    H.run_lattice_op("convT_fwd", w, H.to_cl(x, H.DT[dt]), out, s)
    _check(dt, H.from_cl(out), y.detach(), "convT_fwd")
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    dx = torch.zeros(2, *dims, cin, dtype=H.DT[dt], device="cuda")
    H.run_lattice_op("convT_dgrad", w, H.to_cl(gy, H.DT[dt]), dx, s)
    _check(dt, H.from_cl(dx), x.grad, "convT_dgrad")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_igemm_epilogue_and_channel_chunks(dt):
    """bias + folded BN + PReLU + residual add + statistics; a tight LDS budget forces several channel chunks."""
    torch.manual_seed(3)
    k, s, cin, cout, dims = (3, 3, 3), (1, 1, 1), 64, 32, (8, 8, 8)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = _round(torch.randn(cout, cin, *k) / (cin * 27) ** 0.5, dt)
    b, sc, sh, al = torch.randn(cout), torch.rand(cout) + 0.5, torch.randn(cout), torch.tensor([0.2])
    r = _round(torch.randn(2, cout, *dims), dt)
    pre = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    y = F.prelu(pre * sc.view(1, -1, 1, 1, 1).double() + sh.view(1, -1, 1, 1, 1).double(), al.double()) + r.double()
    out = torch.zeros(2, *dims, cout, dtype=H.DT[dt], device="cuda")
    dev = [t.cuda() for t in (b, sc, sh, al)]
    stats = torch.zeros(L.STAT_SHARDS * 2 * 32, dtype=torch.float64, device="cuda")
    rcl = H.to_cl(r, H.DT[dt])
    H.run_lattice_op("conv_fwd", w, H.to_cl(x, H.DT[dt]), out, s, bias=dev[0].data_ptr(), scale=dev[1].data_ptr(), shift=dev[2].data_ptr(), alpha=dev[3].data_ptr(), act=L.ACT_PRELU,
                     res_mode=L.RES_ADD, res=H.tdesc(rcl), stats=stats.data_ptr(), stats_stride=32, lds_budget=24 * 1024)
    _check(dt, H.from_cl(out), y, "PReLU + RES_ADD + statistics, several chunks")
    st = H.stat_decode(stats).cpu().view(L.STAT_SHARDS, 2, 32).sum(0)
    np.testing.assert_allclose(st[0].numpy(), pre.sum((0, 2, 3, 4)).numpy(), rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(st[1].numpy(), (pre * pre).sum((0, 2, 3, 4)).numpy(), rtol=1e-4)


EPILOGUE_MODES = ["plain", "bias", "eval_prelu", "relu", "sigmoid", "res_add", "relu_mask", "gate", "in1", "accumulate"]
EPILOGUE_SHAPES = [
    # kernel, cin, cout, dims, input split, LDS budget
    ((3, 3, 1), 16, 16, (16, 16, 8), 0, None),
    ((3, 3, 3), 96, 48, (8, 8, 8), 48, 40 * 1024),  # the concat read as a two-part 48 + 48 tensor; the tight budget makes the kernel sum several channel chunks
]
_epilogue_operands = {}


def _epilogue_case(k, cin, cout, dims):
    """Operands and the fp64 convolution of an EPILOGUE_SHAPES row: computed once, shared by the modes, never modified."""
    key = (k, cin, cout, dims)
    if key not in _epilogue_operands:
        g = torch.Generator().manual_seed(41)
        r = lambda *shape: torch.randn(*shape, generator=g)
        x, w = _round(r(2, cin, *dims), "bf16"), _round(r(cout, cin, *k) / (cin * np.prod(k)) ** 0.5, "bf16")
        vec = dict(b=r(cout), sc=torch.rand(cout, generator=g) + 0.5, sh=r(cout), w1=r(cout), b1=r(cout))
        side, x1 = _round(r(2, cout, *dims), "bf16"), _round(r(2, 1, *dims), "bf16")
        gate = torch.rand(2, *dims, generator=g)
        conv = F.conv3d(x.double(), w.double(), padding=P.same_pad(k))
        _epilogue_operands[key] = (x, w, vec, side, x1, gate, conv)
    return _epilogue_operands[key]


@pytest.mark.parametrize("mode", EPILOGUE_MODES)
@pytest.mark.parametrize("k,cin,cout,dims,split,budget", EPILOGUE_SHAPES)
def test_general_kernel_epilogue_modes_match_definition(k, cin, cout, dims, split, budget, mode):
    """Every epilogue mode of the GENERAL bf16 kernel (depth >= 0: the kernel the specialised ones are tested bit-identical to) against the fp64 definition of that
    mode, within one bf16 rounding: plain, bias, eval affine + PReLU, ReLU, sigmoid, residual add, ReLU mask, gated add, accumulate (definition = the stored bf16
    value + the convolution).  VSSEG_RES_IN1 exists in the marching kernel only: the general kernel must refuse it (an error, not another epilogue); it meets its
    definition in test_chained_marching_convolution_equals_the_two_launches."""
    x, w, vec, side, x1, gate, conv = _epilogue_case(k, cin, cout, dims)
    col = lambda v: v.double().view(1, -1, 1, 1, 1)
    dev = {n_: v.cuda() for n_, v in vec.items()}
    xcl = H.to_cl(x, torch.bfloat16)
    xin = H._split_cl(xcl, split) if split else xcl
    side_cl, gate_d, alpha = H.to_cl(side, torch.bfloat16), gate.cuda(), torch.tensor([0.2], device="cuda")
    out = torch.full((2, *dims, cout), float("nan"), dtype=torch.bfloat16, device="cuda")
    kw, ref = {}, conv
    if mode != "plain":
        kw["bias"], ref = dev["b"].data_ptr(), conv + col(vec["b"])
    if mode == "eval_prelu":
        kw.update(scale=dev["sc"].data_ptr(), shift=dev["sh"].data_ptr(), alpha=alpha.data_ptr(), act=L.ACT_PRELU)
        ref = ref * col(vec["sc"]) + col(vec["sh"])
        ref = torch.where(ref > 0, ref, 0.2 * ref)
    elif mode == "relu":
        kw["act"], ref = L.ACT_RELU, ref.clamp(min=0)
    elif mode == "sigmoid":
        kw["act"], ref = L.ACT_SIGMOID, torch.sigmoid(ref)
    elif mode == "res_add":
        kw.update(res=H.tdesc(side_cl), res_mode=L.RES_ADD)
        ref = ref + side.double()
    elif mode == "relu_mask":
        kw.update(res=H.tdesc(side_cl), res_mode=L.RES_RELUMASK)
        ref = ref * (side.double() > 0)
    elif mode == "gate":
        kw.update(res=H.tdesc(side_cl), res_mode=L.RES_GATE, gate=gate_d.data_ptr())
        ref = ref + side.double() * (1.0 + gate.double()).unsqueeze(1)
    elif mode == "accumulate":
        out = side_cl.clone()
        kw["accumulate"], ref = 1, ref + side.double()
    elif mode == "in1":
        x1_cl = H.to_cl(x1, torch.bfloat16)
        kw.update(res_mode=L.RES_IN1, in1=x1_cl.data_ptr(), in1_w=dev["w1"].data_ptr(), in1_b=dev["b1"].data_ptr())
    if budget:
        kw["lds_budget"] = budget
    if mode == "in1":
        with pytest.raises(L.VssegError, match="VSSEG_RES_IN1 needs a marching-kernel plan"):
            H.run_lattice_op("conv_fwd", w, xin, out, (1, 1, 1), **kw)
        return
    keep = H.run_lattice_op("conv_fwd", w, xin, out, (1, 1, 1), **kw)
    assert len(keep) == 1 and keep[0][1].depth >= 0 and (not budget or keep[0][1].nchunks > 1)
    assert_one_rounding(H.from_cl(out), ref, what=f"general kernel, {mode}")


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k,s,cin,cout,dims,tr", [((3, 3, 1), (1, 1, 1), 16, 16, (16, 16, 8), False), ((3, 3, 3), (1, 1, 1), 96, 48, (8, 8, 8), False), ((1, 1, 1), (1, 1, 1), 32, 16, (8, 8, 8), False),
                                                    ((3, 3, 3), (2, 2, 2), 48, 48, (8, 8, 8), False), ((3, 3, 1), (2, 2, 1), 16, 16, (16, 8, 4), False), ((3, 3, 3), (1, 1, 1), 40, 1, (4, 4, 8), False),
                                                    ((3, 3, 1), (1, 1, 1), 1, 16, (16, 16, 4), False), ((3, 3, 3), (2, 2, 2), 96, 80, (3, 1, 4), True), ((3, 3, 1), (2, 2, 1), 32, 16, (8, 8, 4), True)])
def test_wgrad(k, s, cin, cout, dims, tr, dt):
    torch.manual_seed(4)
    pad = P.same_pad(k)
    x = _round(torch.randn(2, cin, *dims), dt)
    if tr:
        w = torch.randn(cin, cout, *k, dtype=torch.float64, requires_grad=True)
        opad = tuple(ss + 2 * p - (kk - 1) - 1 for ss, p, kk in zip(s, pad, k))
        y = F.conv_transpose3d(x.double(), w, stride=s, padding=pad, output_padding=opad)
    else:
        w = torch.randn(cout, cin, *k, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x.double(), w, stride=s, padding=pad)
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    xcl, gcl = H.to_cl(x, H.DT[dt], P.round_up(cin, 8)), H.to_cl(gy, H.DT[dt], P.round_up(cout, 8))
    if tr:
        dw = H.run_wgrad(True, tuple(w.shape), k, s, xcl, gcl, cin, cout)
    else:
        dw = H.run_wgrad(False, tuple(w.shape), k, s, gcl, xcl, cout, cin)
    ref = w.grad.float()
    np.testing.assert_allclose(dw.numpy(), ref.numpy(), atol=(5e-5 if dt == "fp32" else 1e-4) * float(ref.abs().max()))


MARCH_WGRAD_CASES = [
    # cin (H), cout (P), dims, H split, march tile (x steps, rows, z slices)
    (16, 16, (10, 64, 8), 0, (4, 64, 4)),    # K-steps split over the waves; 3 x segments
    (16, 16, (6, 128, 8), 0, (6, 32, 4)),    # four 32-row blocks: each other's halo rows
    (16, 16, (5, 64, 16), 0, (5, 32, 8)),    # TZ 8
    (32, 16, (7, 64, 8), 16, (3, 64, 4)),    # level-0 concat as a two-part H
    (32, 16, (4, 64, 4), 0, (4, 64, 2)),     # TZ 2
    (32, 2, (5, 64, 8), 0, (5, 64, 4)),      # logits convolution: P = dY of 2 channels stored as one 8-channel group
    (16, 32, (6, 64, 8), 0, (2, 64, 4)),
    (32, 32, (9, 64, 8), 0, (4, 64, 4)),     # (tap, cH tile) units split over the waves
    (32, 32, (4, 64, 4), 0, (4, 64, 2)),
    (64, 32, (6, 64, 4), 32, (6, 64, 2)),    # level-1 concat
    (64, 32, (5, 32, 4), 0, (2, 32, 2)),
    (64, 32, (4, 32, 8), 0, (4, 32, 4)),
]


@pytest.mark.parametrize("cin,cout,dims,split,tile", MARCH_WGRAD_CASES)
def test_marching_weight_gradient(cin, cout, dims, split, tile):
    """march = 1 selects the marching weight-gradient kernel (csrc/mwgrad.hip: both operands fetched once, planes of H through an LDS ring).
    Against the fp64 autograd of F.conv3d on the same bf16 operands (the summation order differs from the tile kernel's, so the comparison is
    with the definition), together with the bias gradient it reduces on the side, across x segments, row blocks and image borders."""
    dt, k = "bf16", (3, 3, 1)
    torch.manual_seed(11)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = torch.randn(cout, cin, *k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, padding=P.same_pad(k))
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    xcl, gcl = H.to_cl(x, H.DT[dt], P.round_up(cin, 8)), H.to_cl(gy, H.DT[dt], P.round_up(cout, 8))
    h = H._split_cl(xcl, split) if split else xcl
    db = torch.zeros(16, dtype=torch.float32, device="cuda") if cout >= 16 else None
    if db is not None:
        db = torch.zeros(cout, dtype=torch.float32, device="cuda")
    dw = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl, h, cout, cin, march_tile=tile, dbias=db)
    ref = w.grad.float()
    np.testing.assert_allclose(dw.numpy(), ref.numpy(), atol=1e-4 * float(ref.abs().max()))
    gen = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl, h, cout, cin)  # the tile kernel on the same operands
    np.testing.assert_allclose(dw.numpy(), gen.numpy(), atol=1e-4 * float(ref.abs().max()))
    if db is not None:
        want = gy.double().sum((0, 2, 3, 4)).float()
        np.testing.assert_allclose(db.cpu().numpy(), want.numpy(), atol=1e-4 * float(want.abs().max()) + 1e-3)
    if cout == 2 and cin == 32:  # the logits convolution: P also read as the COMPACT two-channel tensor (4 bytes per voxel instead of the zero-extended 16): bit-identical
        dwc = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl[..., :2].contiguous(), h, cout, cin, march_tile=tile)
        assert torch.equal(dwc, dw)
        gate = torch.rand(2, *dims, device="cuda")
        a = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl, h, cout, cin, march_tile=tile, h_gate=gate)
        b = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl[..., :2].contiguous(), h, cout, cin, march_tile=tile, h_gate=gate)
        assert torch.equal(a, b) and not torch.equal(a, dw)


@pytest.mark.parametrize("c,dims,batch,lx,act,odt", [(16, (9, 128, 8), 2, 4, "sigmoid", "fp32"), (16, (5, 64, 16), 1, 0, "none", "fp32"), (32, (7, 64, 8), 2, 3, "sigmoid", "fp32"),
                                                      (32, (4, 32, 32), 1, 2, "sigmoid", "bf16"), (16, (3, 16, 64), 1, 1, "sigmoid", "fp32"), (32, (12, 256, 4), 1, 5, "none", "fp32")])
def test_narrow_output_convolution_matches_definition(c, dims, batch, lx, act, odt):
    """vsseg_conv_to1 (csrc/nconv.hip): the C -> 1 stride-1 3x3x1 convolution + bias (+ sigmoid) of the attention blocks on the vector ALUs, partial sums exchanged between
    neighbouring threads — against torch's fp64 convolution of the same bf16-rounded operands (weights rounded to bf16 as the kernel and the MFMA launches round them),
    over x segments, image borders in x and y, every supported row count; and against the MFMA launch it replaces (same products, another summation order)."""
    lib = L.lib()
    torch.manual_seed(33)
    x = _round(torch.randn(batch, c, *dims), "bf16")
    w = torch.randn(1, c, 3, 3, 1) * 0.2
    b = torch.randn(1)
    y = F.conv3d(x.double(), _round(w, "bf16").double(), b.double(), padding=(1, 1, 0))
    if act == "sigmoid":
        y = torch.sigmoid(y)
    xcl = H.to_cl(x, torch.bfloat16)
    out = torch.full((batch, *dims, 1), float("nan"), device="cuda", dtype=H.DT[odt])
    wd, bd = w.reshape(-1).cuda(), b.cuda()
    od = L.Tensor(out.data_ptr(), L.F32 if odt == "fp32" else L.BF16, 1, 1, batch, *dims)
    L.check(lib.vsseg_conv_to1(H.tdesc(xcl), wd.data_ptr(), bd.data_ptr(), L.ACT_SIGMOID if act == "sigmoid" else L.ACT_NONE, od, lx, H.stream()), "conv_to1")
    torch.cuda.synchronize()
    got = out.float().cpu().permute(0, 4, 1, 2, 3)
    assert not torch.isnan(got).any()
    if odt == "bf16":
        assert_one_rounding(got, y, what="conv_to1")
    else:
        np.testing.assert_allclose(got.numpy(), y.float().numpy(), atol=2e-5 * max(1.0, float(y.abs().max())))
    if odt == "fp32" and act == "none":  # the general kernel on the same operands
        o2 = torch.zeros(batch, *dims, 8, device="cuda", dtype=torch.float32)
        H.run_lattice_op("conv_fwd", w, xcl, o2, (1, 1, 1), bias=bd.data_ptr())
        np.testing.assert_allclose(got.numpy(), H.from_cl(o2, 1).numpy(), atol=2e-4 * float(y.abs().max()))


def test_narrow_output_convolution_rejects_what_it_does_not_cover():
    lib = L.lib()
    w = torch.zeros(1, 16, 3, 3, 1).reshape(-1).cuda()

    def attempt(c, dims, ocl=1):
        x = torch.zeros(1, *dims, c, device="cuda", dtype=torch.bfloat16)
        out = torch.zeros(1, *dims, ocl, device="cuda", dtype=torch.float32)
        od = L.Tensor(out.data_ptr(), L.F32, ocl, ocl, 1, *dims)
        with pytest.raises(RuntimeError, match="vsseg_conv_to1"):
            L.check(lib.vsseg_conv_to1(H.tdesc(x), w.data_ptr(), None, L.ACT_SIGMOID, od, 0, H.stream()), "conv_to1")

    attempt(48, (4, 32, 16))   # 48 channels
    attempt(16, (4, 24, 16))   # y extent not a power of two
    attempt(16, (4, 32, 8))    # z not a multiple of 512 / y = 16
    attempt(16, (4, 64, 8), 2)  # two output channels


COMPUTE_WGRAD_CASES = [
    # cin (H), cout (P), dims, batch, H split, H chunks per workgroup, bias gradient, workgroups per class (None: one per CU)
    (32, 48, (5, 8, 64), 2, 0, 2, False, None),    # level-2 encoder unit0: one chunk class, two K-step shares; runs of a single x step
    (32, 48, (4, 16, 32), 2, 0, 1, False, 8),      # two classes x four K-step shares; runs that cross strips
    (48, 48, (6, 8, 32), 2, 0, 1, False, None),    # three classes (odd: class = workgroup % 3)
    (96, 48, (4, 8, 64), 2, 48, 2, True, None),    # level-2 attention conv1: the concat as a two-part H, bias gradient on the side
    (96, 48, (7, 24, 32), 1, 0, 2, False, 2),      # two workgroups per class: long runs over several strips, ragged (XCD, class) groups
    (96, 48, (9, 8, 32), 1, 0, 1, False, 4),       # six classes
    (48, 64, (4, 8, 64), 2, 0, 1, False, None),    # level 3: 64 P channels, P tiles split over two waves
    (64, 64, (6, 16, 32), 2, 0, 1, True, 8),
    (128, 64, (3, 8, 64), 1, 64, 1, True, None),   # level-3 concat, eight classes
]


@pytest.mark.parametrize("cin,cout,dims,batch,split,cg,bias,blocks", COMPUTE_WGRAD_CASES)
def test_compute_weight_gradient(cin, cout, dims, batch, split, cg, bias, blocks):
    """march = 2 selects the compute weight-gradient kernel of the stride-1 3x3x3 layers (csrc/cwgrad.hip: the three z-taps of a voxel row share one H
    fragment, all 27 taps of a 16-channel chunk of H accumulate in one wave's registers).  Against the fp64 autograd of F.conv3d on the same bf16 operands
    and against the tile kernel, over volume borders in all three axes, several tiles per workgroup, every wave-role split, a two-part H and the bias
    gradient; run twice: the slab sums are in a fixed order, the result is bit-identical."""
    dt, k = "bf16", (3, 3, 3)
    torch.manual_seed(21)
    x = _round(torch.randn(batch, cin, *dims), dt)
    w = torch.randn(cout, cin, *k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, padding=P.same_pad(k))
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    xcl, gcl = H.to_cl(x, H.DT[dt]), H.to_cl(gy, H.DT[dt])
    h = H._split_cl(xcl, split) if split else xcl
    db = torch.zeros(cout, dtype=torch.float32, device="cuda") if bias else None
    dw = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl, h, cout, cin, compute=cg, dbias=db, blocks=blocks)
    ref = w.grad.float()
    np.testing.assert_allclose(dw.numpy(), ref.numpy(), atol=1e-4 * float(ref.abs().max()))
    gen = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl, h, cout, cin)  # the tile kernel on the same operands
    np.testing.assert_allclose(dw.numpy(), gen.numpy(), atol=1e-4 * float(ref.abs().max()))
    if bias:
        want = gy.double().sum((0, 2, 3, 4)).float()
        np.testing.assert_allclose(db.cpu().numpy(), want.numpy(), atol=1e-4 * float(want.abs().max()) + 1e-3)
    again = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gcl, h, cout, cin, compute=cg, blocks=blocks)
    assert torch.equal(again, dw)


def test_compute_weight_gradient_rejects_what_it_does_not_cover():
    """Outside its domain the compute weight-gradient kernel is an error, never another kernel."""
    lib = L.lib()
    k = (3, 3, 3)

    def attempt(cin, cout, dims, kernel=k, cg=1):
        p = torch.zeros(1, *dims, cout, device="cuda", dtype=torch.bfloat16)
        h = torch.zeros(1, *dims, cin, device="cuda", dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match="compute kernel"):
            H.run_wgrad(False, (cout, cin, *kernel), kernel, (1, 1, 1), p, h, cout, cin, compute=cg)

    attempt(32, 48, (4, 8, 48))            # z extent not a multiple of 32
    attempt(32, 48, (4, 12, 32))           # y extent not a multiple of 8
    attempt(32, 32, (4, 8, 32))            # 32 P channels
    attempt(40, 48, (4, 8, 32))            # H channels not a multiple of 16
    attempt(48, 48, (4, 8, 32), cg=2)      # 3 chunks, 2 per workgroup
    attempt(64, 64, (4, 8, 32), cg=2)      # 64 P channels with two chunks per workgroup
    attempt(32, 48, (4, 8, 32), kernel=(3, 3, 1))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k,cin,cout,dims", [((3, 3, 1), 1, 16, (12, 16, 8)), ((1, 1, 1), 1, 16, (6, 8, 4)), ((3, 3, 1), 16, 1, (12, 16, 8)), ((3, 3, 1), 32, 1, (5, 8, 12)), ((3, 3, 1), 1, 8, (3, 4, 2))])
def test_wgrad_narrow(k, cin, cout, dims, dt):
    """vsseg_wgrad_narrow: the weight gradient of a convolution with one input or one output channel as a bandwidth reduction, against
    torch's fp64 autograd (same bar as the MFMA weight-gradient kernel it replaces on those layers)."""
    lib = L.lib()
    torch.manual_seed(9)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = torch.randn(cout, cin, *k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, padding=P.same_pad(k))
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    dw = torch.zeros(cout, cin, *k, device="cuda")
    if cin == 1:  # t = dY (cout channels), s = x, sign +1: dw[c][0][tap]
        t_cl, s_cl, sign = H.to_cl(gy, H.DT[dt]), H.to_cl(x, H.DT[dt]), 1
    else:  # t = x (cin channels), s = dY, sign -1: dw[0][c][tap]
        t_cl, s_cl, sign = H.to_cl(x, H.DT[dt]), H.to_cl(gy, H.DT[dt]), -1
    scr = torch.zeros(1 << 20, device="cuda")
    db = torch.zeros(1, device="cuda") if sign == -1 else None  # C -> 1: the bias gradient sum(dY) rides in the same slabs
    for _ in range(2):  # accumulates into dw
        L.check(lib.vsseg_wgrad_narrow(H.tdesc(t_cl), s_cl.data_ptr(), k[0], sign, dw.data_ptr(), k[0] * k[1], db.data_ptr() if db is not None else None, scr.data_ptr(), scr.numel(), H.stream()))
    torch.cuda.synchronize()
    ref = 2 * w.grad.float()
    np.testing.assert_allclose(dw.cpu().numpy(), ref.numpy(), atol=(5e-5 if dt == "fp32" else 1e-4) * float(ref.abs().max()))
    if db is not None:
        want = 2 * float(gy.double().sum())
        assert abs(float(db) - want) <= 1e-4 * float(gy.abs().sum()) + 1e-4, (float(db), want)


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("cout,dims", [(16, (12, 16, 8)), (32, (5, 8, 12)), (8, (3, 4, 2))])
def test_wgrad_narrow_with_batchnorm_backward_on_load(cout, dims, p_drop):
    """vsseg_wgrad_narrow_bn: the first block's weight gradient (1 -> C, 3x3x1, the network input has no data gradient) with d(conv output) formed on load from
    (y, dA, keep-mask) instead of read from a tensor vsseg_bn_act_bwd_apply wrote: same values, same summation order -> bit-identical to the two launches."""
    lib = L.lib()
    torch.manual_seed(31)
    n, S = 2, H.stream()
    ycl = H.to_cl(_round(torch.randn(n, cout, *dims) * 1.2 + 0.3, "bf16"), torch.bfloat16)
    dcl = H.to_cl(_round(torch.randn(n, cout, *dims), "bf16"), torch.bfloat16)
    x1 = H.to_cl(_round(torch.randn(n, 1, *dims), "bf16"), torch.bfloat16)
    nvox = n * int(np.prod(dims))
    vec = torch.zeros(6, cout, device="cuda")
    vec[0], vec[1] = torch.randn(cout) * 0.2, torch.rand(cout) + 0.5
    gam, bet, al = (torch.rand(cout) + 0.5).cuda(), (torch.randn(cout) * 0.1).cuda(), torch.tensor([0.25], device="cuda")
    vec[2] = gam * vec[1]
    vec[3] = bet - vec[0] * vec[2]
    vec[4], vec[5] = torch.randn(cout) * 0.05, torch.randn(cout) * 0.05
    keep = None
    if p_drop > 0:
        keep = torch.zeros(nvox * cout // 8, dtype=torch.uint8, device="cuda")
        L.check(lib.vsseg_bn_act_fwd(H.tdesc(ycl), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, 0x1234, 3, L.Tensor(), 0, H.tdesc(torch.zeros_like(ycl)), keep.data_ptr(), S))
    kptr = keep.data_ptr() if keep is not None else None
    dy = torch.zeros_like(ycl)
    L.check(lib.vsseg_bn_act_bwd_apply(H.tdesc(ycl), H.tdesc(dcl), vec[0].data_ptr(), vec[1].data_ptr(), gam.data_ptr(), bet.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, 0x1234, 3,
                                       vec[4].data_ptr(), vec[5].data_ptr(), H.tdesc(dy), kptr, S))
    scr = torch.zeros(1 << 20, device="cuda")
    dw_ref, dw = torch.zeros(cout, 1, 3, 3, 1, device="cuda"), torch.zeros(cout, 1, 3, 3, 1, device="cuda")
    L.check(lib.vsseg_wgrad_narrow(H.tdesc(dy), x1.data_ptr(), 3, 1, dw_ref.data_ptr(), 9, None, scr.data_ptr(), scr.numel(), S))
    L.check(lib.vsseg_wgrad_narrow_bn(H.tdesc(ycl), H.tdesc(dcl), kptr, vec[0].data_ptr(), vec[1].data_ptr(), gam.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), vec[4].data_ptr(), vec[5].data_ptr(),
                                      p_drop, x1.data_ptr(), dw.data_ptr(), 9, scr.data_ptr(), scr.numel(), S))
    torch.cuda.synchronize()
    assert float(dw_ref.abs().max()) > 0 and torch.equal(dw, dw_ref), float((dw - dw_ref).abs().max())


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("hg,sb", [(1, 1), (2, 0), (2, 1), (4, 0), (4, 1), (3, 1)])
def test_wgrad_h_chunk_groups(hg, sb, dt):
    """One workgroup multiplies its P tile with `hgroup` 16-channel chunks of H (incl. a two-part H whose split lies inside a group,
    and a request that does not divide the chunk count: the library clamps it)."""
    torch.manual_seed(14)
    k, s, cin, cout, dims = (3, 3, 1), (1, 1, 1), 64, 32, (16, 12, 8)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = torch.randn(cout, cin, *k, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x.double(), w, padding=P.same_pad(k))
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    ref = w.grad.float()
    xcl, gcl = H.to_cl(x, H.DT[dt]), H.to_cl(gy, H.DT[dt])
    tol = (5e-5 if dt == "fp32" else 1e-4) * float(ref.abs().max())
    dw = H.run_wgrad(False, tuple(w.shape), k, s, gcl, xcl, cout, cin, hgroup=hg, single_buffer=sb)
    np.testing.assert_allclose(dw.numpy(), ref.numpy(), atol=tol)
    # two-part H (the skip-connection concat, both parts 32 channels wide): the split lies inside the 64-channel group of hgroup 4
    dw = H.run_wgrad(False, tuple(w.shape), k, s, gcl, H._split_cl(xcl, 32), cout, cin, hgroup=hg, single_buffer=sb)
    np.testing.assert_allclose(dw.numpy(), ref.numpy(), atol=tol)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", [(16, 16, 16), (12, 10, 8)])
def test_igemm_512_voxel_tiles(dims, dt):
    """MTW = 8 (512-voxel tiles, the MFMA-bound configurations): forward with statistics and a data gradient — whole and ragged tiles."""
    torch.manual_seed(15)
    k, s, cin, cout = (3, 3, 3), (1, 1, 1), 32, 48
    x = _round(torch.randn(2, cin, *dims), dt).requires_grad_(True)
    w = _round(torch.randn(cout, cin, *k) / (cin * 27) ** 0.5, dt)
    b = torch.randn(cout)
    y = F.conv3d(x.double(), w.double(), b.double(), padding=1)
    out = torch.zeros(2, *dims, cout, dtype=H.DT[dt], device="cuda")
    stats = torch.zeros(L.STAT_SHARDS * 2 * 48, dtype=torch.float64, device="cuda")
    bias = b.cuda()
    keep = H.run_lattice_op("conv_fwd", w, H.to_cl(x, H.DT[dt]), out, s, bias=bias.data_ptr(), stats=stats.data_ptr(), stats_stride=48, mtw=8)
    assert keep[0][1].mtw == 8 and keep[0][1].nt == 3
    _check(dt, H.from_cl(out), y.detach(), "mtw 8 forward")
    st = H.stat_decode(stats).cpu().view(L.STAT_SHARDS, 2, 48).sum(0)
    np.testing.assert_allclose(st[0].numpy(), y.detach().sum((0, 2, 3, 4)).numpy(), rtol=1e-4, atol=2e-2)
    # data gradient (48 output channels, NT 3) with the same tile, no auxiliary operand
    gy = _round(torch.randn(*y.shape), dt)
    w48 = _round(torch.randn(cout, 48, *k) / (48 * 27) ** 0.5, dt)
    x48 = torch.randn(2, 48, *dims, dtype=torch.float64, requires_grad=True)
    F.conv3d(x48, w48.double(), padding=1).backward(gy.double())
    dx48 = torch.zeros(2, *dims, 48, dtype=H.DT[dt], device="cuda")
    keep = H.run_lattice_op("conv_dgrad", w48, H.to_cl(gy, H.DT[dt]), dx48, s, mtw=8)
    assert keep[0][1].mtw == 8
    if dt == "bf16":
        assert_one_rounding(H.from_cl(dx48), x48.grad, what="mtw 8 data gradient")
    else:
        np.testing.assert_allclose(H.from_cl(dx48).numpy(), x48.grad.float().numpy(), atol=_tol(dt, x48.grad) * 1.5)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("p_drop,stored,centre", [(0.0, False, (0.3, 1.5)), (0.1, False, (0.3, 1.5)), (0.1, True, (0.3, 1.5)), (0.1, True, (10.0, 0.05))])
def test_bn_dropout_prelu_forward_backward(dt, p_drop, stored, centre):
    """Training-mode BN -> Dropout -> PReLU (+residual): statistics, running stats, forward and all gradients vs the oracle
    fed with the HIP path's own keep-mask (torch's dropout stream cannot be reproduced).  stored: the forward keeps the
    mask bytes and the backward passes read them (what the engine does) instead of regenerating them from (seed, salt, index).
    centre = (mean, std) of the pre-normalisation values: the (10, 0.05) case has |mean| = 200 std, where sum(dz*y) - mean*sum(dz) formed from
    fp32 sums would cancel (the reduce pass centres every element instead)."""
    lib = L.lib()
    torch.manual_seed(5)
    c, dims, n = 48, (8, 8, 4), 2
    if dt == "bf16" and centre[0] > 1:
        pytest.skip("bf16 storage cannot hold values of 10 +- 0.05 (the test is about fp32 accumulation)")
    y = _round(torch.randn(n, c, *dims) * centre[1] + centre[0], dt)
    r = _round(torch.randn(n, c, *dims), dt)
    gout = _round(torch.randn(n, c, *dims), dt)
    sd = {"b.conv.weight": torch.zeros(c, c, 1, 1, 1), "b.conv.bias": torch.zeros(c), "b.norm.weight": torch.rand(c) + 0.5, "b.norm.bias": torch.randn(c) * 0.1,
          "b.norm.running_mean": torch.randn(c) * 0.1, "b.norm.running_var": torch.rand(c) + 0.5, "b.norm.num_batches_tracked": torch.zeros((), dtype=torch.long), "b.act.weight": torch.tensor([0.2])}
    ycl, rcl, gcl = H.to_cl(y, H.DT[dt]), H.to_cl(r, H.DT[dt]), H.to_cl(gout, H.DT[dt])
    nvox = n * int(np.prod(dims))
    # statistics through the same sharded fp64 buffer the conv epilogue fills
    stats = torch.zeros(L.STAT_SHARDS, 2, c, dtype=torch.float64, device="cuda")
    yf = H.from_cl(ycl).double()
    stats[0, 0] = H.stat_encode(yf.sum((0, 2, 3, 4))).cuda()  # (fixed-point, as vsseg_fx_add leaves them)
    stats[0, 1] = H.stat_encode((yf * yf).sum((0, 2, 3, 4))).cuda()
    g, be, al = sd["b.norm.weight"].cuda(), sd["b.norm.bias"].cuda(), sd["b.act.weight"].cuda()
    rm, rv, nb = sd["b.norm.running_mean"].cuda(), sd["b.norm.running_var"].cuda(), torch.zeros(1, dtype=torch.int64, device="cuda")
    vec = torch.zeros(6, c, device="cuda")
    S = H.stream()
    L.check(lib.vsseg_bn_finalize(stats.data_ptr(), c, c, float(nvox), g.data_ptr(), be.data_ptr(), 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(), nb.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), S))
    out = torch.zeros_like(ycl)
    seed, salt = 0x1234ABCD5678, 7
    keep = torch.zeros(nvox * c // 8, dtype=torch.uint8, device="cuda") if stored else None
    kptr = keep.data_ptr() if stored else None
    L.check(lib.vsseg_bn_act_fwd(H.tdesc(ycl), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, seed, salt, H.tdesc(rcl), 1, H.tdesc(out), kptr, S))
    mask = torch.ones(n, *dims, c, device="cuda")
    L.check(lib.vsseg_dropout_mask(mask.data_ptr(), nvox, c, p_drop, seed, salt, S))
    torch.cuda.synchronize()
    if p_drop > 0:
        assert 0.85 < float(mask.mean()) < 0.95
    if stored:  # bit j of byte i = keep decision of element 8*i + j
        bits = ((keep.view(-1, 1).int() >> torch.arange(8, device="cuda").view(1, 8)) & 1).float().view(-1)
        assert torch.equal(bits, mask.view(-1))
        seed ^= 0x5A5A5A5A  # the backward passes must now use the stored bytes: a different seed would regenerate a different mask
    # oracle: BN->dropout(mask)->PReLU on the same y, plus residual
    yy = H.from_cl(ycl).double().requires_grad_(True)
    sd64 = {k2: (v.double() if v.is_floating_point() else v) for k2, v in sd.items()}
    for k2 in ("b.norm.weight", "b.norm.bias", "b.act.weight"):
        sd64[k2].requires_grad_(True)
    ctx = O.Ctx(True, p_drop, masks={"b": mask.cpu().permute(0, 4, 1, 2, 3).double()})
    mean, var = yy.mean((0, 2, 3, 4)), yy.var((0, 2, 3, 4), unbiased=False)
    sh = (1, -1, 1, 1, 1)
    z = (yy - mean.view(sh)) / torch.sqrt(var.view(sh) + 1e-5) * sd64["b.norm.weight"].view(sh) + sd64["b.norm.bias"].view(sh)
    if p_drop > 0:
        z = z * ctx.masks["b"] / (1 - p_drop)
    ref = F.prelu(z, sd64["b.act.weight"]) + H.from_cl(rcl).double()
    _check(dt, H.from_cl(out), ref.detach(), "bn_act_fwd")
    np.testing.assert_allclose(rm.cpu().numpy(), (0.9 * sd["b.norm.running_mean"] + 0.1 * mean.detach().float()).numpy(), atol=1e-5)
    np.testing.assert_allclose(rv.cpu().numpy(), (0.9 * sd["b.norm.running_var"] + 0.1 * (var.detach() * nvox / (nvox - 1)).float()).numpy(), atol=1e-5)
    assert int(nb) == 1
    # backward
    ref.backward(H.from_cl(gcl).double())
    sums = torch.zeros(L.STAT_SHARDS, 3, c, dtype=torch.float64, device="cuda")
    aacc = torch.zeros(L.STAT_SHARDS, dtype=torch.float64, device="cuda")
    L.check(lib.vsseg_bn_act_bwd_reduce(H.tdesc(ycl), H.tdesc(gcl), vec[0].data_ptr(), vec[1].data_ptr(), g.data_ptr(), be.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, seed, salt, sums.data_ptr(), c, aacc.data_ptr(), kptr, S))
    dg, db, da, drb = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(c, device="cuda")
    L.check(lib.vsseg_bn_act_bwd_finalize(sums.data_ptr(), c, aacc.data_ptr(), c, float(nvox), dg.data_ptr(), db.data_ptr(), da.data_ptr(), vec[4].data_ptr(), vec[5].data_ptr(), drb.data_ptr(), S))
    dy = torch.zeros_like(ycl)
    L.check(lib.vsseg_bn_act_bwd_apply(H.tdesc(ycl), H.tdesc(gcl), vec[0].data_ptr(), vec[1].data_ptr(), g.data_ptr(), be.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, seed, salt, vec[4].data_ptr(), vec[5].data_ptr(), H.tdesc(dy), kptr, S))
    torch.cuda.synchronize()
    _check(dt, H.from_cl(dy), yy.grad, "bn_act_bwd_apply")
    np.testing.assert_allclose(dg.cpu().numpy(), sd64["b.norm.weight"].grad.float().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(db.cpu().numpy(), sd64["b.norm.bias"].grad.float().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(da.cpu().numpy(), sd64["b.act.weight"].grad.float().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(drb.cpu().numpy(), H.from_cl(gcl).double().sum((0, 2, 3, 4)).float().numpy(), rtol=1e-4, atol=1e-3)  # bias gradient of a residual conv


@pytest.mark.parametrize("bad", ["nan", "large"])
def test_fixed_point_sums_flag_non_finite_and_out_of_range_partials(bad):
    """The order-independent accumulators are 64-bit fixed point (include/vsseg_hip.h): a NaN gradient, or one whose per-workgroup sum leaves the
    documented range (|v| < 256 for the BatchNorm backward sums), must not come back as a finite wrapped integer.  The partial is clamped, the
    sticky flag is set, and the kernels that decode the sums return NaN — as floating-point atomics would have — until the flag is cleared."""
    import vs_seg_amd as V

    lib = L.lib()
    torch.manual_seed(9)
    c, dims, n = 16, (8, 8, 4), 2
    nvox = n * int(np.prod(dims))
    ycl = H.to_cl(torch.randn(n, c, *dims), torch.float32)
    gout = torch.randn(n, c, *dims)
    if bad == "nan":
        gout[0, 3, 1, 2, 3] = float("nan")
    else:
        gout *= 1.0e6  # sum(dout) of a workgroup ~ 1e6 * sqrt(voxels) >> 256
    gcl = H.to_cl(gout, torch.float32)
    g, be, al = torch.rand(c, device="cuda") + 0.5, torch.zeros(c, device="cuda"), torch.tensor([0.2], device="cuda")
    vec = torch.zeros(6, c, device="cuda")
    vec[1] = 1.0  # invstd
    vec[2] = g    # scale (mean 0, invstd 1)
    S = H.stream()
    assert V.fx_status(reset=True) in (False, True)  # start from a cleared flag whatever ran before
    assert V.fx_status() is False

    def backward_sums():
        sums = torch.zeros(L.STAT_SHARDS, 3, c, dtype=torch.float64, device="cuda")
        aacc = torch.zeros(L.STAT_SHARDS, dtype=torch.float64, device="cuda")
        L.check(lib.vsseg_bn_act_bwd_reduce(H.tdesc(ycl), H.tdesc(gcl), vec[0].data_ptr(), vec[1].data_ptr(), g.data_ptr(), be.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), 0.0, 0, 1, sums.data_ptr(), c, aacc.data_ptr(), None, S))
        dg, db, da = torch.zeros(c, device="cuda"), torch.zeros(c, device="cuda"), torch.zeros(1, device="cuda")
        L.check(lib.vsseg_bn_act_bwd_finalize(sums.data_ptr(), c, aacc.data_ptr(), c, float(nvox), dg.data_ptr(), db.data_ptr(), da.data_ptr(), vec[4].data_ptr(), vec[5].data_ptr(), None, S))
        torch.cuda.synchronize()
        return dg, db, da

    dg, db, da = backward_sums()
    assert V.fx_status() is True
    assert torch.isnan(dg).all() and torch.isnan(db).all() and torch.isnan(da).all() and torch.isnan(vec[4]).all()
    # sticky: the forward statistics and the loss of the same process are poisoned too, until the host clears the flag
    stats = torch.zeros(L.STAT_SHARDS, 2, c, dtype=torch.float64, device="cuda")
    rm, rv, nb = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    L.check(lib.vsseg_bn_finalize(stats.data_ptr(), c, c, float(nvox), g.data_ptr(), be.data_ptr(), 1e-5, 0.1, rm.data_ptr(), rv.data_ptr(), nb.data_ptr(), vec[0].data_ptr(), vec[1].data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), S))
    torch.cuda.synchronize()
    assert torch.isnan(vec[0]).all() and torch.isnan(rm).all()
    assert V.fx_status(reset=True) is True and V.fx_status() is False
    # after the reset, well-scaled gradients give finite sums again
    gcl.copy_(H.to_cl(torch.randn(n, c, *dims), torch.float32))
    vec[1] = 1.0
    vec[2] = g
    vec[0] = 0.0
    vec[3] = 0.0
    dg, db, da = backward_sums()
    assert V.fx_status() is False and torch.isfinite(dg).all() and torch.isfinite(db).all() and torch.isfinite(da).all()


def test_dice_loss_of_nan_logits_is_nan():
    """A diverged network (NaN logits) must show as a NaN loss, as in the reference (ref:params/VSparams.py:463 reads loss.item() every step): the Dice
    sums are fixed-point integers, a NaN partial sum sets the flag and vsseg_dice_finalize returns NaN."""
    import vs_seg_amd as V

    V.fx_status(reset=True)
    y = synth_label(31, (2, 1, 32, 32, 8)).cuda()
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda()
    logits[1, 0, 5, 6, 7] = float("nan")
    loss = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, hardness_weighting=True)((logits.requires_grad_(True), []), y)
    assert torch.isnan(loss).item()
    assert V.fx_status(reset=True) is True
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda().requires_grad_(True)
    loss = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=False, hardness_weighting=True)((logits, []), y)
    assert torch.isfinite(loss).item() and V.fx_status() is False


@pytest.mark.parametrize("c", [32, 96, 160])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_attention_gate_forward_backward(dt, c):
    lib = L.lib()
    torch.manual_seed(6)
    dims, n = (8, 8, 4), 2
    x = _round(torch.randn(n, c, *dims), dt).double().requires_grad_(True)
    pre = torch.randn(n, 1, *dims, dtype=torch.float64, requires_grad=True)
    att = torch.sigmoid(pre)
    out = att * x + x
    gout = _round(torch.randn(n, c, *dims), dt)
    gatt_ext = torch.randn(n, 1, *dims)
    (out * gout.double()).sum().add((att * gatt_ext.double()).sum()).backward()
    xcl, gcl = H.to_cl(x, H.DT[dt]), H.to_cl(gout, H.DT[dt])
    attd = att.detach().float().reshape(n, *dims).contiguous().cuda()
    o = torch.zeros_like(xcl)
    S = H.stream()
    L.check(lib.vsseg_att_apply_fwd(H.tdesc(xcl), attd.data_ptr(), H.tdesc(o), S))
    dx = torch.zeros_like(xcl)
    dpre = torch.zeros(n, *dims, 8, dtype=H.DT[dt], device="cuda")
    ge = gatt_ext.reshape(n, *dims).contiguous().cuda()
    dbias = torch.zeros(1, device="cuda")
    dpre1 = torch.zeros(n, *dims, dtype=H.DT[dt], device="cuda")
    L.check(lib.vsseg_att_apply_bwd(H.tdesc(xcl), attd.data_ptr(), H.tdesc(gcl), ge.data_ptr(), H.tdesc(dx), 0, H.tdesc(dpre), dbias.data_ptr(), dpre1.data_ptr(), S))
    torch.cuda.synchronize()
    _check(dt, H.from_cl(o), out.detach(), "att_apply_fwd")
    _check(dt, H.from_cl(dx), x.grad, "att_apply_bwd dx")
    _check(dt, H.from_cl(dpre, 1), pre.grad, "att_apply_bwd dpre")
    assert float(dpre[..., 1:].float().abs().max()) == 0.0
    assert torch.equal(dpre1, dpre[..., 0])  # the compact copy feeds the z-folded data gradient of the sigmoid convolution
    assert abs(float(dbias) - float(pre.grad.sum())) < 2e-2 * float(pre.grad.abs().sum()) ** 0.5 + 1e-3


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,k,cin,cout,dims,split", [("conv_fwd", (3, 3, 1), 32, 16, (32, 32, 8), 0), ("conv_fwd", (3, 3, 3), 96, 48, (8, 16, 16), 48), ("conv_dgrad", (3, 3, 1), 32, 64, (16, 32, 8), 0),
                                                          ("conv_fwd", (3, 3, 3), 48, 96, (8, 8, 16), 0)])
def test_every_candidate_plan_gives_the_same_convolution(kind, k, cin, cout, dims, split, dt):
    """The autotuner may pick any of `planner.candidate_plans` (channel chunk, voxel tile, output-channel split, prefetch
    depth incl. the single-buffer mode): each of them must compute the same convolution, with bias + BN statistics +
    accumulation exercising every epilogue MODE of the kernel."""
    lib = L.lib()
    torch.manual_seed(21)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = _round(torch.randn(cout, cin, *k) / (cin * np.prod(k)) ** 0.5, dt)
    b = torch.randn(cout)
    xd = x.double().requires_grad_(True)
    y = F.conv3d(xd, w.double(), b.double(), padding=P.same_pad(k))
    if kind == "conv_fwd":
        inp_cl, want, nout, bias = H.to_cl(x, H.DT[dt]), y.detach(), cout, b.cuda()
    else:
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        inp_cl, want, nout, bias = H.to_cl(gy, H.DT[dt]), xd.grad, cin, None
    cls = P.lattice_classes(kind, k, (1, 1, 1))[0]
    cands = P.candidate_plans(kind, tuple(w.shape), cls, dims, inp_cl.element_size(), kc_pad=inp_cl.shape[-1], aux_es=inp_cl.element_size(), in_split=split)
    assert len(cands) >= 2 and (dt == "fp32" or (len(cands) >= 4 and (any(c.depth == L.DEPTH_NOPREFETCH for c in cands) or all(c.nt >= 3 for c in cands if c.depth >= L.DEPTH_NOPREFETCH)) and len({(c.ck, c.mtw, c.nsplit) for c in cands}) >= 3))  # nt >= 3: producer / consumer kernels always prefetch
    parts = H._split_cl(inp_cl, split) if split else None
    for mode in ("plain", "stats", "accumulate"):
        for pl in cands:
            out = torch.zeros(2, *dims, nout, dtype=H.DT[dt], device="cuda")
            ref = want
            kw = {}
            stats = None
            if mode == "stats":
                stats = torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")
                kw = dict(stats=stats.data_ptr(), stats_stride=P.round_up(nout, 16))
            elif mode == "accumulate":
                old = _round(torch.randn(2, nout, *dims), dt)
                out = H.to_cl(old, H.DT[dt])
                ref = want + old.double()
                kw = dict(accumulate=1)
            if bias is not None:
                kw["bias"] = bias.data_ptr()
            wp = H.pack(pl, w, inp_cl.dtype)
            d = H.igemm_desc(pl, wp, H.two_part(*parts) if parts else H.tdesc(inp_cl), H.tdesc(out), **kw)
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"igemm {pl.tile} ck={pl.ck} ns={pl.nsplit} D={pl.depth}")
            torch.cuda.synchronize()
            tag = f"{mode} tile={pl.tile} mtw={pl.mtw} ck={pl.ck} ns={pl.nsplit} D={pl.depth}"
            _check(dt, H.from_cl(out), ref.detach(), tag)
            if stats is not None:
                st = H.stat_decode(stats).cpu().view(L.STAT_SHARDS, 2, -1).sum(0)[:, :nout]
                np.testing.assert_allclose(st[0].numpy(), want.sum((0, 2, 3, 4)).numpy(), rtol=2e-4, atol=2e-2, err_msg=tag)


STREAM_CASES = [
    # kind, kernel, cin, cout, dims, input split
    ("conv_fwd", (3, 3, 1), 16, 16, (16, 24, 8), 0),
    ("conv_fwd", (3, 3, 1), 32, 16, (16, 16, 8), 16),  # skip-connection concat read as a two-part tensor
    ("conv_fwd", (3, 3, 1), 32, 2, (16, 16, 4), 0),    # logits: 2 fp32 channels, scalar stores
    ("conv_fwd", (3, 3, 1), 1, 16, (16, 16, 8), 0),    # network input, zero-extended to 8 channels
    ("conv_fwd", (3, 3, 1), 32, 32, (24, 16, 8), 0),
    ("conv_dgrad", (3, 3, 1), 32, 16, (16, 16, 8), 0),  # K = 16, N = 32
    ("conv_dgrad", (3, 3, 1), 64, 32, (16, 16, 8), 0),  # K = 32, N = 64: four 16-channel tiles per workgroup
    ("conv_dgrad", (1, 1, 1), 64, 32, (16, 8, 8), 0),
    ("conv_fwd", (1, 1, 1), 32, 16, (8, 16, 4), 0),
    ("conv_fwd", (3, 3, 1), 64, 32, (12, 16, 8), 32),  # level-1 concat: 64 input channels, 4x8x4 tile
    ("conv_fwd", (1, 1, 1), 64, 32, (16, 8, 8), 32),
    ("conv_fwd", (1, 1, 1), 96, 48, (8, 16, 8), 48),   # level-2 decoder unit's residual convolution on the concat (12 channel groups, 3 output tiles)
    ("conv_dgrad", (1, 1, 1), 96, 48, (16, 8, 4), 0),  # ... its data gradient: K = 48, N = 96 (6 output tiles)
    ("conv_fwd", (1, 1, 1), 32, 48, (8, 8, 8), 0),     # level-2 encoder unit's residual convolution
    ("conv_dgrad", (1, 1, 1), 32, 48, (8, 16, 4), 0),  # K = 48, N = 32
]


@pytest.mark.parametrize("kind,k,cin,cout,dims,split", STREAM_CASES)
def test_streaming_kernel_equals_general_kernel(kind, k, cin, cout, dims, split):
    """depth -2 selects the compile-time-geometry streaming kernel (csrc/sconv.hip).  Same packed weights, K order and fp32
    accumulation as the general kernel: outputs must be IDENTICAL bit for bit in every epilogue mode (and match the fp64
    definition within the bf16 output rounding); BatchNorm statistics agree up to the order of the fp32 partial sums."""
    lib = L.lib()
    dt = "bf16"
    torch.manual_seed(5)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = _round(torch.randn(cout, cin, *k) / (cin * np.prod(k)) ** 0.5, dt)
    b = torch.randn(cout)
    xd = x.double().requires_grad_(True)
    y = F.conv3d(xd, w.double(), b.double(), padding=P.same_pad(k))
    if kind == "conv_fwd":
        inp_cl, want, nout, bias = H.to_cl(x, H.DT[dt], cpad=P.round_up(cin, 8)), y.detach(), cout, b.cuda()
    else:
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        inp_cl, want, nout, bias = H.to_cl(gy, H.DT[dt], cpad=P.round_up(cout, 8)), xd.grad, cin, None
    cls = P.lattice_classes(kind, k, (1, 1, 1))[0]
    kc = inp_cl.shape[-1]
    gen = P.plan_igemm(kind, tuple(w.shape), cls, dims, 2, kc_pad=kc, in_split=split, aux_es=2)
    gen.pack_map = P.pack_map(gen, tuple(w.shape))
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    sp = P.stream_plan(kind, tuple(w.shape), cls, dims, 2, kc, nreal, kreal)
    assert sp is not None and sp.depth == L.DEPTH_STREAM
    sp.pack_map = P.pack_map(sp, tuple(w.shape))
    parts = H._split_cl(inp_cl, split) if split else None
    odt = torch.float32 if nout == 2 else H.DT[dt]
    res_t = H.to_cl(_round(torch.randn(2, nout, *dims), dt), H.DT[dt])
    gate_t = torch.rand(2, *dims, device="cuda")
    alpha = torch.tensor([0.25], device="cuda")
    modes = ["plain", "stats", "prelu"] + (["accumulate", "res_add", "relu_mask", "gate"] if nout % 4 == 0 else [])
    for mode in modes:
        outs = []
        for pl in (gen, sp):
            out = torch.zeros(2, *dims, nout, dtype=odt, device="cuda")
            kw, stats = {}, None
            if mode == "stats":
                stats = torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")
                kw = dict(stats=stats.data_ptr(), stats_stride=P.round_up(nout, 16))
            elif mode == "prelu":
                kw = dict(act=L.ACT_PRELU, alpha=alpha.data_ptr())
            elif mode == "accumulate":
                out = res_t.clone()
                kw = dict(accumulate=1)
            elif mode in ("res_add", "relu_mask", "gate"):
                kw = dict(res=H.tdesc(res_t), res_mode={"res_add": L.RES_ADD, "relu_mask": L.RES_RELUMASK, "gate": L.RES_GATE}[mode])
                if mode == "gate":
                    kw["gate"] = gate_t.data_ptr()
            if bias is not None:
                kw["bias"] = bias.data_ptr()
            wp = H.pack(pl, w, inp_cl.dtype)
            d = H.igemm_desc(pl, wp, H.two_part(*parts) if parts else H.tdesc(inp_cl), H.tdesc(out), **kw)
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"igemm D={pl.depth} {mode}")
            torch.cuda.synchronize()
            outs.append((out, stats))
        (og, sg), (os_, ss) = outs
        assert torch.equal(og, os_), f"{mode}: streaming kernel differs from the general kernel (max {float((og.float() - os_.float()).abs().max())})"
        if mode == "plain":
            _check("fp32" if odt == torch.float32 else dt, H.from_cl(os_), want, "streaming kernel")
        if mode == "stats":
            a, bb = H.stat_decode(sg).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(ss).view(L.STAT_SHARDS, 2, -1).sum(0)
            np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(bb[0, :nout].cpu().numpy(), want.sum((0, 2, 3, 4)).numpy(), rtol=2e-4, atol=2e-2)


MARCH_CASES = [
    # kind, cin, cout, dims, input split, (tz, mtw), x steps per workgroup
    ("conv_fwd", 16, 16, (10, 128, 8), 0, (4, 8), 4),     # full-Y column (no halo rows at all), 3 x segments (4 + 4 + 2 steps)
    ("conv_fwd", 16, 16, (6, 128, 8), 0, (4, 4), 6),      # two 64-row blocks: rows 63 / 64 are each other's halo
    ("conv_dgrad", 32, 16, (5, 64, 8), 0, (4, 4), 5),     # K = 16, N = 32 (two channel tiles), one segment
    ("conv_fwd", 32, 16, (7, 128, 4), 16, (2, 4), 3),     # level-0 concat read as a two-part tensor, TZ 2
    ("conv_fwd", 32, 2, (4, 128, 4), 0, (2, 4), 4),       # 2-channel fp32 output (logits)
    ("conv_fwd", 16, 32, (6, 64, 16), 0, (8, 8), 6),      # TZ 8: two rows per M-tile
    ("conv_fwd", 32, 32, (9, 64, 8), 0, (4, 4), 4),
    ("conv_dgrad", 64, 32, (6, 64, 8), 0, (4, 2), 6),     # K = 32, N = 64 (four channel tiles), 32-row blocks
    ("conv_fwd", 64, 32, (6, 32, 4), 32, (2, 1), 6),      # level-1 concat, 64 input channels
    ("conv_fwd", 64, 32, (5, 64, 4), 32, (2, 2), 2),
    ("conv_fwd", 1, 16, (6, 64, 8), 0, (8, 8), 3),        # the network input, zero-extended to one 8-channel group
    ("conv_dgrad", 32, 2, (5, 128, 4), 0, (4, 8), 5),     # data gradient of the logits convolution: K = 2 (-> 8), N = 32
    ("conv_dgrad", 32, 2, (6, 64, 16), 0, (4, 4), 3),     # ... several z blocks and x segments; also from the COMPACT two-channel gradient
    ("conv_dgrad", 32, 2, (6, 64, 16), 0, (8, 4), 4),
    ("conv_dgrad", 32, 2, (5, 64, 16), 0, (8, 8), 2),
    ("conv_dgrad", 16, 1, (6, 64, 8), 0, (8, 4), 3),      # data gradient of an attention sigmoid convolution: K = 1 (-> 8), N = 16; also from the COMPACT one-channel gradient
]


@pytest.mark.parametrize("kind,cin,cout,dims,split,shape,lx", MARCH_CASES)
def test_marching_kernel_equals_general_kernel(kind, cin, cout, dims, split, shape, lx):
    """depth -5 selects the marching streaming kernel (csrc/mconv.hip: a workgroup walks along x with a ring of planes in LDS, every input
    voxel fetched once).  Same packed weights, K order and fp32 accumulation as the general kernel: outputs must be IDENTICAL bit for bit in
    every epilogue mode, across x segments, row blocks and the image borders."""
    lib = L.lib()
    dt, k = "bf16", (3, 3, 1)
    torch.manual_seed(9)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, dt)
    b = torch.randn(cout)
    xd = x.double().requires_grad_(True)
    y = F.conv3d(xd, w.double(), b.double(), padding=P.same_pad(k))
    if kind == "conv_fwd":
        inp_cl, want, nout, bias = H.to_cl(x, H.DT[dt], cpad=P.round_up(cin, 8)), y.detach(), cout, b.cuda()
    else:
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        inp_cl, want, nout, bias = H.to_cl(gy, H.DT[dt], cpad=P.round_up(cout, 8)), xd.grad, cin, None
    cls = P.lattice_classes(kind, k, (1, 1, 1))[0]
    kc = inp_cl.shape[-1]
    gen = P.plan_igemm(kind, tuple(w.shape), cls, dims, 2, kc_pad=kc, in_split=split, aux_es=2)
    gen.pack_map = P.pack_map(gen, tuple(w.shape))
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    tz, mtw = shape
    mp = [pl for pl in P.march_plans(kind, tuple(w.shape), cls, dims, 2, kc, nreal, kreal, n=2) if (pl.tile[2], pl.mtw) == (tz, mtw)]
    assert mp, "no marching plan for this shape"
    mps = []
    for depth in P.MARCH_DEPTHS:  # -5: packed weights in LDS, -6: in registers (where instantiated)
        m_ = [pl for pl in mp if pl.depth == depth]
        if m_:
            m_ = dataclasses.replace(m_[0], tile=(lx, m_[0].tile[1], tz))
            m_.pack_map = P.pack_map(m_, tuple(w.shape))
            mps.append(m_)
    assert mps and mps[0].depth == L.DEPTH_MARCH
    parts = H._split_cl(inp_cl, split) if split else None
    odt = torch.float32 if nout == 2 else H.DT[dt]
    res_t = H.to_cl(_round(torch.randn(2, nout, *dims), dt), H.DT[dt])
    gate_t = torch.rand(2, *dims, device="cuda")
    alpha = torch.tensor([0.25], device="cuda")
    modes = ["plain", "stats", "prelu"] + (["accumulate", "res_add", "relu_mask", "gate"] if nout % 4 == 0 else [])
    for mode in modes:
        outs = []
        for pl in (gen, *mps):
            out = torch.zeros(2, *dims, nout, dtype=odt, device="cuda")
            kw, stats = {}, None
            if mode == "stats":
                stats = torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")
                kw = dict(stats=stats.data_ptr(), stats_stride=P.round_up(nout, 16))
            elif mode == "prelu":
                kw = dict(act=L.ACT_PRELU, alpha=alpha.data_ptr())
            elif mode == "accumulate":
                out = res_t.clone()
                kw = dict(accumulate=1)
            elif mode in ("res_add", "relu_mask", "gate"):
                kw = dict(res=H.tdesc(res_t), res_mode={"res_add": L.RES_ADD, "relu_mask": L.RES_RELUMASK, "gate": L.RES_GATE}[mode])
                if mode == "gate":
                    kw["gate"] = gate_t.data_ptr()
            if bias is not None:
                kw["bias"] = bias.data_ptr()
            wp = H.pack(pl, w, inp_cl.dtype)
            d = H.igemm_desc(pl, wp, H.two_part(*parts) if parts else H.tdesc(inp_cl), H.tdesc(out), **kw)
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"igemm D={pl.depth} {mode}")
            torch.cuda.synchronize()
            outs.append((out, stats))
        og, sg = outs[0]
        for pl, (om, sm) in zip(mps, outs[1:]):
            assert torch.equal(og, om), f"{mode}: marching kernel (depth {pl.depth}) differs from the general kernel (max {float((og.float() - om.float()).abs().max())})"
            if mode == "plain":
                _check("fp32" if odt == torch.float32 else dt, H.from_cl(om), want, f"marching kernel depth {pl.depth}")
            if mode == "stats":
                a, bb = H.stat_decode(sg).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(sm).view(L.STAT_SHARDS, 2, -1).sum(0)
                np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-3)
        if (kreal == 1 and mode in ("plain", "stats", "relu_mask", "accumulate")) or (kreal == 2 and mode == "plain"):
            # one / two real input channels: the marching kernel also reads the COMPACT tensor (2 / 4 bytes per voxel instead of the zero-extended 16): bit-identical
            compact = inp_cl[..., :kreal].contiguous()
            out = res_t.clone() if mode == "accumulate" else torch.full((2, *dims, nout), float("nan"), dtype=odt, device="cuda")
            kw, stats = {}, None
            if mode == "stats":
                stats = torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")
                kw = dict(stats=stats.data_ptr(), stats_stride=P.round_up(nout, 16))
            elif mode == "accumulate":
                kw = dict(accumulate=1)
            elif mode == "relu_mask":
                kw = dict(res=H.tdesc(res_t), res_mode=L.RES_RELUMASK)
            if bias is not None:
                kw["bias"] = bias.data_ptr()
            wp = H.pack(mps[0], w, inp_cl.dtype)
            d = H.igemm_desc(mps[0], wp, H.tdesc(compact), H.tdesc(out), **kw)
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"igemm compact input {mode}")
            torch.cuda.synchronize()
            assert torch.equal(out, og), f"{mode}: compact input differs (max {float((out.float() - og.float()).abs().max())})"
            if mode == "stats":
                np.testing.assert_allclose(H.stat_decode(stats).view(L.STAT_SHARDS, 2, -1).sum(0).cpu().numpy(), H.stat_decode(sg).view(L.STAT_SHARDS, 2, -1).sum(0).cpu().numpy(), rtol=1e-5, atol=1e-3)


GATHER_CASES = [
    # kind, cin, cout (of the layer), COARSE dims, (tz, mtw), x steps per workgroup
    ("conv_fwd", 16, 16, (6, 32, 8), (4, 2), 4),        # strided convolution level 0 -> 1: one row block, two z blocks, two x segments (4 + 2)
    ("conv_fwd", 16, 16, (5, 64, 8), (8, 4), 5),        # two row blocks: fine rows 63 / 64 are each other's halo
    ("conv_fwd", 16, 16, (4, 64, 4), (4, 4), 2),        # 64-row columns
    ("conv_fwd", 32, 32, (7, 32, 4), (2, 1), 3),        # level 1 -> 2: TZ 2, eight rows per M-tile
    ("conv_fwd", 32, 32, (5, 32, 8), (4, 2), 5),
    ("conv_fwd", 32, 32, (4, 64, 8), (4, 2), 4),        # two row blocks
    ("convT_dgrad", 32, 16, (6, 32, 8), (4, 2), 3),     # data gradient of the transposed convolution 32 -> 16: K = 16 (dy at the fine level), N = 32
    ("convT_dgrad", 32, 16, (4, 64, 8), (4, 4), 4),
    ("convT_dgrad", 48, 32, (7, 32, 4), (2, 1), 4),     # ... of 48 -> 32: K = 32, N = 48 (three channel tiles)
    ("convT_dgrad", 48, 32, (5, 32, 8), (4, 2), 2),
]


@pytest.mark.parametrize("kind,cin,cout,dims,shape,lx", GATHER_CASES)
def test_gathering_marching_kernel_equals_general_kernel(kind, cin, cout, dims, shape, lx):
    """depth -9 selects the gathering marching kernel (csrc/gconv.hip: the stride-(2,2,1) 3x3x1 launches that read the fine level and write the coarse one — a workgroup walks
    along x with a ring of FINE planes, stored as odd-row / even-row half planes).  Same packed weights, K order and fp32 accumulation as the general kernel with the whole
    input in one chunk: outputs must be IDENTICAL bit for bit in every epilogue it has (plain, statistics, eval affine + PReLU, accumulate), across x segments, row blocks and
    the image borders (16 input channels; with 32 the general kernel sums two 16-channel chunks one after the other, another fp32 summation order: there both kernels meet
    torch's fp64 definition within one bf16 rounding in EVERY mode instead); and equal torch's fp64 result."""
    lib = L.lib()
    dt, k, st = "bf16", (3, 3, 1), (2, 2, 1)
    torch.manual_seed(11)
    fine = (2 * dims[0], 2 * dims[1], dims[2])
    n = 2
    if kind == "conv_fwd":
        x = _round(torch.randn(n, cin, *fine), dt)
        w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, dt)
        want = F.conv3d(x.double(), w.double(), stride=st, padding=P.same_pad(k))
        inp_cl, nout = H.to_cl(x, H.DT[dt]), cout
    else:  # y = convT(x): x coarse [cin], y fine [cout]; the data gradient gathers dy (fine, cout channels) into dx (coarse, cin channels)
        w = _round(torch.randn(cin, cout, *k) / (cin * 9 / 4) ** 0.5, dt)
        xd = torch.zeros(n, cin, *dims, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose3d(xd, w.double(), stride=st, padding=P.same_pad(k), output_padding=(1, 1, 0))
        assert tuple(y.shape[2:]) == fine
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        want, inp_cl, nout = xd.grad, H.to_cl(gy, H.DT[dt]), cin
    assert tuple(want.shape[2:]) == dims
    cls = P.lattice_classes(kind, k, st)
    assert len(cls) == 1
    cls = cls[0]
    kc = inp_cl.shape[-1]
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    gen = P.plan_igemm(kind, tuple(w.shape), cls, dims, 2, kc_pad=kc, aux_es=2)
    gen.pack_map = P.pack_map(gen, tuple(w.shape))
    same_order = gen.nchunks == 1  # (32 input channels: the general kernel's plans stage two 16-channel chunks, its sum over K runs chunk by chunk — equal to fp32 rounding, not bit for bit)
    tz, mtw = shape
    gp = [pl for pl in P.gather_plans(kind, tuple(w.shape), cls, dims, 2, kc, nreal, kreal, n=n) if (pl.tile[2], pl.mtw) == (tz, mtw)]
    assert gp, "no gathering plan for this shape"
    gpl = dataclasses.replace(gp[0], tile=(lx, gp[0].tile[1], tz))
    gpl.pack_map = P.pack_map(gpl, tuple(w.shape))
    bias = torch.randn(nout, device="cuda")
    res_t = H.to_cl(_round(torch.randn(n, nout, *dims), dt), H.DT[dt])
    sc, sh, alpha = torch.rand(nout, device="cuda") + 0.5, torch.randn(nout, device="cuda"), torch.tensor([0.25], device="cuda")
    pre = want + bias.cpu().double().view(1, -1, 1, 1, 1)
    ev = pre * sc.cpu().double().view(1, -1, 1, 1, 1) + sh.cpu().double().view(1, -1, 1, 1, 1)
    defs = {"plain": pre, "stats": pre, "eval": torch.where(ev > 0, ev, 0.25 * ev), "accumulate": pre + H.from_cl(res_t).double()}
    for mode in ("plain", "stats", "eval", "accumulate"):
        outs = []
        for pl in (gen, gpl):
            out = res_t.clone() if mode == "accumulate" else torch.full((n, *dims, nout), float("nan"), dtype=H.DT[dt], device="cuda")
            kw, stats = dict(bias=bias.data_ptr()), None
            if mode == "stats":
                stats = torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")
                kw.update(stats=stats.data_ptr(), stats_stride=P.round_up(nout, 16))
            elif mode == "eval":
                kw.update(scale=sc.data_ptr(), shift=sh.data_ptr(), act=L.ACT_PRELU, alpha=alpha.data_ptr())
            elif mode == "accumulate":
                kw.update(accumulate=1)
            d = H.igemm_desc(pl, H.pack(pl, w, inp_cl.dtype), H.tdesc(inp_cl), H.tdesc(out), **kw)
            if pl.depth == L.DEPTH_GATHER:
                assert lib.vsseg_igemm_lds_bytes(C.byref(d)) == pl.lds
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"igemm D={pl.depth} {mode}")
            torch.cuda.synchronize()
            outs.append((out, stats))
        (og, sg), (om, sm) = outs
        assert not torch.isnan(om.float()).any()
        if same_order:
            assert torch.equal(og, om), f"{mode}: gathering kernel differs from the general kernel (max {float((og.float() - om.float()).abs().max())})"
        else:  # another K order: the two are compared through the definition, in every mode
            assert_one_rounding(H.from_cl(og), defs[mode], what=f"general kernel, {mode}")
        if mode == "plain" or not same_order:
            assert_one_rounding(H.from_cl(om), defs[mode], what=f"gathering kernel, {mode}")
        if mode == "stats":
            a, bb = H.stat_decode(sg).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(sm).view(L.STAT_SHARDS, 2, -1).sum(0)
            np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-3)


def test_gathering_marching_kernel_rejects_what_it_does_not_cover():
    lib = L.lib()
    k, st = (3, 3, 1), (2, 2, 1)
    w = torch.randn(32, 32, *k)
    cls = P.lattice_classes("conv_fwd", k, st)[0]
    assert P.gather_plans("conv_fwd", (64, 64, *k), cls, (8, 32, 8), 2, 64, 64, 64) == []                                       # 64 channels
    assert P.gather_plans("conv_fwd", tuple(w.shape), P.lattice_classes("conv_fwd", k, (1, 1, 1))[0], (8, 32, 8), 2, 32, 32, 32) == []   # stride 1: the marching kernel's
    assert P.gather_plans("conv_fwd", tuple(w.shape), cls, (8, 24, 8), 2, 32, 32, 32) == []                                    # rows not a multiple of the column block
    pl = P.gather_plans("conv_fwd", tuple(w.shape), cls, (8, 32, 8), 2, 32, 32, 32)[0]
    pl.pack_map = P.pack_map(pl, tuple(w.shape))
    x = torch.zeros(1, 16, 64, 8, 32, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, 8, 32, 8, 32, dtype=torch.bfloat16, device="cuda")
    wp = H.pack(pl, w, torch.bfloat16)

    def rejected(mutate, what):
        d = H.igemm_desc(pl, wp, H.tdesc(x), H.tdesc(out))
        mutate(d)
        assert lib.vsseg_igemm(C.byref(d), H.stream()) == L.EINVAL and b"gathering marching kernel" in lib.vsseg_last_error(), what

    rejected(lambda d: setattr(d, "mtw", 3), "mtw")
    rejected(lambda d: setattr(d, "res_mode", L.RES_ADD), "residual epilogue")
    rejected(lambda d: setattr(d, "act", L.ACT_SIGMOID), "sigmoid")
    o32 = torch.zeros(1, 8, 32, 8, 32, dtype=torch.float32, device="cuda")
    d = H.igemm_desc(pl, wp, H.tdesc(x), H.tdesc(o32))
    assert lib.vsseg_igemm(C.byref(d), H.stream()) == L.EINVAL and b"bf16" in lib.vsseg_last_error()


FUSED_BWD_CASES = [
    # cin, cout, dims, (x steps, rows, tz) of the fused launch
    (16, 16, (10, 64, 16), (4, 32, 8)),   # level-0 unit: two row blocks, two z blocks, three x segments (4 + 4 + 2)
    (16, 16, (5, 128, 4), (5, 64, 4)),
    (16, 16, (6, 32, 8), (3, 32, 4)),
    (16, 32, (7, 64, 8), (4, 64, 4)),     # level-1 unit0: 32-channel dy ring, 16-channel x
    (16, 32, (4, 32, 16), (4, 32, 8)),
    (32, 32, (6, 64, 8), (3, 32, 4)),     # waves split the (tap, tile) units of the weight gradient
    (32, 32, (5, 64, 4), (5, 64, 2)),
    (64, 32, (4, 32, 4), (4, 32, 2)),     # level-1 decoder unit: 64-channel x
]


@pytest.mark.parametrize("p_drop", [0.0, 0.1])
@pytest.mark.parametrize("cin,cout,dims,tile", FUSED_BWD_CASES)
def test_fused_conv_backward_equals_separate_launches(cin, cout, dims, tile, p_drop):
    """vsseg_conv_bwd_fused (csrc/mbwd.hip): BatchNorm/dropout/PReLU backward applied on load + data gradient + weight gradient of a stride-1 3x3x1
    Convolution block in one marching launch, against the three launches it replaces on the same operands — vsseg_bn_act_bwd_apply writing dy, the
    data-gradient launch and the weight-gradient launch reading it.  The data gradient must be IDENTICAL bit for bit (same dy values, same packed
    weights, K order and MFMA order); the weight gradient sums the same products in another order (operand roles swapped) and must agree to fp32
    rounding; both are also checked against the fp64 definition."""
    lib = L.lib()
    k, n = (3, 3, 1), 2
    torch.manual_seed(21)
    S = H.stream()
    y = _round(torch.randn(n, cout, *dims) * 1.3 + 0.2, "bf16")
    da = _round(torch.randn(n, cout, *dims), "bf16")
    x = _round(torch.randn(n, cin, *dims), "bf16")
    w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, "bf16")
    ycl, dcl, xcl = H.to_cl(y, torch.bfloat16), H.to_cl(da, torch.bfloat16), H.to_cl(x, torch.bfloat16)
    nvox = n * int(np.prod(dims))
    vec = torch.zeros(6, cout, device="cuda")
    vec[0] = torch.randn(cout) * 0.2 + 0.2      # mean
    vec[1] = torch.rand(cout) + 0.5             # invstd
    gam, bet, al = (torch.rand(cout) + 0.5).cuda(), (torch.randn(cout) * 0.1).cuda(), torch.tensor([0.25], device="cuda")
    vec[2] = gam * vec[1]                       # scale, shift of the folded forward affine
    vec[3] = bet - vec[0] * vec[2]
    vec[4] = torch.randn(cout) * 0.05           # mean(dz), mean(dz * xhat)
    vec[5] = torch.randn(cout) * 0.05
    keep = None
    if p_drop > 0:  # the forward's stored keep-mask bytes
        keep = torch.zeros(nvox * cout // 8, dtype=torch.uint8, device="cuda")
        scratch_out = torch.zeros_like(ycl)
        L.check(lib.vsseg_bn_act_fwd(H.tdesc(ycl), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, 0x77AA, 5, L.Tensor(), 0, H.tdesc(scratch_out), keep.data_ptr(), S))
    kptr = keep.data_ptr() if keep is not None else None
    # ---- the three separate launches
    dy = torch.zeros_like(ycl)
    L.check(lib.vsseg_bn_act_bwd_apply(H.tdesc(ycl), H.tdesc(dcl), vec[0].data_ptr(), vec[1].data_ptr(), gam.data_ptr(), bet.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, 0x77AA, 5,
                                       vec[4].data_ptr(), vec[5].data_ptr(), H.tdesc(dy), kptr, S))
    cls = P.lattice_classes("conv_dgrad", k, (1, 1, 1))[0]
    gen = P.plan_igemm("conv_dgrad", tuple(w.shape), cls, dims, 2, kc_pad=cout, aux_es=0)
    gen.pack_map = P.pack_map(gen, tuple(w.shape))
    dx_ref = torch.zeros(n, *dims, cin, dtype=torch.bfloat16, device="cuda")
    wp_gen = H.pack(gen, w, torch.bfloat16)
    d = H.igemm_desc(gen, wp_gen, H.tdesc(dy), H.tdesc(dx_ref))
    L.check(lib.vsseg_igemm(C.byref(d), S), "igemm dgrad")
    dw_ref = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), dy, xcl, cout, cin)
    # ---- the fused launch
    mps = P.march_plans("conv_dgrad", tuple(w.shape), cls, dims, 2, cout, cin, cout, n=n)
    assert mps, "no marching data-gradient plan (packed-weight layout) for this shape"
    mp = mps[0]
    mp.pack_map = P.pack_map(mp, tuple(w.shape))
    wp = H.pack(mp, w, torch.bfloat16)
    dx = torch.full((n, *dims, cin), float("nan"), dtype=torch.bfloat16, device="cuda")
    dw = torch.zeros(cout * cin * 9, dtype=torch.float32, device="cuda")
    scr = torch.zeros(16 * 1024 * 1024, dtype=torch.float32, device="cuda")
    fd = L.ConvBwdDesc()
    fd.y, fd.dout, fd.x, fd.dx = H.tdesc(ycl), H.tdesc(dcl), H.tdesc(xcl), H.tdesc(dx)
    fd.mean, fd.invstd, fd.gamma, fd.scale, fd.shift, fd.alpha = vec[0].data_ptr(), vec[1].data_ptr(), gam.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr()
    fd.mean_dz, fd.mean_dzx, fd.p_drop, fd.keep = vec[4].data_ptr(), vec[5].data_ptr(), p_drop, kptr
    fd.wpack, fd.dw, fd.tile = wp.data_ptr(), dw.data_ptr(), L.i3(tile)
    fd.scratch, fd.scratch_elems = scr.data_ptr(), scr.numel()
    L.check(lib.vsseg_conv_bwd_fused(C.byref(fd), S), "conv_bwd_fused")
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_ref), f"data gradient differs from the separate launches: max {float((dx.float() - dx_ref.float()).abs().max())}"
    dwf = dw.cpu().reshape(w.shape)
    np.testing.assert_allclose(dwf.numpy(), dw_ref.numpy(), rtol=2e-4, atol=2e-4 * float(dw_ref.abs().max()))
    # ---- fp64 definition on the bf16 dy the separate pass produced
    xd = x.double().requires_grad_(True)
    wd = w.double().requires_grad_(True)
    F.conv3d(xd, wd, None, padding=P.same_pad(k)).backward(H.from_cl(dy).double())
    assert_one_rounding(H.from_cl(dx), xd.grad, what="fused backward dx")
    np.testing.assert_allclose(dwf.numpy(), wd.grad.float().numpy(), rtol=1e-3, atol=1e-3 * float(wd.grad.abs().max()))
    # the second call accumulates into dw (+=), and a shape outside the table is refused loudly
    L.check(lib.vsseg_conv_bwd_fused(C.byref(fd), S), "conv_bwd_fused")
    torch.cuda.synchronize()
    np.testing.assert_allclose(dw.cpu().reshape(w.shape).numpy(), 2 * dwf.numpy(), rtol=1e-5, atol=1e-6)
    fd.tile = L.i3((tile[0], tile[1], 3))
    assert lib.vsseg_conv_bwd_fused(C.byref(fd), S) == L.EINVAL and b"not applicable" in lib.vsseg_last_error()


@pytest.mark.parametrize("same", [True, False])
@pytest.mark.parametrize("cin,cout,dims,tile", [(16, 32, (7, 64, 8), (4, 64, 4)), (16, 32, (9, 32, 16), (4, 32, 4)), (64, 32, (6, 32, 8), (3, 32, 4)), (64, 32, (5, 64, 4), (5, 64, 2)), (64, 32, (4, 32, 4), (4, 32, 2))])
def test_fused_conv_backward_with_residual_convolution(cin, cout, dims, tile, same):
    """vsseg_conv_bwd_fused with the ResidualUnit's 1x1x1 residual convolution riding along (ref:params/networks/blocks/convolutions.py:241-255): dx = conv3x3'(dy) + conv1x1'(dres)
    in one store, dw_res = sum dres x.  `same`: dres is the tensor dout itself (single-subunit decoder units) or another tensor (encoder units).  Against the
    fp64 definition on the bf16 dy the separate pass stored (the separate launches round dx to bf16 between the two terms, the fused one does not: ONE rounding of the
    sum) and against the separate weight-gradient launches."""
    lib = L.lib()
    k, n, p_drop = (3, 3, 1), 2, 0.1
    torch.manual_seed(23)
    S = H.stream()
    y = _round(torch.randn(n, cout, *dims) * 1.3 + 0.2, "bf16")
    da = _round(torch.randn(n, cout, *dims), "bf16")
    dr = da if same else _round(torch.randn(n, cout, *dims), "bf16")
    x = _round(torch.randn(n, cin, *dims), "bf16")
    w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, "bf16")
    wr = _round(torch.randn(cout, cin, 1, 1, 1) / cin ** 0.5, "bf16")
    ycl, dcl, xcl = H.to_cl(y, torch.bfloat16), H.to_cl(da, torch.bfloat16), H.to_cl(x, torch.bfloat16)
    rcl = dcl if same else H.to_cl(dr, torch.bfloat16)
    nvox = n * int(np.prod(dims))
    vec = torch.zeros(6, cout, device="cuda")
    vec[0], vec[1] = torch.randn(cout) * 0.2 + 0.2, torch.rand(cout) + 0.5
    gam, bet, al = (torch.rand(cout) + 0.5).cuda(), (torch.randn(cout) * 0.1).cuda(), torch.tensor([0.25], device="cuda")
    vec[2] = gam * vec[1]
    vec[3] = bet - vec[0] * vec[2]
    vec[4], vec[5] = torch.randn(cout) * 0.05, torch.randn(cout) * 0.05
    keep = torch.zeros(nvox * cout // 8, dtype=torch.uint8, device="cuda")
    L.check(lib.vsseg_bn_act_fwd(H.tdesc(ycl), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, 0x77AA, 5, L.Tensor(), 0, H.tdesc(torch.zeros_like(ycl)), keep.data_ptr(), S))
    dy = torch.zeros_like(ycl)
    L.check(lib.vsseg_bn_act_bwd_apply(H.tdesc(ycl), H.tdesc(dcl), vec[0].data_ptr(), vec[1].data_ptr(), gam.data_ptr(), bet.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr(), p_drop, 0x77AA, 5,
                                       vec[4].data_ptr(), vec[5].data_ptr(), H.tdesc(dy), keep.data_ptr(), S))
    dw_ref = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), dy, xcl, cout, cin)
    dwr_ref = H.run_wgrad(False, tuple(wr.shape), (1, 1, 1), (1, 1, 1), rcl, xcl, cout, cin)
    cls = P.lattice_classes("conv_dgrad", k, (1, 1, 1))[0]
    mp = P.march_plans("conv_dgrad", tuple(w.shape), cls, dims, 2, cout, cin, cout, n=n)[0]
    mp.pack_map = P.pack_map(mp, tuple(w.shape))
    rp = P.residual_dgrad_pack_plan(tuple(wr.shape), dims)
    wp, wpr = H.pack(mp, w, torch.bfloat16), H.pack(rp, wr, torch.bfloat16)
    dx = torch.full((n, *dims, cin), float("nan"), dtype=torch.bfloat16, device="cuda")
    dw = torch.zeros(cout * cin * 9, dtype=torch.float32, device="cuda")
    dwr = torch.zeros(cout * cin, dtype=torch.float32, device="cuda")
    scr = torch.zeros(16 * 1024 * 1024, dtype=torch.float32, device="cuda")
    fd = L.ConvBwdDesc()
    fd.y, fd.dout, fd.x, fd.dx, fd.dres = H.tdesc(ycl), H.tdesc(dcl), H.tdesc(xcl), H.tdesc(dx), H.tdesc(rcl)
    fd.mean, fd.invstd, fd.gamma, fd.scale, fd.shift, fd.alpha = vec[0].data_ptr(), vec[1].data_ptr(), gam.data_ptr(), vec[2].data_ptr(), vec[3].data_ptr(), al.data_ptr()
    fd.mean_dz, fd.mean_dzx, fd.p_drop, fd.keep = vec[4].data_ptr(), vec[5].data_ptr(), p_drop, keep.data_ptr()
    fd.wpack, fd.dw, fd.tile, fd.wpack_res, fd.dw_res = wp.data_ptr(), dw.data_ptr(), L.i3(tile), wpr.data_ptr(), dwr.data_ptr()
    fd.scratch, fd.scratch_elems = scr.data_ptr(), scr.numel()
    L.check(lib.vsseg_conv_bwd_fused(C.byref(fd), S), "conv_bwd_fused")
    torch.cuda.synchronize()
    xd = x.double().requires_grad_(True)
    wd, wrd = w.double().requires_grad_(True), wr.double().requires_grad_(True)
    F.conv3d(xd, wd, None, padding=P.same_pad(k)).backward(H.from_cl(dy).double(), retain_graph=False)
    g3 = xd.grad.clone()
    xd.grad = None
    F.conv3d(xd, wrd, None).backward(H.from_cl(rcl).double())
    want = g3 + xd.grad
    assert_one_rounding(H.from_cl(dx), want, what="fused backward dx + residual convolution")
    np.testing.assert_allclose(dw.cpu().reshape(w.shape).numpy(), dw_ref.numpy(), rtol=2e-4, atol=2e-4 * float(dw_ref.abs().max()))
    np.testing.assert_allclose(dwr.cpu().reshape(wr.shape).numpy(), dwr_ref.numpy(), rtol=2e-4, atol=2e-4 * float(dwr_ref.abs().max()))
    np.testing.assert_allclose(dwr.cpu().reshape(wr.shape).numpy(), wrd.grad.float().numpy(), rtol=1e-3, atol=1e-3 * float(wrd.grad.abs().max()))
    if cin == 64 and same:  # x gated on load from the two-part concat (AttentionBlock2 in front of the unit): bit-identical to the launch on the materialised gated tensor
        att = torch.rand(n, *dims, device="cuda")
        gated = torch.empty_like(xcl)
        L.check(lib.vsseg_att_apply_fwd(H.tdesc(xcl), att.data_ptr(), H.tdesc(gated), S), "att_apply_fwd")
        parts = H._split_cl(xcl, 32)
        outs = []
        for xin, gate in ((H.tdesc(gated), None), (H.two_part(*parts), att.data_ptr())):
            dxg = torch.full((n, *dims, cin), float("nan"), dtype=torch.bfloat16, device="cuda")
            dwg, dwrg = torch.zeros_like(dw), torch.zeros_like(dwr)
            fd.x, fd.dx, fd.dw, fd.dw_res, fd.x_gate = xin, H.tdesc(dxg), dwg.data_ptr(), dwrg.data_ptr(), gate
            L.check(lib.vsseg_conv_bwd_fused(C.byref(fd), S), "conv_bwd_fused (gated x)")
            torch.cuda.synchronize()
            outs.append((dxg, dwg, dwrg))
        assert all(torch.equal(a_, b_) for a_, b_ in zip(outs[0], outs[1])) and float(outs[1][1].abs().max()) > 0
        assert not torch.equal(outs[1][1], dw)  # (the gate does change the weight gradient)


@pytest.mark.parametrize("cin,cout,dims,shape,lx", [(16, 32, (6, 64, 16), (8, 4), 4), (16, 32, (5, 128, 8), (4, 4), 5), (16, 32, (7, 32, 8), (4, 2), 3), (64, 32, (5, 64, 4), (2, 2), 2), (64, 32, (6, 32, 6), (2, 1), 6)])
def test_marching_kernel_with_residual_tiles(cin, cout, dims, shape, lx):
    """vsseg_igemm_desc.res_tiles (csrc/mconv.hip NR): the ResidualUnit's 1x1x1 residual convolution of the same input as extra output tiles of the unit's first
    3x3x1 convolution — centre-tap K-steps only, input read once.  Stored to its own tensor (training: + statistics of the main tiles) it must be BIT-IDENTICAL to
    the two separate launches; added in the epilogue (eval: out = prelu(bn(conv(x))) + residual(x)) it skips the bf16 rounding of the residual tensor."""
    lib = L.lib()
    k, n = (3, 3, 1), 2
    torch.manual_seed(17)
    x = _round(torch.randn(n, cin, *dims), "bf16")
    w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, "bf16")
    wr = _round(torch.randn(cout, cin, 1, 1, 1) / cin ** 0.5, "bf16")
    b, br = torch.randn(cout).cuda(), torch.randn(cout).cuda()
    xcl = H.to_cl(x, torch.bfloat16)
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]
    tz, mtw = shape
    for depth in P.MARCH_DEPTHS:
        mp = [pl for pl in P.march_res_plans(tuple(w.shape), tuple(wr.shape), cls, dims, 2, cin, n=n) if (pl.tile[2], pl.mtw, pl.depth) == (tz, mtw, depth)]
        if not mp and depth == L.DEPTH_MARCH_WREG:  # (weights-in-registers twins exist for some shapes only)
            continue
        assert mp, (depth, [(p_.tile, p_.mtw, p_.depth) for p_ in P.march_res_plans(tuple(w.shape), tuple(wr.shape), cls, dims, 2, cin, n=n)])
        mp = dataclasses.replace(mp[0], tile=(lx, mp[0].tile[1], tz))
        wp = H.pack(mp, w, torch.bfloat16)
        wpr = torch.zeros(mp.pack_map_res.size, dtype=torch.bfloat16, device="cuda")
        mr = torch.from_numpy(mp.pack_map_res).cuda()
        L.check(lib.vsseg_gather_cast(wr.float().reshape(-1).cuda().data_ptr(), mr.data_ptr(), None, wpr.data_ptr(), mr.numel(), L.BF16, H.stream()), "gather_cast")
        # separate launches (general kernel)
        gen = P.plan_igemm("conv_fwd", tuple(w.shape), cls, dims, 2, kc_pad=cin, aux_es=0)
        gen.pack_map = P.pack_map(gen, tuple(w.shape))
        cls1 = P.lattice_classes("conv_fwd", (1, 1, 1), (1, 1, 1))[0]
        gen1 = P.plan_igemm("conv_fwd", tuple(wr.shape), cls1, dims, 2, kc_pad=cin, aux_es=0)
        gen1.pack_map = P.pack_map(gen1, tuple(wr.shape))
        y_ref = torch.zeros(n, *dims, cout, dtype=torch.bfloat16, device="cuda")
        r_ref = torch.zeros_like(y_ref)
        st_ref = torch.zeros(L.STAT_SHARDS * 2 * cout, dtype=torch.float64, device="cuda")
        wpg, wpg1 = H.pack(gen, w, torch.bfloat16), H.pack(gen1, wr, torch.bfloat16)
        d = H.igemm_desc(gen, wpg, H.tdesc(xcl), H.tdesc(y_ref), bias=b.data_ptr(), stats=st_ref.data_ptr(), stats_stride=cout)
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm")
        d = H.igemm_desc(gen1, wpg1, H.tdesc(xcl), H.tdesc(r_ref), bias=br.data_ptr())
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm 1x1x1")
        # one launch, residual tensor stored
        y, r = torch.full_like(y_ref, float("nan")), torch.full_like(y_ref, float("nan"))
        st = torch.zeros_like(st_ref)
        d = H.igemm_desc(mp, wp, H.tdesc(xcl), H.tdesc(y), bias=b.data_ptr(), stats=st.data_ptr(), stats_stride=cout, wpack_res=wpr.data_ptr(), bias_res=br.data_ptr(), res_out=H.tdesc(r))
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm + residual tiles")
        torch.cuda.synchronize()
        assert torch.equal(y, y_ref) and torch.equal(r, r_ref), (depth, float((y.float() - y_ref.float()).abs().max()), float((r.float() - r_ref.float()).abs().max()))
        a, bb = H.stat_decode(st_ref).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(st).view(L.STAT_SHARDS, 2, -1).sum(0)
        np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-3)
        # eval form: folded BatchNorm + PReLU, residual added in the epilogue
        sc, sh, al = (torch.rand(cout) + 0.5).cuda(), torch.randn(cout).cuda() * 0.1, torch.tensor([0.25], device="cuda")
        out = torch.full_like(y_ref, float("nan"))
        d = H.igemm_desc(mp, wp, H.tdesc(xcl), H.tdesc(out), bias=b.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr(), alpha=al.data_ptr(), act=L.ACT_PRELU, wpack_res=wpr.data_ptr(), bias_res=br.data_ptr())
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm + residual tiles (eval)")
        torch.cuda.synchronize()
        yy = F.conv3d(x.double(), w.double(), b.double().cpu(), padding=P.same_pad(k)) * sc.double().cpu().view(1, -1, 1, 1, 1) + sh.double().cpu().view(1, -1, 1, 1, 1)
        want = F.prelu(yy, al.double().cpu()) + F.conv3d(x.double(), wr.double(), br.double().cpu())
        assert_one_rounding(H.from_cl(out), want, what=f"residual tiles, eval, depth {depth}")
        if cin == 64:  # + the attention gate applied on load to the two-part concat (the level-1 decoder unit): bit-identical to the launch on the materialised gated tensor
            att = torch.rand(n, *dims, device="cuda")
            gated = torch.empty_like(xcl)
            L.check(lib.vsseg_att_apply_fwd(H.tdesc(xcl), att.data_ptr(), H.tdesc(gated), H.stream()), "att_apply_fwd")
            parts = H._split_cl(xcl, 32)
            res = []
            for inp, kw in ((H.tdesc(gated), {}), (H.two_part(*parts), dict(in_gate=att.data_ptr()))):
                yg, rg, stg = torch.full_like(y_ref, float("nan")), torch.full_like(y_ref, float("nan")), torch.zeros_like(st_ref)
                d = H.igemm_desc(mp, wp, inp, H.tdesc(yg), bias=b.data_ptr(), stats=stg.data_ptr(), stats_stride=cout, wpack_res=wpr.data_ptr(), bias_res=br.data_ptr(), res_out=H.tdesc(rg), **kw)
                L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm + residual tiles + gate")
                og = torch.full_like(y_ref, float("nan"))
                d = H.igemm_desc(mp, wp, inp, H.tdesc(og), bias=b.data_ptr(), scale=sc.data_ptr(), shift=sh.data_ptr(), alpha=al.data_ptr(), act=L.ACT_PRELU, wpack_res=wpr.data_ptr(), bias_res=br.data_ptr(), **kw)
                L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm + residual tiles + gate (eval)")
                torch.cuda.synchronize()
                res.append((yg, rg, H.stat_decode(stg).view(L.STAT_SHARDS, 2, -1).sum(0), og))
            assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][3], res[1][3]) and not torch.isnan(res[1][3].float()).any()
            np.testing.assert_allclose(res[1][2].cpu().numpy(), res[0][2].cpu().numpy(), rtol=1e-6, atol=1e-4)
    # the general kernel refuses the field loudly
    d = H.igemm_desc(gen, wpg, H.tdesc(xcl), H.tdesc(y), res_tiles=2, wpack_res=wpr.data_ptr())
    assert lib.vsseg_igemm(C.byref(d), H.stream()) != 0


@pytest.mark.parametrize("dims,split,shape,lx", [((7, 128, 4), 16, (2, 4), 3), ((6, 64, 8), 16, (4, 4), 6), ((5, 64, 8), 0, (4, 2), 2)])
def test_attention_gate_on_load_equals_materialised_gate(dims, split, shape, lx):
    """in_gate / h_gate: the marching convolution and the marching weight gradient multiply the input voxels by (1 + att) in LDS (AttentionBlock2,
    ref:params/networks/blocks/attentionblock.py:43-47) instead of reading a gated tensor written by vsseg_att_apply_fwd.  The forward must be
    BIT-IDENTICAL to the same marching launch on the materialised tensor (same fp32 product, same bf16 rounding), the weight gradient too; and equal
    the fp64 convolution of that materialised bf16 tensor (the reference rounds where the kernel does: it reads the stored tensor)."""
    lib = L.lib()
    cin, cout, k = 32, 2, (3, 3, 1)
    torch.manual_seed(13)
    x_cl = H.to_cl(_round(torch.randn(2, cin, *dims), "bf16"), torch.bfloat16)
    att = torch.rand(2, *dims, device="cuda")
    gated = torch.empty_like(x_cl)
    L.check(lib.vsseg_att_apply_fwd(H.tdesc(x_cl), att.data_ptr(), H.tdesc(gated), H.stream()), "att_apply_fwd")
    w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, "bf16")
    b = torch.randn(cout).cuda()
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]
    tz, mtw = shape
    mp = [pl for pl in P.march_plans("conv_fwd", tuple(w.shape), cls, dims, 2, cin, cout, cin, n=2) if (pl.tile[2], pl.mtw) == (tz, mtw)][0]
    mp = dataclasses.replace(mp, tile=(lx, mp.tile[1], tz))
    mp.pack_map = P.pack_map(mp, tuple(w.shape))
    wp = H.pack(mp, w, torch.bfloat16)
    parts = H._split_cl(x_cl, split) if split else None  # (kept alive: the descriptor holds raw pointers)
    xin = H.two_part(*parts) if split else H.tdesc(x_cl)
    outs = []
    for inp, kw in ((H.tdesc(gated), {}), (xin, dict(in_gate=att.data_ptr()))):
        out = torch.zeros(2, *dims, cout, dtype=torch.float32, device="cuda")
        d = H.igemm_desc(mp, wp, inp, H.tdesc(out), bias=b.data_ptr(), **kw)
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "igemm")
        torch.cuda.synchronize()
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), float((outs[0] - outs[1]).abs().max())
    # the definition on the bf16 gated tensor vsseg_att_apply_fwd stored (the marching launch rounds x * (1 + att) to bf16 at the same place); the logits are fp32
    y = F.conv3d(H.from_cl(gated).double(), w.double(), b.cpu().double(), padding=P.same_pad(k))
    _check("fp32", H.from_cl(outs[1]), y, "gate on load")
    # the general kernel refuses the field loudly
    gen = P.plan_igemm("conv_fwd", tuple(w.shape), cls, dims, 2, kc_pad=cin, in_split=split)
    gen.pack_map = P.pack_map(gen, tuple(w.shape))
    d = H.igemm_desc(gen, H.pack(gen, w, torch.bfloat16), xin, H.tdesc(outs[0]), in_gate=att.data_ptr())
    assert lib.vsseg_igemm(C.byref(d), H.stream()) != 0 and b"in_gate" in lib.vsseg_last_error()
    # weight gradient: P = dY of the 2 logits channels stored as one 8-channel group
    gy = torch.zeros(2, *dims, 8, device="cuda")
    gy[..., :cout] = torch.randn(2, *dims, cout, device="cuda")
    gy = gy.to(torch.bfloat16)
    tile = (lx, 32 if dims[0] == 5 else 64, 4)  # the gated weight gradient is instantiated for 4 z slices x 32 / 64 rows
    h = parts if split else x_cl
    dw_gate = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gy, h, cout, cin, march_tile=tile, h_gate=att)
    dw_mat = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), gy, gated, cout, cin, march_tile=tile)
    assert torch.equal(dw_gate, dw_mat), float((dw_gate - dw_mat).abs().max())


CHAIN_CASES = [
    # input channels, output channels of the second convolution, dims (Y = waves * mtw * 16 / tz), input split, (tz, mtw), x steps per workgroup, waves, fetch distance
    (1, 16, (7, 64, 8), 0, (4, 2), 3, 8, 3),      # first ResidualUnit: compact one-channel input, three x segments (3 + 3 + 1)
    (1, 16, (5, 128, 4), 0, (4, 4), 5, 8, 3),     # ... full benchmark height, one segment
    (1, 16, (6, 64, 4), 0, (2, 1), 2, 8, 3),
    (1, 16, (4, 128, 12), 0, (2, 2), 4, 8, 3),    # six z blocks
    (1, 16, (5, 128, 4), 0, (2, 4), 2, 4, 3),     # four waves
    (1, 16, (6, 64, 8), 0, (4, 4), 3, 4, 3),
    (32, 1, (7, 128, 4), 16, (2, 2), 3, 8, 3),    # attention block of the level-0 decoder: two-part (concat) input, fp32 one-channel sigmoid output; one large workgroup per CU
    (32, 1, (6, 64, 8), 16, (4, 2), 6, 8, 3),
    (32, 1, (9, 64, 4), 0, (2, 1), 4, 8, 3),      # one-part input, three segments (4 + 4 + 1)
    (32, 1, (7, 128, 4), 16, (1, 1), 3, 8, 1),    # ... several small workgroups per CU (fetch distance 1): one-voxel columns
    (32, 1, (5, 128, 4), 16, (1, 2), 5, 4, 1),
    (32, 1, (6, 128, 4), 0, (2, 4), 2, 4, 1),
    (32, 1, (6, 128, 4), 16, (2, 2), 6, 8, 1),
    (32, 1, (8, 64, 4), 16, (1, 1), 4, 4, 1),
    (32, 1, (5, 64, 4), 0, (2, 2), 5, 4, 1),
    (32, 1, (5, 64, 8), 0, (2, 1), 3, 8, 1),
]


@pytest.mark.parametrize("cin,cout,dims,split,shape,lx,waves,lead", CHAIN_CASES)
def test_chained_marching_convolution_equals_the_two_launches(cin, cout, dims, split, shape, lx, waves, lead):
    """vsseg_conv_chain (csrc/chain.hip): conv + folded BatchNorm + PReLU -> conv + epilogue as ONE launch with the 16-channel tensor between them in LDS.  Same packed
    weights, K order, MFMA order and epilogue arithmetic as the two marching launches (depth -5) it replaces: the output must be IDENTICAL bit for bit — across x segments
    (the halo planes of h are recomputed), z blocks, the image borders (h is zero outside the image, not conv_a of a padded x) — and equal the torch fp64 definition.
    The 16-channel tensor between the two convolutions is bf16 by design: the first launch's stored output meets ITS definition within one rounding, and the
    definition of the second convolution is built from that stored tensor (the chain is bit-identical to the two launches), so neither check leaves room for a
    second rounding.  The second marching launch is also where the VSSEG_RES_IN1 epilogue (first ResidualUnit) meets its definition."""
    lib = L.lib()
    dt, k, cm = "bf16", (3, 3, 1), 16
    tz, mtw = shape
    assert dims[1] == waves * mtw * 16 // tz
    torch.manual_seed(21)
    x = _round(torch.randn(2, cin, *dims), dt)
    wa = _round(torch.randn(cm, cin, *k) / (cin * 9) ** 0.5, dt)
    wb = _round(torch.randn(cout, cm, *k) / (cm * 9) ** 0.5, dt)
    ba, bb = torch.randn(cm), torch.randn(cout)
    res1 = cin == 1
    sca, sha = (torch.rand(cm) + 0.5, torch.randn(cm) * 0.3) if res1 else (None, None)  # (the attention block's first convolution has no BatchNorm: bias + ReLU)
    act_a = L.ACT_PRELU if res1 else L.ACT_RELU
    scb, shb = (torch.rand(cout) + 0.5, torch.randn(cout) * 0.3) if res1 else (None, None)
    w1, b1 = torch.randn(cout), torch.randn(cout)
    alpha_a, alpha_b = torch.tensor([0.25], device="cuda"), torch.tensor([0.1], device="cuda")
    dev = lambda t: t.cuda() if t is not None else None
    ba_d, bb_d, sca_d, sha_d, scb_d, shb_d, w1_d, b1_d = map(dev, (ba, bb, sca, sha, scb, shb, w1, b1))
    ptr = lambda t: t.data_ptr() if t is not None else None
    act_b = L.ACT_PRELU if res1 else L.ACT_SIGMOID

    # torch fp64 definition of the first convolution
    h = F.conv3d(x.double(), wa.double(), ba.double(), padding=P.same_pad(k))
    if res1:
        h = h * sca.double().view(1, -1, 1, 1, 1) + sha.double().view(1, -1, 1, 1, 1)
    h = torch.where(h > 0, h, (0.25 if res1 else 0.0) * h)

    # the two marching launches
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]
    x_cl = H.to_cl(x, H.DT[dt], cpad=P.round_up(cin, 8))
    compact = x_cl[..., :1].contiguous() if res1 else None
    parts = H._split_cl(x_cl, split) if split else None
    xin = H.tdesc(compact) if res1 else (H.two_part(*parts) if parts else H.tdesc(x_cl))

    def march(w, kc, n_t):
        kreal, nreal = P.gemm_dims("conv_fwd", tuple(w.shape))
        got = [pl for pl in P.march_plans("conv_fwd", tuple(w.shape), cls, dims, 2, kc, nreal, kreal, n=2) if pl.depth == L.DEPTH_MARCH and pl.nt == n_t]
        assert got, "no marching plan"
        pl = got[0]
        pl.pack_map = P.pack_map(pl, tuple(w.shape))
        return pl, H.pack(pl, w, H.DT[dt])

    pa, wpa = march(wa, x_cl.shape[-1], 1)
    pb, wpb = march(wb, cm, 1)
    h_cl = torch.zeros(2, *dims, cm, dtype=H.DT[dt], device="cuda")
    odt = H.DT[dt] if res1 else torch.float32
    want = torch.zeros(2, *dims, cout, dtype=odt, device="cuda")
    d1 = H.igemm_desc(pa, wpa, xin, H.tdesc(h_cl), bias=ptr(ba_d), scale=ptr(sca_d), shift=ptr(sha_d), act=act_a, alpha=alpha_a.data_ptr())
    L.check(lib.vsseg_igemm(C.byref(d1), H.stream()), "igemm A")
    kw = dict(bias=ptr(bb_d), act=act_b, alpha=alpha_b.data_ptr())
    if res1:
        kw.update(scale=ptr(scb_d), shift=ptr(shb_d), res_mode=L.RES_IN1, in1=compact.data_ptr(), in1_w=ptr(w1_d), in1_b=ptr(b1_d))
    d2 = H.igemm_desc(pb, wpb, H.tdesc(h_cl), H.tdesc(want), **kw)
    L.check(lib.vsseg_igemm(C.byref(d2), H.stream()), "igemm B")
    assert_one_rounding(H.from_cl(h_cl), h, what="first launch")
    # torch fp64 definition of the second convolution on the bf16 tensor the first launch stored
    y = F.conv3d(H.from_cl(h_cl).double(), wb.double(), bb.double(), padding=P.same_pad(k))
    if res1:
        y = y * scb.double().view(1, -1, 1, 1, 1) + shb.double().view(1, -1, 1, 1, 1)
        y = torch.where(y > 0, y, 0.1 * y) + x.double() * w1.double().view(1, -1, 1, 1, 1) + b1.double().view(1, -1, 1, 1, 1)
    else:
        y = torch.sigmoid(y)

    # ... and the chain
    got = torch.full((2, *dims, cout), float("nan"), dtype=odt, device="cuda")
    d = L.ChainDesc()
    d.inp, d.out, d.cmid = xin, H.tdesc(got), cm
    d.wpack_a, d.bias_a, d.scale_a, d.shift_a, d.alpha_a, d.act_a = wpa.data_ptr(), ptr(ba_d), ptr(sca_d), ptr(sha_d), alpha_a.data_ptr(), act_a
    d.wpack_b, d.bias_b, d.scale_b, d.shift_b, d.alpha_b, d.act_b = wpb.data_ptr(), ptr(bb_d), ptr(scb_d), ptr(shb_d), alpha_b.data_ptr(), act_b
    if res1:
        d.in1_w, d.in1_b = ptr(w1_d), ptr(b1_d)
    d.tz, d.mtw, d.lx, d.waves, d.lead = tz, mtw, lx, waves, lead
    assert lib.vsseg_conv_chain_lds_bytes(C.byref(d)) > 0, lib.vsseg_last_error()
    L.check(lib.vsseg_conv_chain(C.byref(d), H.stream()), "conv_chain")
    torch.cuda.synchronize()
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got, want), f"chain differs from the two launches (max {float((got.float() - want.float()).abs().max())})"
    _check(dt if res1 else "fp32", H.from_cl(got), y, "chain")  # (the attention map is an fp32 tensor)
    got2 = torch.full_like(got, float("nan"))
    d.out = H.tdesc(got2)
    L.check(lib.vsseg_conv_chain(C.byref(d), H.stream()), "conv_chain")
    torch.cuda.synchronize()
    assert torch.equal(got, got2)  # run-to-run


@pytest.mark.parametrize("dims,shape,lx", [((7, 64, 8), (2, 1), 3), ((6, 64, 8), (4, 2), 6), ((5, 128, 4), (2, 2), 2)])
def test_chained_marching_convolution_with_residual_tiles(dims, shape, lx):
    """The two-sub-unit ResidualUnit of level 1 in inference (ref:params/networks/blocks/convolutions.py:241-255): 16 -> 32 (folded BatchNorm + PReLU) -> 32 (the same) + the
    1x1x1 residual convolution 16 -> 32 of the unit's input, as ONE vsseg_conv_chain launch: stage B multiplies the centre-tap K-step of the input plane it is about to overwrite
    with the residual weights and adds the bf16-rounded result behind its activation.  Bit-identical to the three launches (convolution, residual convolution, convolution + add)."""
    lib = L.lib()
    dt, k, cin, cm, cout = "bf16", (3, 3, 1), 16, 32, 32
    tz, mtw = shape
    assert dims[1] == 8 * mtw * 16 // tz
    torch.manual_seed(33)
    x = _round(torch.randn(2, cin, *dims), dt)
    wa = _round(torch.randn(cm, cin, *k) / (cin * 9) ** 0.5, dt)
    wb = _round(torch.randn(cout, cm, *k) / (cm * 9) ** 0.5, dt)
    wr = _round(torch.randn(cout, cin, 1, 1, 1) / cin ** 0.5, dt)
    vec = lambda n_, s_=1.0: (torch.randn(n_) * s_).cuda()
    ba, bb, br, sha, shb = vec(cm), vec(cout), vec(cout), vec(cm, 0.3), vec(cout, 0.3)
    sca, scb = (torch.rand(cm) + 0.5).cuda(), (torch.rand(cout) + 0.5).cuda()
    al_a, al_b = torch.tensor([0.25], device="cuda"), torch.tensor([0.1], device="cuda")
    x_cl = H.to_cl(x, H.DT[dt])
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]

    def march(w, kc, nt):
        kreal, nreal = P.gemm_dims("conv_fwd", tuple(w.shape))
        pl = [p_ for p_ in P.march_plans("conv_fwd", tuple(w.shape), cls, dims, 2, kc, nreal, kreal, n=2) if p_.depth == L.DEPTH_MARCH and p_.nt == nt][0]
        pl.pack_map = P.pack_map(pl, tuple(w.shape))
        return pl, H.pack(pl, w, H.DT[dt])

    pa, wpa = march(wa, cin, 2)
    pb, wpb = march(wb, cm, 2)
    h_cl = torch.zeros(2, *dims, cm, dtype=H.DT[dt], device="cuda")
    r_cl = torch.zeros(2, *dims, cout, dtype=H.DT[dt], device="cuda")
    want = torch.zeros(2, *dims, cout, dtype=H.DT[dt], device="cuda")
    L.check(lib.vsseg_igemm(C.byref(H.igemm_desc(pa, wpa, H.tdesc(x_cl), H.tdesc(h_cl), bias=ba.data_ptr(), scale=sca.data_ptr(), shift=sha.data_ptr(), act=L.ACT_PRELU, alpha=al_a.data_ptr())), H.stream()), "A")
    H.run_lattice_op("conv_fwd", wr, x_cl, r_cl, (1, 1, 1), bias=br.data_ptr())
    L.check(lib.vsseg_igemm(C.byref(H.igemm_desc(pb, wpb, H.tdesc(h_cl), H.tdesc(want), bias=bb.data_ptr(), scale=scb.data_ptr(), shift=shb.data_ptr(), act=L.ACT_PRELU, alpha=al_b.data_ptr(),
                                                  res=H.tdesc(r_cl), res_mode=L.RES_ADD)), H.stream()), "B")
    rmap = torch.from_numpy(P.residual_tile_pack_map(cin, 2, tuple(wr.shape))).cuda()
    wflat = wr.reshape(-1).to(H.DT[dt]).cuda()
    wpr = torch.where(rmap >= 0, wflat[rmap.clamp(min=0).long()], torch.zeros((), dtype=H.DT[dt], device="cuda"))
    got = torch.full((2, *dims, cout), float("nan"), dtype=H.DT[dt], device="cuda")
    d = L.ChainDesc()
    d.inp, d.out, d.cmid = H.tdesc(x_cl), H.tdesc(got), cm
    d.wpack_a, d.bias_a, d.scale_a, d.shift_a, d.alpha_a, d.act_a = wpa.data_ptr(), ba.data_ptr(), sca.data_ptr(), sha.data_ptr(), al_a.data_ptr(), L.ACT_PRELU
    d.wpack_b, d.bias_b, d.scale_b, d.shift_b, d.alpha_b, d.act_b = wpb.data_ptr(), bb.data_ptr(), scb.data_ptr(), shb.data_ptr(), al_b.data_ptr(), L.ACT_PRELU
    d.res_tiles, d.wpack_res, d.bias_res = 2, wpr.data_ptr(), br.data_ptr()
    d.tz, d.mtw, d.lx, d.waves, d.lead = tz, mtw, lx, 8, 1
    assert lib.vsseg_conv_chain_lds_bytes(C.byref(d)) > 0, lib.vsseg_last_error()
    L.check(lib.vsseg_conv_chain(C.byref(d), H.stream()), "conv_chain")
    torch.cuda.synchronize()
    assert torch.equal(got, want), f"chain differs from the three launches (max {float((got.float() - want.float()).abs().max())})"
    # the definition in fp64.  h and the residual are bf16 tensors by design: each stored tensor meets its own definition within one rounding, and the
    # definition of the output is built from the stored tensors (the chain is bit-identical to the three launches that store them)
    pre = lambda v: v.double().cpu().view(1, -1, 1, 1, 1)
    h = F.conv3d(x.double(), wa.double(), ba.double().cpu(), padding=P.same_pad(k)) * pre(sca) + pre(sha)
    assert_one_rounding(H.from_cl(h_cl), torch.where(h > 0, h, 0.25 * h), what="first launch")
    assert_one_rounding(H.from_cl(r_cl), F.conv3d(x.double(), wr.double(), br.double().cpu()), what="residual convolution")
    y = F.conv3d(H.from_cl(h_cl).double(), wb.double(), bb.double().cpu(), padding=P.same_pad(k)) * pre(scb) + pre(shb)
    y = torch.where(y > 0, y, 0.1 * y) + H.from_cl(r_cl).double()
    assert_one_rounding(H.from_cl(got), y, what="chain with residual tiles")


def test_chained_marching_convolution_rejects_what_it_does_not_cover():
    lib = L.lib()
    x = torch.zeros(1, 4, 64, 4, 32, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, 4, 64, 4, 1, dtype=torch.float32, device="cuda")
    w = torch.zeros(16 * 1024, dtype=torch.bfloat16, device="cuda")

    def desc(**kw):
        d = L.ChainDesc()
        d.inp, d.out, d.cmid, d.wpack_a, d.wpack_b, d.act_b, d.tz, d.mtw, d.lx, d.waves, d.lead = H.tdesc(x), H.tdesc(out), 16, w.data_ptr(), w.data_ptr(), L.ACT_SIGMOID, 2, 1, 4, 8, 3
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d

    assert lib.vsseg_conv_chain_lds_bytes(C.byref(desc())) > 0
    for bad in (dict(tz=4), dict(mtw=2), dict(cmid=32), dict(lx=0), dict(waves=6), dict(lead=2), dict(wpack_b=None), dict(in1_w=w.data_ptr()), dict(scale_b=w.data_ptr()), dict(act_b=7), dict(act_a=L.ACT_SIGMOID)):
        assert lib.vsseg_conv_chain(C.byref(desc(**bad)), H.stream()) == L.EINVAL, bad
        assert b"vsseg_conv_chain" in lib.vsseg_last_error()
    f32_in = torch.zeros(1, 4, 64, 4, 32, dtype=torch.float32, device="cuda")
    assert lib.vsseg_conv_chain(C.byref(desc(inp=H.tdesc(f32_in))), H.stream()) == L.EINVAL


COMPUTE_CASES = [
    # kind, cin, cout, dims, input split
    ("conv_fwd", 32, 48, (8, 16, 32), 0),     # every tile touches the border
    ("conv_fwd", 96, 48, (12, 24, 48), 48),   # level-2 concat read as a two-part tensor; the centre tile is interior
    ("conv_dgrad", 96, 48, (8, 16, 32), 0),   # K = 48, N = 96: two workgroups per voxel tile (nsplit 2)
    ("conv_dgrad", 32, 48, (8, 16, 32), 0),   # K = 48, N = 32: two 16-channel tiles per workgroup
    ("conv_fwd", 64, 64, (8, 8, 16), 0),      # level-3 shape: 2 x 2 channel tiles
    ("conv_dgrad", 128, 64, (8, 8, 16), 0),   # K = 64, N = 128 (the level-3 concat gradient): four workgroups per voxel tile
]


@pytest.mark.parametrize("kind,cin,cout,dims,split", COMPUTE_CASES)
def test_compute_kernel_equals_general_kernel(kind, cin, cout, dims, split):
    """depth -3 selects the compile-time-geometry kernel for the MFMA-bound stride-1 3x3x3 launches (csrc/cconv.hip).  Same packed
    weights, K order and fp32 accumulation as the general kernel: outputs must be IDENTICAL bit for bit in every epilogue mode (and match
    the fp64 definition within the bf16 output rounding); BatchNorm statistics agree up to the order of the fp32 partial sums."""
    lib = L.lib()
    dt, k = "bf16", (3, 3, 3)
    torch.manual_seed(7)
    x = _round(torch.randn(2, cin, *dims), dt)
    w = _round(torch.randn(cout, cin, *k) / (cin * 27) ** 0.5, dt)
    b = torch.randn(cout)
    xd = x.double().requires_grad_(True)
    y = F.conv3d(xd, w.double(), b.double(), padding=P.same_pad(k))
    if kind == "conv_fwd":
        inp_cl, want, nout, bias = H.to_cl(x, H.DT[dt]), y.detach(), cout, b.cuda()
    else:
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        inp_cl, want, nout, bias = H.to_cl(gy, H.DT[dt]), xd.grad, cin, None
    cls = P.lattice_classes(kind, k, (1, 1, 1))[0]
    kc = inp_cl.shape[-1]
    # the general kernel's plan with the same 16-channel chunking: same K order, hence the same fp32 accumulation order
    gen = next(c for c in P.candidate_plans(kind, tuple(w.shape), cls, dims, 2, kc_pad=kc, in_split=split, aux_es=2) if c.ck == 16 and c.depth >= 0)
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    cp = P.compute_plan(kind, tuple(w.shape), cls, dims, 2, kc, nreal, kreal, split)
    assert cp is not None and cp.depth == L.DEPTH_COMPUTE and gen.depth != L.DEPTH_COMPUTE
    cp.pack_map = P.pack_map(cp, tuple(w.shape))
    parts = H._split_cl(inp_cl, split) if split else None
    res_t = H.to_cl(_round(torch.randn(2, nout, *dims), dt), H.DT[dt])
    gate_t = torch.rand(2, *dims, device="cuda")
    alpha = torch.tensor([0.25], device="cuda")
    for mode in ["plain", "stats", "prelu", "accumulate", "res_add", "relu_mask", "gate"]:
        outs = []
        for pl in (gen, cp):
            out = torch.zeros(2, *dims, nout, dtype=H.DT[dt], device="cuda")
            kw, stats = {}, None
            if mode == "stats":
                stats = torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")
                kw = dict(stats=stats.data_ptr(), stats_stride=P.round_up(nout, 16))
            elif mode == "prelu":
                kw = dict(act=L.ACT_PRELU, alpha=alpha.data_ptr())
            elif mode == "accumulate":
                out = res_t.clone()
                kw = dict(accumulate=1)
            elif mode in ("res_add", "relu_mask", "gate"):
                kw = dict(res=H.tdesc(res_t), res_mode={"res_add": L.RES_ADD, "relu_mask": L.RES_RELUMASK, "gate": L.RES_GATE}[mode])
                if mode == "gate":
                    kw["gate"] = gate_t.data_ptr()
            if bias is not None:
                kw["bias"] = bias.data_ptr()
            wp = H.pack(pl, w, inp_cl.dtype)
            d = H.igemm_desc(pl, wp, H.two_part(*parts) if parts else H.tdesc(inp_cl), H.tdesc(out), **kw)
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"igemm D={pl.depth} {mode}")
            torch.cuda.synchronize()
            outs.append((out, stats))
        (og, sg), (oc, sc) = outs
        assert torch.equal(og, oc), f"{mode}: compute kernel differs from the general kernel (max {float((og.float() - oc.float()).abs().max())})"
        if mode == "plain":
            assert_one_rounding(H.from_cl(oc), want, what="compute kernel")
        if mode == "stats":
            a, bb = H.stat_decode(sg).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(sc).view(L.STAT_SHARDS, 2, -1).sum(0)
            np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-3)
            np.testing.assert_allclose(bb[0, :nout].cpu().numpy(), want.sum((0, 2, 3, 4)).numpy(), rtol=2e-4, atol=2e-2)


@pytest.mark.parametrize("kind,cin,cout,dims,mode", [("convT_fwd", 32, 16, (8, 16, 8), "stats"), ("convT_fwd", 32, 16, (16, 8, 4), "plain"), ("convT_fwd", 32, 16, (16, 64, 16), "stats"), ("convT_fwd", 32, 16, (8, 32, 8), "plain"), ("conv_dgrad", 16, 16, (8, 16, 8), "accumulate"),
                                                     ("conv_dgrad", 16, 16, (16, 16, 4), "plain"), ("convT_fwd", 48, 32, (8, 16, 8), "stats"), ("conv_dgrad", 32, 32, (8, 8, 8), "accumulate"),
                                                     ("convT_fwd", 48, 32, (16, 32, 8), "stats"), ("convT_fwd", 48, 32, (8, 64, 16), "plain"),
                                                     ("conv_dgrad", 16, 16, (16, 64, 8), "accumulate"), ("conv_dgrad", 16, 16, (8, 32, 8), "plain"), ("conv_dgrad", 32, 32, (8, 32, 8), "accumulate"),
                                                     ("conv_dgrad", 32, 32, (16, 64, 8), "plain")])
def test_fused_parity_classes_equal_per_class_launches(kind, cin, cout, dims, mode):
    """depth -4: the four output-parity classes of a stride-(2,2,1) 3x3x1 transposed convolution / data gradient as ONE launch of the
    streaming kernel (coarse lattice, 2x2x1 neighbourhood, 4 x 16 output channels, pixel-shuffle store).  Must equal the four per-class
    launches of the general kernel (up to the fp32 summation order of the taps) and torch's fp64 result, with BatchNorm statistics /
    gradient accumulation in the epilogue."""
    lib = L.lib()
    dt, k, st = "bf16", (3, 3, 1), (2, 2, 1)
    torch.manual_seed(21)
    n = 2
    fine = (2 * dims[0], 2 * dims[1], dims[2])
    if kind == "convT_fwd":  # x at the coarse level (cin channels) -> y at the fine level (cout channels)
        x = _round(torch.randn(n, cin, *dims), dt)
        w = _round(torch.randn(cin, cout, *k) / (cin * 9) ** 0.5, dt)
        want = F.conv_transpose3d(x.double(), w.double(), stride=st, padding=P.same_pad(k), output_padding=(1, 1, 0))
        inp_cl, nout = H.to_cl(x, H.DT[dt]), cout
    else:  # dY at the coarse level (cout channels) -> dX at the fine level (cin channels)
        w = _round(torch.randn(cout, cin, *k) / (cin * 9) ** 0.5, dt)
        xd = torch.zeros(n, cin, *fine, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(xd, w.double(), stride=st, padding=P.same_pad(k))
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        want, inp_cl, nout = xd.grad, H.to_cl(gy, H.DT[dt]), cin
    assert tuple(want.shape[2:]) == fine
    prev = H.to_cl(_round(torch.randn(n, nout, *fine), dt), H.DT[dt])
    kw = {}
    if mode == "accumulate":
        kw = dict(accumulate=1)
        want = want + H.from_cl(prev).double()

    def stats_buf():
        return torch.zeros(L.STAT_SHARDS * 2 * nout, dtype=torch.float64, device="cuda")

    # reference: one launch of the general kernel per parity class
    out_a = prev.clone() if mode == "accumulate" else torch.zeros(n, *fine, nout, dtype=H.DT[dt], device="cuda")
    sa = stats_buf()
    H.run_lattice_op(kind, w, inp_cl, out_a, st, **(dict(stats=sa.data_ptr(), stats_stride=nout) if mode == "stats" else kw))
    # fused
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    pls = P.shuffle_plans(kind, tuple(w.shape), k, st, dims, 2, inp_cl.shape[-1], nreal, kreal)
    assert pls is not None and len(pls) == nout // 16 and all(pl.depth == L.DEPTH_STREAM_SHUFFLE for pl in pls)  # 16 channels: one launch; 32: one per px
    out_b = prev.clone() if mode == "accumulate" else torch.zeros_like(out_a)
    sb = stats_buf()
    for pl in pls:
        d = H.igemm_desc(pl, H.pack(pl, w, inp_cl.dtype), H.tdesc(inp_cl), H.tdesc(out_b), **(dict(stats=sb.data_ptr(), stats_stride=nout) if mode == "stats" else kw))
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "fused classes")
    torch.cuda.synchronize()
    assert_one_rounding(H.from_cl(out_b), want, what=f"fused parity classes, {mode}")
    assert_one_rounding(H.from_cl(out_a), want, what=f"per-class launches, {mode}")  # same products, different fp32 summation order of the taps: compared through the definition
    if mode == "stats":
        a, bb = H.stat_decode(sa).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(sb).view(L.STAT_SHARDS, 2, -1).sum(0)
        np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-4, atol=1e-2)
        np.testing.assert_allclose(bb[0, :nout].cpu().numpy(), want.sum((0, 2, 3, 4)).numpy(), rtol=2e-4, atol=5e-2)
    # the marching variants of the launch (csrc/mconv.hip PS; 32 -> 4 x 16 channels): same taps, packed weights, K order and MFMA order as the streaming launch: bit-identical
    mps = P.march_shuffle_plans(pls[0], n) if len(pls) == 1 else []
    assert bool(mps) == (((kind == "convT_fwd" and cin == 32) or (kind == "conv_dgrad" and cin == 16)) and cout == 16 and dims[1] % 32 == 0)  # (column blocks of 32 or 64 coarse rows)
    for mp in mps:
        for lx in sorted({mp.tile[0], max(1, dims[0] // 3)}):  # (also with x segments that do not divide the extent)
            mp2 = dataclasses.replace(mp, tile=(lx, mp.tile[1], mp.tile[2]))
            out_c = prev.clone() if mode == "accumulate" else torch.full_like(out_a, float("nan"))
            sc = stats_buf()
            d = H.igemm_desc(mp2, H.pack(mp2, w, inp_cl.dtype), H.tdesc(inp_cl), H.tdesc(out_c), **(dict(stats=sc.data_ptr(), stats_stride=nout) if mode == "stats" else kw))
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"marching fused classes {mp2.tile} depth {mp2.depth}")
            torch.cuda.synchronize()
            assert torch.equal(out_c, out_b), f"marching variant tile {mp2.tile} mtw {mp2.mtw} depth {mp2.depth} differs (max {float((out_c.float() - out_b.float()).abs().max())})"
            if mode == "stats":
                cc = H.stat_decode(sc).view(L.STAT_SHARDS, 2, -1).sum(0)
                np.testing.assert_allclose(cc.cpu().numpy(), bb.cpu().numpy(), rtol=1e-5, atol=1e-3)


    # 48 -> 32 channels: ALL four classes as ONE marching launch (8 channel tiles, 6 channel groups) against the two streaming launches: bit-identical
    allp = P.march_shuffle_all_plans(kind, tuple(w.shape), k, st, dims, 2, inp_cl.shape[-1], nreal, kreal, n)
    assert bool(allp) == (((kind == "convT_fwd" and cin == 48) or (kind == "conv_dgrad" and cin == 32)) and cout == 32 and dims[1] % 32 == 0)
    for mp in allp:
        for lx in sorted({mp.tile[0], max(1, dims[0] // 3)}):
            mp2 = dataclasses.replace(mp, tile=(lx, mp.tile[1], mp.tile[2]))
            out_c = prev.clone() if mode == "accumulate" else torch.full_like(out_a, float("nan"))
            sc = stats_buf()
            d = H.igemm_desc(mp2, H.pack(mp2, w, inp_cl.dtype), H.tdesc(inp_cl), H.tdesc(out_c), **(dict(stats=sc.data_ptr(), stats_stride=nout) if mode == "stats" else kw))
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"marching all classes {mp2.tile}")
            torch.cuda.synchronize()
            assert torch.equal(out_c, out_b), f"all-class marching launch tile {mp2.tile} mtw {mp2.mtw} differs (max {float((out_c.float() - out_b.float()).abs().max())})"
            if mode == "stats":
                cc = H.stat_decode(sc).view(L.STAT_SHARDS, 2, -1).sum(0)
                np.testing.assert_allclose(cc.cpu().numpy(), bb.cpu().numpy(), rtol=1e-5, atol=1e-3)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("kind,cin,cout,fine,mode", [("convT_fwd", 96, 80, (8, 8, 8), "stats"), ("convT_fwd", 64, 48, (16, 8, 16), "plain"), ("convT_fwd", 80, 64, (4, 4, 4), "residual"),
                                                     ("conv_dgrad", 48, 64, (16, 16, 8), "accumulate"), ("conv_dgrad", 80, 80, (7, 9, 6), "plain"), ("conv_dgrad", 64, 80, (8, 8, 8), "relumask"),
                                                     ("conv_dgrad", 16, 16, (12, 6, 10), "plain")])
def test_class_split_launch_equals_per_class_launches(kind, cin, cout, fine, mode, dt):
    """vsseg_igemm_desc.class_split: the eight output-parity classes of a 3x3x3 stride-(2,2,2) transposed convolution / data gradient as ONE
    launch of the general kernel (workgroup row = class, 1..8 taps each).  Every candidate must equal the eight per-class launches (same
    products; the fp32 summation order may differ with the channel chunk) and torch's fp64 result, for each epilogue the network uses, also
    where the fine lattice is odd-sized (the classes with offset 1 are one voxel shorter)."""
    lib = L.lib()
    k, st = (3, 3, 3), (2, 2, 2)
    torch.manual_seed(23)
    n = 2
    tdt = H.DT[dt]
    if kind == "convT_fwd":
        coarse = tuple(f // 2 for f in fine)
        x = _round(torch.randn(n, cin, *coarse), dt)
        w = _round(torch.randn(cin, cout, *k) / (cin * 27 / 8) ** 0.5, dt)
        want = F.conv_transpose3d(x.double(), w.double(), stride=st, padding=1, output_padding=1)
        inp_cl, nout, q = H.to_cl(x, tdt, P.round_up(cin, 8)), cout, coarse
    else:
        w = _round(torch.randn(cout, cin, *k) / (cout * 27 / 8) ** 0.5, dt)
        xd = torch.zeros(n, cin, *fine, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(xd, w.double(), stride=st, padding=1)
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        want, inp_cl, nout, q = xd.grad, H.to_cl(gy, tdt, P.round_up(cout, 8)), cin, tuple((f + 1) // 2 for f in fine)
    assert tuple(want.shape[2:]) == fine
    prev = H.to_cl(_round(torch.randn(n, nout, *fine), dt), tdt)
    side = H.to_cl(_round(torch.randn(n, nout, *fine), dt), tdt)
    kw = {}
    if mode == "accumulate":
        kw, want = dict(accumulate=1), want + H.from_cl(prev).double()
    elif mode == "residual":
        kw, want = dict(res=H.tdesc(side), res_mode=L.RES_ADD), want + H.from_cl(side).double()
    elif mode == "relumask":
        kw, want = dict(res=H.tdesc(side), res_mode=L.RES_RELUMASK), want * (H.from_cl(side) > 0).double()

    def stats_buf():
        return torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")

    def epi(sbuf):
        return dict(stats=sbuf.data_ptr(), stats_stride=P.round_up(nout, 16)) if mode == "stats" else kw

    out_a = prev.clone() if mode == "accumulate" else torch.zeros(n, *fine, nout, dtype=tdt, device="cuda")
    sa = stats_buf()
    H.run_lattice_op(kind, w, inp_cl, out_a, st, **epi(sa))
    _check(dt, H.from_cl(out_a), want, f"per-class launches, {mode}")
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    aux_es = 0 if mode in ("plain", "stats") else inp_cl.element_size()
    pls = P.class_split_plans(kind, tuple(w.shape), k, st, q, inp_cl.element_size(), inp_cl.shape[-1], nreal, kreal, aux_es=aux_es)
    assert pls and all(pl.nsplit == 8 and len(pl.cls.taps) == 8 for pl in pls)
    for pl in pls:
        out_b = prev.clone() if mode == "accumulate" else torch.zeros_like(out_a)
        sb = stats_buf()
        d = H.igemm_desc(pl, H.pack(pl, w, inp_cl.dtype), H.tdesc(inp_cl), H.tdesc(out_b), **epi(sb))
        L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "class split")
        torch.cuda.synchronize()
        _check(dt, H.from_cl(out_b), want, f"class split, {mode}, {pl.tile} ck={pl.ck}")
        assert dt == "bf16" or float((out_a.float() - out_b.float()).abs().max()) <= 2 * _tol(dt, want)  # (bf16: both are within one rounding of the definition)
        if mode == "stats":
            a, bb = H.stat_decode(sa).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(sb).view(L.STAT_SHARDS, 2, -1).sum(0)
            np.testing.assert_allclose(bb.cpu().numpy(), a.cpu().numpy(), rtol=1e-4, atol=1e-2)
            np.testing.assert_allclose(bb[0, :nout].cpu().numpy(), want.sum((0, 2, 3, 4)).numpy(), rtol=2e-4, atol=5e-2)
    # a descriptor that mixes class_split with what it does not cover is rejected, not misread
    bad = H.igemm_desc(pls[0], H.pack(pls[0], w, inp_cl.dtype), H.tdesc(inp_cl), H.tdesc(out_a))
    bad.nsplit = 4
    assert lib.vsseg_igemm(C.byref(bad), H.stream()) == L.EINVAL and b"class_split" in lib.vsseg_last_error()


@pytest.mark.parametrize("kind,cin,cout,coarse,mode,n", [("convT_fwd", 64, 48, (8, 8, 16), "stats", 2), ("convT_fwd", 64, 48, (4, 16, 8), "plain", 1), ("convT_fwd", 64, 48, (4, 8, 8), "eval", 3),
                                                        ("conv_dgrad", 48, 48, (8, 16, 8), "accumulate", 2), ("conv_dgrad", 48, 48, (4, 8, 16), "plain", 1)])
def test_transition_kernel_equals_class_split_launch_and_definition(kind, cin, cout, coarse, mode, n):
    """Launch plans with depth -8 (csrc/tconv.hip): the eight output-parity classes of the 3x3x3 stride-(2,2,2) transposed convolution 64 -> 48 / of the data gradient of the
    strided convolution 48 -> 48 between levels 2 and 3 (ref:params/networks/nets/unet2d5_spvPA.py:56-93) in one launch — against torch's fp64 result, and BIT FOR BIT
    against the class-split launch of the general kernel on the same packed weights (same K order, one accumulator chain per output value), for the epilogues the network
    uses there (statistics, plain, eval affine + PReLU, accumulate), tiles on every face of the volume, several tiles per workgroup."""
    lib = L.lib()
    k, st = (3, 3, 3), (2, 2, 2)
    torch.manual_seed(29)
    tdt = torch.bfloat16
    fine = tuple(2 * c for c in coarse)
    if kind == "convT_fwd":
        x = _round(torch.randn(n, cin, *coarse), "bf16")
        w = _round(torch.randn(cin, cout, *k) / (cin * 27 / 8) ** 0.5, "bf16")
        want = F.conv_transpose3d(x.double(), w.double(), stride=st, padding=1, output_padding=1)
        inp_cl, nout = H.to_cl(x, tdt, cin), cout
    else:
        w = _round(torch.randn(cout, cin, *k) / (cout * 27 / 8) ** 0.5, "bf16")
        xd = torch.zeros(n, cin, *fine, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(xd, w.double(), stride=st, padding=1)
        gy = _round(torch.randn(*y.shape), "bf16")
        y.backward(gy.double())
        want, inp_cl, nout = xd.grad, H.to_cl(gy, tdt, cout), cin
    assert tuple(want.shape[2:]) == fine and tuple(inp_cl.shape[1:4]) == coarse
    bias = torch.randn(nout, device="cuda")
    want = want + bias.cpu().double().view(1, -1, 1, 1, 1)
    prev = H.to_cl(_round(torch.randn(n, nout, *fine), "bf16"), tdt)
    kw = dict(bias=bias.data_ptr())
    keep = []
    if mode == "accumulate":
        kw["accumulate"] = 1
        want = want + H.from_cl(prev).double()
    elif mode == "eval":
        sc, sh, al = torch.rand(nout, device="cuda") + 0.5, torch.randn(nout, device="cuda"), torch.tensor([0.2], device="cuda")
        keep += [sc, sh, al]
        kw.update(scale=sc.data_ptr(), shift=sh.data_ptr(), alpha=al.data_ptr(), act=L.ACT_PRELU)
        want = want * sc.cpu().double().view(1, -1, 1, 1, 1) + sh.cpu().double().view(1, -1, 1, 1, 1)
        want = torch.where(want > 0, want, 0.2 * want)

    def stats_buf():
        return torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")

    def epi(sbuf):
        return dict(stats=sbuf.data_ptr(), stats_stride=P.round_up(nout, 16), **kw) if mode == "stats" else kw

    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    tps = P.transition_plans(kind, tuple(w.shape), k, st, coarse, 2, inp_cl.shape[-1], nreal, kreal)
    assert len(tps) == 1 and tps[0].depth == L.DEPTH_TRANSITION and len(tps[0].classes) == 8
    tp = tps[0]
    out_t = prev.clone() if mode == "accumulate" else torch.full((n, *fine, nout), float("nan"), dtype=tdt, device="cuda")
    st_t = stats_buf()
    d = H.igemm_desc(tp, H.pack(tp, w, tdt), H.tdesc(inp_cl), H.tdesc(out_t), **epi(st_t))
    assert lib.vsseg_igemm_lds_bytes(C.byref(d)) == tp.lds == P.transition_lds_bytes(inp_cl.shape[-1])
    L.check(lib.vsseg_igemm(C.byref(d), H.stream()), "transition kernel")
    torch.cuda.synchronize()
    got = H.from_cl(out_t)
    assert not torch.isnan(got).any()
    assert_one_rounding(got, want, what=f"transition kernel, {mode}")
    # the class-split launch of the general kernel with the whole input in one channel chunk: the same accumulator chain per output value
    csp = [pl for pl in P.class_split_plans(kind, tuple(w.shape), k, st, coarse, 2, inp_cl.shape[-1], nreal, kreal, aux_es=2 if mode == "accumulate" else 0) if pl.nchunks == 1]
    assert csp
    out_c = prev.clone() if mode == "accumulate" else torch.zeros_like(out_t)
    st_c = stats_buf()
    dc = H.igemm_desc(csp[0], H.pack(csp[0], w, tdt), H.tdesc(inp_cl), H.tdesc(out_c), **epi(st_c))
    L.check(lib.vsseg_igemm(C.byref(dc), H.stream()), "class split")
    torch.cuda.synchronize()
    assert torch.equal(out_t, out_c), f"max {float((out_t.float() - out_c.float()).abs().max())}"
    if mode == "stats":
        a, b = H.stat_decode(st_c).view(L.STAT_SHARDS, 2, -1).sum(0), H.stat_decode(st_t).view(L.STAT_SHARDS, 2, -1).sum(0)
        np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=1e-5, atol=1e-3)


def test_transition_kernel_rejects_what_it_does_not_cover():
    lib = L.lib()
    k, st = (3, 3, 3), (2, 2, 2)
    w = torch.randn(64, 48, *k)
    kreal, nreal = P.gemm_dims("convT_fwd", tuple(w.shape))
    assert P.transition_plans("convT_fwd", tuple(w.shape), k, st, (6, 8, 8), 2, 64, nreal, kreal) == []      # x extent not a multiple of the tile
    assert P.transition_plans("convT_fwd", (80, 64, *k), k, st, (8, 8, 8), 2, 80, 64, 80) == []               # 80 -> 64: the deep-level kernel's
    assert P.transition_plans("conv_fwd", (48, 48, *k), k, st, (8, 8, 8), 2, 48, 48, 48) == []
    tp = P.transition_plans("convT_fwd", tuple(w.shape), k, st, (4, 8, 8), 2, 64, nreal, kreal)[0]
    x = torch.zeros(1, 4, 8, 8, 64, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, 8, 16, 16, 48, dtype=torch.bfloat16, device="cuda")
    wp = H.pack(tp, w, torch.bfloat16)

    def rejected(mutate, what):
        d = H.igemm_desc(tp, wp, H.tdesc(x), H.tdesc(out))
        mutate(d)
        assert lib.vsseg_igemm(C.byref(d), H.stream()) == L.EINVAL and b"transition kernel" in lib.vsseg_last_error(), what

    rejected(lambda d: setattr(d, "mtw", 8), "mtw")
    rejected(lambda d: setattr(d, "class_split", 4), "class_split")
    rejected(lambda d: setattr(d, "res_mode", L.RES_ADD), "residual epilogue")
    o32 = torch.zeros(1, 8, 16, 16, 48, dtype=torch.float32, device="cuda")
    d = H.igemm_desc(tp, wp, H.tdesc(x), H.tdesc(o32))
    assert lib.vsseg_igemm(C.byref(d), H.stream()) == L.EINVAL and b"bf16" in lib.vsseg_last_error()


DEEP_CASES = [
    # kind, kernel, stride, cin, cout, spatial size of the FINER side, mode, input split
    ("conv_fwd", (3, 3, 3), (1, 1, 1), 160, 80, (6, 8, 8), "stats", 80),       # level-4 decoder unit on the two-part concat
    ("conv_fwd", (3, 3, 3), (1, 1, 1), 96, 96, (12, 4, 16), "stats", 0),       # bottleneck
    ("conv_fwd", (3, 3, 3), (1, 1, 1), 80, 40, (5, 3, 7), "relu", 0),          # attention conv1 of the bottleneck, ragged lattice (partial tiles)
    ("conv_fwd", (3, 3, 3), (1, 1, 1), 40, 1, (6, 4, 8), "sigmoid", 0),        # attention conv2: one fp32 output channel
    ("conv_fwd", (1, 1, 1), (1, 1, 1), 80, 96, (6, 4, 8), "plain", 0),         # residual convolution: one K-step group per wave at most
    ("conv_fwd", (3, 3, 3), (2, 2, 2), 64, 64, (12, 8, 16), "stats", 0),       # strided convolution level 3 -> 4
    ("conv_fwd", (3, 3, 3), (1, 1, 1), 64, 80, (6, 8, 8), "residual", 0),
    ("conv_dgrad", (3, 3, 3), (1, 1, 1), 160, 80, (6, 8, 8), "accumulate", 0),  # K = 80 -> N = 160 = 2 x 5 tiles
    ("conv_dgrad", (1, 1, 1), (1, 1, 1), 128, 64, (6, 8, 8), "accumulate", 0),  # N = 128 over 3 x 3 tiles: the last channel tile is padding (no auxiliary read past the row)
    ("conv_dgrad", (3, 3, 3), (1, 1, 1), 80, 40, (6, 4, 8), "relumask", 0),
    ("conv_dgrad", (3, 3, 3), (1, 1, 1), 96, 96, (12, 4, 16), "gate", 0),
    ("convT_dgrad", (3, 3, 3), (2, 2, 2), 80, 64, (12, 8, 16), "plain", 0),
    ("convT_fwd", (3, 3, 3), (2, 2, 2), 96, 80, (8, 8, 8), "stats", 0),         # the parity classes: per class AND all in one launch
    ("convT_fwd", (3, 3, 3), (2, 2, 2), 80, 64, (12, 8, 16), "plain", 0),
    ("conv_dgrad", (3, 3, 3), (2, 2, 2), 64, 64, (12, 8, 16), "accumulate", 0),
    ("conv_dgrad", (3, 3, 3), (2, 2, 2), 80, 80, (7, 9, 6), "plain", 0),        # odd fine lattice: the classes with offset 1 are one voxel shorter
]


@pytest.mark.parametrize("kind,k,st,cin,cout,fine,mode,split", DEEP_CASES)
def test_deep_kernel_matches_definition_and_general_kernel(kind, k, st, cin, cout, fine, mode, split):
    """csrc/dconv.hip (launch plans with depth -7: the small launches of levels 3-5, ref:params/networks/nets/unet2d5_spvPA.py:56-89): every plan `planner.deep_plans` /
    `deep_class_plans` offers computes the convolution of torch's fp64 definition with each epilogue the network uses (bias, BatchNorm statistics, activations, residual /
    accumulate / ReLU mask / gated add, fp32 one-channel output, two-part input), on ragged lattices, with all parity classes in one launch — within ONE bf16
    rounding of the definition in every mode, as the general kernel is (the four waves split the K sum: not bit-identical to it by construction, so the two are
    compared through the definition); twice in a row gives identical bits."""
    lib = L.lib()
    dt, tdt, n = "bf16", torch.bfloat16, 2
    torch.manual_seed(29)
    transposed = kind.startswith("convT")
    strided = tuple(st) != (1, 1, 1)
    coarse = tuple((f + s - 1) // s for f, s in zip(fine, st))
    if transposed:
        w = _round(torch.randn(cin, cout, *k) / (cin * 27 / 8) ** 0.5, dt)
    else:
        w = _round(torch.randn(cout, cin, *k) / (cin * np.prod(k) / (8 if (strided and kind == "conv_dgrad") else 1)) ** 0.5, dt)
    pad = P.same_pad(k)
    if kind == "conv_fwd":
        x = _round(torch.randn(n, cin, *fine), dt)
        want = F.conv3d(x.double(), w.double(), stride=st, padding=pad)
        inp, nout, q, odims = x, cout, tuple(want.shape[2:]), tuple(want.shape[2:])
    elif kind == "convT_fwd":
        x = _round(torch.randn(n, cin, *coarse), dt)
        want = F.conv_transpose3d(x.double(), w.double(), stride=st, padding=1, output_padding=1)
        inp, nout, q, odims = x, cout, coarse, tuple(want.shape[2:])
    elif kind == "conv_dgrad":
        xd = torch.zeros(n, cin, *fine, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(xd, w.double(), stride=st, padding=pad)
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        want, inp, nout, q, odims = xd.grad, gy, cin, coarse if strided else fine, fine
    else:  # convT_dgrad: dX of a transposed convolution = the strided convolution of dY
        xd = torch.zeros(n, cin, *coarse, dtype=torch.float64, requires_grad=True)
        y = F.conv_transpose3d(xd, w.double(), stride=st, padding=1, output_padding=1)
        gy = _round(torch.randn(*y.shape), dt)
        y.backward(gy.double())
        want, inp, nout, q, odims = xd.grad, gy, cin, coarse, coarse
    kreal, nreal = P.gemm_dims(kind, tuple(w.shape))
    assert nreal == nout
    inp_cl = H.to_cl(inp, tdt, P.round_up(kreal, 8))
    parts = H._split_cl(inp_cl, split) if split else None
    xin = H.two_part(*parts) if parts else H.tdesc(inp_cl)
    f32out = mode == "sigmoid"
    bias = torch.randn(nout) * 0.2
    prev = H.to_cl(_round(torch.randn(n, nout, *odims), dt), tdt)
    side = H.to_cl(_round(torch.randn(n, nout, *odims), dt), tdt)
    gate = torch.rand(n, *odims, device="cuda")
    kw, ref = dict(bias=bias.cuda().data_ptr()), want + bias.double().view(1, -1, 1, 1, 1)
    keep = [bias]
    if mode == "accumulate":
        kw, ref = dict(accumulate=1), want + H.from_cl(prev).double()
    elif mode == "residual":
        kw.update(res=H.tdesc(side), res_mode=L.RES_ADD)
        ref = ref + H.from_cl(side).double()
    elif mode == "relumask":
        kw, ref = dict(res=H.tdesc(side), res_mode=L.RES_RELUMASK), want * (H.from_cl(side) > 0).double()
    elif mode == "gate":
        kw, ref = dict(res=H.tdesc(side), res_mode=L.RES_GATE, gate=gate.data_ptr()), want + H.from_cl(side).double() * (1.0 + gate.cpu().double()).unsqueeze(1)
    elif mode == "relu":
        kw["act"], ref = L.ACT_RELU, ref.clamp(min=0)
    elif mode == "sigmoid":
        kw["act"], ref = L.ACT_SIGMOID, torch.sigmoid(ref)
    bdev = bias.cuda()
    if "bias" in kw:
        kw["bias"] = bdev.data_ptr()
    aux_es = 2 if mode in ("accumulate", "residual", "relumask", "gate") else 0

    def fresh():
        if mode == "accumulate":
            return prev.clone()
        return torch.zeros(n, *odims, nout, dtype=torch.float32 if f32out else tdt, device="cuda")

    def stats_buf():
        return torch.zeros(L.STAT_SHARDS * 2 * P.round_up(nout, 16), dtype=torch.float64, device="cuda")

    def launch(plans):
        out, sb = fresh(), stats_buf()
        e = dict(kw, stats=sb.data_ptr(), stats_stride=P.round_up(nout, 16)) if mode == "stats" else kw
        for pl in plans:
            d = H.igemm_desc(pl, H.pack(pl, w, tdt), xin, H.tdesc(out), **e)
            L.check(lib.vsseg_igemm(C.byref(d), H.stream()), f"deep kernel {kind} tile={pl.tile} mt={pl.mtw} nt={pl.nt} ns={pl.nsplit} ck={pl.ck}")
        torch.cuda.synchronize()
        return out, H.stat_decode(sb).view(L.STAT_SHARDS, 2, -1).sum(0)

    classes = P.lattice_classes(kind, k, st)
    general, gstat = launch([P.plan_igemm(kind, tuple(w.shape), c_, q, 2, kc_pad=inp_cl.shape[-1], aux_es=aux_es, in_split=split) for c_ in classes])
    tol = 1e-4 * (float(ref.abs().max()) + 1e-12)  # of the fp32 one-channel output; the bf16 outputs are held to one rounding of the definition

    def meets_definition(out, what):
        if f32out:
            np.testing.assert_allclose(H.from_cl(out).numpy(), ref.float().numpy(), atol=tol, err_msg=what)
        else:
            assert_one_rounding(H.from_cl(out), ref, what=what)

    meets_definition(general, f"general kernel, {mode}")
    variants = []
    per_class = [P.deep_plans(kind, tuple(w.shape), c_, q, 2, inp_cl.shape[-1], nreal, kreal, n, split) for c_ in classes]
    assert all(per_class), "the deep-level kernel is offered for every lattice class of these shapes"
    for i in range(max(len(pc) for pc in per_class)):
        variants.append([pc[min(i, len(pc) - 1)] for pc in per_class])
    if len(classes) > 1:
        cps = P.deep_class_plans(kind, tuple(w.shape), k, st, q, 2, inp_cl.shape[-1], nreal, kreal, n)
        assert cps and all(pl.classes is not None and pl.depth == L.DEPTH_DEEP for pl in cps)
        variants += [[pl] for pl in cps]
    assert all(pl.depth == L.DEPTH_DEEP for v in variants for pl in v)
    for v in variants:
        tag = " | ".join(f"tile={pl.tile} mt={pl.mtw} nt={pl.nt} ns={pl.nsplit} ck={pl.ck} cls={len(pl.classes or [])}" for pl in v[:1])
        out, st_ = launch(v)
        meets_definition(out, f"deep kernel, {mode}, {tag}")
        assert not f32out or float((out.float() - general.float()).abs().max()) <= 2 * tol, tag  # (bf16: both are within one rounding of the definition)
        if mode == "stats":
            np.testing.assert_allclose(st_.cpu().numpy(), gstat.cpu().numpy(), rtol=2e-4, atol=2e-2, err_msg=tag)
            np.testing.assert_allclose(st_[0, :nout].cpu().numpy(), (want + bias.double().view(1, -1, 1, 1, 1)).sum((0, 2, 3, 4)).numpy(), rtol=2e-4, atol=5e-2, err_msg=tag)
        again, st2 = launch(v)
        assert torch.equal(again, out) and torch.equal(st2, st_), f"not run-to-run bit-identical: {tag}"


def test_deep_kernel_rejects_what_it_does_not_cover():
    """depth -7 outside the deep-level kernel's domain is an error with the reason in vsseg_last_error (no silent fallback)."""
    lib = L.lib()
    k = (3, 3, 3)
    w = torch.randn(48, 32, *k)
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]
    pl = P.deep_plans("conv_fwd", tuple(w.shape), cls, (8, 8, 8), 2, 32, 48, 32, 1)[0]
    x = torch.zeros(1, 8, 8, 8, 32, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, 8, 8, 8, 48, dtype=torch.bfloat16, device="cuda")
    wp = H.pack(pl, w, torch.bfloat16)
    d = H.igemm_desc(pl, wp, H.tdesc(x), H.tdesc(out))
    assert lib.vsseg_igemm(C.byref(d), H.stream()) == 0
    for field, val, why in (("mtw", 3, b"mtw"), ("cout_mod", 16, b"z-folded"), ("ck", 24, b"nchunks x ck")):
        bad = H.igemm_desc(pl, wp, H.tdesc(x), H.tdesc(out))
        setattr(bad, field, val)
        assert lib.vsseg_igemm(C.byref(bad), H.stream()) == L.EINVAL and why in lib.vsseg_last_error(), field
    xf = torch.zeros(1, 8, 8, 8, 32, device="cuda")
    bad = H.igemm_desc(pl, wp, H.tdesc(xf), H.tdesc(out))
    assert lib.vsseg_igemm(C.byref(bad), H.stream()) == L.EINVAL and b"bf16" in lib.vsseg_last_error()
    torch.cuda.synchronize()


def test_compute_kernel_rejects_what_it_does_not_cover():
    """depth -3 outside the compute kernel's domain is an error (no silent fallback to the general kernel)."""
    lib = L.lib()
    k, cin, cout, dims = (3, 3, 3), 32, 48, (8, 16, 24)  # 24 is not a multiple of the 16-voxel tile
    w = torch.randn(cout, cin, *k)
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]
    assert P.compute_plan("conv_fwd", tuple(w.shape), cls, dims, 2, cin, cout, cin) is None
    pl = P.plan_igemm("conv_fwd", tuple(w.shape), cls, dims, 2, kc_pad=cin)
    pl.pack_map = P.pack_map(pl, tuple(w.shape))
    x = torch.zeros(1, *dims, cin, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, *dims, cout, dtype=torch.bfloat16, device="cuda")
    d = H.igemm_desc(pl, H.pack(pl, w, x.dtype), H.tdesc(x), H.tdesc(out))
    d.depth = L.DEPTH_COMPUTE
    assert lib.vsseg_igemm(C.byref(d), H.stream()) == L.EINVAL
    assert b"compute kernel" in lib.vsseg_last_error()


def test_streaming_kernel_rejects_what_it_does_not_cover():
    """depth -2 on a launch outside the streaming kernel's domain is an error (no silent fallback to the general kernel)."""
    lib = L.lib()
    k, cin, cout, dims = (3, 3, 1), 16, 16, (12, 16, 8)  # 12 is not a multiple of the 8-voxel tile
    w = torch.randn(cout, cin, *k)
    cls = P.lattice_classes("conv_fwd", k, (1, 1, 1))[0]
    assert P.stream_plan("conv_fwd", tuple(w.shape), cls, dims, 2, cin, cout, cin) is None
    pl = P.plan_igemm("conv_fwd", tuple(w.shape), cls, dims, 2, kc_pad=cin, mtw=4)
    pl.pack_map = P.pack_map(pl, tuple(w.shape))
    x = torch.zeros(1, *dims, cin, dtype=torch.bfloat16, device="cuda")
    out = torch.zeros(1, *dims, cout, dtype=torch.bfloat16, device="cuda")
    d = H.igemm_desc(pl, H.pack(pl, w, x.dtype), H.tdesc(x), H.tdesc(out))
    d.depth = L.DEPTH_STREAM
    assert lib.vsseg_igemm(C.byref(d), H.stream()) == L.EINVAL
    assert b"streaming kernel" in lib.vsseg_last_error()


# ---------------------------------------------------------------------------------------------------------------
# two-part tensors: the skip-connection concat cat([skip, up], 1) (MONAI SkipConnection) addressed as a pair of dense
# tensors.  Every kernel that accepts one must give exactly what it gives on the materialised concatenation.
# ---------------------------------------------------------------------------------------------------------------
def _split_cl(t_cl, c0):
    return H._split_cl(t_cl, c0)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k,c0,c1,cout,dims,budget", [((3, 3, 1), 16, 16, 16, (16, 16, 8), None), ((3, 3, 3), 48, 48, 48, (8, 8, 8), None), ((3, 3, 3), 48, 48, 48, (8, 8, 8), 40 * 1024),
                                                      ((3, 3, 3), 80, 80, 80, (6, 2, 8), None), ((1, 1, 1), 32, 32, 32, (8, 8, 8), None)])
def test_two_part_input_forward_and_wgrad(k, c0, c1, cout, dims, budget, dt):
    torch.manual_seed(11)
    cin = c0 + c1
    x = _round(torch.randn(2, cin, *dims), dt)
    w = _round(torch.randn(cout, cin, *k) / (cin * np.prod(k)) ** 0.5, dt).double().requires_grad_(True)
    y = F.conv3d(x.double(), w, padding=P.same_pad(k))
    xa, xb = _split_cl(H.to_cl(x, H.DT[dt]), c0)
    out = torch.zeros(2, *dims, cout, dtype=H.DT[dt], device="cuda")
    kw = {"lds_budget": budget} if budget else {}
    keep = H.run_lattice_op("conv_fwd", w.detach().float(), (xa, xb), out, (1, 1, 1), **kw)
    if budget:
        assert keep[0][1].nchunks > 1 and c0 % keep[0][1].ck == 0  # several chunks, none straddling the split
    _check(dt, H.from_cl(out), y.detach(), "two-part input")
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    dw = H.run_wgrad(False, tuple(w.shape), k, (1, 1, 1), H.to_cl(gy, H.DT[dt]), (xa, xb), cout, cin)
    ref = w.grad.float()
    np.testing.assert_allclose(dw.numpy(), ref.numpy(), atol=(5e-5 if dt == "fp32" else 1e-4) * float(ref.abs().max()))


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k,c0,c1,cout,dims", [((3, 3, 1), 16, 16, 16, (16, 16, 8)), ((3, 3, 3), 48, 48, 48, (8, 8, 8)), ((3, 3, 3), 80, 80, 80, (6, 2, 8)), ((3, 3, 1), 32, 32, 2, (9, 8, 4))])
def test_two_part_output_dgrad_fresh_accumulate_and_relu_mask(k, c0, c1, cout, dims, dt):
    """The data gradient of a convolution whose input is the concat is written into the two operands' gradient tensors:
    fresh, then accumulated on top of earlier contributions, with the attention-ReLU mask as the residual operand."""
    torch.manual_seed(12)
    cin = c0 + c1
    w = _round(torch.randn(cout, cin, *k) / (cin * np.prod(k)) ** 0.5, dt)
    x = torch.zeros(2, cin, *dims, dtype=torch.float64, requires_grad=True)
    y = F.conv3d(x, w.double(), padding=P.same_pad(k))
    gy = _round(torch.randn(*y.shape), dt)
    y.backward(gy.double())
    want = x.grad
    gcl = H.to_cl(gy, H.DT[dt], P.round_up(cout, 8))
    da, db = torch.zeros(2, *dims, c0, dtype=H.DT[dt], device="cuda"), torch.zeros(2, *dims, c1, dtype=H.DT[dt], device="cuda")
    H.run_lattice_op("conv_dgrad", w, gcl, (da, db), (1, 1, 1))
    got = torch.cat([H.from_cl(da), H.from_cl(db)], 1)
    _check(dt, got, want, "two-part output, fresh")
    # accumulate + mask: operands pre-filled, result = old + dgrad * (mask > 0)
    old = _round(torch.randn(2, cin, *dims), dt)
    mask = _round(torch.randn(2, cin, *dims), dt)
    oa, ob = _split_cl(H.to_cl(old, H.DT[dt]), c0)
    ma, mb = _split_cl(H.to_cl(mask, H.DT[dt]), c0)
    H.run_lattice_op("conv_dgrad", w, gcl, (oa, ob), (1, 1, 1), accumulate=1)
    got = torch.cat([H.from_cl(oa), H.from_cl(ob)], 1)
    ref = old.double() + want
    _check(dt, got, ref, "two-part output, accumulate")  # ref = the stored bf16 value + the convolution: one rounding of the sum
    fa, fb = torch.zeros_like(da), torch.zeros_like(db)
    H.run_lattice_op("conv_dgrad", w, gcl, (fa, fb), (1, 1, 1), res_mode=L.RES_RELUMASK, res=H.two_part(ma, mb))
    got = torch.cat([H.from_cl(fa), H.from_cl(fb)], 1)
    ref = want * (mask.double() > 0)
    if dt == "bf16":
        assert_one_rounding(got, ref, what="two-part output, ReLU mask")
    else:
        np.testing.assert_allclose(got.numpy(), ref.float().numpy(), atol=_tol(dt, want))


@pytest.mark.parametrize("c0", [16, 48, 80])
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_two_part_attention_gate(dt, c0):
    lib = L.lib()
    torch.manual_seed(13)
    dims, n, c = (8, 8, 4), 2, 2 * c0
    x = _round(torch.randn(n, c, *dims), dt).double().requires_grad_(True)
    pre = torch.randn(n, 1, *dims, dtype=torch.float64, requires_grad=True)
    att = torch.sigmoid(pre)
    out = att * x + x
    gout = _round(torch.randn(n, c, *dims), dt)
    (out * gout.double()).sum().backward()
    xa, xb = _split_cl(H.to_cl(x, H.DT[dt]), c0)
    gcl = H.to_cl(gout, H.DT[dt])
    attd = att.detach().float().reshape(n, *dims).contiguous().cuda()
    o = torch.zeros(n, *dims, c, dtype=H.DT[dt], device="cuda")
    S = H.stream()
    L.check(lib.vsseg_att_apply_fwd(H.two_part(xa, xb), attd.data_ptr(), H.tdesc(o), S))
    old = _round(torch.randn(n, c, *dims), dt)
    da, db = _split_cl(H.to_cl(old, H.DT[dt]), c0)
    dpre = torch.zeros(n, *dims, 8, dtype=H.DT[dt], device="cuda")
    L.check(lib.vsseg_att_apply_bwd(H.two_part(xa, xb), attd.data_ptr(), H.tdesc(gcl), None, H.two_part(da, db), 1, H.tdesc(dpre), None, None, S))
    torch.cuda.synchronize()
    _check(dt, H.from_cl(o), out.detach(), "two-part att_apply_fwd")
    ref = old.double() + x.grad
    _check(dt, torch.cat([H.from_cl(da), H.from_cl(db)], 1), ref, "two-part att_apply_bwd dx (accumulated)")
    _check(dt, H.from_cl(dpre, 1), pre.grad, "two-part att_apply_bwd dpre")


def test_logits_gradient_staging_copy_fast_path_equals_the_generic_copy():
    """vsseg_copy_cast fp32 [voxel][2] -> bf16 rows of 8: with VSSEG_ZERO_PADDED the call writes whole rows (channels 2..7 = 0); without the flag it
    must leave the other channels of the row alone.  Same values either way."""
    lib = L.lib()
    torch.manual_seed(3)
    n, dims = 2, (5, 6, 7)
    src = torch.randn(n, *dims, 2, device="cuda")
    sd = L.Tensor(src.data_ptr(), L.F32, 2, 2, n, *dims)
    a = torch.full((n, *dims, 8), 7.0, device="cuda", dtype=torch.bfloat16)
    b = a.clone()
    L.check(lib.vsseg_copy_cast(sd, L.Tensor(a.data_ptr(), L.BF16, 2, 8, n, *dims), H.stream()), "copy")
    L.check(lib.vsseg_copy_cast(sd, L.Tensor(b.data_ptr(), L.BF16, 2, 8, n, *dims, None, 0, L.ZERO_PADDED), H.stream()), "copy (zero-padded rows)")
    torch.cuda.synchronize()
    assert torch.equal(a[..., :2], src.to(torch.bfloat16)) and torch.equal(b[..., :2], a[..., :2])
    assert float(a[..., 2:].float().min()) == 7.0 and float(b[..., 2:].float().abs().max()) == 0.0


def test_fork_event_bound_to_a_kernel_orders_a_second_stream():
    """vsseg_fork_arm / vsseg_fork_disarm / vsseg_stream_wait_event: the kernels a library call launches while an event is armed carry it as their stop event; a second stream
    that waits for it sees what they wrote (a 1 GB cast takes ~0.4 ms: a consumer that did not wait would copy the zeros in front of it); a call that launches no kernel reports 0."""
    lib = L.lib()
    n, dims = 4, (256, 128, 128)
    src = torch.randn(n, *dims, 16, device="cuda")
    mid = torch.zeros(n, *dims, 16, device="cuda", dtype=torch.bfloat16)
    out = torch.zeros_like(mid)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    ev = lib.vsseg_fork_event_create()
    assert ev
    torch.cuda.synchronize()
    L.check(lib.vsseg_fork_arm(ev))
    L.check(lib.vsseg_memset_zero(out.data_ptr(), 64, a.cuda_stream))
    assert lib.vsseg_fork_disarm() == 0  # a memset is not a kernel of the library
    L.check(lib.vsseg_fork_arm(ev))
    L.check(lib.vsseg_copy_cast(L.Tensor(src.data_ptr(), L.F32, 16, 16, n, *dims), L.Tensor(mid.data_ptr(), L.BF16, 16, 16, n, *dims), a.cuda_stream))
    assert lib.vsseg_fork_disarm() == 1
    assert lib.vsseg_fork_disarm() == 0  # nothing armed
    L.check(lib.vsseg_stream_wait_event(b.cuda_stream, ev))
    L.check(lib.vsseg_copy_cast(L.Tensor(mid.data_ptr(), L.BF16, 16, 16, n, *dims), L.Tensor(out.data_ptr(), L.BF16, 16, 16, n, *dims), b.cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(out, src.to(torch.bfloat16))
    assert lib.vsseg_fork_arm(None) == L.EINVAL
    L.check(lib.vsseg_fork_event_destroy(ev))


def test_two_part_tensors_are_rejected_where_unsupported():
    lib = L.lib()
    a = torch.zeros(1, 4, 4, 4, 16, device="cuda")
    t2 = H.two_part(a, a.clone())
    vec = torch.zeros(32, device="cuda")
    assert lib.vsseg_channel_sum(t2, vec.data_ptr(), H.stream()) == L.EINVAL
    assert lib.vsseg_copy_cast(t2, t2, H.stream()) == L.EINVAL
    assert b"two-part" in lib.vsseg_last_error()


@pytest.mark.parametrize("att", [True, False])
@pytest.mark.parametrize("hard", [True, False])
def test_dice_spvpa_loss_matches_reference_golden(att, hard):
    """Loss value and gradients against the golden captured from the REFERENCE's Dice_spvPA (tests/golden/loss.npz)."""
    import vs_seg_amd as V

    g = load("loss.npz")
    shape = (2, 1, 32, 32, 8)
    att_shapes = [(2, 1, 1, 1, 1), (2, 1, 2, 2, 2), (2, 1, 4, 4, 4), (2, 1, 8, 8, 8), (2, 1, 16, 16, 8), (2, 1, 32, 32, 8)]
    y = synth_label(31, shape).cuda()
    logits = (2.0 * synth_input(32, (2, 2, 32, 32, 8))).cuda().requires_grad_(True)
    atts = [torch.sigmoid(synth_input(40 + i, s)).cuda().requires_grad_(True) for i, s in enumerate(att_shapes)] if att else []
    loss = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=hard)((logits, atts), y)
    assert loss.dim() == 0
    loss.backward()
    tag = f"att{int(att)}_hard{int(hard)}"
    assert abs(loss.item() - float(g[tag + ":loss"])) < 5e-6
    np.testing.assert_allclose(logits.grad.cpu().numpy(), g[tag + ":dlogits"], atol=2e-9, rtol=2e-4)
    for i, a in enumerate(atts):
        np.testing.assert_allclose(a.grad.cpu().numpy(), g[f"{tag}:datt{i}"], atol=2e-9, rtol=2e-4)


@pytest.mark.parametrize("layout", ["bf16x2", "bf16x8", "f32x2", "f32x8"])
@pytest.mark.parametrize("nvox_dims", [(32, 32, 8), (5, 3, 7)])  # (16-byte loads, four voxels per thread) / (odd voxel count: the scalar path)
def test_dice_gradient_written_in_the_staged_layouts_equals_the_fp32_gradient_cast(layout, nvox_dims):
    """vsseg_dice_pred_bwd_to (the fused train step) = vsseg_dice_pred_bwd followed by vsseg_copy_cast, bit for bit, in every layout the training plan stages the gradient in."""
    lib = L.lib()
    n, dims = 2, nvox_dims
    nvox = dims[0] * dims[1] * dims[2]
    lg = (2.0 * synth_input(32, (n, *dims, 2))).cuda().contiguous()
    lab = synth_label(31, (n, 1, *dims)).cuda().contiguous()
    coef = torch.tensor([-0.3, 0.02, -0.25, 0.015, -0.31, 0.021, -0.2, 0.017], device="cuda")
    want32 = torch.empty(n, *dims, 2, device="cuda")
    L.check(lib.vsseg_dice_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), None, want32.data_ptr(), H.stream()))
    dt = torch.bfloat16 if layout.startswith("bf16") else torch.float32
    pitch = int(layout[-1])
    got = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    want = torch.full((n, *dims, pitch), 7.0, device="cuda", dtype=dt)
    tdt = L.BF16 if dt == torch.bfloat16 else L.F32
    flags = L.ZERO_PADDED if pitch == 8 else 0
    L.check(lib.vsseg_copy_cast(L.Tensor(want32.data_ptr(), L.F32, 2, 2, n, *dims), L.Tensor(want.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    L.check(lib.vsseg_dice_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 2, pitch, n, *dims, None, 0, flags), H.stream()))
    torch.cuda.synchronize()
    assert torch.equal(got[..., :2], want[..., :2])
    if pitch == 8:  # bf16 rows are written whole (channels 2..7 = 0, as the cast pass writes them); fp32 rows keep what was there
        assert torch.equal(got[..., 2:], want[..., 2:]) if dt == torch.bfloat16 else float(got[..., 2:].min()) == 7.0
    # a destination that is not a 2-channel tensor of the right size is refused
    assert lib.vsseg_dice_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), n, nvox, 1, coef.data_ptr(), None, L.Tensor(got.data_ptr(), tdt, 3, pitch, n, *dims), H.stream()) == L.EINVAL


@pytest.mark.parametrize("att", [True, False])
def test_dice_loss_and_gradients_in_one_call_equal_the_autograd_route(att):
    """Dice_spvPA.forward_backward_into (outside autograd, gradients written into caller-named buffers) = loss.backward(): same loss, same gradients."""
    import vs_seg_amd as V

    shape = (2, 1, 32, 32, 8)
    att_shapes = [(2, 1, 1, 1, 1), (2, 1, 2, 2, 2), (2, 1, 4, 4, 4), (2, 1, 8, 8, 8), (2, 1, 16, 16, 8), (2, 1, 32, 32, 8)]
    y = synth_label(31, shape).cuda()
    lg_cl = (2.0 * synth_input(32, (2, 32, 32, 8, 2))).cuda()
    logits = lg_cl.permute(0, 4, 1, 2, 3).detach().requires_grad_(True)  # channels-last storage, as the network hands it out
    atts = [torch.sigmoid(synth_input(40 + i, s)).cuda().requires_grad_(True) for i, s in enumerate(att_shapes)]
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=att, hardness_weighting=True)
    loss = fn((logits, atts), y)
    loss.backward()
    dst = torch.zeros(2, 32, 32, 8, 2, device="cuda", dtype=torch.bfloat16)
    bufs = [torch.zeros(s[0], *s[2:], device="cuda") for s in att_shapes]
    bufs[2] = None  # a map without a gradient path is skipped
    loss2, written = fn.forward_backward_into((logits.detach(), [a.detach() for a in atts]), y, (L.Tensor(dst.data_ptr(), L.BF16, 2, 2, 2, 32, 32, 8), bufs))
    assert float(loss2) == float(loss)
    assert torch.equal(dst, logits.grad.permute(0, 2, 3, 4, 1).to(torch.bfloat16))
    assert written == ([5, 4, 3, 1, 0] if att else [])
    for i in written:
        assert torch.equal(bufs[i].reshape(-1), atts[i].grad.reshape(-1))


@pytest.mark.parametrize("shape,att_dims", [((2, 1, 32, 32, 8), [(1, 1, 1), (2, 2, 2), (4, 4, 4), (8, 8, 8), (16, 16, 8), (32, 32, 8)]),  # two fused levels + a tail of four
                                            ((1, 1, 24, 8, 12), [(3, 1, 3), (6, 2, 6), (12, 4, 12), (24, 8, 12)]),                       # one fused level + a tail of three
                                            ((2, 1, 16, 16, 4), [(8, 8, 4), (16, 16, 4)])])                                                # one fused level + a tail that is the pooled label itself
def test_dice_fused_passes_equal_the_pass_per_level_sequence(shape, att_dims, monkeypatch):
    """vsseg_dice_level_sums / vsseg_dice_tail_sums / vsseg_dice_att_bwd_levels (fewer passes, fewer launches) against the generic sequence pred_sums + per level maxpool /
    att_sums / att_bwd: same loss and gradients up to the fp32 partial sums of a thread (the sums themselves are fixed-point: order-independent)."""
    import vs_seg_amd as V
    from vs_seg_amd.losses import dice_spvPA as D

    B = shape[0]
    y = synth_label(31, shape).cuda()
    lg_cl = (2.0 * synth_input(32, (B, *shape[2:], 2))).cuda()
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    res = []
    for generic in (False, True):
        if generic:
            monkeypatch.setattr(D, "_fused_plan", lambda *a, **k: None)
        else:
            assert D._fused_plan(B, shape[2:], [(B, 1, *d) for d in att_dims], lg_cl, y, []) is not None
        logits = lg_cl.permute(0, 4, 1, 2, 3).detach().requires_grad_(True)
        atts = [torch.sigmoid(synth_input(40 + i, (B, 1, *d))).cuda().requires_grad_(True) for i, d in enumerate(att_dims)]
        loss = fn((logits, atts), y)
        loss.backward()
        dst = torch.zeros(B, *shape[2:], 2, device="cuda")
        bufs = [torch.zeros(B, *d, device="cuda") for d in att_dims]
        loss2, written = fn.forward_backward_into((logits.detach(), [a.detach() for a in atts]), y, (L.Tensor(dst.data_ptr(), L.F32, 2, 2, B, *shape[2:]), bufs))
        assert float(loss2) == float(loss) and sorted(written) == list(range(len(att_dims)))
        assert torch.equal(dst, logits.grad.permute(0, 2, 3, 4, 1))
        for i in written:
            assert torch.equal(bufs[i].reshape(-1), atts[i].grad.reshape(-1))
        res.append((float(loss), logits.grad.clone(), [a.grad.clone() for a in atts]))
    assert abs(res[0][0] - res[1][0]) < 2e-6
    np.testing.assert_allclose(res[0][1].cpu().numpy(), res[1][1].cpu().numpy(), rtol=2e-5, atol=1e-10)
    for a, b in zip(res[0][2], res[1][2]):
        np.testing.assert_allclose(a.cpu().numpy(), b.cpu().numpy(), rtol=2e-5, atol=1e-10)


def test_adam_matches_torch_golden():
    g = load("adam.npz")
    lib = L.lib()
    p = torch.from_numpy(g["p0"].copy()).cuda()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step, gr in enumerate(g["grads"], 1):
        gd = torch.from_numpy(gr.copy()).cuda()
        L.check(lib.vsseg_adam(p.data_ptr(), gd.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), 1e-4, 0.9, 0.999, 1e-8, 1e-7, 1 - 0.9**step, 1 - 0.999**step, 1.0, H.stream()))
        np.testing.assert_allclose(p.cpu().numpy(), g["after"][step - 1], atol=2e-7, rtol=1e-6)


@pytest.mark.parametrize("vol,roi,ov,mode,swb", [((40, 36, 20), (16, 16, 32), 0.5, "gaussian", 1), ((48, 40, 24), (32, 16, 16), 0.25, "gaussian", 3), ((20, 20, 20), (16, 16, 8), 0.25, "constant", 2)])
def test_sliding_window_blend_matches_oracle(vol, roi, ov, mode, swb):
    """Same (cheap, deterministic) predictor on both sides: isolates window indexing, Gaussian map, blend, normalise, crop."""
    import vs_seg_amd as V

    torch.manual_seed(7)
    x = torch.randn(2, 1, *vol)

    def pred(w):
        return torch.cat([w * 2.0 + 1.0, torch.tanh(w) - 0.5], 1)

    want, starts = O.sliding_window_inference(x, roi, swb, pred, overlap=ov, mode=mode, return_windows=True)
    got = V.sliding_window_inference(x.cuda(), roi, swb, pred, overlap=ov, mode=mode)
    assert tuple(got.shape) == tuple(want.shape)
    np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), atol=2e-6, rtol=2e-6)
    from vs_seg_amd.inferers import importance_map, window_geometry

    assert window_geometry(vol, roi, ov)[4] == starts  # bit-exact patch indexing
    if mode == "gaussian":
        r = window_geometry(vol, roi, ov)[0]
        np.testing.assert_array_equal(importance_map(r, "gaussian", "cpu").numpy(), O.gaussian_importance_map(r).numpy())


@pytest.mark.parametrize("vol,roi,ov,nwin", [((512, 512, 120), (384, 128, 128), 0.5, 14), ((512, 512, 120), (384, 384, 64), 0.25, 12)])
def test_sliding_window_full_size_properties(vol, roi, ov, nwin):
    """BASELINE.json's inference volume (512x512x120) with the benchmark roi and with the reference-native roi.  Size-independent
    properties of the blend: a predictor that is voxel-wise (its output at a voxel depends on that voxel only) must come back
    un-blended whatever the window grid (sum_w imap*f(x) / sum_w imap = f(x)); the window table equals SURVEY App. B.2; the
    output is independent of sw_batch_size bit for bit (windows are blended sequentially in reference order)."""
    import vs_seg_amd as V
    from vs_seg_amd.inferers import window_geometry

    _, padded, pad_before, _, starts = window_geometry(vol, roi, ov)
    assert len(starts) == nwin
    if roi == (384, 128, 128):
        assert starts == [(x, y, 0) for x in (0, 128) for y in range(0, 385, 64)] and padded == (512, 512, 128) and tuple(pad_before) == (0, 0, 4)
    else:
        assert starts == [(x, y, z) for x in (0, 128) for y in (0, 128) for z in (0, 48, 56)]
    torch.manual_seed(8)
    x = torch.randn(1, 1, *vol, device="cuda")

    def pred(w):
        return torch.cat([w * 2.0 + 1.0, torch.tanh(w) - 0.5], 1)

    out1 = V.sliding_window_inference(x, roi, 1, pred, overlap=ov, mode="gaussian")
    assert tuple(out1.shape) == (1, 2, *vol)
    np.testing.assert_allclose(out1.cpu().numpy(), pred(x).cpu().numpy(), atol=3e-6, rtol=3e-6)
    out4 = V.sliding_window_inference(x, roi, 4, pred, overlap=ov, mode="gaussian")
    assert torch.equal(out1, out4)
    # a window-dependent predictor: constant 1 per window in channel 0, window centre weight dominates -> stays within [min,max] (convexity)
    k = [0]

    def pred_idx(w):
        k[0] += 1
        return torch.cat([torch.full_like(w, float(k[0])), torch.zeros_like(w)], 1)

    o = V.sliding_window_inference(x, roi, 1, pred_idx, overlap=ov, mode="gaussian")
    assert k[0] == nwin and float(o[:, 0].min()) >= 1.0 - 1e-5 and float(o[:, 0].max()) <= nwin + 1e-4 and float(o[:, 1].abs().max()) == 0.0


def test_hard_dice_matches_oracle():
    import vs_seg_amd as V

    torch.manual_seed(8)
    logits = torch.randn(1, 2, 24, 20, 12)
    label = synth_label(3, (1, 1, 24, 20, 12))
    want = O.compute_dice_score(logits, label)
    got = V.compute_dice_score(logits.cuda(), label.cuda())
    assert tuple(got.shape) == (1, 1)
    assert abs(float(got) - float(want)) < 1e-6
