"""CPU tests of tests/rounding.py: the bar the bf16 kernel tests apply accepts a correct kernel model and rejects each subtle error.

Kernel model: fp32 accumulation of bf16 operands, the epilogue PReLU(acc * scale + shift) + residual in fp32, ONE round-to-nearest-even to bf16.
The planted errors are the ones a performance change introduces: a truncating store, a rounding in front of the residual add, a running sum
kept in bf16 between 16-channel chunks, one dropped product of the K sum, one element off by one bf16 ulp.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.rounding import assert_one_rounding, rne_bf16

CONVS = [  # tests/test_gpu_ops.py CONVS
    ((3, 3, 1), (1, 1, 1), 16, 16, (16, 16, 8)),
    ((3, 3, 3), (1, 1, 1), 32, 48, (8, 8, 8)),
    ((1, 1, 1), (1, 1, 1), 32, 16, (8, 8, 8)),
    ((3, 3, 1), (2, 2, 1), 16, 16, (16, 16, 4)),
    ((3, 3, 3), (2, 2, 2), 48, 48, (8, 8, 8)),
    ((3, 3, 3), (1, 1, 1), 40, 1, (4, 4, 8)),
    ((3, 3, 1), (1, 1, 1), 32, 2, (8, 8, 4)),
    ((3, 3, 3), (1, 1, 1), 160, 80, (6, 2, 8)),
    ((3, 3, 3), (1, 1, 1), 96, 96, (3, 1, 4)),
]
ALPHA = 0.2


def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def _trunc(x):  # fp32 -> bf16 by dropping the low 16 bits
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


class Case:
    def __init__(self, k, s, cin, cout, dims):
        torch.manual_seed(1)
        self.k, self.s, self.cin, self.pad = k, s, cin, tuple(kk // 2 for kk in k)
        self.x = _bf(torch.randn(2, cin, *dims))
        self.w = _bf(torch.randn(cout, cin, *k) / (cin * np.prod(k)) ** 0.5)
        self.scale, self.shift = (torch.rand(cout) + 0.5).view(1, -1, 1, 1, 1), torch.randn(cout).view(1, -1, 1, 1, 1)
        pre = F.conv3d(self.x.double(), self.w.double(), stride=s, padding=self.pad)
        self.res = _bf(torch.randn(*pre.shape))
        v = pre * self.scale.double() + self.shift.double()
        self.ref = torch.where(v > 0, v, ALPHA * v) + self.res.double()

    def acc(self, w=None, chunk_round=None):
        """The fp32 accumulator; chunk_round: the running sum is stored through it after every 16-channel chunk."""
        w = self.w if w is None else w
        if chunk_round is None:
            return F.conv3d(self.x, w, stride=self.s, padding=self.pad)
        a = None
        for c0 in range(0, self.cin, 16):
            p = F.conv3d(self.x[:, c0:c0 + 16], w[:, c0:c0 + 16], stride=self.s, padding=self.pad)
            a = chunk_round(p if a is None else a + p)
        return a

    def epilogue(self, a, store=_bf, round_before_residual=False):
        v = a * self.scale + self.shift
        v = torch.where(v > 0, v, ALPHA * v)
        if round_before_residual:
            v = _bf(v)
        return store(v + self.res)


@pytest.fixture(scope="module", params=CONVS, ids=lambda c: f"{c[2]}to{c[3]}_k{''.join(map(str, c[0]))}_s{c[1][0]}")
def case(request):
    return Case(*request.param)


def test_fp32_accumulation_with_one_rounding_passes(case):
    share = assert_one_rounding(case.epilogue(case.acc()), case.ref, what="emulation")
    assert share < 1e-2  # (for the record: 0 to 1.3e-4 at these shapes)


def _violations(got, ref):
    with pytest.raises(AssertionError, match="outside one rounding") as err:
        assert_one_rounding(got, ref, what="planted")
    return str(err.value)


def test_truncating_store_is_rejected(case):
    msg = _violations(case.epilogue(case.acc(), store=_trunc), case.ref)
    assert " 0 away from zero" in msg and "one-sided" in msg  # towards zero, never away from it


def test_rounding_before_the_residual_add_is_rejected(case):
    assert "two-sided" in _violations(case.epilogue(case.acc(), round_before_residual=True), case.ref)


def test_bf16_partial_sums_between_channel_chunks_are_rejected(case):
    _violations(case.epilogue(case.acc(chunk_round=_bf)), case.ref)


def test_one_dropped_product_is_rejected(case):
    w = case.w.clone()
    w[:, 0, case.k[0] // 2, case.k[1] // 2, case.k[2] // 2] = 0.0  # the centre tap of channel 0: never padding
    _violations(case.epilogue(case.acc(w=w)), case.ref)


@pytest.mark.parametrize("step", [1, -1])
def test_one_element_off_by_one_ulp_in_65536_is_rejected(step):
    c = Case(*CONVS[0])
    got = case_out = c.epilogue(c.acc())
    assert got.numel() == 65536
    assert_one_rounding(got, c.ref, what="before the plant")
    # an element whose fp64 value lies close to a bf16 value (the interval of one that lies close to a tie holds both neighbours by design)
    r = rne_bf16(c.ref)
    ulp = torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.frexp(c.ref)[1].double() - 8.0)
    dist = ((c.ref - r).abs() / ulp).masked_fill(c.ref.abs() < 0.25 * c.ref.abs().max(), 1.0)
    i = int(dist.reshape(-1).argmin())
    bits = case_out.to(torch.bfloat16).reshape(-1).clone()
    moved = bits.view(torch.int16)
    moved[i] += step  # the neighbouring bf16 value
    msg = _violations(moved.view(torch.bfloat16).reshape(got.shape), c.ref)
    assert msg.startswith("planted: 1 of 65536")


def test_rne_bf16_equals_the_cast_on_fp32_inputs():
    torch.manual_seed(3)
    x = torch.randn(200000) * torch.pow(2.0, torch.randint(-60, 60, (200000,)).float())
    x = torch.cat([x, torch.tensor([0.0, -0.0, 1.0, -1.0, 3.3895313892515355e38, -3.3895313892515355e38, 3.4e38, 1e-39, -1e-40, 2.0 ** -133, 2.0 ** -134, 1.5 * 2.0 ** -133])])
    want = x.to(torch.bfloat16).double()
    got = rne_bf16(x.double())
    assert torch.equal(got, want)
    assert torch.equal(torch.signbit(got), torch.signbit(want))


def test_rne_bf16_ties_go_to_even_and_nothing_is_rounded_twice():
    e = torch.pow(torch.tensor(2.0, dtype=torch.float64), torch.arange(-20, 21, dtype=torch.float64)).view(-1, 1)
    k = torch.arange(128, 256, dtype=torch.float64).view(1, -1)  # 8-bit significands
    for sign in (1.0, -1.0):
        tie = sign * (k + 0.5) * e
        even = sign * torch.where(k % 2 == 0, k, k + 1) * e  # down where k is even, up where it is odd
        assert torch.equal(rne_bf16(tie), even)
        assert torch.equal(tie.float().to(torch.bfloat16).double(), even)  # (ties are fp32 values: the cast agrees)
        # 2^-40 beyond the tie: fp64 sees it, a cast through fp32 rounds it onto the tie first and then to even
        assert torch.equal(rne_bf16(tie + sign * e * 2.0 ** -40), sign * (k + 1) * e)
        assert torch.equal(rne_bf16(tie - sign * e * 2.0 ** -40), sign * k * e)
        twice = (tie + sign * e * 2.0 ** -40).float().to(torch.bfloat16).double()
        assert not torch.equal(twice, sign * (k + 1) * e)


def test_non_finite_outputs_fail():
    ref = torch.linspace(-1, 1, 64, dtype=torch.float64)
    good = ref.to(torch.bfloat16)
    assert_one_rounding(good, ref, what="finite")
    for bad in (float("nan"), float("inf")):
        g = good.clone()
        g[5] = bad
        with pytest.raises(AssertionError, match="1 non-finite"):
            assert_one_rounding(g, ref, what="non-finite")
