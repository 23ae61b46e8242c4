"""-m gpu: the weight-gradient kernels (vsseg_wgrad with the tile kernel, march = 1, march = 2, and vsseg_wgrad_narrow) against the exact-integer oracle
of tests/wgrad_oracle.py, bit for bit.

Operands are non-zero integers of magnitude <= 2 (gate maps {0, 1}), so every partial sum of a weight gradient is an integer below 2^24 and exact in fp32
in any summation order: the fp64 definition is the only admissible answer and every assertion here is an equality.  A mismatch is a finding about a
kernel; its message counts the differing elements and names (tap, cP, cH, got, want) of the first few.  tests/test_wgrad_host.py proves on the host that
the rows reach the launch paths they name and that the equality check trips on planted faults."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import gpu_harness as H  # noqa: E402
from tests import wgrad_oracle as O  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

ES = {"fp32": 4, "bf16": 2}


def _key(case):
    return (case.k, case.s, case.cin, case.cout, case.dims, case.tr, case.batch)


@functools.lru_cache(maxsize=None)
def _operands(key):
    k, s, cin, cout, dims, tr, batch = key
    return O.operands(O.Case("", k, s, cin, cout, dims, tr=tr, batch=batch))


@functools.lru_cache(maxsize=None)
def _want(key, calls, gate, acc):
    """(dW, dbias) after `calls` launches, computed once per problem and left unchanged."""
    k, s, cin, cout, dims, tr, batch = key
    ops = _operands(key)
    return O.expected(O.Case("", k, s, cin, cout, dims, tr=tr, batch=batch), ops, calls=calls, gate=gate, dw0=ops["dw0"] if acc else None, db0=ops["db0"] if acc else 0.0)


@functools.lru_cache(maxsize=8)
def _device(key, dt):
    """P and H as the kernels read them: channels-last, channels zero-padded to the stored pitch."""
    ops = _operands(key)
    cp, ch = ops["p"].shape[1], ops["h"].shape[1]
    return H.to_cl(ops["p"], H.DT[dt], O.P.round_up(cp, 8)), H.to_cl(ops["h"], H.DT[dt], O.P.round_up(ch, 8))


def _launch(case, dt, **kw):
    p_cl, h_cl = _device(_key(case), dt)
    if case.compact_p:
        p_cl = p_cl[..., :case.cp].contiguous()
    h = H._split_cl(h_cl, case.split) if case.split else h_cl
    return H.run_wgrad(case.tr, case.wshape, case.k, case.s, p_cl, h, case.cp, case.ch, **kw)


def _run(case, dt, **kw):
    """One row: launch, compare dw (and dbias) with the oracle; rows with `acc` start from non-zero integers and launch twice.  Returns the failure messages."""
    key, ops, msgs = _key(case), _operands(_key(case)), []
    db = torch.zeros(case.cp, dtype=torch.float32, device="cuda") if case.dbias else None
    dw = None
    for call in range(2 if case.acc else 1):
        start = {} if not case.acc else {"dw0": ops["dw0"], "dbias0": ops["db0"]} if call == 0 else {"dw0": dw}
        dw = _launch(case, dt, dbias=db, **start, **kw)
        want_dw, want_db = _want(key, call + 1, case.gate, case.acc)
        for got, want, what in ((dw, want_dw, "dw"), (db, want_db, "dbias")):
            if got is None:
                continue
            try:
                O.assert_exact(got, want, f"{case.id} [{dt}] {what} after call {call + 1}")
            except AssertionError as e:
                msgs.append(str(e))
    return msgs


def _tile_kw(case, dt):
    m = O.tile_launch(case, ES[dt])
    return dict(hgroup=case.hgroup, single_buffer=case.single_buffer, blocks=case.blocks, scratch_elems=m["scratch"] if case.scratch_wgs else None)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", O.TILE_CASES, ids=lambda c: c.id)
def test_tile_kernel_layer_shapes(case, dt):
    """csrc/wgrad.hip over the layer shapes of the network: every kernel size and stride, both transposed layers, batch 1 / 2 / 3, narrow channel counts stored
    as one 8-channel group, 3 / 5 / 10 chunks of H under a request of hgroup 4, a two-part H split inside a group, whole and ragged tiles, the bias gradient,
    and accumulation into a non-zero dw / dbias over two launches."""
    msgs = _run(case, dt, **_tile_kw(case, dt))
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("sb", O.SWEEP_BUFFERS)
@pytest.mark.parametrize("hg", O.SWEEP_HGROUPS)
@pytest.mark.parametrize("prob", sorted(O.SWEEP_PROBLEMS))
def test_tile_kernel_launch_shapes(prob, hg, sb, dt):
    """One problem under every launch shape of O.SWEEP_POINTS: persistent_blocks below, at and above the tile count and around the multiples of 8 the
    XCD-contiguous walk needs, a scratch that holds exactly 1, 2 and 3 workgroups, 4 to 256 slabs through every regime of vsseg_slab_sum4.  The answer
    does not depend on any of it."""
    msgs = []
    for case in O.sweep_cases(prob, ES[dt], hg, sb):
        msgs += _run(case, dt, **_tile_kw(case, dt))
    assert not msgs, "\n".join(msgs)


def _march_rows():
    return O.MARCH_HAND_CASES + O.march_planner_cases()


@pytest.mark.parametrize("case", _march_rows(), ids=lambda c: c.id)
def test_marching_kernel(case):
    """csrc/mwgrad.hip: every instantiation of planner.MARCH_WGRAD_SHAPES on a hand tile, every tile planner.march_wgrad_tiles returns at q[0] = 17 (two x
    segments, the last one ragged), a two-part H, the compact two-channel P, the gated H operand against the gated definition, dbias where cout >= 16."""
    kw = {}
    if case.gate:
        kw["h_gate"] = _operands(_key(case))["gate"].to(torch.float32).contiguous().cuda()
    msgs = _run(case, "bf16", march_tile=case.tile, **kw)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", O.COMPUTE_CASES, ids=lambda c: c.id)
def test_compute_kernel(case):
    """csrc/cwgrad.hip: every wave-role split, with and without the bias gradient, a two-part H, batch 1 / 2 / 3; two runs are bit-identical."""
    msgs = _run(case, "bf16", compute=case.compute, blocks=case.blocks)
    assert not msgs, "\n".join(msgs)
    again = _launch(case, "bf16", compute=case.compute, blocks=case.blocks)
    assert torch.equal(again, _want(_key(case), 1, False, False)[0].float())


def _narrow(case, dt, calls=2):
    """vsseg_wgrad_narrow on the operands of a case with one input or one output channel, accumulating `calls` times on top of non-zero integers."""
    lib = L.lib()
    key = _key(case)
    ops = _operands(key)
    x, gy = H.to_cl(ops["x"], H.DT[dt]), H.to_cl(ops["dy"], H.DT[dt])  # compact: the one-channel field has pitch 1
    # 1 -> C: t = dY, s = x, sign +1: dw[c][0][tap];  C -> 1: t = x, s = dY, sign -1: dw[0][c][tap]
    t_cl, s_cl, sign = (gy, x, 1) if case.cin == 1 else (x, gy, -1)
    dw = ops["dw0"].to(torch.float32).cuda()
    db = torch.full((1,), ops["db0"], device="cuda") if case.dbias else None
    scr = torch.zeros(1 << 20, device="cuda")
    msgs = []
    for call in range(calls):
        L.check(lib.vsseg_wgrad_narrow(H.tdesc(t_cl), s_cl.data_ptr(), case.k[0], sign, dw.data_ptr(), case.k[0] * case.k[1], db.data_ptr() if db is not None else None, scr.data_ptr(), scr.numel(),
                                       H.stream()), "wgrad_narrow")
        torch.cuda.synchronize()
        want_dw, want_db = _want(key, call + 1, False, True)
        for got, want, what in ((dw, want_dw, "dw"), (db, want_db, "dbias")):
            if got is None:
                continue
            try:
                O.assert_exact(got, want, f"{case.id} [{dt}] {what} after call {call + 1}")
            except AssertionError as e:
                msgs.append(str(e))
    return msgs


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("case", O.NARROW_CASES, ids=lambda c: c.id)
def test_narrow_reduction(case, dt):
    """csrc/wgrad_narrow.hip: 1 -> C and C -> 1, 3x3x1 and 1x1x1, batch 1 / 2 / 3, odd x and z extents with an odd count of four-row groups in y, the bias
    gradient of C -> 1, two accumulating calls on top of a non-zero dw."""
    msgs = _narrow(case, dt)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", O.NARROW_REFUSED, ids=lambda c: c.id)
def test_narrow_reduction_refuses_a_y_extent_that_is_no_multiple_of_four(case):
    """All three extents odd lies outside the kernel's domain (a thread owns four y-consecutive voxels): an error, never another kernel."""
    with pytest.raises(L.VssegError, match="must be a multiple of 4"):
        _narrow(case, "bf16", calls=1)
