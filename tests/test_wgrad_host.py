"""CPU checks of the exact-integer weight-gradient oracle (tests/wgrad_oracle.py) and of its case tables: the two definitions agree, planted faults
trip the equality check tests/test_gpu_wgrad_exact.py uses, every row of the tables reaches the launch paths it names (a host mirror of the launch
arithmetic of csrc/wgrad.hip, mwgrad.hip and cwgrad.hip), and the marching rows cover planner.MARCH_WGRAD_SHAPES.  No GPU."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from tests import wgrad_oracle as O
from vs_seg_amd import planner as P

ES = {"fp32": 4, "bf16": 2}


def _autograd(case, ops):
    pad = P.same_pad(case.k)
    x = ops["x"]
    if case.tr:
        w = torch.zeros(case.cin, case.cout, *case.k, dtype=torch.float64, requires_grad=True)
        opad = tuple(s + 2 * p - (k - 1) - 1 for s, p, k in zip(case.s, pad, case.k))
        y = F.conv_transpose3d(x, w, stride=case.s, padding=pad, output_padding=opad)
    else:
        w = torch.zeros(case.cout, case.cin, *case.k, dtype=torch.float64, requires_grad=True)
        y = F.conv3d(x, w, stride=case.s, padding=pad)
    assert tuple(y.shape[2:]) == case.ydims
    y.backward(ops["dy"])
    return w.grad


DEFINITION_CASES = [O._c(f"def-{i}", k, s, cin, cout, dims, tr=tr, batch=b) for i, (k, s, cin, cout, dims, tr, b) in enumerate([
    (O.K331, O.S1, 3, 5, (5, 4, 3), False, 1), (O.K333, O.S1, 4, 3, (3, 5, 4), False, 3), (O.K111, O.S1, 5, 2, (3, 2, 4), False, 3),
    (O.K331, (2, 2, 1), 3, 4, (7, 6, 3), False, 1), (O.K333, (2, 2, 2), 2, 3, (5, 6, 7), False, 3), (O.K111, (2, 2, 2), 3, 2, (5, 4, 3), False, 1),
    (O.K331, (2, 2, 1), 4, 3, (4, 3, 2), True, 3), (O.K333, (2, 2, 2), 3, 2, (3, 2, 3), True, 1), (O.K333, O.S1, 2, 3, (3, 4, 2), True, 3), (O.K111, (2, 2, 1), 2, 2, (3, 3, 2), True, 1)])]


@pytest.mark.parametrize("case", DEFINITION_CASES, ids=lambda c: f"{c.id}-k{c.k}-s{c.s}-tr{int(c.tr)}-b{c.batch}")
def test_shift_and_sum_equals_autograd(case):
    """The oracle's definition (slicing only) against fp64 autograd of F.conv3d / F.conv_transpose3d: equal exactly (both are integer sums in fp64)."""
    ops = O.operands(case)
    dw, db = O.expected(case, ops)
    assert torch.equal(dw, _autograd(case, ops))
    if not case.tr:
        assert torch.equal(db, ops["dy"].sum((0, 2, 3, 4)))
    dw0 = ops["dw0"]
    dw2, db2 = O.expected(case, ops, calls=2, dw0=dw0, db0=5.0)
    assert torch.equal(dw2, dw0 + 2 * dw) and torch.equal(db2, 5.0 + 2 * db) and float(dw0.abs().max()) > 0


@pytest.mark.parametrize("case", [DEFINITION_CASES[0], DEFINITION_CASES[1]], ids=["331", "333-b3"])
def test_gated_definition_equals_autograd_of_the_gated_input(case):
    ops = O.operands(case)
    gated = dict(ops, x=ops["x"] * (1.0 + ops["gate"]).unsqueeze(1))
    assert set(ops["gate"].unique().tolist()) == {0.0, 1.0} and float(gated["x"].abs().max()) == 4.0
    dw, _ = O.expected(case, ops, gate=True)
    assert torch.equal(dw, _autograd(case, gated)) and not torch.equal(dw, O.expected(case, ops)[0])


def test_operands_are_nonzero_bf16_integers_and_the_range_guard_holds():
    case = O.TILE_CASES[0]
    ops = O.operands(case)
    for name in ("p", "h"):
        assert set(ops[name].unique().tolist()) == set(O.VALUES) and O.is_bf16(ops[name])
    assert torch.equal(O.operands(case)["p"], ops["p"])  # deterministic
    assert not O.is_bf16(torch.tensor([257.0]))
    with pytest.raises(AssertionError, match="operand range"):
        O.expected(O._c("huge", O.K111, O.S1, 8, 8, (64, 64, 64), batch=8), {"p": torch.ones(1), "h": torch.ones(1), "gate": None})
    with pytest.raises(AssertionError, match="non-zero integers"):
        O.expected(case, dict(ops, p=ops["p"] * 0.5))
    with pytest.raises(AssertionError, match="non-zero integers"):
        bad = ops["h"].clone()
        bad[0, 0, 0, 0, 0] = 0.0
        O.expected(case, dict(ops, h=bad))


# ---- planted faults: the equality check of the GPU file must trip on each ----
FAULT = O._c("fault-331-8to2", O.K331, O.S1, 8, 2, (9, 32, 4))  # P = dY: 2 channels, H = X: 8 channels, 9 taps


def _trips(got, want):
    with pytest.raises(AssertionError, match="elements differ"):
        O.assert_exact(got.float(), want, "planted")
    return (got != want).reshape(want.shape[0], want.shape[1], -1)  # [cP][cH][tap]


def test_equality_check_passes_on_the_definition_and_reports_where_it_fails():
    ops = O.operands(FAULT)
    want, db = O.expected(FAULT, ops)
    O.assert_exact(want.float(), want, "definition")
    O.assert_exact(db.float(), db, "bias")
    got = want.float().clone()
    got[1, 3, 2, 1, 0] += 1.0
    with pytest.raises(AssertionError, match=r"1 of 144 elements differ, in taps \[7\]; \(tap 7, cP 1, cH 3: got .*, want"):
        O.assert_exact(got, want, "one element")
    with pytest.raises(AssertionError, match="elements differ"):
        O.assert_exact(torch.full_like(got, float("nan")), want, "nan")


def test_one_voxel_dropped_from_p_changes_every_element_of_every_tap_it_meets():
    ops = O.operands(FAULT)
    want, _ = O.expected(FAULT, ops)
    p = ops["p"].clone()
    p[1, :, 4, 17, 2] = 0.0  # an interior voxel: all nine taps pair it with a voxel of H
    diff = _trips(O.wgrad(p, ops["h"], FAULT.k, FAULT.s), want)
    assert bool(diff.all())  # no operand is zero: every (cP, cH) of every tap changes
    p = ops["p"].clone()
    p[0, :, 0, 0, 0] = 0.0  # a corner voxel: the four taps that stay inside the image
    diff = _trips(O.wgrad(p, ops["h"], FAULT.k, FAULT.s), want)
    assert diff.all(0).all(0).tolist() == [False, False, False, False, True, True, False, True, True]


def test_one_tile_of_32_voxels_counted_twice():
    """A sum over 32 voxels can cancel in single elements, so that a duplicated tile changes EVERY element of a tap is a property of this fixture, checked here."""
    ops = O.operands(FAULT)
    want, _ = O.expected(FAULT, ops)
    again = torch.zeros_like(ops["p"])
    again[1, :, 3, 8:16, :] = ops["p"][1, :, 3, 8:16, :]  # 8 rows x 4 slices of one plane
    assert int((again[:, 0] != 0).sum()) == 32
    diff = _trips(want + O.wgrad(again, ops["h"], FAULT.k, FAULT.s), want)
    assert bool(diff.all(0).all(0).any())


def test_one_tap_paired_with_the_neighbouring_offset():
    ops = O.operands(FAULT)
    want, _ = O.expected(FAULT, ops)
    hp = O.zero_padded(ops["h"], P.same_pad(FAULT.k))
    got = O.wgrad_from_padded(ops["p"], hp, FAULT.k, FAULT.s, tap_shift={(1, 1, 0): (1, 2, 0)})  # the centre tap reads its +y neighbour's voxels
    assert torch.equal(O.wgrad_from_padded(ops["p"], hp, FAULT.k, FAULT.s), want)
    diff = _trips(got, want)
    assert torch.equal(got[:, :, 1, 1, 0], want[:, :, 1, 2, 0]) and diff.any(0).any(0).tolist() == [False] * 4 + [True] + [False] * 4


def test_one_image_border_row_treated_as_inside():
    ops = O.operands(FAULT)
    want, _ = O.expected(FAULT, ops)
    hp = O.zero_padded(ops["h"], P.same_pad(FAULT.k))
    hp[:, :, :, 0, :] = hp[:, :, :, 1, :]  # row y = -1 reads row 0 instead of zeros (a clamped address)
    diff = _trips(O.wgrad_from_padded(ops["p"], hp, FAULT.k, FAULT.s), want)
    assert diff.any(0).any(0).tolist() == [True, False, False] * 3  # the three taps with dy = -1


def test_last_x_segment_of_a_marching_tile_skipped():
    case = O.MARCH_HAND_CASES[0]  # 10 planes in segments of 4: 4 + 4 + 2
    m = O.march_launch(case)
    assert m["nxs"] == 3 and m["last_seg"] == 2
    ops = O.operands(case)
    want, _ = O.expected(case, ops)
    p = ops["p"].clone()
    p[1, :, (m["nxs"] - 1) * m["lx"]:, :case.tile[1], 4:8] = 0.0  # one column block of one sample
    _trips(O.wgrad(p, ops["h"], case.k, case.s), want)


# ---- path audit ----
def _all_tile_rows(es):
    rows = list(O.TILE_CASES)
    for prob, hg, sb in itertools.product(O.SWEEP_PROBLEMS, O.SWEEP_HGROUPS, O.SWEEP_BUFFERS):
        rows += O.sweep_cases(prob, es, hg, sb)
    return rows


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_every_tile_kernel_row_reaches_its_paths(dt):
    es = ES[dt]
    rows = _all_tile_rows(es)
    assert len({r.id for r in rows}) == len(rows)
    seen = set()
    for r in rows:
        m = O.tile_launch(r, es)
        assert r.paths <= m["paths"], (r.id, sorted(r.paths - m["paths"]), m)
        # the occupancy clamp of wg_launch depends on the device: no row may be in its reach, neither by the workgroups it launches nor (sweep) by those it asks for
        assert m["clamp_free"] and m["lds"] <= 160 * 1024, (r.id, m)
        assert r.blocks is None or r.blocks * m["grid_y"] <= 256, (r.id, m)
        assert m["nblk"] == m["grid_x"] * m["wv"] and m["wt"] * m["wv"] == 4 and m["grid_x"] >= 1 and m["scratch"] >= m["hchunks"] * m["slab_chunk"]
        seen |= m["paths"]
    for r in O.TILE_CASES + list(O.SWEEP_PROBLEMS.values()):  # the range guard, at the calls and starting values the GPU file uses
        ops = O.operands(r)
        O.expected(r, ops, calls=2 if r.acc else 1, dw0=ops["dw0"] if r.acc else None, db0=ops["db0"] if r.acc else 0.0)
    need = {"slab<=16", "slab-scalar", "slab-unroll1", "slab-unroll2", "blocks<tiles", "blocks=tiles", "blocks>tiles", "walk-on", "walk-off", "round8", "scratch-cap",
            "npp=0", "npp>0", "hg=1", "hg=2", "hg=3", "hg=4", "wv=1", "wv=4", "batch1", "batch2", "batch3", "dbias", "acc", "transposed", "strided", "p-padded", "h-padded",
            "h-ragged-chunk", "two-part", "split-in-group"}
    assert need <= seen, sorted(need - seen)


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
def test_sweep_problems_are_what_the_sweep_needs(dt):
    es = ES[dt]
    a, b, c = (O.tile_launch(O.SWEEP_PROBLEMS[p], es) for p in "ABC")
    assert a["wv"] == 4 and a["tiles"] >= 32 and b["wv"] == 1 and b["hchunks"] == 4 and c["wv"] == 4 and c["tiles"] * 4 >= 241
    # the clamp of a request of hgroup 1..4 on two and on four chunks of H
    assert [O.tile_launch(O.sweep_cases("A", es, hg, 0)[0], es)["hg"] for hg in (1, 2, 3, 4)] == [1, 2, 2, 2]
    # (four chunks of fp32 H next to a 32-channel P tile: two buffers leave LDS for one chunk, one buffer for two — a request of hgroup 4 is a launch with
    #  hgroup 4 in bf16 only, also in test_gpu_ops.py::test_wgrad_h_chunk_groups)
    want = {("fp32", 0): [1, 1, 1, 1], ("fp32", 1): [1, 2, 2, 2], ("bf16", 0): [1, 2, 2, 4], ("bf16", 1): [1, 2, 2, 4]}
    for sb in (0, 1):
        assert [O.tile_launch(O.sweep_cases("B", es, hg, sb)[0], es)["hg"] for hg in (1, 2, 3, 4)] == want[dt, sb]
    row = next(r for r in O.TILE_CASES if r.id == "331-64to32-split32-hg4")
    assert O.tile_launch(row, es)["hg"] == (4 if dt == "bf16" else 1)
    for prob in "AB":  # a scratch for exactly 1, 2, 3 workgroups launches exactly that many
        got = [O.tile_launch(r, es)["grid_x"] for r in O.sweep_cases(prob, es, 1, 0) if r.scratch_wgs]
        assert got == [1, 2, 3]
    # whole-tile twin rows differ in nothing but the ragged axis
    whole, ragged = (next(r for r in O.TILE_CASES if r.id == i) for i in ("331-32to32-whole", "331-32to32-ragged-y"))
    mw, mr = O.tile_launch(whole, es), O.tile_launch(ragged, es)
    assert mw["npp"] == 0 and mr["npp"] > 0 and mw["tile"] == mr["tile"] and mw["tiles"] == mr["tiles"]


def test_every_marching_row_reaches_its_paths_and_the_rows_cover_every_instantiation():
    rows = O.MARCH_HAND_CASES + O.march_planner_cases()
    assert len({r.id for r in rows}) == len(rows)
    reached, seen = set(), set()
    for r in rows:
        m = O.march_launch(r)
        assert r.paths <= m["paths"] and m["fits"], (r.id, sorted(r.paths - m["paths"]), m)
        assert not r.gate or m["shape"][:2] == (32, 8)  # the only instantiations with the gated H operand
        reached.add(m["shape"])
        seen |= m["paths"]
        O.expected(r, O.operands(r), gate=r.gate)
    assert reached == P.MARCH_WGRAD_SHAPES, (sorted(P.MARCH_WGRAD_SHAPES - reached), sorted(reached - P.MARCH_WGRAD_SHAPES))  # every instantiation is reachable with a small case
    assert {O.march_launch(r)["shape"] for r in O.MARCH_HAND_CASES} == P.MARCH_WGRAD_SHAPES
    assert {"x-segs=1", "x-segs>1", "x-ragged", "row-blocks>1", "two-part", "compact-p", "gate", "dbias", "p-padded", "batch1", "batch2", "batch3", "planner-tile"} <= seen


def test_planner_marching_tiles_have_two_x_segments_with_a_ragged_last_one():
    got = O.march_planner_cases()
    assert {(r.cin, r.cout, r.dims, r.batch) for r in got} == {(a, b, d, n) for a, b, d, n, _ in O.MARCH_PLANNER_PROBLEMS}  # the planner returns tiles for every problem
    assert {r.batch for r in got} == {1, 2, 3} and {r.dims for r in got} == {(17, 64, 8), (17, 128, 8)}
    for r in got:
        m = O.march_launch(r)
        assert (m["lx"], m["nxs"], m["last_seg"]) == (9, 2, 8) and "planner-tile" in r.paths, (r.id, m)
    # at the small q[0] of the hand rows the planner can only return one x segment
    assert all(t[0] == 10 for t in P.march_wgrad_tiles(16, 16, (10, 64, 8), 2))


def test_every_compute_row_reaches_its_paths_and_every_wave_role_split_is_reached():
    splits, insts, seen = set(), set(), set()
    assert len({r.id for r in O.COMPUTE_CASES}) == len(O.COMPUTE_CASES)
    for r in O.COMPUTE_CASES:
        m = O.compute_launch(r)
        assert r.paths <= m["paths"] and m["ok"], (r.id, sorted(r.paths - m["paths"]), m)
        splits.add(m["split"])
        insts.add(m["inst"])
        seen |= m["paths"]
        O.expected(r, O.operands(r))
    assert splits == {(3, 1, 1), (3, 1, 2), (2, 2, 1)}  # (P tiles per wave, P shares, H chunks per workgroup) of cw_launch_inst
    assert insts == {(*s, b) for s in splits for b in (False, True)}
    assert {"pow2-classes", "odd-classes", "two-part", "dbias", "batch1", "batch2", "batch3"} <= seen


def test_narrow_rows():
    rows = O.NARROW_CASES + O.NARROW_REFUSED
    assert len({r.id for r in rows}) == len(rows)
    for r in rows:
        assert (r.cin == 1) != (r.cout == 1) and r.k in (O.K331, O.K111) and r.dbias == (r.cout == 1)
        ops = O.operands(r)
        O.expected(r, ops, calls=2, dw0=ops["dw0"], db0=ops["db0"])
    assert all(r.dims[1] % 4 == 0 for r in O.NARROW_CASES) and all(r.dims[1] % 4 and all(d % 2 for d in r.dims) for r in O.NARROW_REFUSED)
    assert any(r.dims[0] % 2 and r.dims[2] % 2 and (r.dims[1] // 4) % 2 for r in O.NARROW_CASES)
    assert {r.batch for r in O.NARROW_CASES if r.cout == 1} == {1, 2, 3} == {r.batch for r in O.NARROW_CASES if r.cin == 1}
