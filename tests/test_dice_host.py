"""Host audit of tests/dice_oracle.py (runs without a GPU): the by-hand fp64 definitions against oracle.vsseg_oracle and autograd, the restated launch constants
against the source text, every case row against the path it declares, planted faults against the bars, and the exactness of the dyadic inputs."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import vsseg_oracle as O
from tests import dice_oracle as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the definitions
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _autograd(name, supervised, hardness):
    lab5, logits5, atts = D.module_inputs(name)
    lg = logits5.double().requires_grad_(True)
    at = [a.double().requires_grad_(True) for a in atts]
    loss = O.dice_spvpa(lg, at, lab5.double(), supervised_attention=supervised, hardness_weighting=hardness)
    loss.backward()
    return float(loss.detach()), lg.grad, [a.grad for a in at]


@pytest.mark.parametrize("hardness", [True, False])
@pytest.mark.parametrize("supervised", [True, False])
@pytest.mark.parametrize("name", list(D.MODULE_ROWS))
def test_by_hand_definitions_equal_the_oracle_and_its_autograd(name, supervised, hardness):
    lab5, logits5, atts = D.module_inputs(name)
    want, wlog, watts = _autograd(name, supervised, hardness)
    loss, dl, da = D.loss_by_hand(logits5, atts, lab5, supervised, hardness)
    assert abs(float(loss) - want) <= 1e-12 * abs(want)
    assert float((dl - wlog).abs().max()) <= 1e-12 * float(wlog.abs().max())
    for a, w in zip(da, watts):
        if supervised:
            assert float((a - w).abs().max()) <= 1e-12 * float(w.abs().max())
        else:
            assert a is None and w is None


def test_sums_and_finalisation_equal_the_oracle_dice():
    """One level and the prediction term on their own, against oracle.vsseg_oracle.dice."""
    lab5, logits5, atts = D.module_inputs("pyr_12_4_12")
    B = lab5.shape[0]
    a = atts[-1].double()
    f_att = 1.0 - (2.0 * D.att_sums(a, lab5)[:, 0] + D.SMOOTH) / (D.att_sums(a, lab5)[:, 1] + D.att_sums(a, lab5)[:, 2] + D.SMOOTH)
    assert abs(float(f_att.mean()) - float(O.dice(a, lab5.double()))) < 1e-14
    lg = logits5.double().permute(0, 2, 3, 4, 1).reshape(B, -1, 2)
    for hard in (False, True):
        w = 0.6 * torch.abs(torch.softmax(logits5.double(), 1) - O.one_hot(lab5.double(), 2)) + 0.4 if hard else None
        want = O.dice(logits5.double(), lab5.double(), softmax=True, to_onehot_y=True, hardness_weight=w)
        loss, coef = D.finalize(D.pred_sums(lg, lab5.reshape(B, -1), hard))
        assert abs(float(loss) - float(want)) < 1e-14 and coef.numel() == B * 4 + B * 2 and not bool(coef[B * 4:].any())


def test_argmax_and_hard_dice_definitions():
    lg, lab = D.argmax_inputs(1003)
    am = D.argmax2(lg)
    fin = torch.isfinite(lg[:, 0]) & torch.isfinite(lg[:, 1]) & (lg[:, 0] != lg[:, 1])
    assert torch.equal(am[fin], torch.argmax(lg[fin][:, :2], 1))  # torch.argmax away from ties and NaN
    assert int(am[::5].sum()) == 0 and int(am[1003 // 2]) == 0 and int(am[1003 // 3]) == 0
    pg, p, g = D.hard_counts(lg, lab)
    assert float(p) == float(am.sum()) and float(g) == float(lab.sum()) and float(pg) == float((am.double() * lab.double()).sum())
    # the hard Dice of the oracle from these counts (away from NaN logits, which torch.argmax sends to the NaN's class)
    ok = torch.isfinite(lg[:, :2]).all(1)
    pred = lg[ok][:, :2].double().t().reshape(1, 2, -1, 1, 1)
    c = D.hard_counts(lg[ok], lab[ok])
    want = O.compute_dice_score(pred, lab[ok].double().reshape(1, 1, -1, 1, 1))
    assert abs(float((2 * c[0] + D.SMOOTH) / (c[1] + c[2] + D.SMOOTH)) - float(want)) < 1e-12


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the restated launch arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_restated_constants_match_the_source_text():
    src, hdr, py = _read("vs_seg_amd", "csrc", "loss.hip"), _read("include", "vsseg_hip.h"), _read("vs_seg_amd", "losses", "dice_spvPA.py")

    def one(pattern, text=src):
        m = re.findall(pattern, text)
        assert len(m) >= 1 and len(set(m)) == 1, (pattern, m)
        return int(m[0])

    assert one(r"constexpr int DICE_THREADS = (\d+);") == D.DICE_THREADS
    assert one(r"constexpr int DICE_TAIL_THREADS = (\d+);") == D.DICE_TAIL_THREADS
    assert one(r"nb \+= \(int\)std::min<int64_t>\((\d+), win == 1") == D.TAIL_BLOCK_CAP
    assert one(r"win == 1 \? \(nvox \+ (\d+)\) / \d+ :") + 1 == one(r"win == 1 \? \(nvox \+ \d+\) / (\d+) :") == D.TAIL_VOX_PER_BLOCK
    assert one(r": \(nvox \* T \+ (\d+)\) / \d+\)") + 1 == one(r": \(nvox \* T \+ \d+\) / (\d+)\)") == D.TAIL_LANES_PER_BLOCK
    assert one(r"std::min<int64_t>\((\d+), \(d->nvox\[l\] \+ \d+\) / \d+\)") == D.BWD_LEVELS_BLOCK_CAP
    assert one(r"\(d->nvox\[l\] \+ (\d+)\) / \d+\)") + 1 == one(r"\(d->nvox\[l\] \+ \d+\) / (\d+)\)") == D.BWD_LEVELS_VOX
    assert one(r"v < nvox; v \+= \(int64_t\)nb \* (\d+)\) o\[v\]") == D.BWD_THREADS  # the levels kernel strides by its block size
    assert one(r"grid_for\(\(nvox \+ 3\) / 4, (\d+), \d+\)") == D.BWD_THREADS and one(r"grid_for\(\(nvox \+ 3\) / 4, \d+, (\d+)\)") == D.BWD_GRID_CAP
    assert one(r"__launch_bounds__\((\d+)\) void dice_pred_bwd_kernel") == D.BWD_THREADS
    assert one(r"const int cap = n >= (\d+) \? 1 : \d+ / n;") == one(r"const int cap = n >= \d+ \? 1 : (\d+) / n;") == 512
    assert "(items + DICE_THREADS * 2 - 1) / (DICE_THREADS * 2)" in src
    assert one(r"#define VSSEG_DICE_MAX_LEVELS (\d+)", hdr) == D.DICE_MAX_LEVELS and "first[VSSEG_DICE_MAX_LEVELS + 1]" in src
    assert one(r"\nDICE_MAX_LEVELS = (\d+)\n", _read("vs_seg_amd", "_lib.py")) == D.DICE_MAX_LEVELS
    assert one(r"VSSEG_CHECK\(nvox < \(1ll << (\d+)\)") == one(r">= \(1 << (\d+)\) for s in att_shapes", py) == int(math.log2(D.TAIL_MAX_VOX))
    assert "constexpr double VSSEG_FX_DICE = 4294967296.0;" in src and D.FX_DICE == 4294967296.0
    assert "#define SMOOTH 1e-5" in src and D.SMOOTH == 1e-5
    assert "const float __log2_e" not in src and "__expf(l0 - m)" in src  # the exponential the error pieces are written for


def test_sums_rows_reach_the_paths_they_declare():
    names = set()
    for c in D.SUMS_CASES:
        assert c["name"] not in names
        names.add(c["name"])
        off = 8 if c["offset"] else 0
        la = D.sums_launch(c["nvox"], c["n"], c["pitch"], (off,))
        w = c["want"]
        assert la["vector"] == w["vector"], c["name"]
        if "blocks" in w:
            assert la["blocks"] == w["blocks"] == la["cap"], c["name"]
            assert (c["nvox"] // 4 + 2 * D.DICE_THREADS - 1) // (2 * D.DICE_THREADS) >= la["cap"], c["name"]
        if "min_rounds" in w:
            assert la["rounds"] >= w["min_rounds"], c["name"]
        # the attention-map sums share the launch shape (pitch does not exist there)
        assert D.sums_launch(c["nvox"], c["n"], 2, (off,))["blocks"] == la["blocks"]
    # what the issue lists is all there
    assert {c["nvox"] for c in D.SUMS_CASES} >= set(D.NVOX) and {c["n"] for c in D.SUMS_CASES} >= {1, 2, 3, 5, 64, 512}
    assert any(c["offset"] and c["nvox"] % 4 == 0 for c in D.SUMS_CASES) and any(c["pitch"] == 8 for c in D.SUMS_CASES)
    assert D.sums_launch(40000, 64)["rounds"] == 3 and D.sums_launch(40001, 64)["rounds"] == 10 and D.sums_launch(3000, 512)["rounds"] == 2
    # below the cap no thread of the 16-byte loop takes a second round: that is what made these rows necessary
    assert all(D.sums_launch(v, n, 2, (0,))["rounds"] <= 1 for v in (4, 1024) for n in (1, 2, 3, 5))
    assert D.sums_launch(4100, 1, 2, (0,))["rounds"] == 2 and D.sums_launch(4100, 1, 2, (0,))["blocks"] == 2  # (1 025 items on 1 024 threads: one thread, one more item)


def test_level_and_tail_rows_reach_the_paths_they_declare():
    for c in D.LEVEL_CASES:
        la = D.level_launch(c["dims"], c["n"])
        assert la["blocks"] == c["want"]["blocks"], c["name"]
        assert c["dims"][0] % 2 == 0 and c["dims"][1] % 2 == 0 and c["dims"][2] % 4 == 0
    assert D.level_launch((32, 32, 12), 1)["items"] == 768 > D.DICE_THREADS  # the second workgroup has work
    for name, (sdims, levels, want) in D.TAIL_ROWS.items():
        plan, first = D.tail_plan(sdims, levels)
        assert len(first) == D.DICE_MAX_LEVELS + 1 and first[0] == 0 and first[len(levels)] == sum(p["blocks"] for p in plan) == first[-1]
        assert tuple(p["win"] for p in plan) == want["win"], name
        if "T" in want:
            assert tuple(p["T"] for p in plan) == want["T"], name
        assert tuple(i for i, p in enumerate(plan) if p["win"] % p["T"]) == want.get("ragged", tuple(i for i, p in enumerate(plan) if p["win"] % p["T"])), name
        for i in want.get("vector", ()):
            assert plan[i]["vector"], name
        for i in want.get("scalar_win1", ()):
            assert plan[i]["win"] == 1 and not plan[i]["vector"], name
        if "blocks" in want:
            assert tuple(p["blocks"] for p in plan) == want["blocks"], name
        if "busy" in want:  # how many of a level's workgroups start below nvox
            assert tuple(p["busy"] for p in plan) == want["busy"], name
        if "nlevels" in want:
            assert len(levels) == want["nlevels"] == D.DICE_MAX_LEVELS
        assert all(p["nvox"] < D.TAIL_MAX_VOX for p in plan)
    wins = {p["win"] for sd, lv, _ in D.TAIL_ROWS.values() for p in D.tail_plan(sd, lv)[0]}
    assert wins >= {1, 8, 9, 27, 64, 135, 576}
    assert {p["T"] for sd, lv, _ in D.TAIL_ROWS.values() for p in D.tail_plan(sd, lv)[0]} >= {1, 2, 4, 8, 16, 32, 64}
    assert any(p["win"] % p["T"] and p["T"] == 64 for sd, lv, _ in D.TAIL_ROWS.values() for p in D.tail_plan(sd, lv)[0])  # 135 on 64 lanes
    # more than one workgroup WITH voxels on each path of the tail: the 16-byte loop of the source level, and the pooling loop at T = 16 and at T = 64
    plans = [p for sd, lv, _ in D.TAIL_ROWS.values() for p in D.tail_plan(sd, lv)[0]]
    assert any(p["vector"] and p["busy"] >= 2 for p in plans) and any(p["win"] > 1 and p["T"] == 16 and p["busy"] >= 3 for p in plans) and any(p["T"] == 64 and p["busy"] >= 3 for p in plans)
    assert D.tail_plan(*D.TAIL_ROWS["win64_two_workgroups"][:2])[0][0]["busy"] == 1  # (of exactly two pooling workgroups the second starts at nvox)


def test_backward_rows_reach_the_paths_they_declare():
    for nvox in D.NVOX:
        assert D.bwd_launch(nvox, 2, (0, 0, 0))["rounds"] == 1 or nvox % 4  # below the cap no thread of the 16-byte loop takes a second round
        assert D.bwd_launch(nvox, 2, (0, 0, 0))["vector"] == (nvox % 4 == 0) and not D.bwd_launch(nvox, 8, (0, 0, 0))["vector"] and not D.bwd_launch(nvox, 2, (8, 4, 8))["vector"]
    big = D.bwd_launch(D.BWD_BIG, 2, (0, 0, 0))
    assert big["grid"] == D.BWD_GRID_CAP and big["vector"] and big["rounds"] == 2 and D.BWD_BIG % 4 == 0
    assert [D.bwd_levels_blocks(v) for v in D.ATT_BWD_NVOX] == [1, 1, 2, 5]
    assert [D.bwd_launch(v, 2, (0, 0))["vector"] for v in D.ATT_BWD_NVOX] == [False, False, False, True]


def test_module_rows_get_the_plan_they_declare():
    for name, (B, dims, att_dims, plan) in D.MODULE_ROWS.items():
        assert D.fused_plan(B, dims, att_dims) == plan, name
        assert D.fused_plan(B, dims, att_dims, aligned=False) is None
    B, dims, att_dims, _ = D.MODULE_ROWS["ten_levels"]
    assert len(att_dims) == 10 and D.fused_plan(B, dims, att_dims[1:]) == 1  # nine maps: one fused level and a tail of eight; the tenth is one too many for the tail
    assert any(lab[0].sum() == 0 for lab in [D.module_inputs(n)[0] for n in ("pyr_12_4_12", "pyr_9_3_5", "fused_b3")])


def test_restated_fused_plan_is_the_module_s():
    """The restatement against the function itself, on stand-ins for device tensors (only data_ptr() is asked of them)."""
    from vs_seg_amd.losses import dice_spvPA as M

    class P:
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    for name, (B, dims, att_dims, plan) in D.MODULE_ROWS.items():
        shapes = [(B, 1, *d) for d in att_dims]
        assert M._fused_plan(B, dims, shapes, P(256), P(512), [P(1024)] * len(shapes)) == plan, name
        assert M._fused_plan(B, dims, shapes, P(256), P(516), [P(1024)] * len(shapes)) is None


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the inputs
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_dyadic_attention_sums_do_not_depend_on_the_order():
    for n, nvox in ((3, 4101), (1, 36864)):
        a, g = D.make_att(5, n, nvox), D.make_label(5, n, nvox)
        assert bool((a * 256 == torch.round(a * 256)).all()) and float(a.min()) >= 0 and float(a.max()) <= 1 and float(a.max()) == 1.0
        perm = torch.from_numpy(np.random.default_rng(9).permutation(nvox))
        for t in (a, a * g):
            fwd = torch.cumsum(t, 1, dtype=torch.float32)[:, -1]  # one fp32 chain front to back
            assert torch.equal(fwd, torch.cumsum(t[:, perm], 1, dtype=torch.float32)[:, -1]) and torch.equal(fwd.double(), t.double().sum(1))
            assert torch.equal(t.reshape(n, -1, 3).sum(1).sum(1).double(), t.double().sum(1))  # (and a tree)
        ints = D.fx_encode(D.att_sums(a, g))
        assert torch.equal(D.fx_decode(ints), D.att_sums(a, g)) and float(D.att_sums(a, g).max()) < 2.0 ** 16


def test_inputs_are_what_the_rows_say():
    for c in D.SUMS_CASES:
        lab = D.make_label(D._seed(c["name"]), c["n"], c["nvox"], c["label"])
        assert bool(((lab == 0) | (lab == 1)).all())
        if c["label"] == "special":
            assert float(lab[0].min()) == 1.0 and (c["n"] < 2 or float(lab[1].max()) == 0.0)
    lg = D.make_logits(3, 2, 1024, "saturated")
    diff = (lg[..., 1].double() - lg[..., 0].double())
    assert float(diff.abs().max()) <= 40.0 + 1e-5 and int((diff == 0).sum()) > 100 and int((diff.abs() > 39).sum()) > 100 and int(((diff.abs() > 19) & (diff.abs() < 21)).sum()) > 100
    p0, p1 = D.softmax2(lg.float().double())
    sat32 = (p0.float() == 1.0) | (p1.float() == 1.0)
    assert int(sat32.sum()) > 300 and int((sat32 & (p0 != 1.0) & (p1 != 1.0)).sum()) > 100  # 1 in fp32, not yet in fp64: the sign term differs there
    assert D.max_logit_gap(lg) <= 40.0 + 1e-5
    for case in D.TAIL_CASES:
        src, atts = D.tail_inputs(case)
        for d in D.TAIL_ROWS[case["row"]][1]:
            g = D.pool_from(src, d)
            if g[0].numel() > 4 and math.prod(d) < src[0].numel():
                assert 0 < float(g.mean()) < 1, (case["name"], d)  # a pooled level is neither all 0 nor all 1


# ---------------------------------------------------------------------------------------------------------------------------------------------
# the bars, and planted faults
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_error_pieces_are_what_their_derivation_says():
    assert D.rel_term(0.0, False) < D.rel_term(0.0, True) < D.rel_term(40.0, True) < 1.5e-5
    assert abs(D.e_arg(10.0) - 30 * 2.0 ** -24) < 1e-20 and D.ABS_E < 4 * D.U24 and D.REL_W < 30 * D.U24
    # the pieces bound the true fp32 error of the same operations done in numpy fp32 with a correctly rounded exponential (1/2 ulp <= the 1 ulp allowed)
    lg = D.make_logits(11, 1, 4096)
    lab = D.make_label(11, 1, 4096)
    l0, l1 = lg[0, :, 0].numpy(), lg[0, :, 1].numpy()
    m = np.maximum(l0, l1)
    e0, e1 = np.exp(l0 - m, dtype=np.float32), np.exp(l1 - m, dtype=np.float32)
    inv = np.float32(1.0) / (e0 + e1)
    p0, p1 = e0 * inv, e1 * inv
    g0, g1 = (lab[0].numpy() == 0).astype(np.float32), (lab[0].numpy() == 1).astype(np.float32)
    w0, w1 = np.float32(0.6) * np.abs(p0 - g0) + np.float32(0.4), np.float32(0.6) * np.abs(p1 - g1) + np.float32(0.4)
    got = np.stack([w0 * g0 * p0, w0 * g0, w0 * p0, w1 * g1 * p1, w1 * g1, w1 * p1], -1).astype(np.float64)
    ref = D.pred_terms(lg, lab, True)[0].numpy()
    rel = np.abs(got - ref) / np.maximum(ref, 1e-300)
    assert float(rel.max()) <= D.rel_term(D.max_logit_gap(lg), True) - D.CHAIN
    P0, P1 = D.softmax2(lg)
    assert float(np.abs(p0 - P0[0].numpy()).max()) <= D.ABS_P and float(np.abs(w0 - (0.6 * (P0[0] - torch.from_numpy(g0).double()).abs() + 0.4).numpy()).max()) <= D.ABS_W


def _detected(ref, bars, got):
    """A planted fault counts as seen when some compared quantity moves by more than 50 times its bar (any change, for a quantity held to equality: bar None)."""
    for k in ref:
        d = (torch.as_tensor(got[k], dtype=F64) - torch.as_tensor(ref[k], dtype=F64)).abs()
        if bars[k] is None:
            if bool((d != 0).any()):
                return True
        elif bool((d > 50.0 * torch.as_tensor(bars[k], dtype=F64)).any()):
            return True
    return False


def _sums_quantities(lg, lab, att, workgroups):
    """What a sums row compares: the hardness-weighted sums and (I, P) without hardness within sum_bound, G without hardness and the attention sums for equality."""
    hard, plain = D.pred_sums(lg, lab, True), D.pred_sums(lg, lab, False)
    ref = {"hard": hard, "plain_IP": plain[:, [0, 2, 3, 5]], "plain_G": plain[:, [1, 4]], "att": D.att_sums(att, lab)}
    bars = {"hard": D.sum_bound(lg, lab, True, workgroups), "plain_IP": D.sum_bound(lg, lab, False, workgroups)[:, [0, 2, 3, 5]], "plain_G": None, "att": None}
    return ref, bars


@pytest.mark.parametrize("case", D.SUMS_CASES, ids=lambda c: c["name"])
def test_planted_faults_in_the_sums_rows_are_seen(case):
    n, nvox, s = case["n"], case["nvox"], D._seed(case["name"])
    lg, lab, att = D.make_logits(s, n, nvox, case["logits"]).double(), D.make_label(s, n, nvox, case["label"]), D.make_att(s, n, nvox)
    wg = D.sums_launch(nvox, n, case["pitch"], (8 if case["offset"] else 0,))["workgroups"]
    ref, bars = _sums_quantities(lg, lab, att, wg)
    terms_h, terms_p = D.pred_terms(lg, lab, True), D.pred_terms(lg, lab, False)
    a_terms = torch.stack([lab.double() * att.double(), lab.double(), att.double()], -1)
    for v in sorted({0, nvox // 2, nvox - 1}):  # a voxel dropped, and the same voxel counted twice, in the last sample
        for sign in (-1.0, 1.0):
            got = {"hard": ref["hard"].clone(), "plain_IP": ref["plain_IP"].clone(), "plain_G": ref["plain_G"].clone(), "att": ref["att"].clone()}
            got["hard"][n - 1] += sign * terms_h[n - 1, v]
            got["plain_IP"][n - 1] += sign * terms_p[n - 1, v][[0, 2, 3, 5]]
            got["plain_G"][n - 1] += sign * terms_p[n - 1, v][[1, 4]]
            got["att"][n - 1] += sign * a_terms[n - 1, v]
            assert _detected(ref, bars, got), (case["name"], v, sign)
    if n > 1:  # two samples swapped
        perm = [1, 0] + list(range(2, n))
        assert _detected(ref, bars, {k: t[perm] for k, t in ref.items()}), case["name"]
    if nvox <= 2000:  # small rows: the bounded sums alone see a voxel of weight >= 0.4 (larger rows rely on G without hardness, held to equality)
        assert float((50.0 * bars["hard"][:, [1, 4]]).max()) < 0.4, case["name"]


def _window_pool(src5, dims, origin_ratio, window):
    """The pooling loop of the kernels with its pieces apart: out[x, y, z] = max over (a, c, e) in `window` of src[x rx + a, y ry + c, z rz + e] (indices
    wrapped into the sample), so that a wrong window can be planted."""
    B, _, X, Y, Z = src5.shape
    gx, gy, gz = torch.meshgrid(torch.arange(dims[0]), torch.arange(dims[1]), torch.arange(dims[2]), indexing="ij")
    out = torch.full((B, 1, *dims), -math.inf, dtype=F64)
    for a in range(window[0]):
        for c in range(window[1]):
            for e in range(window[2]):
                out = torch.maximum(out, src5.double()[:, :, (gx * origin_ratio[0] + a) % X, (gy * origin_ratio[1] + c) % Y, (gz * origin_ratio[2] + e) % Z])
    return out


def _pool_faults(src5, dims):
    """Faulty pooled labels of one level: the window's axes transposed (every transposition that changes the ratio), and one voxel taken from the window next
    to its own (the first voxel whose neighbour along the last axis with more than one window differs)."""
    ratio = tuple(s // d for s, d in zip(src5.shape[2:], dims))
    ref = D.pool_from(src5, dims)
    assert torch.equal(ref, _window_pool(src5, dims, ratio, ratio))
    out = []
    for i, j in ((0, 1), (0, 2), (1, 2)):
        if ratio[i] != ratio[j] and math.prod(dims) > 1:  # (a one-voxel level pools the whole sample: no window can be wrong there)
            w = list(ratio)
            w[i], w[j] = w[j], w[i]
            out.append((f"window axes {i} and {j} transposed", _window_pool(src5, dims, ratio, w)))
    flat = ref.reshape(ref.shape[0], -1)
    if flat.shape[1] > 1:
        nb = torch.roll(flat, -1, 1)
        idx = torch.nonzero(nb != flat)
        bad = flat.clone()
        if idx.numel():
            bad[idx[0][0], idx[0][1]] = nb[idx[0][0], idx[0][1]]
        out.append(("one voxel from the neighbouring window", bad.reshape(ref.shape)))
    return ref, out


@pytest.mark.parametrize("case", D.POOL_CASES, ids=lambda c: c["name"])
def test_planted_faults_in_the_pooling_rows_are_seen(case):
    src = D.pool_inputs(case)
    assert tuple(src.shape[2:]) == tuple(d * r for d, r in zip(case["dst"], case["ratio"])) and all(d % 2 for d in case["dst"])
    ref, faults = _pool_faults(src, case["dst"])
    assert len(faults) >= (2 if len(set(case["ratio"])) > 1 else 1)
    for what, bad in faults:
        with pytest.raises(AssertionError, match="elements differ"):
            D.assert_equal(bad.reshape(case["n"], -1), ref.reshape(case["n"], -1), what)
    if case["n"] > 1:
        assert not torch.equal(ref[[1, 0, 2]], ref)


@pytest.mark.parametrize("case", D.LEVEL_CASES, ids=lambda c: c["name"])
def test_planted_faults_in_the_level_rows_are_seen(case):
    lg, att, lab5 = D.level_inputs(case)
    n, d = case["n"], case["dims"]
    lab = lab5.reshape(n, -1)
    ref, bars = _sums_quantities(lg.double(), lab, att, D.level_launch(d, n)["workgroups"])
    got = {k: t.clone() for k, t in ref.items()}
    got["att"][n - 1] -= torch.stack([lab[n - 1, -1].double() * att[n - 1, -1].double(), lab[n - 1, -1].double(), att[n - 1, -1].double()])
    assert _detected(ref, bars, got)  # (the last voxel dropped from the attention sums: P moves by a multiple of 2^-8, or it is 0 and G moves)
    got = {k: t.clone() for k, t in ref.items()}
    got["plain_G"][n - 1] += D.pred_terms(lg.double(), lab, False)[n - 1, 0][[1, 4]]
    assert _detected(ref, bars, got)
    pref, faults = _pool_faults(lab5, (d[0] // 2, d[1] // 2, d[2]))
    assert any(w.startswith("window axes") for w, _ in faults)
    for what, bad in faults:
        assert not torch.equal(bad, pref), (case["name"], what)
    if n > 1:
        assert _detected(ref, bars, {k: t[[1, 0, 2]] for k, t in ref.items()})


@pytest.mark.parametrize("case", D.TAIL_CASES, ids=lambda c: c["name"])
def test_planted_faults_in_the_tail_rows_are_seen(case):
    sdims, levels, _ = D.TAIL_ROWS[case["row"]]
    src, atts = D.tail_inputs(case)
    n = case["n"]
    seen = {}
    for i, d in enumerate(levels):
        ref, faults = _pool_faults(src, d)
        sums = D.att_sums(atts[i], ref)
        for what, bad in faults:  # label[i] is held to equality: a fault is seen where it changes anything
            kind = what.split(" ")[0]
            seen[kind] = seen.get(kind, False) or not torch.equal(bad, ref)
        # a dropped and a doubled voxel of the level, in its sums (held to equality: any change is seen)
        g, a = ref.reshape(n, -1)[n - 1, -1], atts[i][n - 1, -1].double()
        assert float(a) != 0 or float(g) != 0
        if n > 1:
            assert not torch.equal(sums[[1, 0, 2]], sums), (case["name"], i)
    # every kind of pooling fault the row's ratios allow is seen at one level at least
    assert seen and all(seen.values()), (case["name"], seen)
    if case["row"] in ("win_1_9_135_odd", "eight_levels"):  # the rows with a window of unequal sides at a level of more than one voxel
        assert seen.get("window")
    # level i's sums written to level i + 1's slot
    allsums = torch.stack([D.att_sums(atts[i], D.pool_from(src, d)) for i, d in enumerate(levels)])
    if len(levels) > 1:
        assert not torch.equal(torch.roll(allsums, 1, 0), allsums)


def _fdiv(n, d):
    """vsseg_fdiv of csrc/common.h on int arrays: the quotient from a float reciprocal, corrected by one."""
    q = (n.astype(np.float32) * (np.float32(1.0) / np.float32(d))).astype(np.int64)
    r = n - q * d
    return q + (r >= d) - (r < 0)


def test_float_reciprocal_division_is_exact_at_the_tail_rows():
    """The tail kernel decodes voxel and window coordinates with vsseg_fdiv: at every divisor and range the rows use, it is the integer quotient."""
    for sdims, levels, _ in D.TAIL_ROWS.values():
        for d in levels:
            nvox, ratio = math.prod(d), [s // t for s, t in zip(sdims, d)]
            for n, div in ((nvox, d[2]), (nvox // d[2], d[1]), (math.prod(ratio), ratio[2]), (ratio[0] * ratio[1], ratio[1])):
                i = np.arange(n)
                assert np.array_equal(_fdiv(i, div), i // div), (sdims, d, div)
    i = np.arange(1 << 22)  # the largest level the tail launch takes
    for div in (1, 3, 5, 7, 12, 127, 128, 384):
        assert np.array_equal(_fdiv(i, div), i // div), div


def test_planted_faults_in_the_backward_rows_are_seen():
    """Every row of BWD_ROWS (pitch, offset and layout do not change the values: one check per (n, nvox, logits, hardness, upstream gradient)).  The bar is absolute
    per sample, so the fault is planted at the voxel where the sample's gradient is largest: left unwritten, written from the voxel where it is smallest, written
    without the upstream gradient; and another sample's coefficients."""
    done = set()
    for row in D.BWD_ROWS:
        key = (row["n"], row["nvox"], row["kind"], row["hard"], row["gs"])
        if key in done:
            continue
        done.add(key)
        n, nvox = row["n"], row["nvox"]
        lg, lab, coef = D.bwd_inputs(row)
        gs = D.GS if row["gs"] else 1.0
        ref = D.dlogits(lg, lab, bool(row["hard"]), coef, gs)
        bar = 2e-5 * ref.reshape(n, -1).abs().max(1).values
        assert float(bar.min()) > 0, key
        for b in range(n):
            mag = ref[b].abs().max(1).values
            v, vmin = int(mag.argmax()), int(mag.argmin())
            faults = [torch.zeros(2, dtype=F64)] + ([ref[b, vmin]] if nvox > 1 else []) + ([ref[b, v] / gs] if row["gs"] else [])
            for bad in faults:
                assert float((bad - ref[b, v]).abs().max()) > 50 * float(bar[b]), (key, b)
        if n > 1:
            swapped = D.dlogits(lg, lab, bool(row["hard"]), coef.reshape(n, 4)[[1, 0, 2]].reshape(-1), gs)
            assert float((swapped[0] - ref[0]).abs().max()) > 50 * float(bar[0]), key
            if nvox <= 4101:
                with pytest.raises(AssertionError):
                    D.check_grad("fp32", swapped.float(), ref, "planted")
        if nvox <= 4101:
            D.check_grad("fp32", ref.float(), ref, "clean")
            D.check_grad("bf16", ref.float().to(torch.bfloat16), ref, "clean")
    assert len(done) >= 8 * 2 * 4 + 4 + 1
    # B1 without the upstream gradient, through the comparison helper
    row = next(r for r in D.BWD_ROWS if r["gs"] and r["n"] == 3 and r["nvox"] == 1024 and r["hard"])
    lg, lab, coef = D.bwd_inputs(row)
    ref = D.dlogits(lg, lab, True, coef, D.GS)
    c2 = coef.clone().double().reshape(3, 2, 2)
    c2[:, 1, 1] /= D.GS
    with pytest.raises(AssertionError):
        D.check_grad("fp32", D.dlogits(lg, lab, True, c2.reshape(-1), D.GS).float(), ref, "B1 without gs")
    # attention-map gradient: equality, so the coefficients of level l applied to level l + 1 (or sample b to b + 1) are seen as soon as they differ
    for l, v in enumerate(D.ATT_BWD_NVOX):
        g = D.make_label(60 + l, 3, v)
        c32 = torch.tensor([-0.3, 0.02, -0.25, 0.015, -0.31, 0.021], dtype=torch.float32)
        want = D.datt_fp32(g, c32, D.GS)
        assert float((want.double() - D.datt(g, c32, D.GS)).abs().max()) < 1e-7
        with pytest.raises(AssertionError, match="elements differ"):
            D.assert_equal(D.datt_fp32(g, torch.roll(c32, 2), D.GS), want, "coefficients of the neighbouring level")
        fma = (c32.double().reshape(3, 2)[:, :1] * np.float32(D.GS)).float().double() * g.double() + (c32.double().reshape(3, 2)[:, 1:] * np.float32(D.GS)).float().double()
        assert torch.equal(fma.float(), want)  # one rounding (a fused multiply-add) or two: the same bits with g in {0, 1}


@pytest.mark.parametrize("n,nl", D.FINALIZE_ROWS)
def test_planted_faults_in_the_finalisation_rows_are_seen(n, nl):
    """The rows the GPU test runs (hand_sums), at their bar of 1 fp32 ulp: a voxel of the smallest weight missing from, or counted twice in, G of the last sample;
    samples swapped; the sums of level l read as level l + 1's."""
    pi, ai = D.hand_sums(n, nl)
    ps, asums = D.fx_decode(pi), (D.fx_decode(ai) if nl else None)
    assert torch.equal(D.fx_encode(ps), pi)
    loss, coef = D.finalize(ps, asums)
    bar, lbar = D.ulp32(coef), float(D.ulp32(loss))

    def seen(l2, c2):
        return abs(float(l2 - loss)) > 50 * lbar or bool(((c2 - coef).abs() > 50 * bar).any())

    for sign in (-1.0, 1.0):
        bad = ps.clone()
        bad[n - 1, 1] += sign * 0.4
        assert seen(*D.finalize(bad, asums))
        if nl:
            bad = asums.clone()
            bad[nl - 1, n - 1] += sign * torch.tensor([1.0 / 256, 0.0, 1.0 / 256], dtype=F64)  # the smallest non-zero voxel of an attention map, on the label
            assert seen(*D.finalize(ps, bad))
    if n > 1:
        assert seen(*D.finalize(ps[[1, 0, 2]], asums))
        if nl:
            assert seen(*D.finalize(ps, asums[:, [1, 0, 2]]))
    if nl > 1:
        assert seen(*D.finalize(ps, torch.roll(asums, 1, 0)))
    assert float(D.ulp32(torch.tensor(1.0, dtype=F64))) == 2.0 ** -23 and float(D.ulp32(torch.tensor(0.75, dtype=F64))) == 2.0 ** -24


@pytest.mark.parametrize("nvox,pitch", D.ARGMAX_ROWS)
def test_planted_faults_in_the_argmax_rows_are_seen(nvox, pitch):
    lg, lab = D.argmax_inputs(nvox, pitch)
    want = D.argmax2(lg)
    tie1 = (lg[:, 1] >= lg[:, 0]).to(torch.int64)  # a tie going to class 1
    assert int((tie1 != want).sum()) >= 1
    assert not torch.equal(D.hard_counts(lg, lab)[1], tie1.sum().double())
    if pitch > 2:
        assert int(D.argmax2(lg[:, [0, 2]]).sum()) == nvox - int(torch.isnan(lg[:, 0]).sum())  # the sentinel, if it were read, wins
    if nvox > 1:  # a voxel dropped or moved: the bytes are held to equality, and neighbours differ
        assert bool((want[1:] != want[:-1]).any())


@pytest.mark.parametrize("hardness", [True, False])
@pytest.mark.parametrize("name", list(D.MODULE_ROWS))
def test_module_rows_bars_and_planted_faults(name, hardness):
    B, dims, att_dims, plan = D.MODULE_ROWS[name]
    lab5, logits5, atts = D.module_inputs(name)
    bars = D.module_bars(name, True, hardness)
    # the denominator precondition of the 5e-6 loss bar, and the sums' part of the gradients' 5e-5
    assert bars["big_denominators"] == (bars["min_denominator"] >= 1.0)
    if bars["big_denominators"]:
        assert bars["loss_bar"] == 5e-6 and bars["rel_sums"] <= 1e-5, (name, bars)
    else:
        assert B > 1 and float(lab5[0].sum()) == 0 and 0 < bars["loss_bar"] < 1e-3, (name, bars)  # an empty sample: the bar comes from the finalisation at sums +- bound
    loss, dl, da = D.loss_by_hand(logits5, atts, lab5, True, hardness)
    nl = len(atts)
    # swapped samples, the coefficients of level l applied to level l + 1, a pooled voxel from the neighbouring window: in the gradients, at 5e-5 max|ref|
    if B > 1:
        assert float((dl[[1, 0] + list(range(2, B))] - dl).abs().max()) > 50 * 5e-5 * float(dl.abs().max())
    lg = logits5.double().permute(0, 2, 3, 4, 1).reshape(B, -1, 2)
    labels = D.pyramid_labels(lab5, [att_dims[nl - l - 1] for l in range(nl)])
    asums = torch.stack([D.att_sums(atts[nl - l - 1], labels[l]) for l in range(nl)])
    _, coef = D.finalize(D.pred_sums(lg, lab5.reshape(B, -1), hardness), asums)
    lev = coef[B * 4:].reshape(nl, B, 2)
    seen = 0
    for l in range(nl - 1):
        i = nl - l - 2  # the map of level l + 1
        if da[i].abs().max() == 0:
            continue
        wrong = D.datt(labels[l + 1], lev[l]).reshape(da[i].shape)
        seen += float((wrong - da[i]).abs().max()) > 50 * 5e-5 * float(da[i].abs().max())
    assert seen >= 1, name
    for l in range(nl):
        flat = labels[l].reshape(B, -1)
        if flat.shape[1] > 1 and bool((torch.roll(flat, -1, 1) != flat).any()):
            i = nl - l - 1
            assert float(lev[l][:, 0].abs().min()) > 50 * 5e-5 * float(da[i].abs().max()), (name, l)  # a voxel of G_l flipped moves its gradient by |A|
    # a voxel dropped from, and counted twice in, a SUM: the last voxel of the last sample that has anything in it.  In the attention sums of level l it moves
    # the loss (bar: the row's loss bar) or that level's d loss / d att (bar: 5e-5 max|ref|) by more than 50 bars at the coarsest level of EVERY row, and from
    # the level MODULE_SUM_FAULT_FINEST[name] on; finer levels hold too many voxels for it.  In the prediction sums it is seen at the small pyramids only.
    ps = D.pred_sums(lg, lab5.reshape(B, -1), hardness)
    lbar = bars["loss_bar"]
    seen_at = []
    for l in range(nl):
        a, g = atts[nl - l - 1].double().reshape(B, -1), labels[l].reshape(B, -1)
        v = int(torch.nonzero((a[B - 1] != 0) | (g[B - 1] != 0)).reshape(-1)[-1])
        t = torch.stack([g[B - 1, v] * a[B - 1, v], g[B - 1, v], a[B - 1, v]])
        ref = D.datt(g, lev[l])
        ok = True
        for sign in (-1.0, 1.0):
            bad = asums.clone()
            bad[l, B - 1] += sign * t
            l2, c2 = D.finalize(ps, bad)
            moved = float((D.datt(g, c2[B * 4:].reshape(nl, B, 2)[l]) - ref).abs().max())
            ok = ok and (abs(float(l2 - loss)) > 50 * lbar or moved > 50 * 5e-5 * float(ref.abs().max()))
        seen_at.append(ok)
    assert seen_at[nl - 1], (name, seen_at)
    assert seen_at.index(True) == MODULE_SUM_FAULT_FINEST[name] and all(seen_at[MODULE_SUM_FAULT_FINEST[name]:]), (name, seen_at)
    terms = D.pred_terms(lg, lab5.reshape(B, -1), hardness)
    dl_flat = D.dlogits(lg, lab5.reshape(B, -1), hardness, coef[: B * 4])
    pred_seen = True
    for v in (0, lg.shape[1] - 1):
        for sign in (-1.0, 1.0):
            bad = ps.clone()
            bad[B - 1] += sign * terms[B - 1, v]
            l2, c2 = D.finalize(bad, asums)
            moved = float((D.dlogits(lg, lab5.reshape(B, -1), hardness, c2[: B * 4]) - dl_flat).abs().max())
            pred_seen = pred_seen and (abs(float(l2 - loss)) > 50 * lbar or moved > 50 * 5e-5 * float(dl_flat.abs().max()))
    assert pred_seen == (name in MODULE_PRED_FAULT_SEEN), (name, pred_seen)


# the finest level (0 = the full resolution) from which a voxel dropped from or doubled in the attention sums is seen in a module row, and the rows where the same
# fault in the prediction sums is seen: 576 voxels a sample and fewer.  At (32, 32, 12) one voxel of 12 288 moves the prediction coefficients by 1 to 5 bars, which
# is why the sums are held to their own bars through the C ABI.  With attention off these rows have the prediction sums alone, and the two large ones cannot show it.
MODULE_SUM_FAULT_FINEST = {"pyr_12_4_12": 1, "pyr_6_10_4": 1, "pyr_9_3_5": 0, "fused_b1": 3, "fused_b3": 3, "ten_levels": 1}
MODULE_PRED_FAULT_SEEN = {"pyr_6_10_4", "pyr_9_3_5", "ten_levels"}


# ---------------------------------------------------------------------------------------------------------------------------------------------
# coverage of the C ABI
# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_every_exported_dice_symbol_is_called_by_the_gpu_test():
    lib_text, test_text = _read("vs_seg_amd", "_lib.py"), _read("tests", "test_gpu_dice.py")
    symbols = set(re.findall(r'"(vsseg_dice_\w+|vsseg_maxpool_label|vsseg_hard_dice_counts|vsseg_argmax2)"', lib_text))
    assert {"vsseg_dice_level_sums", "vsseg_dice_tail_sums", "vsseg_maxpool_label", "vsseg_dice_att_sums", "vsseg_dice_att_bwd", "vsseg_dice_att_bwd_levels", "vsseg_dice_finalize", "vsseg_argmax2",
            "vsseg_hard_dice_counts", "vsseg_dice_pred_sums", "vsseg_dice_pred_bwd", "vsseg_dice_pred_bwd_to"} <= symbols
    # (the cross-entropy and top-k entry points have tests of their own for their terms; here they are called with the term switched off, for the Dice part they share)
    missing = sorted(s for s in symbols if not re.search(r"\b" + s + r"\b", test_text))
    assert not missing, f"not called by tests/test_gpu_dice.py: {missing}"
