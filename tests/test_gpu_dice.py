"""-m gpu: the Dice loss kernels of csrc/loss.hip, one entry point at a time through the C ABI and then the module end to end, against the fp64 definitions of
tests/dice_oracle.py (case tables, bars and their derivations are there; tests/test_dice_host.py audits them without a GPU).

Bars: pooled labels, attention-map sums (decoded from the int64 pattern), G without hardness, hard-Dice counts, argmax bytes and the attention-map gradient:
equality.  Prediction sums through __expf and the reciprocal: dice_oracle.sum_bound (the largest error / bound of every row is printed).  Finalisation: 1 fp32 ulp.
Logits gradient: 2e-5 max|ref| per sample (bf16: one rounding of that).  Module: loss 5e-6 (or the propagated bar), gradients 5e-5 max|ref|."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

import vs_seg_amd as V  # noqa: E402
from oracle import vsseg_oracle as O  # noqa: E402
from tests import dice_oracle as D  # noqa: E402
from tests import gpu_harness as H  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

F64 = torch.float64
NAN = float("nan")
GS = D.GS
WORST = {}  # largest error / bound of the bounded sums, by kernel


def _place(t, off=0, guard=0, fill=7.0):
    """A CPU tensor copied into a fresh device allocation, `off` ELEMENTS behind its (at least 256-byte aligned) start and `guard` elements in front of the end,
    the rest filled with `fill`.  Returns (the whole buffer, the view that holds the data): view.data_ptr() is the deliberately offset pointer."""
    flat = t.reshape(-1)
    buf = torch.full((off + flat.numel() + guard,), fill, dtype=t.dtype, device="cuda")
    view = buf[off: off + flat.numel()]
    view.copy_(flat)
    assert buf.data_ptr() % 256 == 0 and view.data_ptr() == buf.data_ptr() + off * t.element_size()
    return buf, view


def _pitched(lg, pitch):
    """[n, nvox, 2] logits as rows of `pitch` floats; channels 2.. hold NaN, which must not reach anything."""
    if pitch == 2:
        return lg.contiguous()
    out = torch.full((*lg.shape[:-1], pitch), NAN)
    out[..., :2] = lg
    return out


def _refused(rc, text):
    assert rc == L.EINVAL, rc
    msg = L.lib().vsseg_last_error().decode()
    assert text in msg, msg


def _ints(t):
    torch.cuda.synchronize()
    return t.view(torch.int64).cpu().clone()


def _track(key, ratio):
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"dice sums error/bound [{key}]: this row {ratio:.3g}, worst so far {WORST[key]:.3g}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the sums kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.SUMS_CASES, ids=lambda c: c["name"])
def test_pred_and_att_sums(case):
    lib = L.lib()
    n, nvox, pitch, s = case["n"], case["nvox"], case["pitch"], D._seed(case["name"])
    lg, lab, att = D.make_logits(s, n, nvox, case["logits"]), D.make_label(s, n, nvox, case["label"]), D.make_att(s, n, nvox)
    off = case["offset"]
    _, lgd = _place(_pitched(lg, pitch), D.OFF_LOGITS // 4 if off else 0, fill=NAN)
    _, labd = _place(lab, D.OFF_LABEL // 4 if off else 0, fill=NAN)
    _, attd = _place(att, D.OFF_LABEL // 4 if off else 0, fill=NAN)
    la = D.sums_launch(nvox, n, pitch, (lgd.data_ptr(), labd.data_ptr()))
    assert la["vector"] == case["want"]["vector"] and la["blocks"] == case["want"].get("blocks", la["blocks"])
    sums = torch.zeros(n * 6, dtype=F64, device="cuda")
    for hard in (1, 0):
        sums.zero_()
        L.check(lib.vsseg_dice_pred_sums(lgd.data_ptr(), pitch, labd.data_ptr(), n, nvox, hard, sums.data_ptr(), H.stream()), "dice_pred_sums")
        once = _ints(sums)
        L.check(lib.vsseg_dice_pred_sums(lgd.data_ptr(), pitch, labd.data_ptr(), n, nvox, hard, sums.data_ptr(), H.stream()), "dice_pred_sums")
        D.assert_equal(_ints(sums).reshape(n, 6), 2 * once.reshape(n, 6), f"{case['name']}: a second launch into the same sums (hardness {hard})")
        got, ref = D.fx_decode(once).reshape(n, 6), D.pred_sums(lg, lab, bool(hard))
        _track("pred_sums", D.assert_within(got, ref, D.sum_bound(lg, lab, bool(hard), la["workgroups"]), f"{case['name']}: prediction sums, hardness {hard}"))
        if not hard:
            D.assert_equal(got[:, [1, 4]], ref[:, [1, 4]], f"{case['name']}: G without hardness")
    asum = torch.zeros(n * 3, dtype=F64, device="cuda")
    L.check(lib.vsseg_dice_att_sums(attd.data_ptr(), labd.data_ptr(), n, nvox, asum.data_ptr(), H.stream()), "dice_att_sums")
    once = _ints(asum)
    D.assert_equal(once.reshape(n, 3), D.fx_encode(D.att_sums(att, lab)), f"{case['name']}: attention-map sums")
    L.check(lib.vsseg_dice_att_sums(attd.data_ptr(), labd.data_ptr(), n, nvox, asum.data_ptr(), H.stream()), "dice_att_sums")
    D.assert_equal(_ints(asum), 2 * once, f"{case['name']}: a second launch into the same attention sums")
    if case.get("ce"):  # vsseg_ce_sums shares the launch shape: its second grid-stride round is reached only here
        csum = torch.zeros(3, dtype=F64, device="cuda")
        L.check(lib.vsseg_ce_sums(lgd.data_ptr(), pitch, labd.data_ptr(), n, nvox, csum.data_ptr(), H.stream()), "ce_sums")
        got, ref = D.fx_decode(_ints(csum), D.FX_STAT), D.ce_sums(lg, lab)
        D.assert_equal(got[2:], ref[2:], f"{case['name']}: foreground count of vsseg_ce_sums")
        _track("ce_sums", D.assert_within(got[:2], ref[:2], D.ce_bound(lg, lab, la["workgroups"] * n), f"{case['name']}: vsseg_ce_sums"))
    assert V.fx_status() is False


def test_sums_refuse_empty_and_malformed_arguments():
    lib = L.lib()
    x = torch.zeros(64, device="cuda")
    s = torch.zeros(6, dtype=F64, device="cuda")
    _refused(lib.vsseg_dice_pred_sums(x.data_ptr(), 2, x.data_ptr(), 1, 0, 1, s.data_ptr(), H.stream()), "vsseg_dice_pred_sums: bad arguments")
    _refused(lib.vsseg_dice_pred_sums(x.data_ptr(), 2, x.data_ptr(), 0, 4, 1, s.data_ptr(), H.stream()), "vsseg_dice_pred_sums: bad arguments")
    _refused(lib.vsseg_dice_pred_sums(x.data_ptr(), 3, x.data_ptr(), 1, 4, 1, s.data_ptr(), H.stream()), "vsseg_dice_pred_sums: bad arguments")
    _refused(lib.vsseg_dice_att_sums(x.data_ptr(), x.data_ptr(), 1, 0, s.data_ptr(), H.stream()), "vsseg_dice_att_sums: bad arguments")
    _refused(lib.vsseg_dice_att_sums(x.data_ptr(), x.data_ptr(), 0, 4, s.data_ptr(), H.stream()), "vsseg_dice_att_sums: bad arguments")
    torch.cuda.synchronize()
    assert not bool(s.any())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. vsseg_maxpool_label
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.POOL_CASES, ids=lambda c: c["name"])
def test_maxpool_label(case):
    lib = L.lib()
    src = D.pool_inputs(case)
    n, sdims, dst_dims = case["n"], tuple(src.shape[2:]), case["dst"]
    _, srcd = _place(src, fill=NAN)
    buf, dst = _place(torch.full((n, math.prod(dst_dims)), NAN), 4, 4)
    L.check(lib.vsseg_maxpool_label(srcd.data_ptr(), n, L.i3(sdims), L.i3(case["ratio"]), dst.data_ptr(), H.stream()), "maxpool_label")
    torch.cuda.synchronize()
    D.assert_equal(dst.reshape(n, -1), D.pool(src, case["ratio"]).reshape(n, -1), f"{case['name']}: pooled label")
    assert bool((buf[:4] == 7.0).all()) and bool((buf[-4:] == 7.0).all())


def test_maxpool_label_refuses_shapes_that_do_not_divide():
    lib = L.lib()
    x = torch.zeros(5 * 4 * 4, device="cuda")
    for sdims, ratio in (((5, 4, 4), (2, 2, 2)), ((4, 5, 4), (1, 2, 1)), ((4, 4, 5), (1, 1, 4))):
        _refused(lib.vsseg_maxpool_label(x.data_ptr(), 1, L.i3(sdims), L.i3(ratio), x.data_ptr(), H.stream()), "attention pyramid shapes must divide (ref dice_spvPA.py:273)")
    _refused(lib.vsseg_maxpool_label(x.data_ptr(), 1, L.i3((4, 4, 4)), L.i3((0, 1, 1)), x.data_ptr(), H.stream()), "vsseg_maxpool_label: bad arguments")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. vsseg_dice_level_sums
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", D.LEVEL_CASES, ids=lambda c: c["name"])
def test_level_sums(case):
    lib = L.lib()
    n, d = case["n"], case["dims"]
    nvox = math.prod(d)
    lg, att, lab5 = D.level_inputs(case)
    lab = lab5.reshape(n, -1)
    _, lgd = _place(lg, fill=NAN)
    _, attd = _place(att, fill=NAN)
    _, labd = _place(lab, fill=NAN)
    la = D.level_launch(d, n)
    assert la["blocks"] == case["want"]["blocks"]
    want_pool = D.pool(lab5, (2, 2, 1)).reshape(n, -1)
    want_att = D.fx_encode(D.att_sums(att, lab))
    for with_logits in (True, False):
        for with_pooled in (True, False):
            hard = 1 if with_pooled else 0
            psum, asum = torch.zeros(n * 6, dtype=F64, device="cuda"), torch.zeros(n * 3, dtype=F64, device="cuda")
            pbuf, pooled = _place(torch.full((n, nvox // 4), NAN), 4, 4)
            L.check(lib.vsseg_dice_level_sums(lgd.data_ptr() if with_logits else None, attd.data_ptr(), labd.data_ptr(), n, L.i3(d), hard, psum.data_ptr() if with_logits else None, asum.data_ptr(),
                                              pooled.data_ptr() if with_pooled else None, H.stream()), "dice_level_sums")
            what = f"{case['name']} logits={with_logits} pooled={with_pooled}"
            D.assert_equal(_ints(asum).reshape(n, 3), want_att, f"{what}: attention-map sums")
            if with_pooled:
                D.assert_equal(pooled.reshape(n, -1), want_pool, f"{what}: pooled label")
            else:
                assert bool(torch.isnan(pooled).all())
            assert bool((pbuf[:4] == 7.0).all()) and bool((pbuf[-4:] == 7.0).all())
            if with_logits:
                got, ref = D.fx_decode(_ints(psum)).reshape(n, 6), D.pred_sums(lg, lab, bool(hard))
                _track("level_sums", D.assert_within(got, ref, D.sum_bound(lg, lab, bool(hard), la["workgroups"]), f"{what}: prediction sums"))
                if not hard:
                    D.assert_equal(got[:, [1, 4]], ref[:, [1, 4]], f"{what}: G without hardness")
            else:
                assert not bool(_ints(psum).any())
    assert V.fx_status() is False


def test_level_sums_refusals():
    lib = L.lib()
    x = torch.zeros(4096, device="cuda")
    s = torch.zeros(6, dtype=F64, device="cuda")

    def call(dims, att_off=0, logits=True):
        return lib.vsseg_dice_level_sums(x.data_ptr() if logits else None, x.data_ptr() + att_off, x.data_ptr(), 1, L.i3(dims), 1, s.data_ptr(), s.data_ptr(), x.data_ptr() + 8192, H.stream())

    _refused(call((3, 2, 4)), "3 x 2 x 4 is not made of 2 x 2 x 4 blocks")
    _refused(call((2, 5, 4)), "2 x 5 x 4 is not made of 2 x 2 x 4 blocks")
    _refused(call((2, 2, 6)), "2 x 2 x 6 is not made of 2 x 2 x 4 blocks")
    _refused(call((2, 2, 4), att_off=8), "operands must be 16-byte aligned")
    _refused(lib.vsseg_dice_level_sums(x.data_ptr(), x.data_ptr(), x.data_ptr(), 1, L.i3((2, 2, 4)), 1, None, s.data_ptr(), None, H.stream()), "vsseg_dice_level_sums: bad arguments")
    torch.cuda.synchronize()
    assert not bool(s.any())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. vsseg_dice_tail_sums
# ---------------------------------------------------------------------------------------------------------------------------------------------
def _tail_desc(n, sdims, levels, src, atts, labels, sums):
    td = L.DiceTailDesc()
    td.n, td.nlevels, td.src, td.sdims, td.sums = n, len(levels), src.data_ptr(), L.i3(sdims), sums.data_ptr()
    for j, d in enumerate(levels[: L.DICE_MAX_LEVELS]):
        td.att[j], td.label[j] = atts[j].data_ptr(), (None if labels[j] is None else labels[j].data_ptr())
        td.dims[j][0], td.dims[j][1], td.dims[j][2] = d
    return td


@pytest.mark.parametrize("case", D.TAIL_CASES, ids=lambda c: c["name"])
def test_tail_sums(case):
    lib = L.lib()
    sdims, levels, _ = D.TAIL_ROWS[case["row"]]
    n = case["n"]
    src, atts = D.tail_inputs(case)
    _, srcd = _place(src, fill=NAN)
    attd = [_place(a, fill=NAN)[1] for a in atts]
    has_source_level = any(tuple(d) == tuple(sdims) for d in levels)
    for null_source_label in ((False, True) if has_source_level else (False,)):  # label[i] == NULL where level i is the source level: nothing to write
        bufs = [_place(torch.full((n, math.prod(d)), NAN), 4, 4) for d in levels]
        labels = [None if (null_source_label and tuple(d) == tuple(sdims)) else b[1] for d, b in zip(levels, bufs)]
        sums = torch.zeros(len(levels) * n * 3, dtype=F64, device="cuda")
        L.check(lib.vsseg_dice_tail_sums(_tail_desc(n, sdims, levels, srcd, attd, labels, sums), H.stream()), "dice_tail_sums")
        got = _ints(sums).reshape(len(levels), n, 3)
        for i, d in enumerate(levels):
            g = D.pool_from(src, d).reshape(n, -1)
            what = f"{case['name']} level {i} {tuple(d)} (label[{i}] {'NULL' if labels[i] is None else 'given'})"
            if labels[i] is not None:
                D.assert_equal(labels[i].reshape(n, -1), g, f"{what}: pooled label", level=i)
            else:
                assert bool(torch.isnan(bufs[i][1]).all())
            assert bool((bufs[i][0][:4] == 7.0).all()) and bool((bufs[i][0][-4:] == 7.0).all()), what
            D.assert_equal(got[i], D.fx_encode(D.att_sums(atts[i], g)), f"{what}: attention-map sums", level=i)
    assert V.fx_status() is False


def test_tail_sums_refusals():
    lib = L.lib()
    x = torch.zeros(4096, device="cuda")
    sums = torch.zeros(9 * 3, dtype=F64, device="cuda")
    nine = [(4, 4, 4)] * 9
    td = _tail_desc(1, (4, 4, 4), nine, x, [x] * 9, [x] * 9, sums)
    assert td.nlevels == 9 == L.DICE_MAX_LEVELS + 1
    _refused(lib.vsseg_dice_tail_sums(td, H.stream()), "vsseg_dice_tail_sums: bad arguments")
    _refused(lib.vsseg_dice_tail_sums(_tail_desc(1, (4, 4, 4), [(2, 2, 2)], x, [x], [None], sums), H.stream()), "level 0 pools but has no label buffer")
    _refused(lib.vsseg_dice_tail_sums(_tail_desc(1, (4, 4, 4), [(4, 4, 4), (3, 2, 2)], x, [x, x], [None, x], sums), H.stream()), "attention pyramid shapes must divide (ref dice_spvPA.py:273)")
    _refused(lib.vsseg_dice_tail_sums(_tail_desc(0, (4, 4, 4), [(4, 4, 4)], x, [x], [None], sums), H.stream()), "vsseg_dice_tail_sums: bad arguments")
    torch.cuda.synchronize()
    assert not bool(sums.any())


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. vsseg_dice_finalize from hand-encoded sums
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nl", D.FINALIZE_ROWS)
def test_finalize_from_hand_encoded_sums(n, nl):
    lib = L.lib()
    pi, ai = D.hand_sums(n, nl)
    want_loss, want_coef = D.finalize(D.fx_decode(pi), D.fx_decode(ai) if nl else None)
    pd = pi.view(F64).cuda()
    ad = ai.view(F64).cuda() if nl else None
    ncoef = n * 4 + max(nl, 1) * n * 2
    used = n * 4 + nl * n * 2
    outs = []
    ce = torch.zeros(3, dtype=F64, device="cuda")
    rec = torch.tensor([0x3F800000 | (3 << 32), 1, 2, 2, 0, 0, 0, 0], dtype=torch.int64, device="cuda")  # threshold 1.0, 3 passes, n_gt 1, n_eq 2, K 2, sums 0
    for which in ("dice", "ce", "topk"):
        loss, coef, extra = torch.full((1,), 7.0, device="cuda"), torch.full((ncoef,), 7.0, device="cuda"), torch.full((8,), 7.0, device="cuda")
        ap = ad.data_ptr() if nl else None
        if which == "dice":
            L.check(lib.vsseg_dice_finalize(pd.data_ptr(), ap, n, nl, loss.data_ptr(), coef.data_ptr(), H.stream()), "dice_finalize")
        elif which == "ce":
            L.check(lib.vsseg_dice_ce_finalize(pd.data_ptr(), ap, n, nl, ce.data_ptr(), 100, 0.5, 2.0, loss.data_ptr(), coef.data_ptr(), extra.data_ptr(), H.stream()), "dice_ce_finalize")
        else:
            L.check(lib.vsseg_dice_ce_topk_finalize(pd.data_ptr(), ap, n, nl, rec.data_ptr(), 0.5, 2.0, loss.data_ptr(), coef.data_ptr(), extra.data_ptr(), H.stream()), "dice_ce_topk_finalize")
        torch.cuda.synchronize()
        outs.append((loss.cpu(), coef.cpu()))
    loss, coef = outs[0]
    print(f"finalize n={n} levels={nl}: loss {float(loss):.9g} (fp64 {float(want_loss):.12g}), max |coef| {float(want_coef.abs().max()):.6g}")
    D.assert_within(loss.double(), want_loss.reshape(1), D.ulp32(want_loss.reshape(1)), f"finalize n={n} levels={nl}: loss")
    D.assert_within(coef[:used].double().reshape(1, -1), want_coef[:used].reshape(1, -1), D.ulp32(want_coef[:used]).reshape(1, -1), f"finalize n={n} levels={nl}: coefficients")
    assert bool((coef[used:] == 7.0).all())  # (without levels the attention block is not written)
    for which, (l2, c2) in zip(("ce", "topk"), outs[1:]):
        assert torch.equal(c2.view(torch.int32), coef.view(torch.int32)), f"the Dice coefficient block of the {which} finaliser differs from vsseg_dice_finalize's"
    # the terms beside it: 0.5 * 0 / W with the zero CE sums; 0.5 * ((0 + 0) + (2 - 1) * 1.0) / 2 with the hand-made record
    assert torch.equal(outs[1][0], loss) and abs(float(outs[2][0]) - (float(want_loss) + 0.25)) <= 2 * float(D.ulp32(want_loss.reshape(1) + 0.25))
    _refused(lib.vsseg_dice_finalize(pd.data_ptr(), None, n, 1, loss.data_ptr(), coef.data_ptr(), H.stream()), "vsseg_dice_finalize: bad arguments")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. the backward kernels
# ---------------------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = {"f32x2": (torch.float32, 2), "bf16x2": (torch.bfloat16, 2), "bf16x8": (torch.bfloat16, 8), "f32x8": (torch.float32, 8)}
assert tuple(LAYOUTS) == D.BWD_LAYOUTS


def _dst_desc(view, dt, pitch, n, nvox):
    return L.Tensor(view.data_ptr(), L.BF16 if dt == torch.bfloat16 else L.F32, 2, pitch, n, nvox, 1, 1, None, 0, L.ZERO_PADDED if pitch == 8 else 0)


def _check_dst(buf, view, off, guard, dt, pitch, n, nvox, ref, what):
    torch.cuda.synchronize()
    got = view.reshape(n, nvox, pitch).cpu()
    worst = D.check_grad("bf16" if dt == torch.bfloat16 else "fp32", got[..., :2].float() if dt == torch.bfloat16 else got[..., :2], ref, what)
    if pitch == 8:  # bf16 rows are written whole (zeros, as the cast pass writes them); fp32 rows keep what was there
        assert bool((got[..., 2:] == (0.0 if dt == torch.bfloat16 else 7.0)).all()), f"{what}: channels 2..7"
    assert bool((buf[:off] == 7.0).all()) and bool((buf[buf.numel() - guard:] == 7.0).all()), f"{what}: a row outside the destination was written"
    return worst


def _bwd_row(row):
    """One row of dice_oracle.BWD_ROWS: vsseg_dice_pred_bwd and vsseg_dice_pred_bwd_to in the row's layouts (all four unless it names some)."""
    lib = L.lib()
    n, nvox, kind, pitch, hard, gs, offset, ce_too = (row[k] for k in ("n", "nvox", "kind", "pitch", "hard", "gs", "offset", "ce"))
    layouts = {k: LAYOUTS[k] for k in row.get("layouts", D.BWD_LAYOUTS)}
    lg, lab, coef = D.bwd_inputs(row)
    coef = coef.cuda()
    gsd = torch.tensor([GS], device="cuda") if gs else None
    gp = gsd.data_ptr() if gs else None
    ref = D.dlogits(lg, lab, bool(hard), coef.cpu(), float(gsd.cpu()[0]) if gs else 1.0)
    _, lgd = _place(_pitched(lg, pitch), D.OFF_LOGITS // 4 if offset else 0, fill=NAN)
    _, labd = _place(lab, D.OFF_LABEL // 4 if offset else 0, fill=NAN)
    what = f"dlogits n={n} nvox={nvox} {kind} pitch={pitch} hard={hard} gs={gs} offset={offset}"
    args = (lgd.data_ptr(), pitch, labd.data_ptr(), n, nvox, hard, coef.data_ptr())
    la = D.bwd_launch(nvox, pitch, (lgd.data_ptr(), labd.data_ptr()))
    assert la["vector"] == (pitch == 2 and nvox % 4 == 0 and not offset)
    off32 = 4 + (D.OFF_LOGITS // 4 if offset else 0)  # four guard floats (16 bytes) in front, then the deliberate 8 bytes
    buf, out = _place(torch.full((n * nvox * 2,), 7.0), off32, 8)
    L.check(lib.vsseg_dice_pred_bwd(*args, gp, out.data_ptr(), H.stream()), "dice_pred_bwd")
    _check_dst(buf, out, off32, 8, torch.float32, 2, n, nvox, ref, f"{what} vsseg_dice_pred_bwd")
    plain = out.clone()
    for name, (dt, dpitch) in layouts.items():
        es = 2 if dt == torch.bfloat16 else 4
        off = 16 // es + (D.OFF_LOGITS // es if offset else 0)
        buf, dst = _place(torch.full((n * nvox * dpitch,), 7.0, dtype=dt), off, 16)
        rc = lib.vsseg_dice_pred_bwd_to(*args, gp, _dst_desc(dst, dt, dpitch, n, nvox), H.stream())
        if name == "bf16x8" and offset:  # its rows are stored 16 bytes at a time
            _refused(rc, "is not one the training plan stages the gradient in")
            continue
        L.check(rc, "dice_pred_bwd_to")
        _check_dst(buf, dst, off, 16, dt, dpitch, n, nvox, ref, f"{what} vsseg_dice_pred_bwd_to {name}")
        if name == "f32x2":
            assert torch.equal(dst, plain), f"{what}: the fp32 layout of vsseg_dice_pred_bwd_to differs from vsseg_dice_pred_bwd"
    if ce_too:  # the entry points that add a cross-entropy gradient, with that term's coefficients zero: the Dice part they share, at the same bar (they are
        # other instantiations of the kernel: the compiler may fuse other multiply-adds in them, so their bits may differ from vsseg_dice_pred_bwd's by an fp32 rounding)
        zero = torch.zeros(8, device="cuda")
        for fn, fn_to in ((lib.vsseg_dice_ce_pred_bwd, lib.vsseg_dice_ce_pred_bwd_to), (lib.vsseg_dice_ce_topk_pred_bwd, lib.vsseg_dice_ce_topk_pred_bwd_to)):
            b2, o2 = _place(torch.full((n * nvox * 2,), 7.0), off32, 8)
            L.check(fn(*args, zero.data_ptr(), gp, o2.data_ptr(), H.stream()), "dice_ce_pred_bwd")
            b3, o3 = _place(torch.full((n * nvox * 2,), 7.0), off32, 8)
            L.check(fn_to(*args, zero.data_ptr(), gp, _dst_desc(o3, torch.float32, 2, n, nvox), H.stream()), "dice_ce_pred_bwd_to")
            _check_dst(b2, o2, off32, 8, torch.float32, 2, n, nvox, ref, f"{what} {fn.__name__} with zero cross-entropy coefficients")
            _check_dst(b3, o3, off32, 8, torch.float32, 2, n, nvox, ref, f"{what} {fn_to.__name__} with zero cross-entropy coefficients")
            assert torch.equal(o2, o3), f"{what}: {fn_to.__name__} differs from {fn.__name__}"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("nvox", D.NVOX)
def test_pred_bwd_every_layout(nvox, n):
    rows = [r for r in D.BWD_ROWS if r["kind"] == "synth" and (r["nvox"], r["n"]) == (nvox, n)]
    assert len(rows) == 10
    for r in rows:
        _bwd_row(r)


@pytest.mark.parametrize("nvox", [1023, 1024])
def test_pred_bwd_saturated_logits(nvox):
    rows = [r for r in D.BWD_ROWS if r["kind"] == "saturated" and r["nvox"] == nvox]
    assert len(rows) == 3
    for r in rows:
        _bwd_row(r)


def test_pred_bwd_second_grid_stride_round():
    """nvox = 2048 * 256 * 4 + 1028: the grid is at its cap and 257 threads take a second quad.  The WHOLE tensor is compared with the fp64 definition (2 M voxels
    take a fraction of a second on the CPU), not a strided sample of it."""
    (row,) = [r for r in D.BWD_ROWS if r["nvox"] == D.BWD_BIG]
    assert D.bwd_launch(D.BWD_BIG, 2, (0, 0, 0))["rounds"] == 2
    _bwd_row(row)


def test_pred_bwd_refusals():
    lib = L.lib()
    x = torch.zeros(64, device="cuda")
    c = torch.zeros(4, device="cuda")
    _refused(lib.vsseg_dice_pred_bwd(x.data_ptr(), 2, x.data_ptr(), 1, 0, 1, c.data_ptr(), None, x.data_ptr(), H.stream()), "vsseg_dice_pred_bwd: bad arguments")
    _refused(lib.vsseg_dice_pred_bwd(x.data_ptr(), 2, x.data_ptr(), 0, 4, 1, c.data_ptr(), None, x.data_ptr(), H.stream()), "vsseg_dice_pred_bwd: bad arguments")
    _refused(lib.vsseg_dice_pred_bwd_to(x.data_ptr(), 2, x.data_ptr(), 1, 4, 1, c.data_ptr(), None, L.Tensor(x.data_ptr(), L.F32, 2, 2, 1, 5, 1, 1), H.stream()), "destination is not a 2-channel tensor of 4 voxels")
    _refused(lib.vsseg_dice_pred_bwd_to(x.data_ptr(), 2, x.data_ptr(), 1, 4, 1, c.data_ptr(), None, L.Tensor(x.data_ptr(), L.F32, 3, 4, 1, 4, 1, 1), H.stream()), "destination is not a 2-channel tensor of 4 voxels")
    _refused(lib.vsseg_dice_pred_bwd_to(x.data_ptr(), 2, x.data_ptr(), 1, 4, 1, c.data_ptr(), None, L.Tensor(x.data_ptr(), L.BF16, 2, 4, 1, 4, 1, 1), H.stream()), "is not one the training plan stages the gradient in")
    torch.cuda.synchronize()
    assert not bool(x.any())


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("gs", [False, True])
@pytest.mark.parametrize("n", [1, 3])
def test_att_bwd_and_att_bwd_levels(n, gs, offset):
    lib = L.lib()
    nl = len(D.ATT_BWD_NVOX)
    coef = torch.tensor([[[-(0.1 + 0.01 * (3 * l + b)), 0.003 + 0.0007 * (3 * l + b)] for b in range(n)] for l in range(nl)], device="cuda")  # [level][sample][A, B]
    gsd = torch.tensor([GS], device="cuda") if gs else None
    gp = gsd.data_ptr() if gs else None
    o = D.OFF_LABEL // 4 if offset else 0
    labs = [D.make_label(60 + l, n, v) for l, v in enumerate(D.ATT_BWD_NVOX)]
    labd = [_place(g, o, fill=NAN)[1] for g in labs]
    one = [_place(torch.full((n * v,), NAN), 4 + o, 4) for v in D.ATT_BWD_NVOX]
    many = [_place(torch.full((n * v,), NAN), 4 + o, 4) for v in D.ATT_BWD_NVOX]
    bd = L.DiceBwdLevelsDesc()
    bd.n, bd.nlevels, bd.gscale = n, nl, gp
    for l, v in enumerate(D.ATT_BWD_NVOX):
        assert D.bwd_launch(v, 2, (labd[l].data_ptr(), one[l][1].data_ptr()))["vector"] == (v % 4 == 0 and not offset)
        L.check(lib.vsseg_dice_att_bwd(labd[l].data_ptr(), n, v, coef[l].data_ptr(), 1.0 / nl, gp, one[l][1].data_ptr(), H.stream()), "dice_att_bwd")
        bd.label[l], bd.datt[l], bd.nvox[l], bd.coef[l] = labd[l].data_ptr(), many[l][1].data_ptr(), v, coef[l].data_ptr()
    L.check(lib.vsseg_dice_att_bwd_levels(bd, H.stream()), "dice_att_bwd_levels")
    torch.cuda.synchronize()
    for l, v in enumerate(D.ATT_BWD_NVOX):
        want = D.datt_fp32(labs[l], coef[l], float(gsd.cpu()[0]) if gs else None)
        for name, (buf, dst) in (("vsseg_dice_att_bwd", one[l]), ("vsseg_dice_att_bwd_levels", many[l])):
            D.assert_equal(dst.reshape(n, v), want, f"{name} n={n} gs={gs} offset={offset}: level of {v} voxels", level=l)
            assert bool((buf[: 4 + o] == 7.0).all()) and bool((buf[-4:] == 7.0).all())
        assert torch.equal(one[l][1].view(torch.int32), many[l][1].view(torch.int32))
        assert float((want.double() - D.datt(labs[l], coef[l].cpu(), GS if gs else 1.0)).abs().max()) <= 4 * D.U24 * float(coef[l].abs().max())  # (and the fp32 values are the fp64 definition's)


def test_att_bwd_refusals():
    lib = L.lib()
    x = torch.zeros(64, device="cuda")
    _refused(lib.vsseg_dice_att_bwd(x.data_ptr(), 0, 4, x.data_ptr(), 1.0, None, x.data_ptr(), H.stream()), "vsseg_dice_att_bwd: bad arguments")
    _refused(lib.vsseg_dice_att_bwd(x.data_ptr(), 1, 0, x.data_ptr(), 1.0, None, x.data_ptr(), H.stream()), "vsseg_dice_att_bwd: bad arguments")
    _refused(lib.vsseg_dice_att_bwd(None, 1, 4, x.data_ptr(), 1.0, None, x.data_ptr(), H.stream()), "vsseg_dice_att_bwd: bad arguments")
    bd = L.DiceBwdLevelsDesc()
    bd.n, bd.nlevels = 1, L.DICE_MAX_LEVELS + 1
    _refused(lib.vsseg_dice_att_bwd_levels(bd, H.stream()), "vsseg_dice_att_bwd_levels: bad arguments")
    bd.nlevels = 1
    bd.label[0], bd.datt[0], bd.coef[0], bd.nvox[0] = x.data_ptr(), x.data_ptr(), x.data_ptr(), 0
    _refused(lib.vsseg_dice_att_bwd_levels(bd, H.stream()), "level 0 is incomplete")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 7. vsseg_hard_dice_counts and vsseg_argmax2
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nvox,pitch", D.ARGMAX_ROWS)
def test_hard_dice_counts_and_argmax(nvox, pitch):
    lib = L.lib()
    lg, lab = D.argmax_inputs(nvox, pitch)
    _, lgd = _place(lg, fill=NAN)
    _, labd = _place(lab, fill=NAN)
    counts = torch.zeros(3, dtype=F64, device="cuda")
    L.check(lib.vsseg_hard_dice_counts(lgd.data_ptr(), pitch, labd.data_ptr(), nvox, counts.data_ptr(), H.stream()), "hard_dice_counts")
    buf, dst = _place(torch.full((nvox,), 9, dtype=torch.uint8), 16, 16, fill=7)
    L.check(lib.vsseg_argmax2(lgd.data_ptr(), pitch, nvox, dst.data_ptr(), H.stream()), "argmax2")
    torch.cuda.synchronize()
    D.assert_equal(counts.cpu().reshape(1, 3), D.hard_counts(lg[:, :2], lab).reshape(1, 3), f"hard-Dice counts of {nvox} voxels, pitch {pitch}")
    D.assert_equal(dst.cpu().to(torch.int64).reshape(1, -1), D.argmax2(lg[:, :2]).reshape(1, -1), f"argmax of {nvox} voxels, pitch {pitch}")
    assert bool((buf[:16] == 7).all()) and bool((buf[-16:] == 7).all())
    assert int(D.argmax2(lg[:, :2])[::5].sum()) == 0  # the ties are in the input, and want class 0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 8. the module: Dice_spvPA and forward_backward_into against autograd of the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hardness", [True, False])
@pytest.mark.parametrize("supervised", [True, False])
@pytest.mark.parametrize("name", list(D.MODULE_ROWS))
def test_module_against_autograd_of_the_oracle(name, supervised, hardness, monkeypatch):
    from vs_seg_amd.losses import dice_spvPA as M

    B, dims, att_dims, plan = D.MODULE_ROWS[name]
    lab5, logits5, atts = D.module_inputs(name)
    bars = D.module_bars(name, supervised, hardness)
    if bars["big_denominators"]:
        assert bars["loss_bar"] == 5e-6 and bars["min_denominator"] >= 1.0 and bars["rel_sums"] <= 1e-5
    # the fp64 reference: autograd of the oracle
    lg64 = logits5.double().requires_grad_(True)
    at64 = [a.double().requires_grad_(True) for a in atts]
    want = O.dice_spvpa(lg64, at64, lab5.double(), supervised_attention=supervised, hardness_weighting=hardness)
    want.backward()
    plans = []
    real = M._fused_plan
    monkeypatch.setattr(M, "_fused_plan", lambda *a, **k: plans.append(real(*a, **k)) or plans[-1])
    fn = V.Dice_spvPA(to_onehot_y=True, softmax=True, supervised_attention=supervised, hardness_weighting=hardness)
    y = lab5.cuda()
    lgd = logits5.cuda().requires_grad_(True)
    atd = [a.cuda().requires_grad_(True) for a in atts]
    loss = fn((lgd, atd), y)
    loss.backward()
    assert D.fused_plan(B, dims, att_dims) == plan and plans == ([plan] if supervised else []), (plans, plan)
    err = abs(float(loss) - float(want))
    print(f"{name} supervised={supervised} hardness={hardness}: plan {plan}, loss {float(loss):.9g} oracle {float(want):.12g} |diff| {err:.3g} (bar {bars['loss_bar']:.3g}, min G + P {bars['min_denominator']:.4g})")
    assert math.isfinite(float(loss)) and err <= bars["loss_bar"]
    D.assert_within(lgd.grad.reshape(1, -1), lg64.grad.reshape(1, -1), 5e-5 * float(lg64.grad.abs().max()), f"{name}: d loss / d logits")
    for i, (a, w) in enumerate(zip(atd, at64)):
        if supervised:
            D.assert_within(a.grad.reshape(B, -1), w.grad.reshape(B, -1), 5e-5 * float(w.grad.abs().max()), f"{name}: d loss / d att[{i}]", level=len(atts) - 1 - i)
        else:
            assert a.grad is None and w.grad is None
    # the one-call route writes the same loss and the same gradients where it is told to
    dst = torch.full((B, *dims, 2), 7.0, device="cuda")
    bufs = [torch.full((B, *d), 7.0, device="cuda") for d in att_dims]
    loss2, written = fn.forward_backward_into((lgd.detach(), [a.detach() for a in atd]), y, (L.Tensor(dst.data_ptr(), L.F32, 2, 2, B, *dims), bufs))
    torch.cuda.synchronize()
    assert torch.equal(loss2, loss.detach()) and torch.equal(dst, lgd.grad.permute(0, 2, 3, 4, 1))
    assert sorted(written) == (list(range(len(atts))) if supervised else [])
    for i in written:
        assert torch.equal(bufs[i].reshape(-1), atd[i].grad.reshape(-1)), f"{name}: attention map {i} of forward_backward_into"
    assert V.fx_status() is False
