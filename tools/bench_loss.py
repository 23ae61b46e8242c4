"""Micro-benchmark of the loss kernels at the benchmark shape (tuning tool): every launch of the fused loss phase alone, and the coarse-level tail launch by level subset.

    python tools/bench_loss.py [--batch 4] [--dims 384 128 128]

With --ce_weight LAMBDA [--ce_foreground_weight W] it times the cross-entropy term instead: the whole loss phase of the fused train step (Dice_spvPA.forward_backward_into,
gradient of the logits written as bf16) with ce_weight = 0 and with the term, in the same process, at the benchmark shape and at batch 2 of 384x384x64, and the two launches
the term adds or changes.

    python tools/bench_loss.py --ce_weight 1 [--ce_foreground_weight 1]

With --ce_topk PCT as well it times the top-k term (Dice_spvPA(ce_topk=PCT)): the loss phase with ce_weight = 0, with the plain term and with the top-k term, alternating
in the same process, at the same two shapes, for N(0, 1) logits and for the confident logits of a trained network, and the launches of the top-k term one by one.

    python tools/bench_loss.py --ce_weight 1 --ce_topk 10        # profiles/topk_loss_bench.txt

With any of --tversky_beta BETA, --focal_tversky_gamma GAMMA, --batch_dice, --ce_focal_gamma GAMMA it times the region and focal options (Dice_spvPA(tversky_beta=, ...)): the
loss phase of the plain loss, of the region options alone, of the plain cross-entropy term, of the focal term and of everything together, alternating in one process, at
the same two shapes, and the focal sums pass and backward beside the plain term's.

    python tools/bench_loss.py --ce_weight 1 --tversky_beta 0.7 --focal_tversky_gamma 0.75 --batch_dice --ce_focal_gamma 2        # profiles/region_loss_bench.txt
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import _lib as L  # noqa: E402


def timed(fn, reps=20):
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def bench_ce(lam, wfg, shapes):
    """The loss phase with and without the cross-entropy term, interleaved (three rounds each, the median), and the launches of the term on their own."""
    import vs_seg_amd as V

    lib = L.lib()
    S = torch.cuda.current_stream().cuda_stream
    ratios = [(2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (2, 2, 2)]
    print(f"loss phase of the fused train step (forward_backward_into, bf16 gradient of the logits), ce_weight 0 against ce_weight {lam}, ce_foreground_weight {wfg}")
    for B, d0 in shapes:
        dims = [d0]
        for r in ratios:
            dims.append(tuple(x // y for x, y in zip(dims[-1], r)))
        nvox = d0[0] * d0[1] * d0[2]
        torch.manual_seed(0)
        lg = torch.randn(B, *d0, 2, device="cuda")
        logits = lg.permute(0, 4, 1, 2, 3)  # channels-last storage, as the network hands it out
        lab = (torch.rand(B, 1, *d0, device="cuda") > 0.999).float()  # about one voxel in a thousand
        atts = [torch.rand(B, 1, *d, device="cuda") for d in reversed(dims)]
        dst = torch.empty(B, *d0, 2, device="cuda", dtype=torch.bfloat16)
        bufs = [torch.empty(B, *a.shape[2:], device="cuda") for a in atts]
        landing = (L.Tensor(dst.data_ptr(), L.BF16, 2, 2, B, *d0), bufs)
        off = V.Dice_spvPA(to_onehot_y=True, softmax=True)
        on = V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=lam, ce_foreground_weight=wfg)
        t_off, t_on = [], []
        for _ in range(3):
            t_off.append(timed(lambda: off.forward_backward_into((logits, atts), lab, landing)))
            t_on.append(timed(lambda: on.forward_backward_into((logits, atts), lab, landing)))
        a, b = sorted(t_off)[1], sorted(t_on)[1]
        l0, l1 = float(off.forward_backward_into((logits, atts), lab, landing)[0]), float(on.forward_backward_into((logits, atts), lab, landing)[0])
        print(f"batch {B} of {d0[0]}x{d0[1]}x{d0[2]} ({B * nvox / 1e6:.1f} M voxels): loss {l0:.6f} -> {l1:.6f}")
        print(f"  loss phase, ce_weight 0       {a:8.1f} us   (rounds: {', '.join(f'{t:.1f}' for t in t_off)})")
        print(f"  loss phase, ce_weight {lam:<7g} {b:8.1f} us   (rounds: {', '.join(f'{t:.1f}' for t in t_on)})")
        print(f"  added by the term             {b - a:8.1f} us")
        sums = torch.zeros(3, dtype=torch.float64, device="cuda")
        coef = torch.full((B * 4,), 1e-6, device="cuda")
        cek = torch.full((2,), 1e-8, device="cuda")
        l2 = lab.reshape(B, *d0)
        t = timed(lambda: lib.vsseg_ce_sums(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, sums.data_ptr(), S))
        print(f"  vsseg_ce_sums                 {t:8.1f} us   ({B * nvox * 12 / t / 1e6:.2f} TB/s over logits + label)")
        t0 = timed(lambda: lib.vsseg_dice_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), None, landing[0], S))
        t1 = timed(lambda: lib.vsseg_dice_ce_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), cek.data_ptr(), None, landing[0], S))
        print(f"  vsseg_dice_pred_bwd_to bf16   {t0:8.1f} us")
        print(f"  vsseg_dice_ce_pred_bwd_to     {t1:8.1f} us   ({t1 - t0:+.1f} us)")


def bench_topk(lam, wfg, pct, shapes):
    """The loss phase without the cross-entropy term, with the plain term and with the top-k term, alternating in one process (three rounds each, the median), and the
    launches the top-k term adds, one by one.  Twice per shape: N(0, 1) logits, whose values spread over many histogram bins, and the logits of a trained network — the
    background confidently right (logit difference 16 +- 2: values around 1e-7), the foreground undecided — where a few bins take almost every voxel."""
    import vs_seg_amd as V

    lib = L.lib()
    S = torch.cuda.current_stream().cuda_stream
    ratios = [(2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (2, 2, 2)]
    print(f"loss phase of the fused train step (forward_backward_into, bf16 gradient of the logits): ce_weight 0, ce_weight {lam} (plain term), ce_weight {lam} with ce_topk {pct}; ce_foreground_weight {wfg}")
    for B, d0 in shapes:
        dims = [d0]
        for r in ratios:
            dims.append(tuple(x // y for x, y in zip(dims[-1], r)))
        nvox = d0[0] * d0[1] * d0[2]
        budget = {(4, (384, 128, 128)): 259.0, (2, (384, 384, 64)): 227.0}.get((B, d0))
        torch.manual_seed(0)
        lab = (torch.rand(B, 1, *d0, device="cuda") > 0.999).float()  # about one voxel in a thousand
        atts = [torch.rand(B, 1, *d, device="cuda") for d in reversed(dims)]
        dst = torch.empty(B, *d0, 2, device="cuda", dtype=torch.bfloat16)
        bufs = [torch.empty(B, *a.shape[2:], device="cuda") for a in atts]
        landing = (L.Tensor(dst.data_ptr(), L.BF16, 2, 2, B, *d0), bufs)
        fns = [("ce_weight 0", V.Dice_spvPA(to_onehot_y=True, softmax=True)), (f"ce_weight {lam:g}", V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=lam, ce_foreground_weight=wfg)),
               (f"ce_weight {lam:g} ce_topk {pct:g}", V.Dice_spvPA(to_onehot_y=True, softmax=True, ce_weight=lam, ce_foreground_weight=wfg, ce_topk=pct))]
        for kind in ("N(0, 1) logits", "trained logits"):
            lg = torch.randn(B, *d0, 2, device="cuda")
            if kind == "trained logits":
                lg[..., 0] += 8.0 * (1.0 - lab.reshape(B, *d0))
                lg[..., 1] -= 8.0 * (1.0 - lab.reshape(B, *d0))
            logits = lg.permute(0, 4, 1, 2, 3)  # channels-last storage, as the network hands it out
            times = [[] for _ in fns]
            for _ in range(3):
                for t, (_, fn) in zip(times, fns):
                    t.append(timed(lambda: fn.forward_backward_into((logits, atts), lab, landing)))
            med = [sorted(t)[1] for t in times]
            losses = [float(fn.forward_backward_into((logits, atts), lab, landing)[0]) for _, fn in fns]
            rec = [int(v) for v in fns[2][1].topk_record.cpu().tolist()]
            print(f"batch {B} of {d0[0]}x{d0[1]}x{d0[2]} ({B * nvox / 1e6:.1f} M voxels), {kind}: losses {', '.join(f'{v:.6f}' for v in losses)}; K {rec[3]}, n_gt {rec[1]}, n_eq {rec[2]}")
            for (name, _), m, t in zip(fns, med, times):
                print(f"  loss phase, {name:<28s} {m:8.1f} us   (rounds: {', '.join(f'{x:.1f}' for x in t)})")
            print(f"  top-k against ce_weight 0                {med[2] - med[0]:8.1f} us" + (f"   (budget of an optional family: 1 % of the step = {budget:.0f} us)" if budget else ""))
            print(f"  top-k against the plain term             {med[2] - med[1]:8.1f} us")
            sums = torch.zeros(B * 6 + L.topk_scratch_bytes() // 8, dtype=torch.float64, device="cuda")
            rec_at = sums.data_ptr() + 8 * B * 6
            coef = torch.full((B * 4 + 6 * B * 2,), 1e-6, device="cuda")
            tk = torch.zeros(8, device="cuda")
            l2 = lab.reshape(B, *d0)
            k = V.topk_count(B * nvox, pct)

            def select():
                lib.vsseg_memset_zero(sums.data_ptr(), sums.numel() * 8, S)
                L.check(lib.vsseg_ce_topk_select(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, wfg, k, rec_at, S))

            t = timed(select)
            print(f"  vsseg_ce_topk_select (3 x histogram + scan) {t:6.1f} us   ({3 * B * nvox * 12 / t / 1e6:.2f} TB/s over three reads of logits + label)")
            t = timed(lambda: lib.vsseg_dice_ce_topk_finalize(sums.data_ptr(), None, B, 0, rec_at, lam, wfg, coef.data_ptr(), coef.data_ptr(), tk.data_ptr(), S))
            print(f"  vsseg_dice_ce_topk_finalize   {t:8.1f} us")
            cek = torch.full((2,), 1e-8, device="cuda")
            t0 = timed(lambda: lib.vsseg_dice_ce_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), cek.data_ptr(), None, landing[0], S))
            t1 = timed(lambda: lib.vsseg_dice_ce_topk_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), tk.data_ptr(), None, landing[0], S))
            print(f"  vsseg_dice_ce_pred_bwd_to bf16 {t0:7.1f} us")
            print(f"  vsseg_dice_ce_topk_pred_bwd_to {t1:7.1f} us   ({t1 - t0:+.1f} us)")
            t = timed(lambda: lib.vsseg_ce_sums(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, sums.data_ptr(), S))
            print(f"  vsseg_ce_sums (the plain term's pass) {t:6.1f} us")


def bench_region(lam, wfg, region, gc, shapes):
    """The loss phase of the plain loss, the region options alone, the plain cross-entropy term, the focal term and all together, alternating in one process (three rounds
    each, the median), and the launches the focal term adds or changes beside the plain term's."""
    import vs_seg_amd as V

    lib = L.lib()
    S = torch.cuda.current_stream().cuda_stream
    ratios = [(2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (2, 2, 2)]
    rk = dict(tversky_beta=region[0], focal_tversky_gamma=region[1], batch_dice=region[2]) if region else dict(tversky_beta=0.5)
    gc = gc or 2.0
    lam = lam or 1.0
    print(f"loss phase of the fused train step (forward_backward_into, bf16 gradient of the logits): region options {rk}, ce_weight {lam}, ce_foreground_weight {wfg}, ce_focal_gamma {gc}")
    for B, d0 in shapes:
        dims = [d0]
        for r in ratios:
            dims.append(tuple(x // y for x, y in zip(dims[-1], r)))
        nvox = d0[0] * d0[1] * d0[2]
        budget = {(4, (384, 128, 128)): 259.0, (2, (384, 384, 64)): 227.0}.get((B, d0))
        torch.manual_seed(0)
        lg = torch.randn(B, *d0, 2, device="cuda")
        logits = lg.permute(0, 4, 1, 2, 3)  # channels-last storage, as the network hands it out
        lab = (torch.rand(B, 1, *d0, device="cuda") > 0.999).float()  # about one voxel in a thousand
        atts = [torch.rand(B, 1, *d, device="cuda") for d in reversed(dims)]
        dst = torch.empty(B, *d0, 2, device="cuda", dtype=torch.bfloat16)
        bufs = [torch.empty(B, *a.shape[2:], device="cuda") for a in atts]
        landing = (L.Tensor(dst.data_ptr(), L.BF16, 2, 2, B, *d0), bufs)
        mk = lambda **kw: V.Dice_spvPA(to_onehot_y=True, softmax=True, **kw)  # noqa: E731
        fns = [("plain loss", mk()), ("region options", mk(**rk)), (f"ce_weight {lam:g}", mk(ce_weight=lam, ce_foreground_weight=wfg)),
               (f"ce_weight {lam:g} focal {gc:g}", mk(ce_weight=lam, ce_foreground_weight=wfg, ce_focal_gamma=gc)),
               ("region options + focal", mk(ce_weight=lam, ce_foreground_weight=wfg, ce_focal_gamma=gc, **rk))]
        times = [[] for _ in fns]
        for _ in range(3):
            for t, (_, fn) in zip(times, fns):
                t.append(timed(lambda: fn.forward_backward_into((logits, atts), lab, landing)))
        med = [sorted(t)[1] for t in times]
        losses = [float(fn.forward_backward_into((logits, atts), lab, landing)[0]) for _, fn in fns]
        print(f"batch {B} of {d0[0]}x{d0[1]}x{d0[2]} ({B * nvox / 1e6:.1f} M voxels): losses {', '.join(f'{v:.6f}' for v in losses)}")
        for (name, _), m, t in zip(fns, med, times):
            print(f"  loss phase, {name:<28s} {m:8.1f} us   (rounds: {', '.join(f'{x:.1f}' for x in t)})")
        print(f"  region options against the plain loss    {med[1] - med[0]:8.1f} us")
        print(f"  focal term against the plain term        {med[3] - med[2]:8.1f} us")
        print(f"  everything against the plain loss        {med[4] - med[0]:8.1f} us" + (f"   (budget of an optional family: 1 % of the step = {budget:.0f} us)" if budget else ""))
        sums = torch.zeros(3, dtype=torch.float64, device="cuda")
        coef = torch.full((B * 6,), 1e-6, device="cuda")
        cek = torch.full((2,), 1e-8, device="cuda")
        l2 = lab.reshape(B, *d0)
        t0 = timed(lambda: lib.vsseg_ce_sums(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, sums.data_ptr(), S))
        t1 = timed(lambda: lib.vsseg_ce_focal_sums(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, gc, sums.data_ptr(), S))
        print(f"  vsseg_ce_sums                 {t0:8.1f} us   ({B * nvox * 12 / t0 / 1e6:.2f} TB/s over logits + label)")
        print(f"  vsseg_ce_focal_sums           {t1:8.1f} us   ({B * nvox * 12 / t1 / 1e6:.2f} TB/s, {t1 - t0:+.1f} us)")
        o = L.LossOpts()
        o.ce_mode, o.ce_weight, o.ce_foreground_weight, o.ce_focal_gamma, o.tversky_beta, o.focal_tversky_gamma = L.CE_FOCAL, lam, wfg, gc, rk["tversky_beta"], rk.get("focal_tversky_gamma", 1.0)
        t0 = timed(lambda: lib.vsseg_dice_ce_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), cek.data_ptr(), None, landing[0], S))
        t1 = timed(lambda: L.check(lib.vsseg_loss_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), cek.data_ptr(), o, None, landing[0], S)))
        o.region = 1
        t2 = timed(lambda: L.check(lib.vsseg_loss_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), cek.data_ptr(), o, None, landing[0], S)))
        print(f"  vsseg_dice_ce_pred_bwd_to bf16        {t0:8.1f} us")
        print(f"  vsseg_loss_pred_bwd_to focal          {t1:8.1f} us   ({t1 - t0:+.1f} us)")
        print(f"  vsseg_loss_pred_bwd_to region + focal {t2:8.1f} us   ({t2 - t0:+.1f} us)")
        o.ce_mode, o.batch_dice = L.CE_NONE, int(rk.get("batch_dice", False))
        t0 = timed(lambda: lib.vsseg_dice_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), None, landing[0], S))
        t1 = timed(lambda: L.check(lib.vsseg_loss_pred_bwd_to(lg.data_ptr(), 2, l2.data_ptr(), B, nvox, 1, coef.data_ptr(), None, o, None, landing[0], S)))
        print(f"  vsseg_dice_pred_bwd_to bf16           {t0:8.1f} us")
        print(f"  vsseg_loss_pred_bwd_to region         {t1:8.1f} us   ({t1 - t0:+.1f} us)")
        fsums = torch.full((B * 6 + 6 * B * 3,), 3.0, dtype=torch.float64, device="cuda")  # (fixed-point slots: any bit pattern is a value)
        fout = torch.zeros(1 + B * 6 + 6 * B * 2, device="cuda")
        t0 = timed(lambda: lib.vsseg_dice_finalize(fsums.data_ptr(), fsums.data_ptr() + 8 * B * 6, B, 6, fout.data_ptr(), fout.data_ptr() + 4, S))
        t1 = timed(lambda: L.check(lib.vsseg_loss_finalize(fsums.data_ptr(), fsums.data_ptr() + 8 * B * 6, B, 6, None, nvox, o, fout.data_ptr(), fout.data_ptr() + 4, None, S)))
        print(f"  vsseg_dice_finalize                   {t0:8.1f} us")
        print(f"  vsseg_loss_finalize region            {t1:8.1f} us   ({t1 - t0:+.1f} us)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--dims", type=int, nargs=3, default=[384, 128, 128])
    ap.add_argument("--ce_weight", type=float, default=0.0, help="> 0: time the loss phase with and without the cross-entropy term instead (at the benchmark shape and at batch 2 of 384x384x64)")
    ap.add_argument("--ce_foreground_weight", type=float, default=1.0)
    ap.add_argument("--ce_topk", type=float, default=0.0, metavar="PCT", help="> 0 (with --ce_weight): time the loss phase without the term, with the plain term and with the top-k term over the hardest PCT percent")
    ap.add_argument("--tversky_beta", type=float, default=None, metavar="BETA", help="time the region and focal options: the Tversky ratio with this beta")
    ap.add_argument("--focal_tversky_gamma", type=float, default=1.0, metavar="GAMMA")
    ap.add_argument("--batch_dice", action="store_true")
    ap.add_argument("--ce_focal_gamma", type=float, default=0.0, metavar="GAMMA", help="(with --ce_weight) the exponent of the focal cross-entropy term")
    a = ap.parse_args()
    from vs_seg_amd import check_ce, check_ce_topk, check_region

    try:
        lam, wfg = check_ce(a.ce_weight, a.ce_foreground_weight)
        pct = check_ce_topk(a.ce_topk, lam)
        region, gc = check_region(a.tversky_beta, a.focal_tversky_gamma, a.batch_dice, a.ce_focal_gamma, lam, pct)
    except ValueError as e:
        ap.error(str(e))
    if region is not None or gc > 0:
        bench_region(lam, wfg, region, gc, [(a.batch, tuple(a.dims)), (2, (384, 384, 64))])
        return
    if pct > 0:
        bench_topk(lam, wfg, pct, [(a.batch, tuple(a.dims)), (2, (384, 384, 64))])
        return
    if lam > 0:
        bench_ce(lam, wfg, [(a.batch, tuple(a.dims)), (2, (384, 384, 64))])
        return
    lib = L.lib()
    S = torch.cuda.current_stream().cuda_stream
    B, d0 = a.batch, tuple(a.dims)
    ratios = [(2, 2, 1), (2, 2, 1), (2, 2, 2), (2, 2, 2), (2, 2, 2)]
    dims = [d0]
    for r in ratios:
        dims.append(tuple(x // y for x, y in zip(dims[-1], r)))
    nv = [d[0] * d[1] * d[2] for d in dims]
    lg = torch.randn(B, *d0, 2, device="cuda")
    lab = (torch.rand(B, *d0, device="cuda") > 0.97).float()
    atts = [torch.rand(B, *d, device="cuda") for d in dims]
    labels = [lab] + [torch.zeros(B, *d, device="cuda") for d in dims[1:]]
    sums = torch.zeros(B * 6 + 6 * B * 3, dtype=torch.float64, device="cuda")
    ps, asum = sums.data_ptr(), sums.data_ptr() + 8 * B * 6
    coef = torch.full((B * 4 + 6 * B * 2,), 0.01, device="cuda")
    out32 = torch.empty(B, *d0, 2, device="cuda")
    out16 = torch.empty(B, *d0, 2, device="cuda", dtype=torch.bfloat16)
    gatt = [torch.empty(B, *d, device="cuda") for d in dims]
    print(f"batch {B}, levels {dims}")
    print(f"  pred_sums                 {timed(lambda: lib.vsseg_dice_pred_sums(lg.data_ptr(), 2, lab.data_ptr(), B, nv[0], 1, ps, S)):7.1f} us")
    for l in range(6):
        print(f"  att_sums level {l}          {timed(lambda: lib.vsseg_dice_att_sums(atts[l].data_ptr(), labels[l].data_ptr(), B, nv[l], asum, S)):7.1f} us")
    for l in range(5):
        print(f"  maxpool {l}->{l + 1}              {timed(lambda: lib.vsseg_maxpool_label(labels[l].data_ptr(), B, L.i3(dims[l]), L.i3(ratios[l]), labels[l + 1].data_ptr(), S)):7.1f} us")
    print(f"  level_sums 0 (+ logits)   {timed(lambda: lib.vsseg_dice_level_sums(lg.data_ptr(), atts[0].data_ptr(), lab.data_ptr(), B, L.i3(dims[0]), 1, ps, asum, labels[1].data_ptr(), S)):7.1f} us")
    print(f"  level_sums 1              {timed(lambda: lib.vsseg_dice_level_sums(None, atts[1].data_ptr(), labels[1].data_ptr(), B, L.i3(dims[1]), 1, ps, asum, labels[2].data_ptr(), S)):7.1f} us")
    for lv in ([2, 3, 4, 5], [2], [3], [4], [5], [3, 4, 5]):
        td = L.DiceTailDesc()
        td.n, td.nlevels, td.src, td.sdims, td.sums = B, len(lv), labels[2].data_ptr(), L.i3(dims[2]), asum
        for j, l in enumerate(lv):
            td.att[j], td.label[j] = atts[l].data_ptr(), (None if l == 2 else labels[l].data_ptr())
            td.dims[j][0], td.dims[j][1], td.dims[j][2] = dims[l]
        print(f"  tail levels {str(lv):14s} {timed(lambda: L.check(lib.vsseg_dice_tail_sums(td, S))):7.1f} us")
    print(f"  finalize                  {timed(lambda: lib.vsseg_dice_finalize(ps, asum, B, 6, coef.data_ptr(), coef.data_ptr(), S)):7.1f} us")
    print(f"  pred_bwd fp32             {timed(lambda: lib.vsseg_dice_pred_bwd(lg.data_ptr(), 2, lab.data_ptr(), B, nv[0], 1, coef.data_ptr(), None, out32.data_ptr(), S)):7.1f} us")
    print(f"  pred_bwd_to bf16 compact  {timed(lambda: lib.vsseg_dice_pred_bwd_to(lg.data_ptr(), 2, lab.data_ptr(), B, nv[0], 1, coef.data_ptr(), None, L.Tensor(out16.data_ptr(), L.BF16, 2, 2, B, *d0), S)):7.1f} us")
    for l in range(6):
        print(f"  att_bwd level {l}           {timed(lambda: lib.vsseg_dice_att_bwd(labels[l].data_ptr(), B, nv[l], coef.data_ptr(), 1.0, None, gatt[l].data_ptr(), S)):7.1f} us")
    bd = L.DiceBwdLevelsDesc()
    bd.n, bd.nlevels, bd.gscale = B, 4, None
    for j, l in enumerate([2, 3, 4, 5]):
        bd.label[j], bd.datt[j], bd.nvox[j], bd.coef[j] = labels[l].data_ptr(), gatt[l].data_ptr(), nv[l], coef.data_ptr()
    print(f"  att_bwd levels 2-5        {timed(lambda: lib.vsseg_dice_att_bwd_levels(bd, S)):7.1f} us")


if __name__ == "__main__":
    main()
