"""Cost of the optimiser additions (csrc/optim.hip): the update launches at the model's own flat parameter count, and the fused train step with gradient-norm clipping
on and off, alternating in one process, at the benchmark shape and at batch 2 of 384x384x64.  The budget is the project's 1 % of the step per optional feature, measured
against the unclipped Adam arm of the same process.

    python tools/bench_optim.py [--steps 10] [--rounds 3] [--max_grad_norm 12]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd import _lib as L  # noqa: E402


def timed(fn, reps=50):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


def bench_kernels(n, max_norm):
    lib = L.lib()
    S = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    p, g = 0.1 * torch.randn(n, device="cuda"), 1e-3 * torch.randn(n, device="cuda")
    m, v, buf = torch.zeros_like(p), torch.zeros_like(p), torch.zeros_like(p)
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    need = lib.vsseg_grad_norm_scratch_bytes(n)
    scratch = torch.empty(need // 8, dtype=torch.float64, device="cuda")
    adam_args = (n, 1e-4, 0.9, 0.999, 1e-8, 1e-7, 0.1, 0.001, 1.0)

    def norm():
        L.check(lib.vsseg_grad_norm(g.data_ptr(), n, 1.0, max_norm, scratch.data_ptr(), need, rec.data_ptr(), S), "grad_norm")

    def adam():
        L.check(lib.vsseg_adam(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), *adam_args, S), "adam")

    def adam_clipped(decoupled=0):
        L.check(lib.vsseg_adam_clipped(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), *adam_args, decoupled, rec.data_ptr(), S), "adam_clipped")

    def sgd():
        L.check(lib.vsseg_sgd(p.data_ptr(), g.data_ptr(), buf.data_ptr(), n, 1e-2, 0.99, 3e-5, 1, 1.0, rec.data_ptr(), S), "sgd")

    mb = n * 4 / 1e6
    print(f"update launches over the model's flat buffers: {n} fp32 elements ({mb:.1f} MB per buffer), back to back on one stream")
    rows = (("vsseg_adam", adam, 7), ("vsseg_grad_norm (2 launches)", norm, 1), ("vsseg_adam_clipped, coupled", adam_clipped, 7), ("vsseg_adam_clipped, decoupled", lambda: adam_clipped(1), 7),
            ("vsseg_sgd, Nesterov", sgd, 5), ("norm + vsseg_adam_clipped", lambda: (norm(), adam_clipped()), 8), ("norm + vsseg_sgd", lambda: (norm(), sgd()), 6))
    out = {}
    for name, fn, passes in rows:
        t = timed(fn)
        out[name] = t
        print(f"  {name:32s} {t:7.1f} us   ({passes * mb / t:5.2f} TB/s over {passes} buffer passes, the buffers resident in the 256 MB cache)")  # MB / us = TB/s
    return out


def bench_step(batch, dims, steps, rounds, max_norm, dtype="bf16"):
    import vs_seg_amd as V
    from vs_seg_amd import parallel as DP
    from vs_seg_amd.params import HP

    torch.manual_seed(0)
    model = V.UNet2d5_spvPA(dimensions=3, in_channels=1, out_channels=2, num_res_units=2, norm="batch", dropout=0.1, attention_module=True, compute_dtype=dtype, **HP).to("cuda")
    model.reuse_output_buffers = True
    loss_fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    img = torch.randn(batch, 1, *dims, device="cuda")
    lab = torch.zeros(batch, 1, *dims, device="cuda")
    lab[1:, :, dims[0] // 2 - 16 : dims[0] // 2 + 16, dims[1] // 2 - 8 : dims[1] // 2 + 8, dims[2] // 2 - 4 : dims[2] // 2 + 4] = 1.0
    arms = (("Adam (the reference's step)", V.Adam(model.parameters(), lr=1e-4, weight_decay=1e-7)),
            (f"Adam, max_grad_norm {max_norm:g}", V.Adam(model.parameters(), lr=1e-4, weight_decay=1e-7, max_grad_norm=max_norm)),
            (f"SGD Nesterov, max_grad_norm {max_norm:g}", V.SGD(model.parameters(), lr=1e-4, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=max_norm)))
    trainers = [DP.DataParallelTrainer(model.train(), loss_fn, opt) for _, opt in arms]
    for t in trainers:
        for _ in range(3):
            t.step(img, lab)
    times = [[] for _ in arms]
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for i, t in enumerate(trainers):
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                loss = t.step(img, lab)
            e1.record()
            torch.cuda.synchronize()
            times[i].append(e0.elapsed_time(e1) / steps)
    print(f"fused train step, {dtype}, batch {batch} of {dims[0]}x{dims[1]}x{dims[2]}: {rounds} alternating rounds of {steps} steps per arm, the median round (last loss {float(loss):.4f})")
    med = [sorted(t)[len(t) // 2] for t in times]
    for (name, opt), t, ms in zip(arms, times, med):
        extra = "" if ms is med[0] else f"   {1e3 * (ms - med[0]):+7.1f} us = {100 * (ms - med[0]) / med[0]:+.2f} % of the step"
        print(f"  {name:34s} {ms:8.3f} ms   (rounds: {', '.join(f'{x:.3f}' for x in t)}){extra}")
        if opt.max_grad_norm is not None:
            print(f"    grad_norm_stats: {opt.grad_norm_stats()}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max_grad_norm", type=float, default=12.0)
    a = ap.parse_args()
    import vs_seg_amd as V
    from vs_seg_amd.params import HP

    n = int(V.UNet2d5_spvPA(dimensions=3, in_channels=1, out_channels=2, num_res_units=2, norm="batch", dropout=0.1, attention_module=True, compute_dtype="bf16", **HP).to("cuda").flat_parameters()[0].numel())
    k = bench_kernels(n, a.max_grad_norm)
    added = k["norm + vsseg_adam_clipped"] - k["vsseg_adam"]
    for batch, dims in ((4, (384, 128, 128)), (2, (384, 384, 64))):
        med = bench_step(batch, dims, a.steps, a.rounds, a.max_grad_norm)
        budget = 10.0 * med[0]  # 1 % of the step, in us
        print(f"  budget: 1 % of the unclipped Adam step = {budget:.1f} us; the launches of clipping add {added:.1f} us back to back "
              f"(vsseg_grad_norm {k['vsseg_grad_norm (2 launches)']:.1f} us, vsseg_adam_clipped {k['vsseg_adam_clipped, coupled'] - k['vsseg_adam']:+.1f} us against vsseg_adam): "
              f"{'within' if added <= budget else 'OVER — vsseg_grad_norm is the launch that exceeds it'} the budget; measured in the step: {1e3 * (med[1] - med[0]):+.1f} us")


if __name__ == "__main__":
    main()
