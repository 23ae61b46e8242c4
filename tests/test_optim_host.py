"""CPU tests of the optimiser additions (vs_seg_amd.SGD / AdamW / max_grad_norm, --optimizer / --momentum / --nesterov / --weight_decay / --clip_grad_norm /
--lr_schedule / --poly_power): the range checks, the command-line flags, poly_lr against torch's PolynomialLR, the exported entry points and their argument checks,
and the kernels' update formulas (tests/optim_oracle.py, numpy fp32) against torch.optim."""
import argparse

import numpy as np
import pytest
import torch

import vs_seg_amd as V
from tests import optim_oracle as OO
from vs_seg_amd import _lib as L

NAN, INF = float("nan"), float("inf")


def test_check_optimizer_accepts_and_rejects():
    d = V.check_optimizer()
    assert d == dict(optimizer="adam", momentum=0.99, nesterov=False, weight_decay=1e-7, clip_grad_norm=0.0, lr_schedule="halving", poly_power=0.9)
    good = [dict(optimizer="adamw", weight_decay=1e-2), dict(optimizer="sgd"), dict(optimizer="sgd", momentum=0.0), dict(optimizer="sgd", momentum=0.9, nesterov=True),
            dict(optimizer="sgd", nesterov=True, weight_decay=3e-5, clip_grad_norm=12, lr_schedule="poly", poly_power=0.9), dict(clip_grad_norm=1.0), dict(clip_grad_norm=0),
            dict(lr_schedule="poly"), dict(lr_schedule="poly", poly_power=2), dict(weight_decay=0)]
    for kw in good:
        got = V.check_optimizer(**kw)
        for k, v in kw.items():
            assert got[k] == v and type(got[k]) is (type(v) if isinstance(v, (str, bool)) else float)
    assert V.check_optimizer("sgd")["momentum"] == 0.99 and V.check_optimizer(lr_schedule="poly")["poly_power"] == 0.9
    bad = [dict(optimizer="lamb"), dict(optimizer=None), dict(lr_schedule="cosine"),
           dict(optimizer="sgd", momentum=1.0), dict(optimizer="sgd", momentum=-0.1), dict(optimizer="sgd", momentum=NAN), dict(optimizer="sgd", momentum=INF), dict(optimizer="sgd", momentum="x"),
           dict(optimizer="sgd", momentum=0.0, nesterov=True),
           dict(clip_grad_norm=-1.0), dict(clip_grad_norm=NAN), dict(clip_grad_norm=INF), dict(clip_grad_norm=None),
           dict(lr_schedule="poly", poly_power=0.0), dict(lr_schedule="poly", poly_power=-1.0), dict(lr_schedule="poly", poly_power=NAN), dict(lr_schedule="poly", poly_power=INF),
           dict(weight_decay=-1e-7), dict(weight_decay=NAN), dict(weight_decay=INF)]
    for kw in bad:
        with pytest.raises(ValueError):
            V.check_optimizer(**kw)
    for kw in (dict(optimizer="adam", momentum=0.9), dict(optimizer="adamw", momentum=0.99), dict(optimizer="adam", nesterov=True), dict(optimizer="adamw", nesterov=True), dict(poly_power=0.9),
               dict(lr_schedule="halving", poly_power=2.0)):
        with pytest.raises(ValueError, match="no effect"):  # flags that would silently do nothing
            V.check_optimizer(**kw)


def _parse(argv):
    from vs_seg_amd.params import VSparams

    try:
        return VSparams(argparse.ArgumentParser(), argv)
    except RuntimeError as e:  # "no GPU visible": raised after the arguments are parsed and checked
        assert "no GPU" in str(e)
        return None


def test_command_line_flags_default_to_the_reference_and_reject_bad_values():
    ap = argparse.ArgumentParser()
    try:
        from vs_seg_amd.params import VSparams

        VSparams(ap, [])
    except RuntimeError as e:
        assert "no GPU" in str(e)
    assert ap.get_default("optimizer") == "adam" and ap.get_default("weight_decay") == 1e-7 and ap.get_default("clip_grad_norm") == 0.0 and ap.get_default("lr_schedule") == "halving"
    assert ap.get_default("nesterov") is False and ap.get_default("momentum") is None and ap.get_default("poly_power") is None  # None: not given (0.99 / 0.9 where they apply)
    for bad in (["--optimizer", "lamb"], ["--momentum", "0.9"], ["--nesterov"], ["--optimizer", "adamw", "--nesterov"], ["--optimizer", "sgd", "--momentum", "1"],
                ["--optimizer", "sgd", "--momentum", "-0.5"], ["--optimizer", "sgd", "--momentum", "nan"], ["--optimizer", "sgd", "--momentum", "0", "--nesterov"],
                ["--clip_grad_norm", "-1"], ["--clip_grad_norm", "nan"], ["--clip_grad_norm", "inf"], ["--clip_grad_norm", "x"], ["--weight_decay", "-1"], ["--weight_decay", "nan"],
                ["--lr_schedule", "cosine"], ["--poly_power", "0.9"], ["--lr_schedule", "poly", "--poly_power", "0"], ["--lr_schedule", "poly", "--poly_power", "-2"],
                ["--lr_schedule", "poly", "--poly_power", "inf"]):
        with pytest.raises(SystemExit):
            _parse(bad)
    for good in ([], ["--optimizer", "sgd", "--nesterov", "--weight_decay", "3e-5", "--clip_grad_norm", "12", "--lr_schedule", "poly"], ["--optimizer", "adamw", "--weight_decay", "0.01"],
                 ["--optimizer", "sgd", "--momentum", "0"], ["--clip_grad_norm", "0"]):
        p = _parse(good)
        if p is not None:
            assert p.optimizer == (good[1] if good and good[0] == "--optimizer" else "adam")


def test_flags_reach_the_object_and_the_log(monkeypatch):
    """The checked values and log_parameters need no device: build the object past the device check."""
    from vs_seg_amd import params as P

    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(P.DP, "init_distributed", lambda: (0, 1, 0))
    new = ("optimizer", "momentum", "nesterov", "clip_grad_norm", "lr_schedule", "poly_power")
    cases = (([], dict(optimizer="adam", weight_decay=1e-7, clip_grad_norm=0.0, lr_schedule="halving"), ()),
             (["--optimizer", "sgd", "--nesterov", "--weight_decay", "3e-5", "--clip_grad_norm", "12", "--lr_schedule", "poly"],
              dict(optimizer="sgd", momentum=0.99, nesterov=True, weight_decay=3e-5, clip_grad_norm=12.0, lr_schedule="poly", poly_power=0.9), new),
             (["--optimizer", "adamw", "--weight_decay", "0.01"], dict(optimizer="adamw", weight_decay=0.01), ("optimizer",)),
             (["--clip_grad_norm", "5"], dict(optimizer="adam", clip_grad_norm=5.0), ("clip_grad_norm",)),
             (["--lr_schedule", "poly", "--poly_power", "2"], dict(lr_schedule="poly", poly_power=2.0), ("lr_schedule", "poly_power")))
    for argv, want, logged in cases:
        p = P.VSparams(argparse.ArgumentParser(), argv)
        for k, v in want.items():
            assert getattr(p, k) == v, (argv, k)
        lines = []
        p.logger = type("Log", (), {"info": staticmethod(lines.append)})()
        p.log_parameters()
        for k in new:
            assert any(ln.split()[:2] == [k, "="] for ln in lines) == (k in logged), (argv, k)
        assert any(ln.split() == ["weight_decay", "=", str(want.get("weight_decay", 1e-7))] for ln in lines)  # logged as before, now with the flag's value


@pytest.mark.parametrize("power", [0.9, 2.0])
def test_poly_lr_is_torch_polynomial_lr(power):
    lr0, n = 1e-2, 10
    w = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([w], lr=lr0)
    sched = torch.optim.lr_scheduler.PolynomialLR(opt, total_iters=n, power=power)
    for epoch in range(n):
        want = opt.param_groups[0]["lr"]
        got = V.poly_lr(lr0, epoch, n, power)
        assert abs(got - want) <= 1e-12 * lr0, (epoch, got, want)  # torch multiplies factors epoch by epoch: a few ulp of fp64 from the closed form
        opt.step()
        sched.step()
    assert V.poly_lr(lr0, 0, n, power) == lr0 and V.poly_lr(lr0, n, n, power) == 0.0
    with pytest.raises(ValueError):
        V.poly_lr(lr0, 0, 0, power)


def test_library_exports_the_entry_points_and_refuses_bad_arguments():
    lib = L.lib()
    assert lib.vsseg_version() >= 15
    for name in ("vsseg_grad_norm_scratch_bytes", "vsseg_grad_norm", "vsseg_sgd", "vsseg_adam_clipped"):
        assert name in L.SYMBOLS and getattr(lib, name).argtypes
    import ctypes

    assert ctypes.sizeof(L.ClipRecord) == 64 and L.ClipRecord.coef.offset == 8 and L.ClipRecord.skip.offset == 12 and L.ClipRecord.norm_max.offset == 48
    S, T = L.GRAD_NORM_SHARD, L.GRAD_NORM_FINAL
    assert S > 0 and S % 4 == 0 and T > 0
    # scratch: one fp64 partial per shard
    assert lib.vsseg_grad_norm_scratch_bytes(0) >= 8 and lib.vsseg_grad_norm_scratch_bytes(S) == 8 and lib.vsseg_grad_norm_scratch_bytes(S + 1) == 16 and lib.vsseg_grad_norm_scratch_bytes(S * T + 5) == 8 * (T + 1)
    assert lib.vsseg_grad_norm_scratch_bytes(-1) == L.EINVAL and b"vsseg_grad_norm_scratch_bytes" in lib.vsseg_last_error()
    # refused before any launch (the "pointers" are never dereferenced): null pointers, n < 0, max_norm not finite or <= 0, too little scratch
    for args in ((None, 8, 1.0, 1.0, 256, 8, 512, None), (1024, 8, 1.0, 1.0, None, 8, 512, None), (1024, 8, 1.0, 1.0, 256, 8, None, None), (1024, -1, 1.0, 1.0, 256, 8, 512, None),
                 (1024, 8, 1.0, 0.0, 256, 8, 512, None), (1024, 8, 1.0, -1.0, 256, 8, 512, None), (1024, 8, 1.0, NAN, 256, 8, 512, None), (1024, 8, 1.0, INF, 256, 8, 512, None),
                 (1024, 8, NAN, 1.0, 256, 8, 512, None), (1024, S + 1, 1.0, 1.0, 256, 8, 512, None), (1024, 8, 1.0, 1.0, 256, 8, 516, None)):
        assert lib.vsseg_grad_norm(*args) == L.EINVAL and b"vsseg_grad_norm" in lib.vsseg_last_error(), args
    for args in ((None, 1024, 2048, 8, 0.1, 0.9, 0.0, 0, 1.0, None, None), (1024, None, 2048, 8, 0.1, 0.9, 0.0, 0, 1.0, None, None), (1024, 2048, None, 8, 0.1, 0.9, 0.0, 0, 1.0, None, None),
                 (1024, 2048, 4096, -1, 0.1, 0.9, 0.0, 0, 1.0, None, None), (1024, 2048, 4096, 8, 0.1, 1.0, 0.0, 0, 1.0, None, None), (1024, 2048, 4096, 8, 0.1, -0.1, 0.0, 0, 1.0, None, None),
                 (1024, 2048, 4096, 8, 0.1, NAN, 0.0, 0, 1.0, None, None), (1024, 2048, 4096, 8, 0.1, 0.0, 0.0, 1, 1.0, None, None)):
        assert lib.vsseg_sgd(*args) == L.EINVAL and b"vsseg_sgd" in lib.vsseg_last_error(), args
    assert lib.vsseg_sgd(1024, 2048, None, 0, 0.1, 0.0, 0.0, 0, 1.0, None, None) == 0  # momentum 0 needs no buffer; n == 0: nothing is launched
    for args in ((None, 2048, 4096, 8192, 8), (1024, None, 4096, 8192, 8), (1024, 2048, None, 8192, 8), (1024, 2048, 4096, None, 8), (1024, 2048, 4096, 8192, -1)):
        for decoupled in (0, 1):
            assert lib.vsseg_adam_clipped(*args, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0, decoupled, None, None) == L.EINVAL and b"vsseg_adam_clipped" in lib.vsseg_last_error(), args
    assert lib.vsseg_adam_clipped(1024, 2048, 4096, 8192, 0, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.1, 0.001, 1.0, 1, None, None) == 0


def test_optimizer_classes_are_exported_and_refuse_foreign_parameters():
    assert issubclass(V.AdamW, V.Adam) and issubclass(V.SGD, torch.optim.Optimizer)
    w = [torch.nn.Parameter(torch.zeros(3))]
    for make in (lambda: V.SGD(w, lr=0.1), lambda: V.AdamW(w), lambda: V.Adam(w, max_grad_norm=1.0)):
        with pytest.raises(ValueError, match="flat parameter buffer"):
            make()
    for kw in (dict(momentum=1.0), dict(momentum=-0.1), dict(momentum=0.0, nesterov=True), dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(max_grad_norm=NAN), dict(max_grad_norm=INF)):
        with pytest.raises(ValueError):
            V.SGD(w, lr=0.1, **kw)


# ---- the kernels' formulas against torch.optim -------------------------------------------------------------------------------------------------------
N = 100_003
ATOL, RTOL = 2e-7, 1e-6  # the bars tests/test_gpu_ops.py::test_adam_matches_torch_golden holds Adam to


def problem(seed=7, n=N, steps=3):
    """p ~ 0.1 N(0, 1); gradients spanning 1e-6 .. 1e-1 in magnitude, both signs."""
    rng = np.random.default_rng(seed)
    p = (0.1 * rng.standard_normal(n)).astype(np.float32)
    gs = [(10.0 ** rng.uniform(-6, -1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32) for _ in range(steps)]
    return p, gs


@pytest.mark.parametrize("nesterov", [True, False])
def test_sgd_formula_matches_torch(nesterov):
    p0, gs = problem()
    kw = dict(lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=nesterov)
    _, want = OO.run("sgd", torch.from_numpy(p0), [torch.from_numpy(g) for g in gs], **kw)
    p, buf = p0.copy(), np.zeros_like(p0)
    for g, w in zip(gs, want):
        p, buf = OO.sgd_by_hand(p, g, buf, 1e-2, 0.99, 3e-5, nesterov)
        np.testing.assert_allclose(p, w.numpy(), atol=ATOL, rtol=RTOL)


def test_adamw_formula_matches_torch():
    p0, gs = problem(seed=8)
    _, want = OO.run("adamw", torch.from_numpy(p0), [torch.from_numpy(g) for g in gs], lr=1e-3, weight_decay=1e-2)
    p, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for t, (g, w) in enumerate(zip(gs, want), 1):
        p, m, v = OO.adamw_by_hand(p, g, m, v, t, 1e-3, 0.9, 0.999, 1e-8, 1e-2)
        np.testing.assert_allclose(p, w.numpy(), atol=ATOL, rtol=RTOL)


def test_oracle_norm_and_coefficient():
    g = torch.tensor([3.0, 4.0])
    assert OO.grad_norm(g) == 5.0 and OO.grad_norm(g, 0.5) == 2.5 and OO.grad_norm([g, g]) == pytest.approx(50.0**0.5, rel=1e-15)
    assert OO.clip_coef(5.0, None) == 1.0 and OO.clip_coef(5.0, 10.0) == 1.0 and OO.clip_coef(NAN, 1.0) == 0.0 and OO.clip_coef(INF, 1.0) == 0.0
    assert OO.clip_coef(5.0, 1.0) == np.float32(1.0 / (5.0 + 1e-6))
    # fp32 squares of 1e-30 underflow, of 1e25 overflow: the oracle's norm is fp64
    assert OO.grad_norm(torch.full((100,), 1e-30)) == pytest.approx(float(np.float32(1e-30)) * 10.0, rel=1e-14) and np.isfinite(OO.grad_norm(torch.full((100,), 1e25)))
    # a clipped step is the unclipped step on the scaled gradient; a non-finite norm leaves the parameters alone
    p0, gs = problem(n=1000, steps=1)
    (n1,), (a,) = OO.run("sgd", torch.from_numpy(p0), [torch.from_numpy(gs[0])], max_norm=0.5 * OO.grad_norm(torch.from_numpy(gs[0])), lr=0.1)
    (_,), (b,) = OO.run("sgd", torch.from_numpy(p0), [torch.from_numpy(gs[0]) * torch.tensor(OO.clip_coef(n1, 0.5 * n1))], lr=0.1)
    assert torch.equal(a, b) and not torch.equal(a, torch.from_numpy(p0))
    bad = torch.from_numpy(gs[0]).clone()
    bad[5] = INF
    (nb,), (c,) = OO.run("sgd", torch.from_numpy(p0), [bad], max_norm=1.0, lr=0.1)
    assert np.isinf(nb) and torch.equal(c, torch.from_numpy(p0))
