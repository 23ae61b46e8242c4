"""-m gpu: gradient-norm clipping, SGD and AdamW (vsseg_grad_norm / vsseg_sgd / vsseg_adam_clipped, vs_seg_amd.SGD / AdamW / Adam(max_grad_norm=), the VSparams flags)
against the CPU oracle of tests/optim_oracle.py: fp64 norm, torch.nn.utils.clip_grad_norm_'s coefficient rounded once to fp32, torch.optim on the CPU.

Bars: the norm to rtol 1e-12 of fp64 (a fixed tree of fp64 additions over <= 3.5 M squares), the coefficient to 1 fp32 ulp, flat updates atol 2e-7 / rtol 1e-6
(tests/test_gpu_ops.py::test_adam_matches_torch_golden), the model's tensors atol 5e-7 / rtol 1e-6 (tests/test_gpu_network.py::test_adam_step_and_grad_accumulation)."""
import argparse
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import vs_seg_amd as V  # noqa: E402
from oracle import vsseg_oracle as O  # noqa: E402
from tests import gpu_harness as H  # noqa: E402
from tests import optim_oracle as OO  # noqa: E402
from tests.helpers import synth_input, synth_label  # noqa: E402
from vs_seg_amd import _lib as L  # noqa: E402

S, T = L.GRAD_NORM_SHARD, L.GRAD_NORM_FINAL
HP, SEED, SHAPE = O.HP, 61, (2, 1, 32, 32, 8)
N = 100_003
ATOL, RTOL = 2e-7, 1e-6


def _model(dropout=0.0):
    torch.manual_seed(77)
    m = V.UNet2d5_spvPA(dimensions=3, in_channels=1, out_channels=2, channels=HP["channels"], strides=HP["strides"], kernel_sizes=HP["kernel_sizes"], sample_kernel_sizes=HP["sample_kernel_sizes"],
                        num_res_units=2, norm="batch", dropout=dropout, attention_module=True, compute_dtype="fp32")
    m.load_state_dict(O.seeded_state_dict(True, SEED))
    return m.to("cuda")


def _batch():
    return synth_input(SEED, SHAPE).cuda(), synth_label(SEED, SHAPE).cuda()


@functools.lru_cache(maxsize=None)
def _model_size() -> int:
    return int(_model().flat_parameters()[0].numel())


@functools.lru_cache(maxsize=None)
def _grad(n: int, seed: int = 3) -> torch.Tensor:
    """CPU fp32, magnitudes 1e-6 .. 1e-1, both signs (shared; never written)."""
    rng = np.random.default_rng(seed + n % 1000)
    return torch.from_numpy((10.0 ** rng.uniform(-6, -1, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _norm_oracle(n: int, gscale: float) -> float:
    return OO.grad_norm(_grad(n), gscale)


def _record(t: torch.Tensor) -> L.ClipRecord:
    return L.ClipRecord.from_buffer_copy(t.cpu().numpy().tobytes())


def _norm(g: torch.Tensor, gscale: float, max_norm: float, rec=None):
    """One vsseg_grad_norm call on the device tensor g; returns (record tensor, decoded record)."""
    lib = L.lib()
    rec = torch.zeros(8, dtype=torch.float64, device="cuda") if rec is None else rec
    need = lib.vsseg_grad_norm_scratch_bytes(g.numel())
    assert need >= 8
    scratch = torch.full((need // 8,), float("nan"), dtype=torch.float64, device="cuda")  # every partial that is read must have been written
    L.check(lib.vsseg_grad_norm(g.data_ptr(), g.numel(), gscale, max_norm, scratch.data_ptr(), need, rec.data_ptr(), H.stream()), "grad_norm")
    torch.cuda.synchronize()
    return rec, _record(rec)


def _ulps(a, b) -> int:
    return abs(int(np.float32(a).view(np.int32)) - int(np.float32(b).view(np.int32)))


def _sizes():
    return [0, 1, 3, S - 1, S, S + 1, S * T + 5, "model"]


@pytest.mark.parametrize("gscale", [1.0, 0.5])
@pytest.mark.parametrize("n", _sizes())
def test_grad_norm_matches_fp64_and_is_reproducible(n, gscale):
    n = _model_size() if n == "model" else n
    g = _grad(n).cuda()
    want = _norm_oracle(n, gscale)
    max_norm = 1.0  # below the norm at the large sizes (coefficient < 1), above it at the small ones (coefficient 1)
    rec, r = _norm(g, gscale, max_norm)
    print(f"n {n} gscale {gscale}: norm {r.norm!r} (oracle {want!r}, rel {abs(r.norm - want) / max(want, 1e-300):.2e}), coef {r.coef!r} (oracle {OO.clip_coef(want, max_norm)!r})")
    assert abs(r.norm - want) <= 1e-12 * want
    assert _ulps(r.coef, OO.clip_coef(want, max_norm)) <= 1 and r.skip == 0
    assert (r.steps, r.clipped, r.skipped) == (1, int(r.coef < 1.0), 0) and r.norm_sum == r.norm and r.norm_max == r.norm
    if n == 0:
        assert r.norm == 0.0 and r.coef == 1.0
    if n >= S * T:
        assert r.coef < 1.0
    _, again = _norm(g, gscale, max_norm)
    assert np.float64(again.norm).view(np.int64) == np.float64(r.norm).view(np.int64) and np.float32(again.coef).view(np.int32) == np.float32(r.coef).view(np.int32)


@pytest.mark.parametrize("n", [S + 1, 3 * S + 7])
def test_grad_norm_of_a_buffer_that_is_not_16_byte_aligned_has_the_same_bits(n):
    """The guarded scalar path adds the elements in the vector path's order."""
    g = _grad(n).cuda()
    shifted = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    shifted[1:] = g
    assert shifted[1:].data_ptr() % 16 == 4 and g.data_ptr() % 16 == 0
    _, a = _norm(g, 1.0, 1.0)
    _, b = _norm(shifted[1:], 1.0, 1.0)
    assert np.float64(a.norm).view(np.int64) == np.float64(b.norm).view(np.int64) and abs(a.norm - _norm_oracle(n, 1.0)) <= 1e-12 * a.norm


def test_grad_norm_squares_in_fp64():
    n = S + 3
    tiny = float(np.float32(1e-30))
    assert np.float32(tiny) * np.float32(tiny) == 0.0  # the fp32 square underflows
    _, r = _norm(torch.full((n,), 1e-30, dtype=torch.float32, device="cuda"), 1.0, 1.0)
    assert r.norm > 0 and abs(r.norm - tiny * np.sqrt(np.float64(n))) <= 1e-12 * r.norm and r.coef == 1.0 and r.skip == 0
    huge = float(np.float32(1e25))
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(huge) * np.float32(huge))  # the fp32 square overflows
    _, r = _norm(torch.full((n,), 1e25, dtype=torch.float32, device="cuda"), 1.0, 12.0)
    assert np.isfinite(r.norm) and abs(r.norm - huge * np.sqrt(np.float64(n))) <= 1e-12 * r.norm and r.skip == 0 and r.clipped == 1
    assert _ulps(r.coef, OO.clip_coef(r.norm, 12.0)) <= 1 and r.coef > 0


# ---- update kernels on flat buffers ---------------------------------------------------------------------------------------------------------------
KINDS = {
    "sgd_nesterov": ("sgd", dict(lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=True)),
    "sgd_plain": ("sgd", dict(lr=1e-2, momentum=0.99, weight_decay=3e-5, nesterov=False)),
    "sgd_no_momentum": ("sgd", dict(lr=1e-2, momentum=0.0, weight_decay=3e-5, nesterov=False)),
    "adam": ("adam", dict(lr=1e-4, weight_decay=1e-7)),
    "adamw": ("adamw", dict(lr=1e-3, weight_decay=1e-2)),
}
CLIPS = {"clips": 1.0, "above": 100.0}  # the norms of _grad(N) are about 6.6


@functools.lru_cache(maxsize=None)
def _flat_problem():
    rng = np.random.default_rng(11)
    return torch.from_numpy((0.1 * rng.standard_normal(N)).astype(np.float32)), tuple(_grad(N, seed=20 + i) for i in range(3))


@functools.lru_cache(maxsize=None)
def _flat_oracle(kind: str, max_norm):
    p0, gs = _flat_problem()
    name, kw = KINDS[kind]
    return OO.run(name, p0, gs, max_norm=max_norm, **kw)


def _device_step(name, kw, p, g, state, t, rec_ptr, gscale=1.0):
    lib = L.lib()
    if name == "sgd":
        buf = state.get("buf")
        L.check(lib.vsseg_sgd(p.data_ptr(), g.data_ptr(), None if buf is None else buf.data_ptr(), p.numel(), kw["lr"], kw["momentum"], kw["weight_decay"], int(kw["nesterov"]), gscale, rec_ptr, H.stream()), "sgd")
    else:
        L.check(lib.vsseg_adam_clipped(p.data_ptr(), g.data_ptr(), state["m"].data_ptr(), state["v"].data_ptr(), p.numel(), kw["lr"], 0.9, 0.999, 1e-8, kw["weight_decay"], 1 - 0.9**t, 1 - 0.999**t, gscale,
                                       int(name == "adamw"), rec_ptr, H.stream()), "adam_clipped")


def _new_state(name, kw, p):
    if name == "sgd":
        return {"buf": torch.zeros_like(p)} if kw["momentum"] > 0 else {}
    return {"m": torch.zeros_like(p), "v": torch.zeros_like(p)}


@pytest.mark.parametrize("clip", list(CLIPS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_update_kernels_match_torch_optim(kind, clip):
    name, kw = KINDS[kind]
    max_norm = CLIPS[clip]
    p0, gs = _flat_problem()
    norms, want = _flat_oracle(kind, max_norm)
    p = p0.cuda()
    state = _new_state(name, kw, p)
    rec = torch.zeros(8, dtype=torch.float64, device="cuda")
    for t, g in enumerate(gs, 1):
        gd = g.cuda()
        _, r = _norm(gd, 1.0, max_norm, rec)
        assert abs(r.norm - norms[t - 1]) <= 1e-12 * r.norm and _ulps(r.coef, OO.clip_coef(norms[t - 1], max_norm)) <= 1
        assert (r.coef < 1.0) == (clip == "clips")
        _device_step(name, kw, p, gd, state, t, rec.data_ptr())
        torch.cuda.synchronize()
        got = p.cpu().numpy()
        print(f"{kind} {clip} step {t}: max |d| {np.abs(got - want[t - 1].numpy()).max():.3e}")
        np.testing.assert_allclose(got, want[t - 1].numpy(), atol=ATOL, rtol=RTOL)
        assert torch.equal(gd.cpu(), g)  # the gradient itself is not clipped
    if clip == "above":  # coefficient 1: the unclipped optimiser
        _, plain = _flat_oracle(kind, None)
        assert all(torch.equal(a, b) for a, b in zip(plain, want))
        assert _record(rec).clipped == 0
    else:
        assert _record(rec).clipped == 3
    assert not np.array_equal(p.cpu().numpy(), p0.numpy())


def test_update_kernels_without_a_record_and_with_a_scale():
    """A null record is coefficient 1; gscale multiplies the gradient (the data-parallel mean)."""
    p0, gs = _flat_problem()
    for kind in ("sgd_nesterov", "adamw"):
        name, kw = KINDS[kind]
        _, want = OO.run(name, p0, gs, max_norm=None, grad_scale=0.5, **kw)
        p = p0.cuda()
        state = _new_state(name, kw, p)
        for t, g in enumerate(gs, 1):
            _device_step(name, kw, p, g.cuda(), state, t, None, gscale=0.5)
            torch.cuda.synchronize()
            np.testing.assert_allclose(p.cpu().numpy(), want[t - 1].numpy(), atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("offset", [0, 1])
def test_adam_clipped_without_record_and_coupled_is_vsseg_adam_bit_for_bit(offset):
    lib = L.lib()
    p0, gs = _flat_problem()
    n = N - offset

    def bufs():
        return [torch.zeros(N, dtype=torch.float32, device="cuda")[offset:] for _ in range(3)]  # offset 1: buffers that are only 4-byte aligned

    (pa, ma, va), (pb, mb, vb) = bufs(), bufs()
    pa.copy_(p0[offset:])
    pb.copy_(p0[offset:])
    for t, g in enumerate(gs, 1):
        gd = g.cuda()[offset:]
        args = (n, 1e-4, 0.9, 0.999, 1e-8, 1e-7, 1 - 0.9**t, 1 - 0.999**t, 0.37)
        L.check(lib.vsseg_adam(pa.data_ptr(), gd.data_ptr(), ma.data_ptr(), va.data_ptr(), *args, H.stream()), "adam")
        L.check(lib.vsseg_adam_clipped(pb.data_ptr(), gd.data_ptr(), mb.data_ptr(), vb.data_ptr(), *args, 0, None, H.stream()), "adam_clipped")
    torch.cuda.synchronize()
    assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and not torch.equal(pa.cpu(), p0[offset:])


def test_unaligned_buffers_take_the_scalar_path_with_the_same_result():
    p0, gs = _flat_problem()
    name, kw = KINDS["sgd_nesterov"]
    res = []
    for offset in (0, 1):
        hold = [torch.zeros(N + 1, dtype=torch.float32, device="cuda") for _ in range(3)]
        p, g, buf = (h[offset : offset + N] for h in hold)
        p.copy_(p0)
        g.copy_(gs[0])
        _device_step(name, kw, p, g, {"buf": buf}, 1, None)
        torch.cuda.synchronize()
        assert all(float(h[N if offset == 0 else 0]) == 0.0 for h in hold)  # nothing outside the n elements was written
        res.append((p.clone(), buf.clone()))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])


# ---- the classes on the real model ------------------------------------------------------------------------------------------------------------------
def _first_gradient(m):
    """One backward of the batch without a step: the flat gradient the first step will see."""
    x, y = _batch()
    loss_fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    for p in m.parameters():
        p.grad = None
    loss_fn(m(x), y).backward()
    torch.cuda.synchronize()
    return m.flat_parameters()[1]


@functools.lru_cache(maxsize=None)
def _first_norm() -> float:
    return OO.grad_norm(_first_gradient(_model().train()))


def _make(kind, m, max_grad_norm):
    if kind == "sgd":
        return V.SGD(m.parameters(), lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5, max_grad_norm=max_grad_norm)
    return V.AdamW(m.parameters(), lr=1e-3, weight_decay=1e-2, max_grad_norm=max_grad_norm)


def _train3(kind, max_grad_norm, oracle=None, steps=3):
    """Three DataParallelTrainer steps; with `oracle` (a Stepper factory) the GPU's own p.grad feeds the CPU optimiser after every step."""
    from vs_seg_amd import parallel as DP

    m = _model().train()
    opt = _make(kind, m, max_grad_norm)
    trainer = DP.DataParallelTrainer(m, V.Dice_spvPA(to_onehot_y=True, softmax=True), opt)
    assert trainer.fused_mean and opt.grad_scale == 1.0
    ref = oracle([p.detach() for p in m.parameters()]) if oracle else None
    x, y = _batch()
    norms = []
    for it in range(steps):
        trainer.step(x, y)
        torch.cuda.synchronize()
        if ref is not None:
            grads = [p.grad.detach().cpu().clone() for p in m.parameters()]
            want_norm = ref.step(grads)
            got_norm = float(opt.last_grad_norm)
            norms.append(got_norm)
            assert opt.last_grad_norm.is_cuda and opt.last_grad_norm.dtype == torch.float64 and abs(got_norm - want_norm) <= 1e-12 * want_norm
            for (k, p), t in zip(m.named_parameters(), ref.values()):
                np.testing.assert_allclose(p.detach().cpu().numpy(), t.numpy(), atol=5e-7, rtol=1e-6, err_msg=f"{k} step {it + 1}")
    return m, opt, norms


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_classes_match_torch_optim_on_the_model(kind):
    max_norm = 0.5 * _first_norm()  # below the first step's norm
    kw = dict(lr=1e-2, momentum=0.99, nesterov=True, weight_decay=3e-5) if kind == "sgd" else dict(lr=1e-3, weight_decay=1e-2)
    m, opt, norms = _train3(kind, max_norm, oracle=lambda ps: OO.Stepper(kind, ps, max_norm, **kw))
    st = opt.grad_norm_stats(reset=False)
    print(f"{kind}: norms {norms}, max_grad_norm {max_norm}, stats {st}")
    assert norms[0] > max_norm and st["steps"] == 3 and st["clipped"] >= 1 and st["skipped"] == 0 and st["max_norm"] == max(norms) and abs(st["mean_norm"] - sum(norms) / 3) <= 1e-12 * st["mean_norm"]
    assert abs(norms[0] - _first_norm()) <= 1e-12 * norms[0]


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_three_steps_twice_give_the_same_bits(kind):
    max_norm = 0.5 * _first_norm()
    (a, _, _), (b, _, _) = _train3(kind, max_norm), _train3(kind, max_norm)
    assert torch.equal(a.flat_parameters()[0], b.flat_parameters()[0])


def test_adam_with_default_keywords_is_the_plain_vsseg_adam_step():
    lib = L.lib()
    m = _model().train()
    opt = V.Adam(m.parameters(), lr=1e-4, weight_decay=1e-7)
    assert opt.max_grad_norm is None and opt.param_groups[0]["decoupled_weight_decay"] is False and opt.last_grad_norm is None
    x, y = _batch()
    loss_fn = V.Dice_spvPA(to_onehot_y=True, softmax=True)
    flat, gflat = m.flat_parameters()
    p, mm, vv = flat.clone(), torch.zeros_like(flat), torch.zeros_like(flat)
    for t in (1, 2):
        opt.zero_grad()
        loss_fn(m(x), y).backward()
        opt.step()
        L.check(lib.vsseg_adam(p.data_ptr(), gflat.data_ptr(), mm.data_ptr(), vv.data_ptr(), p.numel(), 1e-4, 0.9, 0.999, 1e-8, 1e-7, 1 - 0.9**t, 1 - 0.999**t, 1.0, H.stream()), "adam")
        torch.cuda.synchronize()
        assert torch.equal(p, flat), t
    st = opt.state[opt.param_groups[0]["params"][0]]
    assert torch.equal(st["exp_avg"], mm) and torch.equal(st["exp_avg_sq"], vv) and st["step"] == 2
    assert opt.grad_norm_stats() == dict(steps=0, clipped=0, skipped=0, mean_norm=0.0, max_norm=0.0)


def test_sgd_state_dict_round_trip_continues_bit_identically():
    from vs_seg_amd import parallel as DP

    max_norm = 0.5 * _first_norm()
    m, opt, _ = _train3("sgd", max_norm, steps=2)
    sd = copy.deepcopy(opt.state_dict())
    assert [k for k in sd["state"][0]] == ["momentum_buffer"] and sd["state"][0]["momentum_buffer"].numel() == m.flat_parameters()[0].numel()
    m2 = _model().train()
    m2.load_state_dict(copy.deepcopy(m.state_dict()))
    opt2 = _make("sgd", m2, max_norm)
    opt2.load_state_dict(sd)
    x, y = _batch()
    for mod, o in ((m, opt), (m2, opt2)):
        DP.DataParallelTrainer(mod, V.Dice_spvPA(to_onehot_y=True, softmax=True), o).step(x, y)
    torch.cuda.synchronize()
    assert torch.equal(m.flat_parameters()[0], m2.flat_parameters()[0])
    b1, b2 = (o.state[o.param_groups[0]["params"][0]]["momentum_buffer"] for o in (opt, opt2))
    assert torch.equal(b1, b2) and b1.data_ptr() != b2.data_ptr() and float(b1.abs().max()) > 0


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_a_non_finite_gradient_skips_the_step(kind):
    """One Inf, then one NaN in the gradient: parameters and optimiser state stay bitwise untouched, the steps count as skipped and not as clipped, and the next finite
    step updates.  (Non-finite values only pass through arithmetic here.)"""
    m = _model().train()
    g0 = _first_gradient(m).clone()
    flat, gflat = m.flat_parameters()
    opt = _make(kind, m, 0.5 * _first_norm())
    twin_m = _model().train()
    _first_gradient(twin_m)
    twin_m.flat_parameters()[1].copy_(g0)
    twin = _make(kind, twin_m, 0.5 * _first_norm())

    def state():
        st = opt.state[opt.param_groups[0]["params"][0]]
        return [flat.clone()] + [st[k].clone() for k in (("momentum_buffer",) if kind == "sgd" else ("exp_avg", "exp_avg_sq"))]

    opt.step()  # a finite step first: the state is not all zeros
    twin.step()
    before = state()
    for bad in (float("inf"), float("nan")):
        gflat.copy_(g0)
        gflat[12345] = bad
        opt.step()
        torch.cuda.synchronize()
        assert not np.isfinite(float(opt.last_grad_norm))
        for a, b in zip(before, state()):
            assert torch.equal(a, b)
    st = opt.grad_norm_stats(reset=False)
    assert (st["steps"], st["skipped"], st["clipped"]) == (3, 2, 1) and abs(st["max_norm"] - _first_norm()) <= 1e-12 * st["max_norm"] and abs(st["mean_norm"] - st["max_norm"]) <= 1e-12 * st["max_norm"]
    gflat.copy_(g0)
    twin_m.flat_parameters()[1].copy_(g0)
    opt.step()
    twin.step()
    torch.cuda.synchronize()
    after = state()
    assert all(torch.isfinite(t).all() for t in after) and not torch.equal(after[0], before[0])
    if kind == "sgd":  # no host step counter: exactly the run without the two skipped steps
        assert torch.equal(after[0], twin_m.flat_parameters()[0])
    assert opt.grad_norm_stats()["steps"] == 4


def test_grad_norm_statistics_and_reset():
    m = _model().train()
    _first_gradient(m)
    flat, gflat = m.flat_parameters()
    opt = V.SGD(m.parameters(), lr=1e-3, max_grad_norm=3.5)
    for v in (1.0, 2.0, 3.0, 4.0, 10.0):
        gflat.zero_()
        gflat[7] = -v  # the norm is exactly v
        opt.step()
    assert float(opt.last_grad_norm) == 10.0
    assert opt.grad_norm_stats(reset=False) == dict(steps=5, clipped=2, skipped=0, mean_norm=4.0, max_norm=10.0)
    assert opt.grad_norm_stats(reset=True) == dict(steps=5, clipped=2, skipped=0, mean_norm=4.0, max_norm=10.0)
    assert opt.grad_norm_stats() == dict(steps=0, clipped=0, skipped=0, mean_norm=0.0, max_norm=0.0)
    gflat[7] = 2.0
    opt.step()
    assert opt.grad_norm_stats() == dict(steps=1, clipped=0, skipped=0, mean_norm=2.0, max_norm=2.0)
    assert float(gflat[7]) == 2.0  # p.grad stays unclipped


# ---- VSparams ---------------------------------------------------------------------------------------------------------------------------------------
class _Loader:
    """Two synthetic batches per epoch; notes the learning rate the optimiser holds while the epoch runs."""

    batch_size = 2

    def __init__(self, nbatches, seen=None, opt=None):
        self.nbatches, self.seen, self.opt = nbatches, seen, opt

    def __len__(self):
        return self.nbatches * self.batch_size

    def __iter__(self):
        if self.seen is not None:
            self.seen.append(self.opt.param_groups[0]["lr"])
        x, y = _batch()
        for _ in range(self.nbatches):
            yield {"image": x, "label": y}


def _vsparams(tmp_path, extra):
    from vs_seg_amd.params import VSparams

    p = VSparams(argparse.ArgumentParser(), ["--debug", "--num_epochs", "4", "--data_root", str(tmp_path) + "/", "--compute_dtype", "fp32", "--train_batch_size", "2"] + extra)
    lines = []
    p.logger = type("Log", (), {"info": staticmethod(lines.append), "error": staticmethod(lines.append)})()
    p.create_results_folders()
    return p, lines


def test_set_and_get_optimizer_builds_the_class_the_flag_names(tmp_path):
    for extra, cls, check in (([], V.Adam, lambda o: type(o) is V.Adam and o.max_grad_norm is None and o.param_groups[0]["weight_decay"] == 1e-7 and not o.param_groups[0]["decoupled_weight_decay"]),
                              (["--optimizer", "adamw", "--weight_decay", "0.01", "--clip_grad_norm", "2"], V.AdamW, lambda o: o.max_grad_norm == 2.0 and o.param_groups[0]["weight_decay"] == 0.01 and o.param_groups[0]["decoupled_weight_decay"]),
                              (["--optimizer", "sgd", "--nesterov", "--weight_decay", "3e-5", "--clip_grad_norm", "12", "--initial_learning_rate", "0.01"], V.SGD,
                               lambda o: o.max_grad_norm == 12.0 and o.param_groups[0]["momentum"] == 0.99 and o.param_groups[0]["nesterov"] and o.param_groups[0]["weight_decay"] == 3e-5 and o.param_groups[0]["lr"] == 0.01),
                              (["--optimizer", "sgd", "--momentum", "0.9"], V.SGD, lambda o: o.max_grad_norm is None and o.param_groups[0]["momentum"] == 0.9 and not o.param_groups[0]["nesterov"])):
        p, _ = _vsparams(tmp_path, extra)
        opt = p.set_and_get_optimizer(_model())
        assert isinstance(opt, cls) and check(opt), extra


@pytest.mark.parametrize("flags", ["nnunet", "defaults"])
def test_training_loop_sets_the_poly_rate_and_logs_the_norm_line_only_when_asked(tmp_path, flags):
    extra = ["--optimizer", "sgd", "--nesterov", "--weight_decay", "3e-5", "--clip_grad_norm", "12", "--lr_schedule", "poly", "--initial_learning_rate", "0.01"] if flags == "nnunet" else []
    p, lines = _vsparams(tmp_path, extra)
    model, loss_fn = p.set_and_get_model(), p.set_and_get_loss_function()
    opt = p.set_and_get_optimizer(model)
    seen = []
    losses, metrics = p.run_training_algorithm(model, loss_fn, opt, _Loader(2, seen, opt), _Loader(0))
    assert len(losses) == 4 and np.isfinite(losses).all() and len(metrics) == 2
    norm_lines = [ln for ln in lines if "gradient norm" in ln]
    poly_lines = [ln for ln in lines if "Polynomial learning rate" in ln]
    halving = [ln for ln in lines if "Dividing learning rate" in ln]
    if flags == "nnunet":
        want = [0.01 * (1 - e / 4) ** 0.9 for e in range(4)]
        assert seen == [V.poly_lr(0.01, e, 4, 0.9) for e in range(4)] and np.allclose(seen, want, rtol=1e-15, atol=0)
        assert len(poly_lines) == 4 and not halving
        assert len(norm_lines) == 4 and all("/2 steps at 12.0" in ln and "skipped 0" in ln for ln in norm_lines), norm_lines
        assert opt.grad_norm_stats()["steps"] == 0  # read and reset every epoch
    else:
        assert seen == [1e-4, 1e-4, 1e-4, 5e-5] and len(halving) == 1  # --debug halves every 3 epochs, as before
        assert not norm_lines and not poly_lines
    assert V.fx_status() is False
