"""CPU oracle of the clipped optimiser step (vs_seg_amd.SGD / Adam / AdamW with max_grad_norm, vsseg_grad_norm + vsseg_sgd / vsseg_adam_clipped):
the L2 norm of grad_scale * g in fp64, the coefficient min(1, max_norm / (norm + 1e-6)) of torch.nn.utils.clip_grad_norm_ in fp64 rounded once to fp32, multiplied
into the fp32 gradient, then one step of torch.optim.SGD / Adam / AdamW on the CPU.  (torch's own clip_grad_norm_ accumulates the norm in fp32: on 300k elements
spanning five decades it is off from fp64 by 1.2e-5 relative, so it is not the oracle of the norm.)

Also the kernels' update formulas written out in numpy fp32 (sgd_by_hand, adamw_by_hand), which tests/test_optim_host.py holds against torch.optim."""
import numpy as np
import torch


def grad_norm(grads, grad_scale=1.0) -> float:
    """fp64 L2 norm of grad_scale * g over all tensors of `grads` (a tensor or a list of tensors)."""
    grads = [grads] if torch.is_tensor(grads) else list(grads)
    total = sum(float((g.detach().double().cpu() * float(grad_scale)).pow(2).sum()) for g in grads)
    return float(np.sqrt(np.float64(total)))


def clip_coef(norm: float, max_norm) -> np.float32:
    """fp32 coefficient: 1 without clipping, 0 for a non-finite norm (the step is skipped)."""
    if max_norm is None:
        return np.float32(1.0)
    if not np.isfinite(norm):
        return np.float32(0.0)
    return np.float32(min(1.0, float(max_norm) / (float(norm) + 1e-6)))


def make_optimizer(kind: str, params, **kw):
    if kind == "sgd":
        return torch.optim.SGD(params, lr=kw["lr"], momentum=kw.get("momentum", 0.0), dampening=0.0, weight_decay=kw.get("weight_decay", 0.0), nesterov=kw.get("nesterov", False))
    cls = {"adam": torch.optim.Adam, "adamw": torch.optim.AdamW}[kind]
    return cls(params, lr=kw["lr"], betas=kw.get("betas", (0.9, 0.999)), eps=kw.get("eps", 1e-8), weight_decay=kw.get("weight_decay", 0.0))


class Stepper:
    """torch.optim on CPU copies of the parameters; step(grads) clips as described above and returns the fp64 norm.  A non-finite norm skips the step."""

    def __init__(self, kind: str, params, max_norm=None, grad_scale=1.0, **kw):
        self.params = [torch.nn.Parameter(p.detach().float().cpu().clone()) for p in ([params] if torch.is_tensor(params) else params)]
        self.opt = make_optimizer(kind, self.params, **kw)
        self.max_norm, self.grad_scale = max_norm, float(grad_scale)

    def step(self, grads) -> float:
        grads = [grads] if torch.is_tensor(grads) else list(grads)
        norm = grad_norm(grads, self.grad_scale)
        if self.max_norm is not None and not np.isfinite(norm):
            return norm
        c = torch.tensor(clip_coef(norm, self.max_norm))
        for p, g in zip(self.params, grads):
            p.grad = (g.detach().float().cpu() * self.grad_scale) * c  # fp32 products, in the kernels' order
        self.opt.step()
        return norm

    def values(self):
        return [p.detach().clone() for p in self.params]


def run(kind: str, p0, grads_per_step, max_norm=None, grad_scale=1.0, **kw):
    """(norms, parameters after each step) of the steps over `grads_per_step` on one flat tensor."""
    s = Stepper(kind, p0, max_norm, grad_scale, **kw)
    norms, after = [], []
    for g in grads_per_step:
        norms.append(s.step(g))
        after.append(s.values()[0])
    return norms, after


# ---- the kernels' formulas, numpy fp32 (csrc/optim.hip: sgd_elem, adam_elem) ------------------------------------------------------------------------
F = np.float32


def sgd_by_hand(p, g, buf, lr, mu, wd, nesterov, coef=1.0, gscale=1.0):
    """One vsseg_sgd step; returns (p, buf).  buf starts as zeros."""
    gg = g * F(gscale) * F(coef) + F(wd) * p
    d = gg
    if mu > 0:
        buf = F(mu) * buf + gg
        d = gg + F(mu) * buf if nesterov else buf
    return (p - F(lr) * d).astype(F), buf.astype(F)


def adamw_by_hand(p, g, m, v, t, lr, b1, b2, eps, wd, decoupled=True, coef=1.0, gscale=1.0):
    """One vsseg_adam_clipped step (t = 1, 2, ...); returns (p, m, v)."""
    gg = g * F(gscale) * F(coef)
    if decoupled:
        p = p * F(1.0 - float(F(lr)) * float(F(wd)))
    else:
        gg = gg + F(wd) * p
    m = F(b1) * m + (F(1) - F(b1)) * gg
    v = F(b2) * v + (F(1) - F(b2)) * gg * gg
    step_size = F(lr) / F(1.0 - b1**t)
    inv_sqrt_bc2 = F(1) / np.sqrt(F(1.0 - b2**t))
    p = p - step_size * m / (np.sqrt(v) * inv_sqrt_bc2 + F(eps))
    return p.astype(F), m.astype(F), v.astype(F)
