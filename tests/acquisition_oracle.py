"""numpy fp64 restatement of `vsseg_patch_acquisition` (include/vsseg_hip.h: thick slices T, ghosting G, spike S, y = S(G(T(v)))) and the DERIVED bounds on what fp32 may
do to it: nothing here is measured except COS_MEASURED_ULP, which says how.  Test infrastructure only."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -24  # fp32: a correctly rounded operation is within EPS * |result| of the exact one
TINY = 2.0 ** -126  # the absolute error of a result that underflows
TWO_PI_F = float(np.float32(6.2831853))  # the constant of the spike's argument
# cosf: no document or header of the device library states a bound, so it is measured (tests/test_gpu_acquisition_augment.py::test_cosf_error_against_fp64: the entry
# point itself on a zero patch with amp = 1, where the output IS cosf(theta) and theta is reproduced bit for bit on the host; against cos in fp64).  Measured on an
# MI355X: max |cosf - cos64| = 1.50 ulp over 6 x 2880 arguments in [0, 4 pi] (six phases, every 2 pi t / 2880 behind each).  The bar is 4 x that figure.
COS_MEASURED_ULP = 1.50
COS_ULP = 4.0 * COS_MEASURED_ULP


def gamma(n):
    """The constant of a sum of n terms accumulated in fp32 in ANY order: at most n roundings on a term."""
    return n * EPS / (1.0 - n * EPS)


# ---- thick slices ----
def slabs(rz, f, o):
    """(first z, last z) of every slab of a column of rz voxels: slab k holds the z with (z + o) // f == k; the first and the last may be short."""
    K = (rz - 1 + o) // f + 1
    return [(max(k * f - o, 0), min((k + 1) * f - o, rz) - 1) for k in range(K)]


def thick_weights(rz, f, o):
    """Per output z: (a, b, phi), the two slabs and the fraction of `out = m_a + phi (m_b - m_a)`."""
    sl = slabs(rz, f, o)
    K, c = len(sl), [(lo + hi) / 2.0 for lo, hi in sl]
    a, b, phi = np.zeros(rz, int), np.zeros(rz, int), np.zeros(rz)
    for z in range(rz):
        k = (z + o) // f
        ka, kb = (k, k + 1) if z >= c[k] else (k - 1, k)
        if ka < 0:
            ka = kb = 0
        if kb > K - 1:
            ka = kb = K - 1
        a[z], b[z], phi[z] = ka, kb, 0.0 if ka == kb else (z - c[ka]) / (c[kb] - c[ka])
    return a, b, phi


def thick(v, f, o=0):
    """(T(v), tolerance) in fp64; v is [rx, ry, rz].  f == 1: v itself, tolerance 0.
      mean      a slab of cnt voxels summed in fp32 and divided once: |dm| <= gamma(cnt) * mean |v| (cnt - 1 additions and the division)
      phi       z - c_a and c_b - c_a are small multiples of 0.5 and exact; the division rounds once: |dphi| <= EPS phi
      result    m_b - m_a rounds (EPS |m_b - m_a|, weight phi), dphi multiplies it, the fused step rounds (EPS |out|); the errors of the two means enter with the
                weights 1 - phi and phi.  2 EPS phi |m_b - m_a| is written with a 3: the second-order terms."""
    v = np.asarray(v, np.float64)
    if f == 1:
        return v, np.zeros_like(v)
    rz = v.shape[2]
    sl = slabs(rz, f, o)
    m = np.stack([v[:, :, lo:hi + 1].mean(axis=2) for lo, hi in sl], axis=2)
    tm = np.stack([gamma(hi - lo + 1) * np.abs(v[:, :, lo:hi + 1]).mean(axis=2) for lo, hi in sl], axis=2) + TINY
    a, b, phi = thick_weights(rz, f, o)
    out = m[:, :, a] + phi * (m[:, :, b] - m[:, :, a])
    tol = (1.0 - phi) * tm[:, :, a] + phi * tm[:, :, b] + 3.0 * EPS * phi * np.abs(m[:, :, b] - m[:, :, a]) + EPS * np.abs(out) + TINY
    return out, tol


# ---- ghosting ----
def ghost_kspace(u, axis, n, alpha):
    """The definition: along `axis` every n-th k-space line is scaled by 1 - alpha, the DC line is left alone."""
    U = np.fft.fft(np.asarray(u, np.float64), axis=axis)
    k = np.arange(u.shape[axis])
    scale = np.where((k % n == 0) & (k != 0), 1.0 - alpha, 1.0)
    shape = [1] * u.ndim
    shape[axis] = -1
    return np.fft.ifft(U * scale.reshape(shape), axis=axis).real


def ghost(u, axis, n, alpha, u_tol=0.0):
    """(G(u), tolerance) in fp64 with alpha at its fp32 value: out = u[i] - (alpha / n) sum_j u[(i + j s) mod N] + alpha mu, s = N / n.
      mu        the device's fp64 sum runs in another order (relative error about N 2^-53, nothing beside fp32) and is rounded to fp32 once: at most 1 ulp of mu away
      c         alpha / n rounds once: EPS c
      S         n terms in fp32 in any order: gamma(n) A with A = sum_j |u_j| >= |S|
      fused     fmaf(-c, S, u) rounds (EPS |u - c S|), fmaf(alpha, mu, .) rounds (EPS |out|)
      source    G is linear: an error u_tol of its input passes through with the same weights, all taken positive."""
    u = np.asarray(u, np.float64)
    alpha, N = float(np.float32(alpha)), u.shape[axis]
    assert n >= 2 and N % n == 0 and 0.0 < alpha <= 1.0
    s, c = N // n, alpha / n
    S = sum(np.roll(u, -j * s, axis=axis) for j in range(n))
    A = sum(np.roll(np.abs(u), -j * s, axis=axis) for j in range(n))
    mu = u.mean(axis=axis, keepdims=True)
    out = u - c * S + alpha * mu
    tol = (gamma(n) * (1.0 + EPS) + EPS) * c * A + EPS * np.abs(u - c * S) + alpha * np.spacing(np.abs(mu).astype(np.float32)).astype(np.float64) + EPS * np.abs(out) + TINY
    ut = np.broadcast_to(np.asarray(u_tol, np.float64), u.shape)
    tol = tol + ut + c * sum(np.roll(ut, -j * s, axis=axis) for j in range(n)) + alpha * ut.mean(axis=axis, keepdims=True)
    return out, tol


# ---- spike ----
def spike_kspace(w, amp, k, phase):
    """The definition: amp rx ry / 2 e^{+-i phase} added at (kx, ky) and at (-kx, -ky) of every z slice."""
    w = np.asarray(w, np.float64)
    rx, ry = w.shape[:2]
    W = np.fft.fft2(w, axes=(0, 1))
    W[k[0] % rx, k[1] % ry] += amp * rx * ry / 2.0 * np.exp(1j * phase)
    W[-k[0] % rx, -k[1] % ry] += amp * rx * ry / 2.0 * np.exp(-1j * phase)
    return np.fft.ifft2(W, axes=(0, 1)).real


def spike_t(roi, k):
    """t[x, y] = ((kx x mod rx) ry + (ky y mod ry) rx) mod (rx ry), in integers."""
    rx, ry = int(roi[0]), int(roi[1])
    x, y = np.arange(rx, dtype=np.int64)[:, None], np.arange(ry, dtype=np.int64)[None, :]
    return (((int(k[0]) * x) % rx) * ry + ((int(k[1]) * y) % ry) * rx) % (rx * ry)


def spike(w, amp, k, phase, w_tol=0.0):
    """(S(w), tolerance) in fp64 with amp and phase at their fp32 values: out = w + amp cos(2 pi t / (rx ry) + phase).
      theta     (float)t, (float)(rx ry) and their quotient round once each (3 EPS of a ratio < 1), 6.2831853f is 0.47 EPS above 2 pi: 4 EPS of 2 pi ratio with the
                second-order terms; the fused step rounds: EPS theta.  cos is 1-Lipschitz.
      cosf      COS_ULP ulp of the value (measured: above)
      fused     EPS |out|."""
    w = np.asarray(w, np.float64)
    amp, phase = float(np.float32(amp)), float(np.float32(phase))
    rx, ry = w.shape[:2]
    ratio = spike_t((rx, ry), k)[:, :, None] / float(rx * ry)
    theta = 2.0 * np.pi * ratio + phase
    cs = np.cos(theta)
    out = w + amp * cs
    dtheta = 4.0 * EPS * 2.0 * np.pi * ratio + EPS * theta
    dcos = dtheta + COS_ULP * np.spacing(np.maximum(np.abs(cs), TINY).astype(np.float32)).astype(np.float64)
    return out, abs(amp) * dcos + EPS * np.abs(out) + TINY + np.asarray(w_tol, np.float64)


_STAGES = (thick, ghost, spike)  # (job's arguments carry the names of the record's fields, which shadow the stage functions)
NEUTRAL = dict(thick=1, thick_offset=0, ghost_axis=0, ghosts=0, ghost_alpha=0.0, spike_amp=0.0, spike_k=(0, 0), spike_phase=0.0)


def job(v, thick=1, thick_offset=0, ghost_axis=0, ghosts=0, ghost_alpha=0.0, spike_amp=0.0, spike_k=(0, 0), spike_phase=0.0, **_):
    """(fp64 result, tolerance) of one job of vsseg_patch_acquisition, named as the fields of vsseg_acquisition_job; the neutral job returns (v, 0)."""
    out, tol = _STAGES[0](v, thick, thick_offset)
    if ghosts:
        out, tol = _STAGES[1](out, ghost_axis, ghosts, ghost_alpha, tol)
    if float(spike_amp) != 0.0:
        out, tol = _STAGES[2](out, spike_amp, spike_k, spike_phase, tol)
    return out, tol


# ---- the device's argument of the cosine, bit for bit (for the measurement of cosf only) ----
def _round32(q):
    """The fp32 value nearest to the Fraction q (ties to even)."""
    c = np.float32(float(q))  # within one fp32 step of the right answer: fp64 rounds first
    best = c
    for cand in (np.nextafter(c, np.float32(-np.inf)), np.nextafter(c, np.float32(np.inf))):
        d, e = abs(Fraction(float(cand)) - q), abs(Fraction(float(best)) - q)
        if d < e or (d == e and (int(np.float32(cand).view(np.uint32)) & 1) == 0):
            best = cand
    return np.float32(best)


def spike_theta32(roi, k, phase):
    """theta[x, y] = fmaf(6.2831853f, (float)t / (float)(rx ry), phase) as the device forms it, in exact rational arithmetic rounded once."""
    t = spike_t(roi, k)
    den = np.float32(int(roi[0]) * int(roi[1]))
    ratio = (t.astype(np.float32) / den).astype(np.float32)  # numpy's fp32 conversion and division are correctly rounded
    ph = Fraction(float(np.float32(phase)))
    vals = {r: _round32(Fraction(TWO_PI_F) * Fraction(float(r)) + ph) for r in np.unique(ratio)}
    return np.vectorize(lambda r: vals[r], otypes=[np.float32])(ratio)
