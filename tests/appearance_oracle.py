"""numpy fp64 restatement of `vsseg_patch_filter` and `vsseg_patch_tone` (include/vsseg_hip.h) and the DERIVED bounds on what fp32 may do to them: nothing here is
measured except POW_ULP, which says how.  Test infrastructure only."""
import numpy as np

EPS = 2.0 ** -24  # fp32: a correctly rounded operation is within EPS * |result| of the exact one
TINY = 2.0 ** -126  # the absolute error of a result that underflows
DEN = float(np.float32(1e-7))  # the 1e-7f of the gamma map
# powf: no document or header of the device library states a bound, so it is measured (tests/test_gpu_appearance_augment.py::test_powf_error_against_fp64: the entry
# point itself, on inputs with min 0 and max 4, where out / 4 IS powf(x / 4, gamma); against pow in fp64).  Measured on an MI355X: max |powf - pow64| = 1.21 ulp
# over 2 x 49152 bases in [0, 1] at gamma 0.7 and 1.5.  The bar is 4 x that figure and not below 2 ulp.
POW_MEASURED_ULP = 1.21
POW_ULP = max(4.0 * POW_MEASURED_ULP, 2.0)
POW_REL = POW_ULP * 2.0 ** -23  # one ulp is at most 2^-23 of the value


# ---- host-side derived quantities ----
def radius(sigma):
    return int(np.ceil(3.0 * float(sigma)))


def taps(sigma):
    """fp32 half-taps w_0 .. w_R as the device gets them, R = ceil(3 sigma): exp(-k^2 / 2 sigma^2) normalised in fp64 to w_0 + 2 sum w_k = 1, rounded once."""
    k = np.arange(radius(sigma) + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return (w / (w[0] + 2.0 * w[1:].sum())).astype(np.float32)


def coarse_size(roi, f):
    return tuple(max(1, int(np.floor(int(roi[a]) * float(f) + 0.5))) for a in range(2))


def q_index(n, roi):
    """Source index of every coarse sample of an axis: floor((2i + 1) roi / (2n)) in integers."""
    i = np.arange(int(n), dtype=np.int64)
    return (2 * i + 1) * int(roi) // (2 * int(n))


def reflect(i, n):
    """The edge-repeating reflection (..., 1, 0 | 0, 1, ..., n-1 | n-1, n-2, ...) of period 2n, for any integer i."""
    m = np.mod(np.asarray(i, np.int64), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


# ---- blur ----
def _blur_axis(v, w, axis):
    n, R = v.shape[axis], len(w) - 1
    p = np.arange(n)
    out = np.zeros_like(v, dtype=np.float64)
    for k in range(-R, R + 1):
        out += float(w[abs(k)]) * np.take(v, reflect(p + k, n), axis=axis)
    return out


def blur(v, w):
    """u = G_y(G_x(v)) in fp64 with the fp32 taps w; v is [rx, ry, rz]."""
    return _blur_axis(_blur_axis(np.asarray(v, np.float64), w, 0), w, 1)


def blur_tolerance(v, w):
    """Pointwise bound on |fp32 blur - fp64 blur|.  A sum of n = 2R + 1 terms accumulated in fp32 in ANY order, fused or not, puts at most n roundings on a term:
    |fl(sum) - sum| <= g sum |w| |v| with g = gamma_n = n EPS / (1 - n EPS).  Pass one leaves e1 <= g G_x|v|; pass two sees G_x v + e1 and adds its own g G_y|G_x v + e1|:
    e <= G_y e1 + g (1 + g) G_y G_x |v| <= (2 g + g^2) G_y G_x |v|   (the taps are >= 0, so G|v| is the blur of |v|), plus an underflow per term."""
    n = 2 * (len(w) - 1) + 1
    g = n * EPS / (1.0 - n * EPS)
    return (2.0 * g + g * g) * blur(np.abs(np.asarray(v, np.float64)), w) + 2 * n * TINY


# ---- low resolution ----
def _axis(n, roi):
    p = np.arange(roi, dtype=np.float64)
    t = np.clip((p + 0.5) * n / roi - 0.5, 0.0, n - 1.0)
    i0 = np.floor(t).astype(np.int64)
    i1 = np.minimum(i0 + 1, n - 1)
    q = q_index(n, roi)
    return q[i0], q[i1], t - i0


def lowres(u, coarse):
    """Nearest-neighbour sampling at coarse[0] x coarse[1] in-plane positions, bilinear interpolation back, fp64; u is [rx, ry, rz]."""
    u = np.asarray(u, np.float64)
    x0, x1, fx = _axis(coarse[0], u.shape[0])
    y0, y1, fy = _axis(coarse[1], u.shape[1])
    fx, fy = fx[:, None, None], fy[None, :, None]
    lo = u[x0][:, y0] + fy * (u[x0][:, y1] - u[x0][:, y0])
    hi = u[x1][:, y0] + fy * (u[x1][:, y1] - u[x1][:, y0])
    return lo + fx * (hi - lo)


def lowres_tolerance(u, coarse, u_tol=0.0):
    """Bound on |fp32 low resolution of the device's u - fp64 low resolution of the oracle's u| (one number for the patch).
      t         (p + 0.5) is exact; the product, the division and the subtraction round once each, each within EPS of a value <= n_a: |dt| <= 3 EPS n_a.  phi = t - i0 is exact.
                The value is continuous and piecewise linear in t, also across a change of floor(t), so dt moves it by at most dt times the largest slope along that axis:
                the largest difference L_a of neighbouring coarse samples (an axis with n_a == roi_a is not interpolated: no term).
      fused     each fmaf(phi, b - a, a): b - a rounds (EPS |b - a| phi), the fmaf rounds (EPS |result|): <= 3 EPS M with M = max |u|; the first level passes through the second
                with a weight <= 1, the second adds its own: 6 EPS M, rounded up to 8.
      source    the device interpolates ITS u: a convex combination of errors each <= max u_tol."""
    u = np.asarray(u, np.float64)
    tol = 8.0 * EPS * float(np.abs(u).max()) + float(np.max(u_tol)) + TINY
    for a in range(2):
        n, roi = int(coarse[a]), u.shape[a]
        if n != roi and n > 1:
            c = np.take(u, q_index(n, roi), axis=a)
            tol += 3.0 * EPS * n * float(np.abs(np.diff(c, axis=a)).max())
    return tol


def filter_job(v, w=None, coarse=None):
    """(fp64 result, tolerance) of one job of vsseg_patch_filter: half-taps w (None or empty: no blur), coarse in-plane size (None or the roi: no low resolution)."""
    v = np.asarray(v, np.float64)
    u, tol = v, 0.0
    if w is not None and len(w) > 1:
        u, tol = blur(v, w), blur_tolerance(v, w)
    if coarse is not None and tuple(coarse) != v.shape[:2]:
        u, tol = lowres(u, coarse), lowres_tolerance(u, coarse, tol)
    return u, tol


# ---- tone ----
def mean_bound(mu64):
    """|mu - fl32(mu64)| <= 1 ulp of mu: the device's S is an fp64 sum in another order (relative error about n 2^-53, nothing beside fp32), which can at most move the one
    rounding to fp32 to the neighbouring value."""
    return float(np.spacing(np.float32(abs(mu64))))


def contrast(x, c, stats):
    """(y, tolerance, clamped mask) of T(x) = clip((x - mu) c + mu, mn, mx) with the DEVICE's stats (mn, mx, mu: fp32 values) and c at its fp32 value.
    x - mu rounds (EPS |x - mu|, times c), the fused step rounds (EPS |result|); the clamp is exact and 1-Lipschitz."""
    x = np.asarray(x, np.float64)
    mn, mx, mu = (float(s) for s in stats[:3])
    c = float(np.float32(c))
    if c == 1.0:
        return x, np.zeros_like(x), np.zeros(x.shape, bool)
    raw = (x - mu) * c + mu
    return np.clip(raw, mn, mx), EPS * (np.abs(x - mu) * c + np.abs(raw)) + TINY, (raw < mn) | (raw > mx)


def tone(x, c, g, stats):
    """(out, tolerance) of one job of vsseg_patch_tone in fp64, with the device's stats.
    gamma: out = base^g r + a, base = (y - a) / (r + 1e-7f).  With ty, ta, tb the contrast bounds of y, a = T(mn), b = T(mx):
      numerator   |d(y - a)| <= ty + ta + EPS |y - a|;      denominator   |d den| <= ta + tb + EPS |r| + EPS den  (r = b - a rounds, the sum rounds)
      base        |d base| <= (|d num| + base |d den|) / den + EPS base  (correctly rounded division)
      power       pow is monotone in its base, so |pow(base +- d) - pow(base)| is evaluated at the two ends of the interval (this IS the relative error of the base
                  amplified by gamma, and stays finite at base = 0 for gamma < 1), plus POW_REL of the value for powf itself
      result      r |d pow| + pow (ta + tb + EPS |r|) + ta, and the final fused step: EPS |out|."""
    y, ty, _ = contrast(x, c, stats)
    g = float(np.float32(g))
    if g == 1.0:
        return y, ty
    mn, mx = float(stats[0]), float(stats[1])
    (a, b), (ta, tb), _ = contrast(np.array([mn, mx]), c, stats)
    r, den = b - a, b - a + DEN
    base = (y - a) / den
    dr = ta + tb + EPS * abs(r)
    dbase = (ty + ta + EPS * np.abs(y - a) + base * (dr + EPS * den)) / den + EPS * base
    p = base ** g
    dp = np.maximum(np.abs((base + dbase) ** g - p), np.abs(np.maximum(base - dbase, 0.0) ** g - p)) + POW_REL * p
    out = p * r + a
    return out, r * dp + p * dr + ta + EPS * np.abs(out) + TINY


# ---- the inputs of the tone tests: standard normal, so that c = 1.25 clamps at least one voxel (the extremes) and at most half of them ----
TONE_SIZES = (105, 2805, 49152, 135168)  # one, a few and all of the 128 shards of 1024-element chunks
TONE_JOBS = ((0.75, 1.0), (1.25, 1.0), (1.0, 0.7), (1.0, 1.5), (1.25, 0.7), (1.0, 1.0))


def tone_input(n):
    """fp32 [len(TONE_JOBS), n], another content per job."""
    return np.random.default_rng(1000 + n).standard_normal((len(TONE_JOBS), n)).astype(np.float32)
