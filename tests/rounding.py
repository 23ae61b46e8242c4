"""Rounding-aware comparison of a bf16 kernel output with its fp64 definition.

A bf16 kernel of this project accumulates in fp32 and rounds ONCE, to nearest even, when it stores.  With operands that are bf16 values on both
sides the only differences from the fp64 definition are the fp32 accumulator's error (the bar of the fp32 parity mode: 2e-5 of the largest
output) and that one rounding.  `assert_one_rounding` holds an output to exactly that: every element lies between the bf16 roundings of
ref - e and ref + e.  A truncating store, a rounding in front of the residual add, a running sum kept in bf16 or a dropped product leave that
interval in a large share of the elements (tests/test_rounding_host.py plants each of them).
"""
import torch

E_REL = 2e-5  # the fp32 accumulator bar (tests/test_gpu_ops.py `_tol`), relative to max |ref|


def rne_bf16(ref64: torch.Tensor) -> torch.Tensor:
    """The bf16 value nearest to each fp64 element, ties to even, returned as fp64.  Computed on the fp64 value itself (frexp -> round the
    8-bit significand -> ldexp; torch.round is half-to-even): a cast through fp32 would round twice.  Signed zeros keep their sign, values
    below the smallest normal round on the subnormal grid, values beyond the largest finite bf16 become +-inf."""
    x = ref64.detach().to(torch.float64)
    m, ex = torch.frexp(x)  # x = m * 2^ex, 0.5 <= |m| < 1 (0 -> m = 0, ex = 0)
    ex = ex.to(torch.float64).clamp(min=-125.0)  # bf16 subnormals: the grid below 2^-126 is that of the smallest normal binade
    quantum = torch.pow(torch.tensor(2.0, dtype=torch.float64), ex - 8.0)  # exact: a power of two
    out = torch.round(x / quantum) * quantum  # x / quantum is exact (scaling by a power of two); 8 significant bits: 1 implicit + 7 stored
    out = torch.where(out.abs() >= 2.0 ** 128, torch.copysign(torch.full_like(out, float("inf")), x), out)
    return torch.where(torch.isfinite(x), out, x)


def assert_one_rounding(got: torch.Tensor, ref64: torch.Tensor, *, e=None, what: str = "") -> float:
    """Every element of `got` (a bf16 tensor, or its float image) satisfies rne_bf16(ref - e) <= got <= rne_bf16(ref + e); NaN and inf fail.
    e defaults to 2e-5 * max|ref|: the accumulators of the bf16 path are fp32, exactly as in the fp32 mode, whose bar this is.
    Prints and returns the share of elements with got != rne_bf16(ref) (for the record, not asserted)."""
    g = got.detach().to("cpu").to(torch.float64)
    ref = ref64.detach().to("cpu").to(torch.float64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} against reference {tuple(ref.shape)}"
    if e is None:
        e = E_REL * float(ref.abs().max())
    e = float(e)
    lo, hi = rne_bf16(ref - e), rne_bf16(ref + e)
    below, above = g < lo, g > hi
    bad = below | above | ~torch.isfinite(g)
    share = float((g != rne_bf16(ref)).double().mean()) if g.numel() else 0.0
    print(f"one-rounding [{what}]: {g.numel()} elements, share != RNE(ref) {share:.3g}, e {e:.3g}, violations {int(bad.sum())}")
    if bad.any():
        nb, na, nn = int(below.sum()), int(above.sum()), int((~torch.isfinite(g)).sum())
        excess = torch.where(below, lo - g, torch.where(above, g - hi, torch.zeros_like(g)))
        excess = torch.where(torch.isfinite(g), excess, torch.full_like(g, float("inf")))
        i = int(excess.reshape(-1).argmax())
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape)) if g.dim() else ()
        toward = bad & (g.abs() < torch.minimum(lo.abs(), hi.abs()))
        away = bad & (g.abs() > torch.maximum(lo.abs(), hi.abs()))
        nz, nw = int(toward.sum()), int(away.sum())
        if nn == int(bad.sum()):
            sided = "non-finite values"
        elif (nb == 0) != (na == 0):
            sided = "one-sided in value: a bias or a truncation"
        elif (nz == 0) != (nw == 0):
            sided = "one-sided in magnitude: a truncation or a bias"
        else:
            sided = "two-sided: a double rounding"
        need = float((g - ref).abs()[torch.isfinite(g)].max()) if bool(torch.isfinite(g).any()) else float("inf")
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {g.numel()} elements outside one rounding of the fp64 result ({nb} below, {na} above, {nz} towards zero, {nw} away from zero, {nn} non-finite; {sided}); "
            f"worst at {idx}: got {float(g.reshape(-1)[i])!r}, ref {float(ref.reshape(-1)[i])!r}, interval [{float(lo.reshape(-1)[i])!r}, {float(hi.reshape(-1)[i])!r}], "
            f"excess {float(excess.reshape(-1)[i]):.3g}; e {e:.3g}, max |got - ref| {need:.3g}, share != RNE(ref) {share:.3g}")
    return share
