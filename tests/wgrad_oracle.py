"""Exact-integer oracle of the weight-gradient kernels (csrc/wgrad.hip, mwgrad.hip, cwgrad.hip, wgrad_narrow.hip), on the CPU in fp64.

Operands are small non-zero integers ({-2, -1, 1, 2}; gate maps {0, 1}), so every product (|.| <= 4, <= 8 behind a gate) and every partial sum of a weight
gradient is an integer below 2^24: exact in an fp32 accumulator in ANY summation order, on the bf16 MFMA path, the fp32 MFMA path, the slab sums and the
narrow reductions alike.  The fp64 definition below is then the only admissible answer, bit for bit; `expected` asserts the range that makes this true, so
the GPU tests need no tolerance.  Because no operand is zero, a dropped, duplicated or mis-paired voxel-tap contribution of ONE voxel changes every
element of that tap's gradient (tests/test_wgrad_host.py checks this on planted faults instead of claiming it).

The case tables of tests/test_gpu_wgrad_exact.py live here as data; every row names the launch paths it is there to reach (`paths`), and
tests/test_wgrad_host.py proves from a host mirror of the launch arithmetic (`tile_launch`, `march_launch`, `compute_launch`) that it reaches them.

No GPU and no built library is needed to import this module."""
import zlib
from dataclasses import dataclass, replace
from typing import Optional, Tuple

import torch

from vs_seg_amd import planner as P

VALUES = (-2.0, -1.0, 1.0, 2.0)
EXACT_LIMIT = 1 << 24  # integers below 2^24 in magnitude are fp32 numbers, and so is every sum of them that stays below it


# ---------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One weight-gradient problem of a Conv3d (or ConvTranspose3d: tr) layer cin -> cout on an input of `dims`, and how it is launched."""
    id: str
    k: Tuple[int, int, int]
    s: Tuple[int, int, int]
    cin: int
    cout: int
    dims: Tuple[int, int, int]
    tr: bool = False
    batch: int = 2
    split: int = 0                      # two-part H: channels of the first part
    hgroup: int = 0                     # tile kernel: requested H chunks per workgroup
    single_buffer: int = 0
    blocks: Optional[int] = None        # persistent_blocks (None: the planner's)
    scratch_wgs: Optional[int] = None   # tile kernel: the scratch holds the slabs of exactly this many workgroups
    dbias: bool = False
    acc: bool = False                   # non-zero initial dw (and dbias), two calls in a row
    tile: Optional[Tuple[int, int, int]] = None  # marching kernel: (x steps per workgroup, rows, z slices)
    compact_p: bool = False             # marching kernel: P read as the compact two-channel tensor
    gate: bool = False                  # marching kernel: H multiplied by (1 + gate) on load
    compute: int = 0                    # compute kernel: H chunks per workgroup
    paths: frozenset = frozenset()

    # Conv3d: P = dY (cout), H = X (cin), lattice = dY.  ConvTranspose3d: P = X (cin), H = dY (cout), lattice = X.
    @property
    def ydims(self):
        return tuple(d * s for d, s in zip(self.dims, self.s)) if self.tr else tuple(-(-d // s) for d, s in zip(self.dims, self.s))

    @property
    def cp(self):
        return self.cin if self.tr else self.cout

    @property
    def ch(self):
        return self.cout if self.tr else self.cin

    @property
    def q(self):
        return self.dims if self.tr else self.ydims

    @property
    def hdims(self):
        return self.ydims if self.tr else self.dims

    @property
    def wshape(self):
        return (self.cp, self.ch, *self.k)

    @property
    def cp_stored(self):
        return P.round_up(self.cp, 8)

    @property
    def ch_stored(self):
        return P.round_up(self.ch, 8)


def _c(id, k, s, cin, cout, dims, paths=(), **kw):
    return Case(id, tuple(k), tuple(s), cin, cout, tuple(dims), paths=frozenset(paths), **kw)


S1, K331, K333, K111 = (1, 1, 1), (3, 3, 1), (3, 3, 3), (1, 1, 1)

# ---- tile kernel (march = 0), run in fp32 and bf16 ----
TILE_CASES = [
    # the nine layer shapes of test_gpu_ops.py::test_wgrad
    _c("331-16to16", K331, S1, 16, 16, (16, 16, 8), {"npp=0", "slab<=16"}),
    _c("333-96to48", K333, S1, 96, 48, (8, 8, 8), {"npp=0"}),
    _c("111-32to16", K111, S1, 32, 16, (8, 8, 8), {"wv=4"}),
    _c("333s222-48to48", K333, (2, 2, 2), 48, 48, (8, 8, 8), {"strided"}),
    _c("331s221-16to16", K331, (2, 2, 1), 16, 16, (16, 8, 4), {"strided"}),
    _c("333-40to1", K333, S1, 40, 1, (4, 4, 8), {"p-padded", "h-ragged-chunk", "npp>0"}),
    _c("331-1to16", K331, S1, 1, 16, (16, 16, 4), {"h-padded"}),  # cin 1 stored as 8
    _c("T333s222-96to80", K333, (2, 2, 2), 96, 80, (3, 1, 4), {"transposed", "strided", "npp>0"}, tr=True),
    _c("T331s221-32to16", K331, (2, 2, 1), 32, 16, (8, 8, 4), {"transposed", "strided"}, tr=True),
    # batch 1 and 3
    _c("331-16to16-b1", K331, S1, 16, 16, (16, 16, 8), {"batch1"}, batch=1),
    _c("331-16to16-b3", K331, S1, 16, 16, (16, 16, 8), {"batch3"}, batch=3),
    _c("333s222-48to48-b1", K333, (2, 2, 2), 48, 48, (8, 8, 8), {"batch1", "strided"}, batch=1),
    _c("333s222-48to48-b3", K333, (2, 2, 2), 48, 48, (8, 8, 8), {"batch3", "strided"}, batch=3),
    # narrow channel counts stored as one 8-channel group
    _c("331-32to2", K331, S1, 32, 2, (8, 8, 4), {"p-padded", "npp>0"}),
    _c("111-1to16", K111, S1, 1, 16, (6, 8, 4), {"h-padded", "wv=4"}),
    # 3, 5 and 10 chunks of H: a request of hgroup 4 clamps to 3, 1 and 2
    _c("331-40to16-hg4", K331, S1, 40, 16, (8, 8, 4), {"hg=3", "h-ragged-chunk"}, hgroup=4),
    _c("331-80to16-hg4", K331, S1, 80, 16, (8, 8, 4), {"hg=1"}, hgroup=4),
    _c("331-160to32-hg4", K331, S1, 160, 32, (8, 8, 4), {"hg=2"}, hgroup=4),
    # two-part H, the split inside the 64-channel group of hgroup 4
    # (the first row is the problem of test_gpu_ops.py::test_wgrad_h_chunk_groups: in bf16 it runs hgroup 4, in fp32 the LDS clamps it to 1 and with one
    #  buffer to 2 — tests/test_wgrad_host.py pins that; the second row's group of 4 fits in both element types)
    _c("331-64to32-split32-hg4", K331, S1, 64, 32, (16, 12, 8), {"two-part", "npp>0"}, split=32, hgroup=4),
    _c("331-64to16-split32-hg4", K331, S1, 64, 16, (8, 8, 4), {"hg=4", "two-part", "split-in-group"}, split=32, hgroup=4),
    _c("331-64to32-split32-hg2-sb", K331, S1, 64, 32, (16, 12, 8), {"hg=2", "two-part"}, split=32, hgroup=2, single_buffer=1),  # the split between two groups
    # every tile whole (no P coordinate table) and its twin with one ragged axis
    _c("331-32to32-whole", K331, S1, 32, 32, (8, 16, 8), {"npp=0"}),
    _c("331-32to32-ragged-y", K331, S1, 32, 32, (8, 15, 8), {"npp>0"}),
    # bias gradient through the tile kernel; accumulation into non-zero dw / dbias over two calls
    _c("331-16to16-bias-acc", K331, S1, 16, 16, (16, 16, 8), {"dbias", "acc"}, dbias=True, acc=True),
    _c("111-32to16-bias-acc", K111, S1, 32, 16, (8, 8, 8), {"dbias", "acc", "wv=4"}, dbias=True, acc=True),
    _c("333-96to48-bias", K333, S1, 96, 48, (8, 8, 8), {"dbias"}, dbias=True),
    _c("331-32to2-bias-acc-b3", K331, S1, 32, 2, (8, 8, 4), {"dbias", "acc", "p-padded", "batch3"}, dbias=True, acc=True, batch=3),
    # the bias rows lie behind the slabs of the workgroups ASKED for: a grid rounded down to a multiple of 8, a grid cut by the scratch
    _c("111-32to16-bias-pb9", K111, S1, 32, 16, (16, 16, 16), {"dbias", "round8", "wv=4"}, dbias=True, blocks=9),
    _c("111-32to16-bias-scr2", K111, S1, 32, 16, (16, 16, 16), {"dbias", "scratch-cap", "wv=4"}, dbias=True, scratch_wgs=2),
    _c("331-64to32-bias-scr3-hg4", K331, S1, 64, 32, (16, 12, 8), {"dbias", "scratch-cap", "wv=1"}, dbias=True, scratch_wgs=3, hgroup=4),
    _c("333s222-48to48-acc-b1", K333, (2, 2, 2), 48, 48, (8, 8, 8), {"acc", "batch1", "strided"}, acc=True, batch=1),
    _c("T331s221-32to16-acc", K331, (2, 2, 1), 32, 16, (8, 8, 4), {"acc", "transposed"}, tr=True, acc=True),
]

# ---- launch-shape sweep of the tile kernel ----
SWEEP_PROBLEMS = {
    "A": _c("sweepA-111-32to16", K111, S1, 32, 16, (16, 16, 16)),   # wv = 4, 32 tiles
    "B": _c("sweepB-331-64to32", K331, S1, 64, 32, (16, 12, 8)),    # wv = 1, four chunks of H
    "C": _c("sweepC-111-32to16", K111, S1, 32, 16, (16, 16, 32)),   # wv = 4, 64 tiles: more than 240 slabs
}
# (persistent_blocks: a number or an expression in the tile count, scratch sized for this many workgroups or None, paths)
SWEEP_POINTS = {
    "A": [(1, None, {"blocks<tiles", "walk-off", "slab<=16"}), (2, None, {"walk-off", "slab<=16"}), (7, None, {"walk-off", "slab-scalar"}),
          (8, None, {"walk-on", "slab-scalar"}), (9, None, {"round8", "walk-on"}), (16, None, {"walk-on", "slab-scalar"}),
          ("tiles-1", None, {"blocks<tiles", "round8", "slab-scalar"}), ("tiles", None, {"blocks=tiles", "walk-on", "slab-unroll1"}),
          ("tiles+5", None, {"blocks>tiles", "slab-unroll1"}),
          ("tiles", 1, {"scratch-cap", "slab<=16"}), ("tiles", 2, {"scratch-cap", "slab<=16"}), ("tiles", 3, {"scratch-cap", "slab<=16"})],
    "B": [(1, None, {"blocks<tiles", "walk-off"}), (2, None, {"walk-off"}), (7, None, {"walk-off"}), (8, None, {"walk-on"}), (9, None, {"round8"}),
          (16, None, {"blocks=tiles", "walk-on"}), ("tiles-1", None, {"blocks<tiles", "round8"}), ("tiles", None, {"blocks=tiles"}), ("tiles+5", None, {"blocks>tiles"}),
          ("tiles", 1, {"scratch-cap"}), ("tiles", 2, {"scratch-cap"}), ("tiles", 3, {"scratch-cap"})],
    "C": [("tiles-1", None, {"round8", "slab-unroll1"}), ("tiles", None, {"blocks=tiles", "walk-on", "slab-unroll2"}), ("tiles+5", None, {"blocks>tiles", "slab-unroll2"})],
}
SWEEP_HGROUPS, SWEEP_BUFFERS = (1, 2, 3, 4), (0, 1)


def sweep_cases(problem: str, es: int, hgroup: int, single_buffer: int):
    """The rows of one (problem, element size, hgroup, single_buffer) cell of the sweep, `blocks` resolved against the planner's tile count."""
    base = SWEEP_PROBLEMS[problem]
    tiles = tile_launch(base, es)["tiles"]
    out = []
    for spec, wgs, paths in SWEEP_POINTS[problem]:
        blocks = spec if isinstance(spec, int) else tiles + {"tiles-1": -1, "tiles": 0, "tiles+5": 5}[spec]
        out.append(replace(base, id=f"{base.id}-pb{spec}-scr{wgs}-hg{hgroup}-sb{single_buffer}", blocks=blocks, scratch_wgs=wgs, hgroup=hgroup, single_buffer=single_buffer, paths=frozenset(paths)))
    return out


# ---- marching kernel (march = 1), bf16, stride-1 3x3x1 ----
def _m(cin, cout, dims, split, tile, paths=(), **kw):
    tag = "".join(f"-{k}" for k, v in kw.items() if v and k in ("compact_p", "gate")) + (f"-b{kw['batch']}" if "batch" in kw else "")
    return _c(f"m{cin}to{cout}-{'x'.join(map(str, dims))}-t{'x'.join(map(str, tile))}{tag}", K331, S1, cin, cout, dims, paths, split=split, tile=tuple(tile), dbias=cout >= 16, **kw)


MARCH_HAND_CASES = [
    # the twelve rows of test_gpu_ops.py::MARCH_WGRAD_CASES with their hand tiles
    _m(16, 16, (10, 64, 8), 0, (4, 64, 4), {"x-segs>1", "x-ragged", "dbias"}),
    _m(16, 16, (6, 128, 8), 0, (6, 32, 4), {"x-segs=1", "row-blocks>1", "dbias"}),
    _m(16, 16, (5, 64, 16), 0, (5, 32, 8), {"row-blocks>1"}),
    _m(32, 16, (7, 64, 8), 16, (3, 64, 4), {"two-part", "x-ragged"}),
    _m(32, 16, (4, 64, 4), 0, (4, 64, 2)),
    _m(32, 2, (5, 64, 8), 0, (5, 64, 4), {"p-padded"}),
    _m(16, 32, (6, 64, 8), 0, (2, 64, 4), {"x-segs>1"}),
    _m(32, 32, (9, 64, 8), 0, (4, 64, 4), {"x-ragged"}),
    _m(32, 32, (4, 64, 4), 0, (4, 64, 2)),
    _m(64, 32, (6, 64, 4), 32, (6, 64, 2), {"two-part"}),
    _m(64, 32, (5, 32, 4), 0, (2, 32, 2), {"x-ragged"}),
    _m(64, 32, (4, 32, 8), 0, (4, 32, 4)),
    # the logits convolution: compact two-channel P, the gated H operand, both
    _m(32, 2, (5, 64, 8), 0, (5, 64, 4), {"compact-p"}, compact_p=True),
    _m(32, 2, (5, 64, 8), 0, (2, 64, 4), {"gate", "x-ragged"}, gate=True),
    _m(32, 2, (5, 64, 8), 16, (2, 64, 4), {"gate", "compact-p", "two-part"}, gate=True, compact_p=True),
    _m(32, 2, (5, 32, 4), 0, (5, 32, 4), {"gate"}, gate=True, batch=3),
    # the instantiations of planner.MARCH_WGRAD_SHAPES the rows above leave out
    _m(16, 16, (5, 64, 8), 0, (3, 64, 8), {"x-ragged"}),
    _m(32, 16, (5, 64, 4), 0, (2, 32, 4), {"row-blocks>1"}),
    _m(32, 2, (5, 32, 4), 0, (5, 32, 4), {"p-padded"}, batch=1),
    _m(16, 32, (4, 32, 8), 0, (2, 32, 8)),
    _m(16, 32, (5, 64, 4), 0, (3, 32, 4), {"row-blocks>1", "x-ragged"}),
    _m(32, 32, (5, 32, 4), 0, (2, 32, 4), {"x-ragged"}, batch=3),
]

# problems whose tiles come from planner.march_wgrad_tiles: q[0] = 17 makes it return two x segments, 9 + 8 planes
MARCH_PLANNER_PROBLEMS = [
    # cin, cout, dims, batch, H split
    (16, 16, (17, 64, 8), 1, 0), (16, 16, (17, 128, 8), 3, 0), (32, 16, (17, 64, 8), 2, 16), (32, 2, (17, 128, 8), 1, 0),
    (16, 32, (17, 64, 8), 3, 0), (32, 32, (17, 128, 8), 2, 0), (64, 32, (17, 64, 8), 1, 32), (64, 32, (17, 128, 8), 2, 0),
]


def march_planner_cases():
    """Every tile planner.march_wgrad_tiles returns for the problems above (what the engine's tuner tries), as rows."""
    out = []
    for cin, cout, dims, batch, split in MARCH_PLANNER_PROBLEMS:
        for tile in P.march_wgrad_tiles(cin, P.round_up(cout, 8), dims, batch):
            out.append(_m(cin, cout, dims, split, tile, {"x-segs>1", "x-ragged", "planner-tile"}, batch=batch))
    return out


# ---- compute kernel (march = 2), bf16, stride-1 3x3x3 ----
def _w(cin, cout, dims, batch, split, cg, bias, blocks, paths=()):
    return _c(f"c{cin}to{cout}-{'x'.join(map(str, dims))}-b{batch}-cg{cg}", K333, S1, cin, cout, dims, paths, batch=batch, split=split, compute=cg, dbias=bias, blocks=blocks)


COMPUTE_CASES = [
    # the nine rows of test_gpu_ops.py::COMPUTE_WGRAD_CASES
    _w(32, 48, (5, 8, 64), 2, 0, 2, False, None, {"ntp3-cg2", "pow2-classes"}),
    _w(32, 48, (4, 16, 32), 2, 0, 1, False, 8, {"ntp3-cg1", "pow2-classes"}),
    _w(48, 48, (6, 8, 32), 2, 0, 1, False, None, {"ntp3-cg1", "odd-classes"}),
    _w(96, 48, (4, 8, 64), 2, 48, 2, True, None, {"ntp3-cg2", "two-part", "dbias", "odd-classes"}),
    _w(96, 48, (7, 24, 32), 1, 0, 2, False, 2, {"ntp3-cg2", "odd-classes"}),
    _w(96, 48, (9, 8, 32), 1, 0, 1, False, 4, {"ntp3-cg1", "odd-classes"}),
    _w(48, 64, (4, 8, 64), 2, 0, 1, False, None, {"ntp4-cg1", "odd-classes"}),
    _w(64, 64, (6, 16, 32), 2, 0, 1, True, 8, {"ntp4-cg1", "dbias", "pow2-classes"}),
    _w(128, 64, (3, 8, 64), 1, 64, 1, True, None, {"ntp4-cg1", "two-part", "dbias", "pow2-classes"}),
    # batch 3, and the bias gradient of the 48-channel split with one chunk per workgroup
    _w(32, 48, (4, 16, 32), 3, 0, 1, True, 8, {"ntp3-cg1", "dbias", "batch3"}),
]

# ---- narrow reduction (vsseg_wgrad_narrow), fp32 and bf16: one input or one output channel ----
NARROW_CASES = [
    # the five rows of test_gpu_ops.py::test_wgrad_narrow
    _c("n331-1to16", K331, S1, 1, 16, (12, 16, 8)),
    _c("n111-1to16", K111, S1, 1, 16, (6, 8, 4)),
    _c("n331-16to1", K331, S1, 16, 1, (12, 16, 8), dbias=True),
    _c("n331-32to1", K331, S1, 32, 1, (5, 8, 12), dbias=True),
    _c("n331-1to8", K331, S1, 1, 8, (3, 4, 2)),
    # batch 1 and 3 of one C -> 1 and one 1 -> C row
    _c("n331-16to1-b1", K331, S1, 16, 1, (12, 16, 8), {"batch1"}, dbias=True, batch=1),
    _c("n331-16to1-b3", K331, S1, 16, 1, (12, 16, 8), {"batch3"}, dbias=True, batch=3),
    _c("n331-1to16-b1", K331, S1, 1, 16, (12, 16, 8), {"batch1"}, batch=1),
    _c("n331-1to16-b3", K331, S1, 1, 16, (12, 16, 8), {"batch3"}, batch=3),
    # odd extents: x and z odd, y an odd multiple of the four rows a thread owns (the library refuses a y extent that is no multiple of 4, see NARROW_REFUSED)
    _c("n331-32to1-odd", K331, S1, 32, 1, (5, 12, 3), {"odd-extents"}, dbias=True),
    _c("n331-1to16-odd", K331, S1, 1, 16, (7, 20, 5), {"odd-extents"}),
]
# all three extents odd: outside the kernel's domain (a thread owns four y-consecutive voxels), which is an error and never another kernel
NARROW_REFUSED = [_c("n331-16to1-allodd", K331, S1, 16, 1, (5, 7, 3), {"all-odd"}, dbias=True), _c("n331-1to16-allodd", K331, S1, 1, 16, (5, 7, 3), {"all-odd"})]


# ---------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------
def _generator(name: str) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(zlib.crc32(name.encode()))
    return g


def int_field(g: torch.Generator, shape) -> torch.Tensor:
    """fp64, uniform in {-2, -1, 1, 2}: never zero."""
    return torch.tensor(VALUES, dtype=torch.float64)[torch.randint(0, 4, tuple(shape), generator=g)]


def operands(case: Case) -> dict:
    """The operands of a case, a function of its shape only (rows that launch the same problem differently share them): x and dY as NCDHW fp64
    tensors of non-zero integers, P / H as the kernels name them, a {0, 1} gate map over the voxels of H, and integer starting values of dw and dbias."""
    g = _generator(f"{case.k}{case.s}{case.cin}{case.cout}{case.dims}{case.tr}{case.batch}")
    x = int_field(g, (case.batch, case.cin, *case.dims))
    gy = int_field(g, (case.batch, case.cout, *case.ydims))
    gate = torch.randint(0, 2, (case.batch, *case.hdims), generator=g).to(torch.float64)
    dw0 = torch.randint(-8, 9, case.wshape, generator=g).to(torch.float64)
    p, h = (x, gy) if case.tr else (gy, x)
    return {"x": x, "dy": gy, "p": p, "h": h, "gate": gate, "dw0": dw0, "db0": 5.0}


def is_bf16(t: torch.Tensor) -> bool:
    return bool(torch.equal(t.to(torch.bfloat16).to(t.dtype), t))


# ---------------------------------------------------------------------------------------------------------------
# definition
# ---------------------------------------------------------------------------------------------------------------
def zero_padded(h: torch.Tensor, pad) -> torch.Tensor:
    out = torch.zeros(h.shape[0], h.shape[1], *(d + 2 * p for d, p in zip(h.shape[2:], pad)), dtype=h.dtype)
    out[:, :, pad[0]:pad[0] + h.shape[2], pad[1]:pad[1] + h.shape[3], pad[2]:pad[2] + h.shape[4]] = h
    return out


def wgrad_from_padded(p: torch.Tensor, hp: torch.Tensor, kernel, stride, tap_shift=None) -> torch.Tensor:
    """dW[cP][cH][tap] = sum over samples and lattice voxels q of P[q][cP] * Hp[q * stride + tap][cH], Hp = H with its `same` padding in place.
    tap_shift {tap: tap read instead}: for planted faults only."""
    q = p.shape[2:]
    dw = torch.zeros(p.shape[1], hp.shape[1], *kernel, dtype=torch.float64)
    for kx in range(kernel[0]):
        for ky in range(kernel[1]):
            for kz in range(kernel[2]):
                ox, oy, oz = (tap_shift or {}).get((kx, ky, kz), (kx, ky, kz))
                hs = hp[:, :, ox:ox + (q[0] - 1) * stride[0] + 1:stride[0], oy:oy + (q[1] - 1) * stride[1] + 1:stride[1], oz:oz + (q[2] - 1) * stride[2] + 1:stride[2]]
                dw[:, :, kx, ky, kz] = torch.einsum("npxyz,nhxyz->ph", p, hs)
    return dw


def wgrad(p: torch.Tensor, h: torch.Tensor, kernel, stride, gate: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The weight gradient of Conv3d (P = dY, H = X: dW[co][ci]) and of ConvTranspose3d (P = X, H = dY: dW[ci][co]) with `same` padding, as a direct
    shift-and-sum; H is multiplied by (1 + gate) per voxel where a gate map is given."""
    p, h = p.double(), h.double()
    if gate is not None:
        h = h * (1.0 + gate.double()).unsqueeze(1)
    return wgrad_from_padded(p, zero_padded(h, P.same_pad(kernel)), kernel, stride)


def expected(case: Case, ops: dict, calls: int = 1, gate: bool = False, dw0: Optional[torch.Tensor] = None, db0: float = 0.0):
    """(dW, dbias) the kernels must produce bit for bit after `calls` accumulating launches on top of dw0 / db0; dbias = sum of P (= dY) over samples and
    voxels.  Asserts the range that makes fp32 accumulation exact in any order."""
    n, (q0, q1, q2) = case.batch, case.q
    start = 0.0 if dw0 is None else float(dw0.abs().max())
    assert calls * 8 * n * q0 * q1 * q2 + max(start, abs(db0)) < EXACT_LIMIT, "operand range: a partial sum could leave the exact integers of fp32"
    for name in ("p", "h"):
        t = ops[name]
        assert is_bf16(t) and bool((t != 0).all()) and bool((t == t.round()).all()) and float(t.abs().max()) <= 2, f"{name}: operands must be non-zero integers of magnitude <= 2"
    g = ops["gate"] if gate else None
    assert g is None or bool(((g == 0) | (g == 1)).all())
    dw = calls * wgrad(ops["p"], ops["h"], case.k, case.s, g)
    if dw0 is not None:
        assert bool((dw0 == dw0.round()).all())
        dw = dw + dw0.double()
    db = db0 + calls * ops["p"].double().sum((0, 2, 3, 4))
    assert float(dw.abs().max()) < EXACT_LIMIT and float(db.abs().max()) < EXACT_LIMIT
    return dw, db


# ---------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------
def mismatch_report(got: torch.Tensor, want: torch.Tensor, what: str = "", first: int = 8) -> str:
    """Count of differing elements of a weight gradient [cP][cH][taps...] and, for the first few, (tap, cP, cH, got, want)."""
    g, w = got.detach().cpu().double(), want.detach().cpu().double()
    g3, w3 = g.reshape(g.shape[0], g.shape[1], -1), w.reshape(w.shape[0], w.shape[1], -1)
    bad = (g3 != w3) | torch.isnan(g3)
    idx = bad.nonzero()
    taps = sorted(set(int(i[2]) for i in idx))
    rows = [f"(tap {int(t)}, cP {int(a)}, cH {int(b)}: got {float(g3[a, b, t])!r}, want {float(w3[a, b, t])!r})" for a, b, t in idx[:first]]
    return f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, in taps {taps[:27]}; " + ", ".join(rows)


def assert_exact(got: torch.Tensor, want: torch.Tensor, what: str = ""):
    """Bit-for-bit equality of an fp32 result with its fp64 definition (an integer below 2^24, hence an fp32 number)."""
    want32 = want.to(torch.float32)
    assert torch.equal(want32.double(), want.double()), "the expected value is not an fp32 number"
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == want32.shape, (got.dtype, tuple(got.shape), tuple(want32.shape))
    assert torch.equal(got, want32), mismatch_report(got.reshape(got.shape[0], -1, 1) if got.dim() < 3 else got, want32.reshape(got.shape[0], -1, 1) if got.dim() < 3 else want32, what)


# ---------------------------------------------------------------------------------------------------------------
# host mirrors of the launch arithmetic
# ---------------------------------------------------------------------------------------------------------------
TILE_SCRATCH = 8 * 1024 * 1024      # floats gpu_harness.run_wgrad hands the tile and marching kernels
COMPUTE_SCRATCH = 48 * 1024 * 1024  # ... the compute kernel


def slab_bucket(nblk: int) -> str:
    """The regime of vsseg_slab_sum4 (csrc/common.h) for `nblk` slabs: each of the 16 block-lanes adds at most one slab; the scalar remainder loop alone;
    the 8-deep unrolled loop once (block-lane 0: 112 < nblk <= 240); more than once."""
    return "slab<=16" if nblk <= 16 else "slab-scalar" if nblk <= 112 else "slab-unroll1" if nblk <= 240 else "slab-unroll2"


def tile_launch(case: Case, es: int) -> dict:
    """vsseg_wgrad (csrc/wgrad.hip) for march = 0, from planner.plan_wgrad: every quantity that selects a path of the launch.  The occupancy clamp of
    wg_launch (256 * per_cu / grid.y, per_cu in 1..4) depends on the device; `clamp_free` says that it cannot bite (gx * grid.y <= 256)."""
    wp = P.plan_wgrad(case.tr, case.wshape, case.k, case.s, case.q, es)
    ntaps, tile, ntp, q, hs = len(wp.taps), wp.tile, wp.ntp, case.q, case.s
    ntile = [-(-q[a] // tile[a]) for a in range(3)]
    tiles = case.batch * ntile[0] * ntile[1] * ntile[2]
    wt = 4 if ntaps >= 4 else (2 if ntaps >= 2 else 1)
    wv = 4 // wt
    maxt = -(-ntaps // wt)
    maxt_t = 1 if maxt <= 1 else (3 if maxt <= 3 else 7)
    tvox = tile[0] * tile[1] * tile[2]
    p_row = ntp * 16 * es
    halo = []
    for a in range(3):
        offs = [t[0][a] for t in wp.taps]
        halo.append((tile[a] - 1) * hs[a] + max(offs) - min(offs) + 1)
    hvox = halo[0] * halo[1] * halo[2]
    hchunks = -(-case.ch // 16)
    nbuf = 1 if case.single_buffer else 2

    def lds_need(g):
        return P.round_up(tvox * 4, 16) + nbuf * (tvox * p_row + hvox * g * 16 * es) + (-(-(tvox * (p_row >> 4)) // 256) + -(-(hvox * g * es) // 256)) * 1024

    hg = min(max(case.hgroup, 1), 4)
    while hg > 1 and (hchunks % hg or maxt_t * ntp * hg > 42 or hvox * hg * 16 * es > 16 * 256 * 16 or lds_need(hg) > 160 * 1024):
        hg -= 1
    npp = -(-(tvox * (p_row >> 4)) // 256)
    if ntp * 16 <= case.cp_stored and all(q[a] % tile[a] == 0 for a in range(3)):
        npp = 0
    slab_chunk = ntaps * ntp * 256
    per_blk = wv * (hchunks * slab_chunk + (ntp * 16 if case.dbias else 0))
    scratch = TILE_SCRATCH if case.scratch_wgs is None else case.scratch_wgs * per_blk
    req = (wp.blocks if case.blocks is None else case.blocks) or 256
    gx = min(req, tiles)
    cap = scratch // per_blk
    capped = gx > cap
    gx = min(gx, cap)
    grid_y = hchunks // hg
    grid_x = gx & ~7 if gx >= 8 else gx
    nblk = grid_x * wv
    paths = {slab_bucket(nblk), "npp=0" if npp == 0 else "npp>0", f"hg={hg}", f"wv={wv}", f"batch{case.batch}",
             "blocks<tiles" if req < tiles else "blocks=tiles" if req == tiles else "blocks>tiles", "walk-on" if grid_x % 8 == 0 else "walk-off"}
    paths |= {"round8"} if grid_x != gx else set()
    paths |= {"scratch-cap"} if capped else set()
    paths |= {"dbias"} if case.dbias else set()
    paths |= {"acc"} if case.acc else set()
    paths |= {"transposed"} if case.tr else set()
    paths |= {"strided"} if max(case.s) > 1 else set()
    paths |= {"p-padded"} if ntp * 16 > case.cp_stored or case.cp_stored > case.cp else set()
    paths |= {"h-padded"} if case.ch_stored > case.ch else set()
    paths |= {"h-ragged-chunk"} if hchunks * 16 > case.ch_stored else set()
    paths |= {"two-part"} if case.split else set()
    paths |= {"split-in-group"} if case.split and hg > 1 and case.split % (16 * hg) else set()
    return {"tile": tile, "ntile": ntile, "tiles": tiles, "wt": wt, "wv": wv, "maxt": maxt, "hg": hg, "npp": npp, "hchunks": hchunks, "slab_chunk": slab_chunk, "per_blk": per_blk,
            "scratch": scratch, "req": req, "gx": gx, "grid_x": grid_x, "grid_y": grid_y, "nblk": nblk, "lds": lds_need(hg), "clamp_free": gx * grid_y <= 256, "paths": paths}


def march_launch(case: Case) -> dict:
    """vsseg_mwgrad_launch (csrc/mwgrad.hip): the instantiation (H channels, P channels as stored, tz, M-tiles per wave) a tile selects, the x segments, the grid."""
    lx, tyb, tz = case.tile
    X, Y, Z = case.q
    assert case.k == K331 and case.s == S1 and not case.tr and tz in (2, 4, 8) and (tyb * tz) % 64 == 0 and Y % tyb == 0 and Z % tz == 0 and case.ch % 16 == 0
    mt = tyb * tz // 64
    lx = min(lx, X)
    nxs, nyb, nzb = -(-X // lx), Y // tyb, Z // tz
    grid = case.batch * nxs * nyb * nzb
    ntp = case.cp_stored // 16 if case.cp_stored >= 16 else 1
    per_blk = (case.ch // 16) * 9 * ntp * 256 + (ntp * 16 if case.dbias else 0)
    paths = {slab_bucket(grid), "x-segs>1" if nxs > 1 else "x-segs=1", f"batch{case.batch}"}
    paths |= {"x-ragged"} if X % lx else set()
    paths |= {"row-blocks>1"} if nyb > 1 else set()
    paths |= {"two-part"} if case.split else set()
    paths |= {"compact-p"} if case.compact_p else set()
    paths |= {"gate"} if case.gate else set()
    paths |= {"dbias"} if case.dbias else set()
    paths |= {"p-padded"} if case.cp_stored > case.cp else set()
    paths |= {"planner-tile"} if tuple(case.tile) in P.march_wgrad_tiles(case.ch, case.cp_stored, case.q, case.batch) else set()
    return {"shape": (case.ch, case.cp_stored, tz, mt), "lx": lx, "nxs": nxs, "last_seg": X - (nxs - 1) * lx, "grid": grid, "fits": grid * per_blk <= TILE_SCRATCH, "paths": paths}


def compute_launch(case: Case) -> dict:
    """vsseg_cwgrad_launch (csrc/cwgrad.hip): the wave-role split (P tiles per wave, P shares, H chunks per workgroup), the chunk classes, the workgroups per class."""
    X, Y, Z = case.q
    assert case.k == K333 and case.s == S1 and not case.tr and Y % 8 == 0 and Z % 32 == 0 and case.cp in (48, 64) and case.ch % 16 == 0
    ntp, cg = case.cp // 16, case.compute
    assert cg in (1, 2) and not (ntp == 4 and cg != 1) and (case.ch // 16) % cg == 0 and (case.ch // 16) // cg <= 8
    ps = 2 if ntp == 4 else 1
    ksh = 4 // (ps * cg)
    hchunks = case.ch // 16
    ncls = hchunks // cg
    pow2 = ncls & (ncls - 1) == 0
    gpc = 256 // ncls
    gpc = gpc & ~7 if pow2 else gpc
    per_wg = ksh * (hchunks * 27 * ntp * 256 + (ntp * 16 if case.dbias else 0))
    cap = COMPUTE_SCRATCH // per_wg
    if gpc > cap:
        gpc = cap & ~7 if pow2 else cap
    if case.blocks and gpc > case.blocks:
        gpc = case.blocks & ~7 if pow2 else case.blocks
    nblk = gpc * ksh
    paths = {f"ntp{ntp}-cg{cg}", "pow2-classes" if pow2 else "odd-classes", slab_bucket(nblk), f"batch{case.batch}"}
    paths |= {"two-part"} if case.split else set()
    paths |= {"dbias"} if case.dbias else set()
    return {"split": (ntp // ps, ps, cg), "inst": (ntp // ps, ps, cg, case.dbias), "ncls": ncls, "gpc": gpc, "ok": gpc >= (8 if pow2 else 1), "nblk": nblk, "paths": paths}
