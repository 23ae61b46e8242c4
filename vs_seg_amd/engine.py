"""Lowers the static network program (vs_seg_amd.graph) to HIP launches through the C ABI and runs them.

One `Plan` per (batch, spatial size, train/eval) signature holds every activation/gradient buffer, every prepared
ctypes descriptor and two launch lists (forward, backward).  Running a step is a flat loop over prepared launches on
torch's current HIP stream — no allocation, no host synchronisation, capturable in a hipGraph.

torch tensors are used only as device-memory containers.  There is no CPU/eager fallback: a missing extension raises.
"""
from __future__ import annotations

import collections
import ctypes as C
import dataclasses
import functools
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import planner as P
from .graph import HP, AttGate, ConvBnAct, ConvPlain, Layer, Program, TensorSpec, build_program, level_dims

BN_EPS = 1e-5  # torch.nn.BatchNorm3d defaults (ref:params/networks/blocks/convolutions.py:152 passes no arguments)
BN_MOMENTUM = 0.1
ACT_CODE = {"none": L.ACT_NONE, "relu": L.ACT_RELU, "sigmoid": L.ACT_SIGMOID}


def _tdtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return L.F32
    if t.dtype == torch.bfloat16:
        return L.BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


TUNED_DEFAULTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned_gfx950.json")


def _tune_cache() -> dict:
    """launch signature -> [tile, nt, nsplit, ck] of the plan measured fastest.  Seeded from the in-tree file of plans tuned on an
    MI355X for the benchmark shapes and from $VSSEG_TUNE_CACHE; new measurements are written back to $VSSEG_TUNE_CACHE if set."""
    if getattr(_tune_cache, "data", None) is None:
        import json

        _tune_cache.data, _tune_cache.dirty = {}, False
        for f in (TUNED_DEFAULTS, os.environ.get("VSSEG_TUNE_CACHE")):
            if f and os.path.exists(f):
                try:
                    _tune_cache.data.update(json.load(open(f)))
                except (OSError, ValueError):
                    pass
    return _tune_cache.data


def _tune_cache_save():
    f = os.environ.get("VSSEG_TUNE_CACHE")
    if f and getattr(_tune_cache, "dirty", False):
        import json

        tmp = f"{f}.{os.getpid()}.tmp"
        json.dump(_tune_cache.data, open(tmp, "w"), indent=0, sort_keys=True)
        os.replace(tmp, f)
        _tune_cache.dirty = False


def _cache_usable(key: str, cands=()) -> bool:
    """May the cached entry for this key be used?  Not under VSSEG_AUTOTUNE=force, and not when one of `cands` has a depth named in VSSEG_RETUNE_DEPTHS
    (e.g. "-6": such launches are measured again although a choice is cached — how the plans of a NEW kernel variant get into the cache without
    re-measuring every launch: tools/tune_shapes.py)."""
    if key not in _tune_cache() or os.environ.get("VSSEG_AUTOTUNE", "1") == "force":
        return False
    retune = {int(v) for v in os.environ.get("VSSEG_RETUNE_DEPTHS", "").split(",") if v.strip()}
    return not any(pl.depth in retune for pl in cands)


class ParamLayout:
    """Offsets of every state_dict entry inside the flat buffers owned by the model (params fp32, buffers fp32, counters int64)."""

    def __init__(self, manifest):
        self.param_off: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.buf_off: Dict[str, Tuple[int, Tuple[int, ...]]] = {}
        self.cnt_off: Dict[str, int] = {}
        self.order = [k for k, _ in manifest]
        po = bo = co = 0
        for key, shape in manifest:
            n = int(np.prod(shape)) if len(shape) else 1
            if key.endswith("num_batches_tracked"):
                self.cnt_off[key] = co
                co += 1
            elif "running_" in key:
                self.buf_off[key] = (bo, tuple(shape))
                bo += n
            else:
                self.param_off[key] = (po, tuple(shape))
                po += (n + 3) // 4 * 4  # keep every tensor 16-byte aligned inside the flat buffer
        self.n_param, self.n_buf, self.n_cnt = po, bo, co


@dataclass
class _Choice:
    """One implicit-GEMM launch of a layer (one lattice class): the candidate plans and, once lowered, the chosen one."""

    cands: List[P.IgemmPlan]  # default (heuristic) plan first
    woff: int  # offset of the layer's weight inside the flat parameter buffer
    wshape2: Optional[tuple] = None  # merged 1x1x1 residual convolution: its weight shape ...
    woff2: int = 0  # ... and flat offset
    chosen: Optional[P.IgemmPlan] = None
    map_off: int = -1  # element offset of the chosen plan's packed weights inside Plan.wpack
    tuned_ms: Optional[list] = None  # autotuner measurements, one per candidate
    wshape: tuple = ()
    cached: bool = False  # the choice came from the tuned-plan cache, nothing was measured
    fold: int = 0  # z-folded formulation (planner.FOLD z-neighbours as channels): the launch runs on reinterpreted tensors
    cmod: int = 0  # ... and output channel c is real channel c % cmod for the per-channel vectors
    alt: Optional["_Choice"] = None  # on the first lattice class of a multi-class op: all classes as ONE launch (planner.class_split_plans)
    probe_plan: Optional[P.IgemmPlan] = None  # plan of the last probe lowering (Plan._igemm(probe=True))
    woff_res: int = 0  # plans with residual tiles (planner.march_res_plans): flat offset of the 1x1x1 residual convolution's weight ...
    map_off_res: int = -1  # ... and the element offset of its packed weights inside Plan.wpack
    compact: object = None  # Plan._compact_choice's answer once asked: the marching plans reading a compact one-channel input as their own choice, False: there are none
    is_compact: bool = False  # this IS such a choice


@dataclass
class _ConvPlans:
    fwd: List[_Choice]
    dgrad: List[_Choice]
    wgrad: Optional[P.WgradPlan]
    fold_fwd: bool = False


# The device addresses every launch that touches one BatchNorm layer takes (one record per layer and plan, Plan.bn): parameters, running statistics and counter; the layer's
# columns of the six rows of Plan.vec and of the two rows of Plan.stats; the PReLU-slope gradient accumulator; the layer's dropout salt (| SEED_INDIRECT: the kernels read
# the seed through Plan.seed_dev); channels rounded up to 16 (the stride of the statistics); the dropout keep-mask bytes (training with dropout) or None.
_BnLayer = collections.namedtuple("_BnLayer", "gamma beta alpha rmean rvar counter mean invstd scale shift mean_dz mean_dzx stats_fwd stats_bwd slope salt cpad keep")


class _Slot:
    """A launch argument that is filled in at run time (dropout seed, external gradient pointers)."""

    def __init__(self, kind, name=None):
        self.kind, self.name = kind, name


class Launch:
    """One entry of a plan's launch lists: the runner calls `fn(*args, stream)`.  `args` is the list it reads (Plan._index_slots substitutes `_Slot` entries in
    place); `desc` is the ctypes descriptor where args[0] is byref(desc) — the record keeps it alive — else None; `meta` is what the profiles report (name, kind,
    tag, flops, bytes), None where a launch reports nothing.  The rest decides the schedule: `side` = goes to the side stream under Engine.overlap (the weight
    gradients); `own_dy` / `late_ok` = Plan._move_late_wgrads may move it to the end of the main stream's list, `late` = it did; `scratch_at` = position in `args`
    of a partial-sum scratch pointer followed by its element count, where those are arguments and not descriptor fields."""

    __slots__ = ("fn", "args", "desc", "meta", "side", "own_dy", "late_ok", "late", "scratch_at")

    def __init__(self, fn, args: list, meta: Optional[dict] = None, *, desc=None, side=False, own_dy=False, late_ok=False, scratch_at: Optional[int] = None):
        self.fn, self.args, self.desc, self.meta = fn, args, desc, meta
        self.side, self.own_dy, self.late_ok, self.late, self.scratch_at = side, own_dy, late_ok, False, scratch_at

    @property
    def name(self) -> str:
        """What timer events, the timer's `only` filter and error messages call this launch."""
        if self.meta is not None and "name" in self.meta:
            return self.meta["name"]
        return getattr(self.fn, "__name__", "memset")


def fill_igemm_desc(d: L.IgemmDesc, pl: P.IgemmPlan):
    """Everything of a launch descriptor that its plan decides (the tensors, the packed weights and the epilogue are the caller's)."""
    d.q, d.is_, d.os, d.oo = L.i3(pl.q), L.i3(pl.cls.is_), L.i3(pl.cls.os), L.i3(pl.cls.oo)
    d.ntaps = pl.ntaps
    for t, (off, _) in enumerate(pl.cls.taps):
        d.tap_off[t][0], d.tap_off[t][1], d.tap_off[t][2] = off
    d.tile = L.i3(pl.tile)
    d.mtw, d.nt, d.nsplit, d.ck, d.nchunks, d.ksteps, d.depth = pl.mtw, pl.nt, pl.nsplit, pl.ck, pl.nchunks, pl.ksteps, pl.depth
    d.res_tiles = pl.res_tiles
    if P.is_shuffle(pl):  # fused output-parity classes: output channel tile t is class t, its channels are the real channels 0..nc-1
        d.cout_mod = pl.nc
    d.class_split = len(pl.classes) if pl.classes is not None else 0
    for s_, c_ in enumerate(pl.classes or ()):  # workgroup row s_ = lattice class s_: its output offset and its taps (indices into the union tap table above)
        d.class_oo[s_][0], d.class_oo[s_][1], d.class_oo[s_][2] = c_.oo
        d.class_ntaps[s_] = len(c_.taps)
        for i, t in enumerate(pl.class_taps(s_)):
            d.class_tap[s_][i] = t


def fill_wgrad_desc(d: L.WgradDesc, wg: P.WgradPlan):
    """The geometry of a weight-gradient launch: lattice, taps, tile and the strides of the weight tensor."""
    d.q, d.hs, d.ntaps = L.i3(wg.q), L.i3(wg.hs), len(wg.taps)
    for t, (off, widx) in enumerate(wg.taps):
        d.tap_off[t][0], d.tap_off[t][1], d.tap_off[t][2] = off
        d.tap_widx[t] = widx
    d.tile, d.ntp = L.i3(wg.tile), wg.ntp
    d.stride_p, d.stride_h, d.stride_tap = wg.stride_p, wg.stride_h, wg.stride_tap


class Plan:
    def __init__(self, eng: "Engine", n: int, dims: Tuple[int, int, int], train: bool):
        self.eng, self.n, self.dims, self.train = eng, n, tuple(dims), train
        self.lv = level_dims(dims, eng.hp)
        self.compact_input: Optional[torch.Tensor] = None  # [N,X,Y,Z,1] copy of the network input for the z-folded first-layer launches
        self.needs_padded_input = False  # set by the first launch descriptor that reads the 8-channel zero-extended copy of the network input (_desc): staged per step only then
        self.fwd: List[Launch] = []
        self.fwd_pre: List[Launch] = []  # eval only: launches that depend on parameters / buffers alone (BatchNorm folding); re-run with the weight packing when those change
        self.params_key = None  # parameter version the packed weights + folded BatchNorm constants of an eval plan belong to
        self.bwd: List[Launch] = []
        self.bufs: Dict[str, torch.Tensor] = {}
        self.grads: Dict[str, torch.Tensor] = {}
        self.flat_ptr = eng.flat.data_ptr()
        self.timer = None  # or {'only': None (every launch) | set of Launch.name, 'events': [], optional 'active': bool}: Plan.run appends (name, meta, e0, e1) HIP-event pairs to 'events'
        self.generation = 0  # bumped by every training forward: a backward belongs to exactly one forward of this plan
        # The launch lists have FIXED kernel arguments (the dropout seed is read from `seed_dev`, external gradients are staged into
        # plan-owned buffers), so after two eager warm-up runs each list is captured in a hipGraph and replayed: one host call per list
        # instead of ~100-230 ctypes launches (VSSEG_GRAPHS=0 keeps the eager loop; the event-timed profiling mode always runs eagerly).
        self.seed_dev = torch.zeros(1, dtype=torch.int64, device=eng.device)
        self.gatt_buf: Dict[str, torch.Tensor] = {}
        self._gatt_set: Dict[str, bool] = {}
        self._fork_events: list = []  # events of the side-stream forks (created once, re-recorded every step)
        self.bwd_pre: List[Launch] = []  # backward launches that read caller-owned memory (the loss' gradient of the logits): never captured
        self._graphs: Dict[str, object] = {}
        self._graph_runs: Dict[str, int] = {}
        self._tune_gflat: Optional[torch.Tensor] = None  # scratch copy of the gradient buffer the measured weight-gradient launches accumulate into
        self.class_split_ms: list = []  # (key, [per-class ms, one-launch ms]) of every class-split decision this plan measured
        # Autotune (default on a GPU): every launch measures its candidate plans on the real buffers at lowering time and keeps
        # the fastest.  VSSEG_AUTOTUNE=0 keeps the heuristic plan (deterministic; what the CPU dry-run lowering always uses).
        self.tune = (not eng.dry_run) and os.environ.get("VSSEG_AUTOTUNE", "1") != "0"
        self._maps: List[np.ndarray] = []
        self._maps2: List[np.ndarray] = []
        self._map_len = 0
        self._wpack_fixups: list = []  # (descriptor, packed-weight pointer field, element offset): wpack is allocated after every launch chose its plan
        # the lowering passes, in this order: the fusion decisions consult the ones before them
        for lowering_pass in (self._decide_merged, self._plan_convs, self._decide_resn, self._bn_records, self._decide_res1_fused, self._decide_eval_in1, self._decide_gate_onload,
                              self._decide_chains, self._lower_forward, self._lower_backward, self._finish_pack):
            lowering_pass()
        self._index_slots()

    # ------------------------------------------------------------------ helpers
    def _alloc(self, spec: TensorSpec, store: Dict[str, torch.Tensor]) -> torch.Tensor:
        root = spec.root
        if root.name not in store:
            dt = torch.float32 if root.kind == "f32" else self.eng.tdtype
            store[root.name] = torch.zeros((self.n, *self.lv[root.level], root.c), dtype=dt, device=self.eng.device)
        return store[root.name]

    def _desc(self, spec: TensorSpec, store=None) -> L.Tensor:
        if spec.parts is not None:  # skip-connection concat: the pair of its dense operands
            return L.Tensor.two_part(self._desc(spec.parts[0], store), self._desc(spec.parts[1], store))
        buf = self._alloc(spec, self.bufs if store is None else store)
        if store is None and spec.root.name == self.eng.prog.input.name:
            self.needs_padded_input = True  # (every reader of the padded copy gets its descriptor here; the compact copy goes through _xdesc)
        x, y, z = self.lv[spec.level]
        return L.Tensor(buf.data_ptr() + spec.c0 * buf.element_size(), _tdtype(buf), spec.c, spec.root.c, self.n, x, y, z)

    def _xdesc(self, spec: TensorSpec, folded: bool) -> L.Tensor:
        """Input descriptor of a convolution; the z-folded launches of the 1-channel network input read its compact copy."""
        if folded and spec.root.name == self.eng.prog.input.name:
            self.compact_input = self._raw("input:c1", 0, 1)
            return self._tdesc(self.compact_input, 0)
        return self._desc(spec)

    def _raw(self, name: str, level: int, c: int, dtype=None) -> torch.Tensor:
        if name not in self.bufs:
            self.bufs[name] = torch.zeros((self.n, *self.lv[level], c), dtype=dtype or self.eng.tdtype, device=self.eng.device)
        return self.bufs[name]

    def _tdesc(self, buf: torch.Tensor, level: int, c: Optional[int] = None) -> L.Tensor:
        x, y, z = self.lv[level]
        return L.Tensor(buf.data_ptr(), _tdtype(buf), c or buf.shape[-1], buf.shape[-1], self.n, x, y, z)

    def _dpre_desc(self, buf: torch.Tensor, level: int) -> L.Tensor:
        """d(pre-sigmoid) as vsseg_att_apply_bwd writes it: the 8-channel group in front of a row of 8 or 16 channels."""
        t = self._tdesc(buf, level)
        return L.Tensor(t.ptr, t.dtype, 8, t.pitch, t.n, t.x, t.y, t.z)

    def _pp(self, key: str) -> int:  # device address of a parameter inside the flat fp32 buffer
        return self.flat_ptr + 4 * self.eng.layout.param_off[key][0]

    def _gp(self, key: str) -> int:  # ... of its gradient
        return self.eng.gflat.data_ptr() + 4 * self.eng.layout.param_off[key][0]

    def _bp(self, key: str) -> int:
        return self.eng.bflat.data_ptr() + 4 * self.eng.layout.buf_off[key][0]

    def _cp(self, key: str) -> int:
        return self.eng.cflat.data_ptr() + 8 * self.eng.layout.cnt_off[key]

    def _vox(self, level: int) -> int:
        x, y, z = self.lv[level]
        return self.n * x * y * z

    # ------------------------------------------------------------------ conv planning + weight pack buffer
    def _decide_merged(self):
        """A 1x1x1 residual conv added to a plain (no BatchNorm) conv of the same input merges into that conv's centre tap."""
        prog = self.eng.prog
        self.merged: Dict[str, ConvPlain] = {}  # residual-conv prefix -> the convolution that absorbed it
        self.absorbs: Dict[str, ConvPlain] = {}  # absorbing conv prefix -> the residual conv op
        for op in prog.ops:
            a = prog.producer(op.res) if (isinstance(op, ConvPlain) and op.res is not None and op.act == "none") else None
            if a is not None and a.x is op.x and a.act == "none" and a.layer.kernel == (1, 1, 1) and all(k % 2 == 1 for k in op.layer.kernel):
                self.merged[a.layer.prefix] = op
                self.absorbs[op.layer.prefix] = a

    def _choices(self, kind, Lr, q, kc_pad, aux_es, in_split, absorbed, fold=False) -> List[_Choice]:
        """The launches of one convolution / data gradient (one per lattice class, or fewer where classes fuse) with their candidate plans."""
        eng = self.eng
        out = []
        woff = eng.layout.param_off[Lr.wkey][0]
        if eng.fuse_classes and not fold and absorbed is None and not in_split:
            # the four output-parity classes of a stride-(2,2,1) transposed convolution / data gradient as ONE streaming-kernel launch
            # (planner.shuffle_plan): the per-class launches each read the whole input
            kreal, nreal = P.gemm_dims(kind, Lr.wshape)
            sps = P.shuffle_plans(kind, Lr.wshape, Lr.kernel, Lr.stride, q, eng.es, kc_pad, nreal, kreal)
            if sps is not None:  # (+ the marching variants where they exist: measured against the streaming launch by the tuner; the untuned lowering keeps the streaming one)
                got = [_Choice([sp] + (P.march_shuffle_plans(sp, self.n) if self.tune else []), woff, wshape=tuple(Lr.wshape)) for sp in sps]
                allc = P.march_shuffle_all_plans(kind, Lr.wshape, Lr.kernel, Lr.stride, q, eng.es, kc_pad, nreal, kreal, self.n) if (self.tune and len(sps) == 2) else []
                if allc:  # 32 output channels: ONE marching launch for all four classes against the two streaming launches (decided by measurement, _use_class_split)
                    got[0].alt = _Choice(allc, woff, wshape=tuple(Lr.wshape))
                return got
        alt = None
        if not fold and absorbed is None:
            # ... and those of the 3x3x3 stride-(2,2,2) transitions of the deep levels as ONE launch of the general kernel (workgroup row = class)
            kreal, nreal = P.gemm_dims(kind, Lr.wshape)
            csp = P.class_split_plans(kind, Lr.wshape, Lr.kernel, Lr.stride, q, eng.es, kc_pad, nreal, kreal, aux_es=aux_es, in_split=in_split) if kind in ("convT_fwd", "conv_dgrad") else None
            # ... or of the deep-level kernel (csrc/dconv.hip: a workgroup loads the halo of its coarse tile once and runs the classes one after the other)
            dcp = P.deep_class_plans(kind, Lr.wshape, Lr.kernel, Lr.stride, q, eng.es, kc_pad, nreal, kreal, self.n, in_split) if (eng.deep != "0" and kind in ("convT_fwd", "conv_dgrad")) else []
            # ... or of the transition kernel (csrc/tconv.hip: levels 2 <-> 3, the waves split the voxels, a stage per class)
            tcp = P.transition_plans(kind, Lr.wshape, Lr.kernel, Lr.stride, q, eng.es, kc_pad, nreal, kreal, in_split) if (eng.transition and self.tune and kc_pad is not None and kind in ("convT_fwd", "conv_dgrad")) else []
            if eng.deep == "force" and dcp:
                alt = _Choice(dcp if self.tune else dcp[:1], woff, wshape=tuple(Lr.wshape))
            elif csp or ((dcp or tcp) and self.tune):  # an alternative to the per-class launches below, decided per op at lowering time (Plan._use_class_split)
                alt = _Choice(((csp or []) + dcp + tcp) if self.tune else csp[:1], woff, wshape=tuple(Lr.wshape))
        for cls in P.lattice_classes(kind, Lr.kernel, Lr.stride):
            if fold:  # one real input or output channel, no taps along z: 8 z-neighbours become the channel group (planner.FOLD)
                cands = P.folded_candidate_plans(kind, Lr.wshape, cls, q, eng.es, aux_es=aux_es, heuristic_only=not self.tune)
                out.append(_Choice(cands, woff, wshape=tuple(Lr.wshape), fold=P.FOLD, cmod=P.gemm_dims(kind, Lr.wshape)[1]))
                continue
            if self.tune:
                cands = P.candidate_plans(kind, Lr.wshape, cls, q, eng.es, kc_pad=kc_pad, aux_es=aux_es, in_split=in_split, n=self.n)
                if eng.deep == "0":
                    cands = [pl for pl in cands if P.kernel_of(pl) != "dconv"]
                elif eng.deep == "force" and any(P.kernel_of(pl) == "dconv" for pl in cands):
                    cands = [pl for pl in cands if P.kernel_of(pl) == "dconv"]
            else:
                cands = [P.plan_igemm(kind, Lr.wshape, cls, q, eng.es, kc_pad=kc_pad, aux_es=aux_es, in_split=in_split)]
                if eng.deep == "force":  # untuned lowering with the deep-level kernel wherever it is offered (tests: the whole network through csrc/dconv.hip's domain)
                    kr_, nr_ = P.gemm_dims(kind, Lr.wshape)
                    dp = P.deep_plans(kind, Lr.wshape, cls, q, eng.es, kc_pad if kc_pad is not None else P.round_up(kr_, 8), nr_, kr_, self.n, in_split)
                    if dp:
                        cands = dp[:1]
            out.append(_Choice(cands, woff, absorbed.layer.wshape if absorbed is not None else None, eng.layout.param_off[absorbed.layer.wkey][0] if absorbed is not None else 0, wshape=tuple(Lr.wshape)))
        out[0].alt = alt
        return out

    def _plan_convs(self):
        eng = self.eng
        self.cplans: Dict[str, _ConvPlans] = {}
        self.wide_dpre: set = set()  # sigmoid convolutions whose d(pre-sigmoid) buffer is 16 channels wide (channel 0 real)
        for op in eng.prog.ops:
            if not isinstance(op, (ConvBnAct, ConvPlain)):
                continue
            Lr = op.layer
            if Lr.prefix in self.merged:
                self.cplans[Lr.prefix] = _ConvPlans([], [], None)
                continue
            absorbed = self.absorbs.get(Lr.prefix)
            dims_in = self.lv[Lr.level]
            kind = "convT_fwd" if Lr.transposed else "conv_fwd"
            dims_out = P.out_dims(kind, dims_in, Lr.kernel, Lr.stride)
            assert dims_out == self.lv[Lr.out_level]
            aux_es = 0 if (op.res is None or absorbed is not None) else (4 if op.res.kind == 'f32' else eng.es)
            can_fold = (absorbed is None and op.res is None and op.x.parts is None and op.x.base is None and op.out.base is None
                        and P.foldable(Lr.kernel, Lr.stride, Lr.transposed, Lr.cin, Lr.cout, dims_in))
            # Measured (tools: bench.py --profile, VSSEG_ZFOLD=all): folding pays on the narrow-OUTPUT side only — the attention sigmoid
            # convolution 16->1 drops from 0.51 to 0.33 ms (its input is read as 128 real channels, the 1-channel map is written as
            # 32-byte rows).  On the narrow-INPUT side (network input 1->16, dY of the sigmoid conv) the folded output rows are 256 B
            # wide and every 16-channel N-tile stores 32-byte fragments of them: 0.46 -> 0.50 ms and 0.51 -> 0.70 ms, so those stay unfolded.
            fold_fwd = can_fold and Lr.cout == 1
            fwd = self._choices(kind, Lr, dims_in if Lr.transposed else dims_out, op.x.c, aux_es, op.x.parts[0].c if op.x.parts else 0, absorbed, fold=fold_fwd)
            dgrad, wg = [], None
            if self.train:
                if op.x.root.name != eng.prog.input.name:  # the network input needs no gradient
                    dk = "convT_dgrad" if Lr.transposed else "conv_dgrad"
                    q = dims_in if Lr.transposed else tuple((d + s - 1) // s for d, s in zip(dims_in, Lr.stride))
                    # the data gradient of a 3x3x3 C -> 1 convolution (the sigmoid convolutions of levels 2-3) reads d(pre-sigmoid) as ONE 16-channel chunk so that the compute
                    # kernel (csrc/cconv.hip) is among its candidates: 0.16 -> 0.06 ms at level 2 (the general kernel on an 8-channel zero-extension was the only plan)
                    wide = (eng.wide_dpre and self.tune and eng.es == 2 and Lr.cout == 1 and not Lr.transposed and Lr.kernel == (3, 3, 3) and tuple(Lr.stride) == (1, 1, 1)
                            and not any(v % t for v, t in zip(q, P.COMPUTE_TILE)) and P.compute_split(Lr.cin) is not None)
                    if wide:
                        self.wide_dpre.add(Lr.prefix)
                    dgrad = self._choices(dk, Lr, q, 16 if wide else P.round_up(Lr.cout, 8), eng.es, 0, absorbed)
                wg = P.plan_wgrad(Lr.transposed, Lr.wshape, Lr.kernel, Lr.stride, dims_in if Lr.transposed else dims_out, eng.es)
            self.cplans[Lr.prefix] = _ConvPlans(fwd, dgrad, wg, fold_fwd)

    def _decide_resn(self):
        """ResidualUnit: the 1x1x1 residual convolution of the SAME input rides along in the unit's first 3x3x1 convolution (vsseg_igemm_desc.res_tiles, csrc/mconv.hip
        NR: the input is read once for both, ref:params/networks/blocks/convolutions.py:241-255) where a marching plan with residual tiles is instantiated."""
        eng = self.eng
        self.resn: Dict[str, ConvPlain] = {}     # unit convolution prefix -> the residual convolution op riding along
        self.resn_of: Dict[str, str] = {}        # residual convolution prefix -> unit convolution prefix
        if eng.resn and eng.es == 2:
            for op in eng.prog.ops:
                if not isinstance(op, ConvBnAct) or not op.layer.stride1_3x3x1 or op.x.parts is not None or op.x.base is not None:
                    continue
                Lr = op.layer
                rc = eng.prog.residual_conv(op)
                if rc is not None and (rc.layer.prefix in self.merged or rc.out.kind != "act"):  # (merged: the plan's question, not the graph's; the residual tiles are stored in the compute dtype)
                    rc = None
                if rc is None or len(self.cplans[Lr.prefix].fwd) != 1 or self.cplans[Lr.prefix].fold_fwd:
                    continue
                cls = P.lattice_classes("conv_fwd", Lr.kernel, Lr.stride)[0]
                plans = P.march_res_plans(Lr.wshape, rc.layer.wshape, cls, self.lv[Lr.level], eng.es, op.x.c, self.n)
                if not plans:
                    continue
                self.cplans[Lr.prefix].fwd = [_Choice(plans if self.tune else plans[:1], eng.layout.param_off[Lr.wkey][0], wshape=tuple(Lr.wshape), woff_res=eng.layout.param_off[rc.layer.wkey][0])]
                self.resn[Lr.prefix], self.resn_of[rc.layer.prefix] = rc, Lr.prefix

    @staticmethod
    def _flat_map(m: np.ndarray, woff: int) -> np.ndarray:
        """A plan's weight gather map (indices into the layer's weight, -1 = zero) as indices into the flat parameter buffer."""
        return np.where(m >= 0, m + woff, -1).astype(np.int32)

    def _gather_tmp(self, m: np.ndarray, woff: int) -> torch.Tensor:
        """The weights such a map packs, gathered into a temporary buffer (what a measured candidate launch reads)."""
        eng = self.eng
        md = torch.from_numpy(self._flat_map(m, woff)).to(eng.device)
        wp = torch.empty(md.numel(), dtype=eng.tdtype, device=eng.device)
        L.check(eng.lib.vsseg_gather_cast(eng.flat.data_ptr(), md.data_ptr(), None, wp.data_ptr(), md.numel(), L.BF16 if eng.es == 2 else L.F32, torch.cuda.current_stream().cuda_stream), "gather_cast")
        return wp

    @staticmethod
    def _event_ms(launch) -> float:
        """HIP-event time of one call of `launch` on the current stream."""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def _time_launch(self, launch) -> float:
        """ms of one launch (a zero-argument callable that returns the library's status): one checked launch as warm-up, then the best of Engine.tune_reps
        event-timed ones (5: with 3 the choice between near-equal plans flipped from run to run by up to 0.5 ms per step).  inf: the library rejected it."""
        if launch():
            return float("inf")
        return min((self._event_ms(launch) for _ in range(self.eng.tune_reps)), default=float("inf"))

    def _tune_gflat_delta(self) -> int:
        """Byte distance from the live gradient buffer to the scratch copy of it that measured weight-gradient launches accumulate into."""
        if self._tune_gflat is None:
            self._tune_gflat = torch.zeros_like(self.eng.gflat)
        return self._tune_gflat.data_ptr() - self.eng.gflat.data_ptr()

    def _register(self, ch: _Choice, pl: P.IgemmPlan):
        """Append the chosen plan's weight gather map(s) to the step's pack list."""
        ch.chosen, ch.map_off = pl, self._map_len
        self._maps.append(self._flat_map(pl.pack_map, ch.woff))
        if ch.wshape2 is not None:
            self._maps2.append(self._flat_map(P.pack_map_centre(pl, ch.wshape2), ch.woff2))
        else:
            self._maps2.append(np.full(pl.pack_map.size, -1, np.int32))
        self._map_len += pl.pack_map.size
        if pl.res_tiles:  # the residual convolution's tiles: their own gather map behind the main one
            ch.map_off_res = self._map_len
            self._maps.append(self._flat_map(pl.pack_map_res, ch.woff_res))
            self._maps2.append(np.full(pl.pack_map_res.size, -1, np.int32))
            self._map_len += pl.pack_map_res.size

    def _finish_pack(self):
        eng = self.eng
        self.pack_map = torch.from_numpy(np.concatenate(self._maps)).to(eng.device)
        self.pack_map2 = torch.from_numpy(np.concatenate(self._maps2)).to(eng.device) if self.absorbs else None
        assert self.pack_map2 is None or self.pack_map2.numel() == self.pack_map.numel()
        self.wpack = torch.zeros(self._map_len, dtype=eng.tdtype, device=eng.device)
        for d, attr, off in self._wpack_fixups:
            setattr(d, attr, self.wpack.data_ptr() + eng.es * off)
        del self._maps, self._maps2, self._wpack_fixups
        if self.train:  # the state the backward emitters shared
            del self._written, self._staged, self._grad_alias, self._absorbed_res, self._early_res, self._gate_fuse, self._folded_bias
        self._tune_gflat = None
        _tune_cache_save()

    def _choose(self, ch: _Choice, d: L.IgemmDesc) -> P.IgemmPlan:
        """Tuned-plan cache lookup (same launch signature measured before, in this process or in a cache file), else measure."""
        p0 = ch.cands[0]
        key = (f"{p0.kind}|f{ch.fold}|w{ch.wshape}|is{p0.cls.is_}os{p0.cls.os}oo{p0.cls.oo}|q{p0.q}|n{self.n}|es{self.eng.es}|kc{p0.kc}|acc{int(d.accumulate)}|res{int(d.res_mode)}"
               f"|st{int(bool(d.stats))}|two{int(bool(d.inp.ptr2))}{int(bool(d.out.ptr2))}" + ("|gin" if bool(d.in_gate) else "") + ("|cs" if p0.classes is not None else "")
               + (f"|rn{p0.res_tiles}{int(bool(d.res_out.ptr))}" if p0.res_tiles else "") + ("|c1" if (d.inp.c == 1 and p0.kc == 8) else ("|c2" if (d.inp.c == 2 and d.inp.pitch == 2 and p0.kc == 8) else ""))
)
        cache = _tune_cache()
        if _cache_usable(key, ch.cands):
            hit = cache[key]
            for pl in ch.cands:
                if [list(pl.tile), pl.nt, pl.nsplit, pl.ck, pl.depth] == (hit if len(hit) > 4 else hit + [1]):
                    ch.cached = True
                    return pl
        pl = self._autotune(ch, d)
        # the choice always enters the IN-PROCESS cache: later plans of this process replay it, and under data parallel rank 0 broadcasts this cache so that every rank runs
        # the same kernels.  VSSEG_DEEP=0 / force are experiment modes: their restricted candidate lists are never written to the cache FILE
        cache[key] = [list(pl.tile), pl.nt, pl.nsplit, pl.ck, pl.depth]
        if self.eng.deep == "1":
            _tune_cache.dirty = True
        return pl

    def _autotune(self, ch: _Choice, d: L.IgemmDesc) -> P.IgemmPlan:
        """Measure every candidate of one launch with its real operands and epilogue (Plan._time_launch)."""
        launch = functools.partial(self.eng.lib.vsseg_igemm, C.byref(d), torch.cuda.current_stream().cuda_stream)
        times = []
        for pl in ch.cands:
            wp = self._gather_tmp(pl.pack_map, ch.woff)
            fill_igemm_desc(d, pl)
            d.wpack = wp.data_ptr()
            if pl.res_tiles:
                wpr = self._gather_tmp(pl.pack_map_res, ch.woff_res)
                d.wpack_res = wpr.data_ptr()
            times.append(self._time_launch(launch))  # a candidate the kernel rejects (inf) is simply not chosen
        ch.tuned_ms = times
        i = int(np.argmin(times))
        if times[i] > 0.97 * times[0]:  # keep the default unless a candidate is clearly faster (timer noise on the tiny layers)
            i = 0
        return ch.cands[i]

    @staticmethod
    def _fold_desc(t: L.Tensor, fold: int) -> L.Tensor:
        """[N,X,Y,Z,C] dense -> the bit-identical [N,X,Y,Z/fold,fold*C] view."""
        assert t.c == t.pitch and not t.ptr2 and t.z % fold == 0, "z-folding needs a dense, single-part tensor"
        return L.Tensor(t.ptr, t.dtype, t.c * fold, t.pitch * fold, t.n, t.x, t.y, t.z // fold)

    def _igemm_classes(self, lst, chs: List[_Choice], inp: L.Tensor, out: L.Tensor, *, res: Optional[L.Tensor] = None, **kw):
        """All lattice classes of one convolution (the output-parity classes of a transposed convolution / of a strided data gradient): each is
        its own launch and reads the WHOLE input (the stride-(2,2,1) transitions of levels 0-2 run all classes in one streaming-kernel launch
        instead, planner.shuffle_plans)."""
        if chs[0].alt is not None and self._use_class_split(chs, inp, out, res, kw):
            chs = [chs[0].alt]  # ... or every class in one launch of the general kernel, where that is faster (the deep levels)
        for ch in chs:
            self._igemm(lst, ch, inp, out, res=res, **kw)

    CLASS_SPLIT_MAX_VOXELS = 100_000  # heuristic of the untuned lowering: class-split launches below this many coarse voxels (measured: tools/bench_class_split.py)

    def _use_class_split(self, chs: List[_Choice], inp: L.Tensor, out: L.Tensor, res, kw) -> bool:
        """One class-split launch or one launch per class?  The split launch wins where the per-class launches are a handful of workgroups each
        (levels 3-5: 0.23 -> 0.09 ms, 0.18 -> 0.03 ms); at level 2 with batch 4 every workgroup of the split launch fetches the union halo and
        keeps the LDS of the 8-tap class, and the tuned per-class launches are faster (0.27 against 0.38 ms).  Measured once per launch signature."""
        alt = chs[0].alt
        p0 = alt.cands[0]
        nb = kw.get("nb") or self.n
        if not self.tune:
            return P.kernel_of(p0) == "dconv" or nb * p0.q[0] * p0.q[1] * p0.q[2] <= self.CLASS_SPLIT_MAX_VOXELS
        if alt.chosen is not None or chs[0].chosen is not None:  # a further launch of the same op (another sample): same decision
            return alt.chosen is not None
        key = (f"use_cs|{p0.kind}|w{alt.wshape}|q{p0.q}|n{nb}|es{self.eng.es}|kc{p0.kc}|acc{int(kw.get('accumulate', 0))}|res{int(kw.get('res_mode', 0))}"
               f"|st{int(bool(kw.get('stats')))}|two{int(bool(inp.ptr2))}{int(bool(out.ptr2))}" + ("|gate" if kw.get("gate") else ""))
        cache = _tune_cache()
        if _cache_usable(key, [pl for ch in (list(chs) + [alt]) for pl in ch.cands]):
            return bool(cache[key])
        eng = self.eng
        stream = torch.cuda.current_stream().cuda_stream
        times = []
        for variant in (chs, [alt]):  # lower both into scratch lists (plans chosen as usual, nothing registered), pack their weights, time the launches
            tmp, packs = [], []
            for ch in variant:
                self._igemm(tmp, ch, inp, out, res=res, probe=True, **kw)
                wp = self._gather_tmp(ch.probe_plan.pack_map, ch.woff)
                tmp[-1].desc.wpack = wp.data_ptr()
                packs.append(wp)

            def run():
                for launch in tmp:
                    L.check(launch.fn(*launch.args, stream), "class-split decision")

            times.append(min(self._event_ms(run) for _ in range(1 + eng.tune_reps)))  # (not _time_launch: here every run is timed, the first included, and a rejected launch is an error)
        use = times[1] < times[0]
        cache[key] = int(use)  # in-process always (every later plan and, under data parallel, every rank repeats the choice); the cache FILE only outside the experiment modes
        if self.eng.deep == "1":
            _tune_cache.dirty = True
        self.class_split_ms.append((key, times))
        return use

    def _igemm(self, lst, ch: _Choice, inp: L.Tensor, out: L.Tensor, *, bias=0, bias2=0, scale=0, shift=0, alpha=0, act=L.ACT_NONE, res: Optional[L.Tensor] = None,
               res_mode=L.RES_NONE, accumulate=0, stats=0, stats_stride=0, ncls=1, gate=0, nb: Optional[int] = None, in_gate=0, probe=False, res_out: Optional[L.Tensor] = None, bias_res=0,
               in1=None):
        """probe: build the launch (plan chosen / measured as usual) WITHOUT making it part of the step — no packed-weight registration
        (Plan._use_class_split times two alternative lowerings of an op this way; ch.probe_plan = the plan it used)."""
        nb = self.n if nb is None else nb
        d = L.IgemmDesc()
        d.gate = gate or None
        d.in_gate = in_gate or None
        if ch.fold:
            inp, out, res = self._fold_desc(inp, ch.fold), self._fold_desc(out, ch.fold), (self._fold_desc(res, ch.fold) if res is not None else None)
            d.cout_mod = ch.cmod
        d.inp, d.out = inp, out
        d.bias, d.bias2, d.scale, d.shift, d.alpha = bias or None, bias2 or None, scale or None, shift or None, alpha or None
        d.act, d.res_mode, d.accumulate = act, res_mode, accumulate
        if res is not None:
            d.res = res
        d.stats, d.stats_stride = stats or None, stats_stride
        d.bias_res = bias_res or None
        if in1 is not None:  # VSSEG_RES_IN1: (one-channel tensor, weights, bias) of a 1 -> C 1x1x1 convolution added behind the activation
            d.in1, d.in1_w, d.in1_b = in1
        if res_out is not None:
            d.res_out = res_out
        if ch.chosen is not None:  # a further launch of the same lattice class (another sample): same plan, same packed weights
            pl = ch.chosen
        else:
            pl = self._choose(ch, d) if (self.tune and len(ch.cands) > 1) else ch.cands[0]
            if probe:
                ch.probe_plan = pl
            else:
                self._register(ch, pl)
        fill_igemm_desc(d, pl)
        if not probe:
            self._wpack_fixups.append((d, "wpack", ch.map_off))
            if pl.res_tiles:
                self._wpack_fixups.append((d, "wpack_res", ch.map_off_res))
        nvalid = nb  # output voxels this lattice class writes
        for a, oa in enumerate((out.x, out.y, out.z)):
            nvalid *= min(pl.q[a], -(-(oa - pl.cls.oo[a]) // pl.cls.os[a]))
        if P.is_shuffle(pl):
            nvalid = nb * out.x * out.y * out.z * (pl.nt * 16 // pl.nc) // 4  # the parity classes this launch writes
        taps_eff = 2.25 if P.is_shuffle(pl) else pl.ntaps
        if pl.classes is not None:  # every output voxel, by the class it belongs to (27 / 8 taps per voxel on average for 3x3x3 stride 2)
            nvalid, taps_eff = nb * out.x * out.y * out.z, sum(len(c_.taps) for c_ in pl.classes) / len(pl.classes)
        es_in, es_out = (2 if inp.dtype == L.BF16 else 4), (2 if out.dtype == L.BF16 else 4)
        tuned = " tuned[cache]" if ch.cached else ("" if ch.tuned_ms is None else f" tuned[{ch.cands.index(pl)}/{len(ch.cands)} {ch.tuned_ms[0]:.3f}->{min(ch.tuned_ms):.3f}ms]")
        fold_tag = f" zfold{ch.fold}" if ch.fold else ""
        rn = pl.res_tiles * 16 if pl.res_tiles else 0  # output channels of the 1x1x1 residual convolution riding along
        meta = dict(tag=f"{pl.kind}{fold_tag} q={pl.q} K={pl.kreal}x{pl.ntaps} N={pl.nc}{'+res' + str(rn) if rn else ''} tile={pl.tile} ck={pl.ck} ns={pl.nsplit} D={pl.depth} lds={pl.lds}{tuned}", name=self._igemm_name(pl, inp), kind="mfma",
                    flops=2.0 * nvalid * (taps_eff * pl.kreal * pl.nc + pl.kreal * rn) / max(ch.fold, 1),
                    # algorithmic bytes: input once + output once (+ the residual / mask / gated operand or the previous gradient an
                    # accumulating launch has to read: one more output-sized tensor)
                    bytes=float(nvalid) * pl.nc * es_out * (2 if (accumulate or res is not None) else 1) + float(nb) * inp.x * inp.y * inp.z * pl.kreal * es_in / (1 if pl.classes is not None else ncls)
                    + (float(nvalid) * rn * es_out if res_out is not None else 0.0))
        lst.append(Launch(self.eng.lib.vsseg_igemm, [C.byref(d)], meta, desc=d))

    def _march_cands(self, ch: _Choice, Lr: Layer) -> List[P.IgemmPlan]:
        """The marching-kernel plans of a stride-1 3x3x1 forward launch: those among its candidates when the autotuner listed them, else
        planner.march_plans' deterministic list (the untuned lowering then takes the first one)."""
        got = [pl for pl in ch.cands if P.is_march(pl)]
        if got or len(ch.cands) != 1:
            return got
        p0 = ch.cands[0]
        got = P.march_plans(p0.kind, Lr.wshape, p0.cls, p0.q, self.eng.es, p0.kc, p0.nc, p0.kreal, self.n)
        for pl in got:
            if pl.pack_map is None:
                pl.pack_map = P.pack_map(pl, Lr.wshape)
        return got

    def _compact_choice(self, ch: _Choice, Lr: Layer) -> Optional[_Choice]:
        """A convolution launch whose input has ONE real channel (the network input, the pre-sigmoid gradient of an attention map), on the marching kernel reading the
        COMPACT one-channel tensor (csrc/mconv.hip C1: 2 bytes per voxel from HBM instead of the 16 of the zero-extended channel group): the marching plans (weights in
        LDS) of the launch as their own choice, or None where there is none / the switch is off."""
        if not self.eng.compact_c1 or self.eng.es != 2 or ch.fold or not ch.cands or ch.cands[0].kc != 8 or ch.cands[0].kreal not in (1, 2):
            return None  # (two real channels: the gradient of the logits, csrc/mconv.hip CC = 2)
        if ch.compact is None:
            cands = [pl for pl in self._march_cands(ch, Lr) if pl.depth == L.DEPTH_MARCH]
            ch.compact = _Choice(cands, ch.woff, wshape=ch.wshape, wshape2=ch.wshape2, woff2=ch.woff2, is_compact=True) if cands else False  # (a merged residual convolution stays merged)
            if ch.compact:
                ch.compact.compact = ch.compact  # (asked again with the new choice: itself)
        return ch.compact or None

    def _logits_compact(self, Lr: Layer, x: TensorSpec) -> bool:
        """Whether BOTH backward launches of the logits convolution can read the gradient of the two logits compact: a marching data-gradient plan (csrc/mconv.hip CC = 2)
        and a marching weight-gradient tile with the compact P operand (csrc/mwgrad.hip PC2, instantiated for 32 input channels)."""
        cp = self.cplans[Lr.prefix]
        if (not self.eng.compact_c1 or self.eng.es != 2 or not Lr.stride1_3x3x1 or Lr.cout != 2 or Lr.cin != 32
                or len(cp.dgrad) != 1 or x.parts is not None or x.base is not None or self._compact_choice(cp.dgrad[0], Lr) is None):
            return False
        return bool(P.march_wgrad_tiles(Lr.cin, 8, cp.wgrad.q, self.n, self.eng.wgrad_scratch().numel()))

    @staticmethod
    def _igemm_name(pl: P.IgemmPlan, inp: L.Tensor) -> str:
        """Kernel group of a convolution launch in the profiles: which of the kernels its plan runs on."""
        kernel = P.kernel_of(pl)
        if kernel == "igemm":
            return f"igemm<{'bf16' if inp.dtype == L.BF16 else 'f32'},{pl.nt},{pl.mtw}>"
        args = {"dconv": f"{pl.mtw},{pl.nt}", "tconv": f"{pl.ck // 8}"}.get(kernel, f"{pl.nt}")
        return f"{kernel}<bf16,{args}>"

    def _ew_meta(self, name: str, level: int, passes_c: int, dtype_es: Optional[int] = None) -> dict:
        """Launch metadata of a streaming kernel: algorithmic bytes = (channels read + written per voxel, summed over its tensor
        passes) x voxels x element size.  `passes_c` = that per-voxel channel count."""
        es = self.eng.es if dtype_es is None else dtype_es
        return dict(name=name, kind="hbm", flops=0.0, bytes=float(self._vox(level)) * passes_c * es, tag=f"L{level} {passes_c} ch/voxel")

    # ------------------------------------------------------------------ lowering: per-layer BatchNorm records
    def _bn_records(self):
        eng, dev, nsh = self.eng, self.eng.device, L.STAT_SHARDS
        bn_layers = [op.layer for op in eng.prog.ops if isinstance(op, ConvBnAct)]
        cpad = [P.round_up(Lr.cout, 16) for Lr in bn_layers]
        tot_c = max(sum(cpad), 1)
        # fp64 sharded statistics: row 0 forward (sum, sumsq), row 1 backward (sum dz, sum dz*xhat, sum dout) + PReLU-slope accumulators
        self.stats = torch.zeros(2, nsh * 3 * tot_c + nsh * max(len(bn_layers), 1), dtype=torch.float64, device=dev)
        self.vec = torch.zeros(6, tot_c, dtype=torch.float32, device=dev)  # mean, invstd, scale, shift, mean_dz, mean_dzx
        self.p_drop = float(eng.dropout_p) if self.train else 0.0
        row, sp, vp = self.stats.shape[1], self.stats.data_ptr(), self.vec.data_ptr()
        self.bn: Dict[str, _BnLayer] = {}
        self.bn_info = {}
        o = v = 0
        for i, (Lr, cp) in enumerate(zip(bn_layers, cpad)):
            pre = Lr.prefix
            # Dropout keep-mask bytes (one byte per voxel and 8-channel group = 1/16 of the bf16 activation): written by the forward, read by both backward passes,
            # which are otherwise VALU-bound on running Philox4x32-10 again (measured: the three BN kernels ran at the same ~90-130 G iterations/s whatever they moved)
            keep = self._raw("keep:" + pre, Lr.out_level, Lr.cout // 8, dtype=torch.uint8).data_ptr() if self.p_drop > 0.0 else None
            self.bn[pre] = _BnLayer(self._pp(pre + ".norm.weight"), self._pp(pre + ".norm.bias"), self._pp(pre + ".act.weight"), self._bp(pre + ".norm.running_mean"),
                                    self._bp(pre + ".norm.running_var"), self._cp(pre + ".norm.num_batches_tracked"), *(vp + 4 * (r * tot_c + v) for r in range(6)),
                                    sp + 8 * o, sp + 8 * (row + o), sp + 8 * (row + nsh * 3 * tot_c + nsh * i), (i + 1) | L.SEED_INDIRECT, cp, keep)
            self.bn_info[pre] = (Lr, i + 1)
            o += nsh * 3 * cp
            v += cp

    # ------------------------------------------------------------------ lowering: fusion decisions (program + switches + planner; each consults the earlier ones)
    def _first_unit_residual(self, op) -> Optional[ConvPlain]:
        """The 1 -> C 1x1x1 residual convolution of the network input that the ConvBnAct `op` adds (first encoder ResidualUnit), or None."""
        pr = self.eng.prog.producer(op.res) if (isinstance(op, ConvBnAct) and op.res is not None) else None
        ok = pr is not None and pr.layer.cin == 1 and pr.layer.kernel == (1, 1, 1) and pr.x.root.name == self.eng.prog.input.name and pr.act == "none" and pr.res is None
        return pr if ok else None

    def _decide_res1_fused(self):
        """First encoder ResidualUnit (in_channels = 1): its 1x1x1 residual convolution is x1[v]*w[c] + b[c]; in training it is computed inside the BN/dropout/PReLU
        kernel that adds it (vsseg_bn_act_fwd_res1) instead of by an igemm launch that writes a 16-channel tensor for that kernel to read back."""
        found = [self._first_unit_residual(op) for op in self.eng.prog.ops] if self.train else []
        self.res1_fused: Dict[str, ConvPlain] = {pr.layer.prefix: pr for pr in found if pr is not None}  # residual-conv prefix -> op: its own launch is skipped

    def _decide_eval_in1(self):
        """... and in eval inside the epilogue of the convolution it is added to (VSSEG_RES_IN1), where that convolution has a marching plan."""
        eng = self.eng
        self.eval_in1: Dict[str, ConvPlain] = {}  # prefix of the convolution whose epilogue adds the residual -> the residual convolution op
        if self.train or eng.es != 2 or eng.dry_run:
            return
        for op in eng.prog.ops:
            pr = self._first_unit_residual(op)
            if pr is None or op.x.parts is not None or op.x.base is not None:
                continue
            cpo = self.cplans[op.layer.prefix]
            if op.layer.stride1_3x3x1 and len(cpo.fwd) == 1 and not cpo.fold_fwd and op.layer.prefix not in self.resn and self._march_cands(cpo.fwd[0], op.layer):
                self.eval_in1[op.layer.prefix] = pr
                self.res1_fused[pr.layer.prefix] = pr  # (its own launch is skipped)

    def _decide_gate_onload(self):
        """Attention gates applied ON LOAD (ref:params/networks/blocks/attentionblock.py:43-47: out = att.repeat(C) * x + x): where the gated tensor's only
        reader is ONE stride-1 3x3x1 convolution (with its merged 1x1x1 residual) that runs on the marching kernel, that convolution and its weight
        gradient read x and the attention map and multiply in LDS (csrc/mconv.hip MODE 3, csrc/mwgrad.hip GIN): vsseg_att_apply_fwd is not launched and
        the gated tensor (2c channels at the level's resolution) is neither written nor read back.  Level 0 of this network (the logits convolution)."""
        eng, prog = self.eng, self.eng.prog
        self.gate_onload: Dict[str, AttGate] = {}
        if eng.es != 2:  # (independent of the autotuner: VSSEG_AUTOTUNE=0 lowers the same graph, with the first marching plan)
            return
        for g in prog.ops:
            if not isinstance(g, AttGate):
                continue
            readers = [o for o in prog.readers(g.out) if getattr(o, "att", None) is not g.out]  # (Program.readers also counts readers as an attention map; this decision never did)
            # (b) a ResidualUnit whose first 3x3x1 convolution carries the unit's 1x1x1 residual convolution as residual tiles (self.resn) and whose backward is the
            #     fused launch (csrc/mbwd.hip, x gated on load): the level-1 decoder unit.  Both readers of the gated tensor are then one forward launch.
            unit = [o for o in readers if isinstance(o, ConvBnAct) and o.layer.prefix in self.resn]
            if (len(unit) == 1 and len(readers) == 2 and self.resn[unit[0].layer.prefix] in readers and unit[0].x is g.out and (unit[0].layer.cin, unit[0].layer.cout) == (64, 32)
                    and g.x.c == 64 and (not self.train or P.fused_bwd_tiles(32, 64, self.lv[unit[0].layer.level], self.n, 48 * 1024 * 1024, res=True))):
                self.gate_onload[g.out.name] = g
                continue
            main = [o for o in readers if isinstance(o, ConvPlain) and o.layer.prefix not in self.merged]
            if len(main) != 1 or any(o is not main[0] and not (isinstance(o, ConvPlain) and self.merged.get(o.layer.prefix) is main[0]) for o in readers):
                continue
            c = main[0]
            Lc, cpc = c.layer, self.cplans[c.layer.prefix]
            if (Lc.stride1_3x3x1 and Lc.cin == 32 and Lc.cout <= 8 and c.x is g.out and len(cpc.fwd) == 1 and not cpc.fold_fwd and g.x.c == Lc.cin and self._march_cands(cpc.fwd[0], Lc)
                    and (not self.train or P.march_wgrad_tiles(Lc.cin, 8, self.lv[Lc.level], self.n, eng.wgrad_scratch().numel()))):
                self.gate_onload[g.out.name] = g

    def _decide_chains(self):
        """Chained marching convolutions (csrc/chain.hip, vsseg_conv_chain; inference only): two consecutive stride-1 3x3x1 convolutions whose intermediate 16-channel tensor has
        no other reader run as ONE launch with that tensor in LDS — the first ResidualUnit of the encoder (1 -> 16 -> 16 with the residual convolution of the network input in
        the second epilogue) and the attention block of the finest decoder level (32 -> 16 + ReLU -> 1 + sigmoid).  201 MB per patch are neither written nor read back, per pair."""
        eng, prog = self.eng, self.eng.prog
        self.chain_first: Dict[str, tuple] = {}  # prefix of the first convolution -> (first op, second op, plan)
        self.chain_second: set = set()           # prefixes of the second convolutions: emitted with the first
        # inference only (in training a BatchNorm needs the whole tensor between the two convolutions; the attention block, which has none, measured no gain: DESIGN 3.11)
        if eng.chain == "0" or eng.es != 2 or eng.dry_run or self.train:
            return
        for a in prog.ops:
            if not isinstance(a, (ConvBnAct, ConvPlain)) or not a.layer.stride1_3x3x1 or a.layer.cout not in (16, 32) or a.res is not None or a.x.base is not None or a.out.base is not None:
                continue
            pa_ = a.layer.prefix
            unit = eng.chain != "l0" and pa_ in self.resn and (a.layer.cin, a.layer.cout) == (16, 32) and a.x.parts is None  # a two-sub-unit ResidualUnit whose residual convolution rides along
            if (pa_ in self.resn) != unit or (a.layer.cout == 32) != unit or pa_ in self.merged or pa_ in self.absorbs or pa_ in self.resn_of or a.x.name in self.gate_onload:
                continue
            readers = [o for o in prog.readers(a.out) if o is not a]  # (here a reader as an attention map counts, too)
            if len(readers) != 1 or not isinstance(readers[0], type(a)) or readers[0].x is not a.out:
                continue
            b = readers[0]
            pb_ = b.layer.prefix
            if not b.layer.stride1_3x3x1 or b.layer.cin != a.layer.cout or pb_ in self.resn or pb_ in self.merged or pb_ in self.absorbs or b.out.base is not None or a.out in (prog.logits, *prog.att_maps):
                continue
            if unit:  # 16 -> 32 -> 32 + the residual convolution's output (which then never exists): the residual tensor's only reader must be the second sub-unit
                rcv = self.resn[pa_]
                ok = (isinstance(b, ConvBnAct) and b.layer.cout == 32 and b.res is rcv.out
                      and sum(1 for o in prog.ops if getattr(o, "res", None) is rcv.out or getattr(o, "x", None) is rcv.out) == 1)
                compact, cin = False, 16
            elif isinstance(a, ConvBnAct):  # the first ResidualUnit: compact network input, the unit's residual convolution already folded into the second epilogue (eval_in1)
                ok = a.x.root.name == prog.input.name and a.x.real == 1 and eng.compact_c1 and b.layer.cout == 16 and pb_ in self.eval_in1 and b.res is not None
                compact, cin = True, 8
            else:  # the attention block: conv + ReLU -> conv + sigmoid -> the fp32 attention map
                ok = a.act == "relu" and b.act == "sigmoid" and b.layer.cout == 1 and b.res is None and b.out.kind == "f32" and a.layer.cin == 32 and (a.x.parts is None or a.x.parts[0].c % 16 == 0)
                compact, cin = False, a.layer.cin
            plan_c = P.chain_plan(cin, compact, self.lv[a.layer.level], self.n, a.layer.cout) if ok else None
            if plan_c is None:
                continue
            self.chain_first[pa_] = (a, b, plan_c)
            self.chain_second.add(pb_)

    # ------------------------------------------------------------------ lowering: forward emission
    def _lower_forward(self):
        for op in self.eng.prog.ops:
            if isinstance(op, AttGate):
                if op.out.name not in self.gate_onload:
                    self.fwd.append(Launch(self.eng.lib.vsseg_att_apply_fwd, [self._desc(op.x), self._alloc(op.att, self.bufs).data_ptr(), self._desc(op.out)], self._ew_meta("att_apply_fwd", op.x.level, 2 * op.x.c + 2)))
            elif op.layer.prefix in self.chain_second:  # emitted with the first convolution of its chain
                continue
            elif op.layer.prefix in self.chain_first:
                self._emit_chain(*self.chain_first[op.layer.prefix])
            elif isinstance(op, ConvBnAct):
                self._emit_conv_bn_act(op)
            else:
                self._emit_conv_plain(op)
        self.out_logits = self._alloc(self.eng.prog.logits, self.bufs)
        self.out_atts = [self._alloc(a, self.bufs) for a in self.eng.prog.att_maps]

    def _emit_chain(self, a, b, plan_c):
        eng, lib = self.eng, self.eng.lib
        La, Lb = a.layer, b.layer
        q = self.lv[La.level]
        d = L.ChainDesc()
        bn = isinstance(a, ConvBnAct)
        rcv = self.resn.get(La.prefix)
        compact = bn and rcv is None
        d.inp, d.out, d.cmid = (self._xdesc(a.x, True) if compact else self._desc(a.x)), self._desc(b.out), La.cout
        d.bias_a, d.bias_b = self._pp(La.bkey), self._pp(Lb.bkey)
        if bn:
            ba, bb = self.bn[La.prefix], self.bn[Lb.prefix]
            for Lr, r in ((La, ba), (Lb, bb)):
                self.fwd_pre.append(Launch(lib.vsseg_bn_fold_eval, [r.gamma, r.beta, r.rmean, r.rvar, BN_EPS, r.scale, r.shift, Lr.cout]))
            d.scale_a, d.shift_a, d.alpha_a, d.act_a = ba.scale, ba.shift, ba.alpha, L.ACT_PRELU
            d.scale_b, d.shift_b, d.alpha_b, d.act_b = bb.scale, bb.shift, bb.alpha, L.ACT_PRELU
            if compact:
                pr1 = self.eval_in1[Lb.prefix]
                d.in1_w, d.in1_b = self._pp(pr1.layer.wkey), self._pp(pr1.layer.bkey)
            else:
                d.res_tiles, d.bias_res = 2, self._pp(rcv.layer.bkey)
        else:
            d.act_a, d.act_b = L.ACT_RELU, L.ACT_SIGMOID
        d.tz, d.mtw, d.lx, d.waves, d.lead = plan_c["tz"], plan_c["mtw"], plan_c["lx"], plan_c["waves"], plan_c["lead"]
        for attr, Lr, kc in (("wpack_a", La, 8 if compact else La.cin), ("wpack_b", Lb, La.cout)):
            pl = P.chain_pack_plan(tuple(Lr.wshape), q, eng.es, kc, self.n)
            assert pl is not None, "no marching pack layout for a chained convolution"
            ch = _Choice([pl], eng.layout.param_off[Lr.wkey][0], wshape=tuple(Lr.wshape))
            if attr == "wpack_a" and rcv is not None:  # + the residual convolution's centre-tap tiles behind the first convolution's weights
                pl = dataclasses.replace(pl, res_tiles=2)
                pl.pack_map_res = P.residual_tile_pack_map(kc, 2, tuple(rcv.layer.wshape))
                ch.woff_res = eng.layout.param_off[rcv.layer.wkey][0]
            self._register(ch, pl)
            self._wpack_fixups.append((d, attr, ch.map_off))
            if pl.res_tiles:
                self._wpack_fixups.append((d, "wpack_res", ch.map_off_res))
        dummy = torch.zeros(16, dtype=eng.tdtype, device=eng.device)
        d.wpack_a = d.wpack_b = dummy.data_ptr()
        d.wpack_res = dummy.data_ptr() if rcv is not None else None  # (placeholders for the domain check; the real pointers are set once the packed-weight buffer exists)
        if lib.vsseg_conv_chain_lds_bytes(C.byref(d)) < 0:
            raise RuntimeError("vsseg_conv_chain rejected a launch the planner offered: " + lib.vsseg_last_error().decode())
        nvox = float(self.n) * q[0] * q[1] * q[2]
        cin_r = a.x.real
        meta = dict(tag=f"chain q={q} K={cin_r}x9 -> {La.cout}x9 -> N={Lb.cout}{'+res' if rcv is not None else ''} tz={plan_c['tz']} waves={plan_c['waves']} mtw={plan_c['mtw']} lead={plan_c['lead']} lx={plan_c['lx']}",
                    name=f"chain<bf16,{8 if compact else La.cin}>", kind="mfma", flops=2.0 * nvox * (9 * (cin_r * La.cout + La.cout * Lb.cout) + (cin_r * Lb.cout if rcv is not None else 0)),
                    bytes=nvox * (cin_r * eng.es + Lb.cout * (4 if b.out.kind == "f32" else eng.es) + (La.cout * eng.es if (self.train and not bn) else 0)))
        self.fwd.append(Launch(lib.vsseg_conv_chain, [C.byref(d)], meta, desc=d))

    def _emit_conv_bn_act(self, op: ConvBnAct):
        prog, lib, F = self.eng.prog, self.eng.lib, self.fwd
        Lr, cp, pre = op.layer, self.cplans[op.layer.prefix], op.layer.prefix
        b = self.bn[pre]
        glu = self.gate_onload.get(op.x.name)  # the attention gate in front of the unit is applied on load: read x (the concat) and the attention map
        cc1 = self._compact_choice(cp.fwd[0], Lr) if (len(cp.fwd) == 1 and op.x.root.name == prog.input.name and pre not in self.resn) else None
        if cc1 is not None:  # the network input as a compact one-channel tensor (marching plans only)
            cp.fwd[0] = cc1
        xin = self._desc(glu.x) if glu is not None else self._xdesc(op.x, cp.fold_fwd or cc1 is not None)
        out = self._desc(op.out)
        fused_res = prog.producer(op.res) if op.res is not None else None
        if fused_res is not None and fused_res.layer.prefix not in self.res1_fused:
            fused_res = None
        res = self._desc(op.res) if (op.res is not None and fused_res is None) else None
        rcv = self.resn.get(pre)  # the unit's 1x1x1 residual convolution rides along (same input): stored to its own tensor, or (eval, single-subunit units) added in the epilogue
        rkw = dict(bias_res=self._pp(rcv.layer.bkey)) if rcv is not None else {}
        if glu is not None:
            assert rcv is not None
            rkw["in_gate"] = self._alloc(glu.att, self.bufs).data_ptr()
        if rcv is not None and (self.train or op.res is not rcv.out):
            rkw["res_out"] = self._desc(rcv.out)
        if self.train:
            seed = self.seed_dev.data_ptr()  # the kernels read the seed through seed_dev (the salt carries SEED_INDIRECT)
            yd = self._tdesc(self._raw("y:" + pre, Lr.out_level, Lr.cout), Lr.out_level)
            self._igemm_classes(F, cp.fwd, xin, yd, bias=self._pp(Lr.bkey), stats=b.stats_fwd, stats_stride=b.cpad, ncls=len(cp.fwd), **rkw)
            F.append(Launch(lib.vsseg_bn_finalize, [b.stats_fwd, b.cpad, Lr.cout, float(self._vox(Lr.out_level)), b.gamma, b.beta, BN_EPS, BN_MOMENTUM, b.rmean, b.rvar,
                                                    b.counter, b.mean, b.invstd, b.scale, b.shift]))
            if fused_res is not None:
                x1 = self._xdesc(fused_res.x, True)  # compact 1-channel copy of the network input
                F.append(Launch(lib.vsseg_bn_act_fwd_res1, [yd, b.scale, b.shift, b.alpha, self.p_drop, seed, b.salt, x1.ptr, self._pp(fused_res.layer.wkey), self._pp(fused_res.layer.bkey), out, b.keep],
                                self._ew_meta("bn_act_fwd", Lr.out_level, 2 * Lr.cout + 1)))
            else:
                F.append(Launch(lib.vsseg_bn_act_fwd, [yd, b.scale, b.shift, b.alpha, self.p_drop, seed, b.salt, res if res is not None else L.Tensor(), 1 if res is not None else 0, out, b.keep],
                                self._ew_meta("bn_act_fwd", Lr.out_level, (3 if res is not None else 2) * Lr.cout)))
            return
        self.fwd_pre.append(Launch(lib.vsseg_bn_fold_eval, [b.gamma, b.beta, b.rmean, b.rvar, BN_EPS, b.scale, b.shift, Lr.cout]))  # depends on parameters only
        if rcv is not None and op.res is rcv.out:  # out = act(bn(conv(x))) + residual(x) entirely inside the launch: the residual tensor does not exist
            res = None
        pr1 = self.eval_in1.get(pre)
        if pr1 is not None:  # the first ResidualUnit: its 1 -> C residual convolution of the network input is x1 * w + b in this launch's epilogue (marching plans only)
            ch0 = cp.fwd[0]
            cp.fwd[0] = _Choice(self._march_cands(ch0, Lr), ch0.woff, wshape=ch0.wshape)
            x1 = self._xdesc(pr1.x, True)
            self._igemm(F, cp.fwd[0], xin, out, bias=self._pp(Lr.bkey), scale=b.scale, shift=b.shift, alpha=b.alpha, act=L.ACT_PRELU, res_mode=L.RES_IN1,
                        in1=(x1.ptr, self._pp(pr1.layer.wkey), self._pp(pr1.layer.bkey)))
            return
        self._igemm_classes(F, cp.fwd, xin, out, bias=self._pp(Lr.bkey), scale=b.scale, shift=b.shift, alpha=b.alpha, act=L.ACT_PRELU, res=res,
                            res_mode=L.RES_ADD if res is not None else L.RES_NONE, ncls=len(cp.fwd), **rkw)

    def _emit_conv_plain(self, op: ConvPlain):
        eng, lib, F = self.eng, self.eng.lib, self.fwd
        Lr, cp = op.layer, self.cplans[op.layer.prefix]
        if Lr.prefix in self.merged or Lr.prefix in self.res1_fused or Lr.prefix in self.resn_of:  # computed inside the convolution / elementwise kernel it is added to
            return
        absorbed = self.absorbs.get(Lr.prefix)
        bias2 = self._pp(absorbed.layer.bkey) if absorbed is not None else 0
        gl = self.gate_onload.get(op.x.name)
        if gl is not None:  # the attention gate in front of this convolution is applied on load: read x and the attention map, marching plans only
            ch0 = cp.fwd[0]
            gch = _Choice(self._march_cands(ch0, Lr), ch0.woff, ch0.wshape2, ch0.woff2, wshape=ch0.wshape)
            cp.fwd[0] = gch
            self._igemm(F, gch, self._desc(gl.x), self._desc(op.out), bias=self._pp(Lr.bkey), bias2=bias2, act=ACT_CODE[op.act], in_gate=self._alloc(gl.att, self.bufs).data_ptr())
            return
        # the C -> 1 stride-1 3x3x1 convolution that closes an attention block of the two finest levels: a bandwidth kernel on the vector ALUs (csrc/nconv.hip: every
        # input voxel read once, partial sums exchanged between neighbouring threads) instead of an MFMA launch with one real output channel
        yext, zext = self.lv[Lr.level][1], self.lv[Lr.level][2]
        if (eng.narrow_fwd and eng.es == 2 and not eng.dry_run and Lr.cout == 1 and Lr.cin in (16, 32) and Lr.stride1_3x3x1
                and absorbed is None and op.res is None and op.x.parts is None and op.x.base is None and op.out.base is None and op.act in ("none", "sigmoid")
                and yext in (16, 32, 64, 128, 256) and zext % (512 // yext) == 0):
            xd, od = self._desc(op.x), self._desc(op.out)
            if od.c == 1 and od.pitch == 1 and not xd.ptr2:
                nzb = zext // (512 // yext)
                nxs = max(1, round(256 / (self.n * nzb)))  # about one 512-thread workgroup per CU (measured best at batch 1 and 4 on both levels: tools/bench_nconv.py)
                lx = -(-self.lv[Lr.level][0] // nxs)
                nq = float(self._vox(Lr.level))
                F.append(Launch(lib.vsseg_conv_to1, [xd, self._pp(Lr.wkey), self._pp(Lr.bkey), ACT_CODE[op.act], od, lx],
                                dict(name="nconv<bf16>", kind="hbm", flops=2.0 * nq * 9 * Lr.cin, bytes=nq * (2.0 * Lr.cin + (4.0 if od.dtype == L.F32 else 2.0)), tag=f"{Lr.prefix[-40:]} {Lr.cin}->1 k={Lr.kernel} lx={lx}")))
                return
        xin, out = self._xdesc(op.x, cp.fold_fwd), self._desc(op.out)
        res = self._desc(op.res) if (op.res is not None and absorbed is None) else None
        for ch in cp.fwd:
            self._igemm(F, ch, xin, out, bias=self._pp(Lr.bkey), bias2=bias2, act=ACT_CODE[op.act], res=res, res_mode=L.RES_ADD if res is not None else L.RES_NONE)

    # ------------------------------------------------------------------ lowering: backward emission
    def _lower_backward(self):
        """Ops in reverse.  Several decisions below depend on the order of emission (what `_written` holds when a fused launch / a gate fusion asks; `_absorbed_res`
        is filled by a fused launch that runs before its residual convolution is visited); the state they share lives in these attributes until _finish_pack."""
        ops = self.eng.prog.ops
        if not self.train:
            return
        self._written: Dict[str, bool] = {}  # gradient buffers (by root tensor) that hold a first contribution
        self._staged: Dict[str, L.Tensor] = {}  # the staged gradient of the logits: "c" compact or "p" zero-padded
        self._grad_alias = {op.res.name: op.out for op in ops if not isinstance(op, AttGate) and op.res is not None and op.res.name.endswith(":res")}  # residual-conv output -> the tensor it is added into (shares its gradient)
        self._absorbed_res: set = set()  # residual convolutions whose data / weight gradient a fused launch produces
        self._early_res: set = set()  # residual convolutions whose backward was issued with the block their output is added to
        self._gate_fuse: Dict[str, tuple] = {}  # relu-conv prefix -> (d(gated) descriptor, attention map pointer) of the gate fused into its data gradient
        self._folded_bias: set = set()  # plain convolutions whose bias gradient is produced by another kernel's reduction
        for op in reversed(ops):
            if isinstance(op, ConvBnAct):
                self._bwd_conv_bn_act(op)
            elif isinstance(op, ConvPlain):
                self._bwd_conv_plain(op)
            else:
                self._bwd_att_gate(op)
        self._move_late_wgrads()

    def _logits_grad(self, compact: bool) -> L.Tensor:
        """The loss' fp32 gradient of the logits staged in the compute dtype by the eager prelude: zero-extended to one 8-channel group, or (the marching kernels'
        compact operands, csrc/mconv.hip CC = 2 / csrc/mwgrad.hip PC2) as it is, two channels per voxel."""
        staged, logits = self._staged, self.eng.prog.logits
        assert not staged or ("c" in staged) == compact, "the gradient of the logits is staged in one layout"
        if not staged:
            if compact:
                buf = self._raw("g:logits2", 0, logits.c)
                self.glogits_dst = staged["c"] = self._tdesc(buf, 0)
            else:
                buf = self._raw("g:logits8", 0, 8)  # channels 2..7 stay zero
                staged["p"] = self._tdesc(buf, 0)
                self.glogits_dst = L.Tensor(buf.data_ptr(), _tdtype(buf), logits.c, 8, self.n, *self.lv[0], None, 0, L.ZERO_PADDED)
            self.bwd_pre.append(Launch(self.eng.lib.vsseg_copy_cast, [_Slot("glogits"), self.glogits_dst]))
        return staged["c" if compact else "p"]

    def _contribution(self, spec: TensorSpec) -> int:
        """accumulate flag for adding a gradient contribution into g[spec] (first full-width contribution overwrites)."""
        if spec.parts is not None:  # both operands of a concat receive their first contribution together
            flags = [self._contribution(p) for p in spec.parts]
            assert flags[0] == flags[1], f"operands of {spec.name} have inconsistent gradient state"
            return flags[0]
        root = spec.root.name
        if self._written.get(root):
            return 1
        self._written[root] = True
        if spec.c != spec.root.c:  # first contribution covers only a channel slice: start from zero
            gbuf = self._alloc(spec, self.grads)
            self.bwd.append(Launch(self.eng.lib.vsseg_memset_zero, [gbuf.data_ptr(), gbuf.numel() * gbuf.element_size()]))
            return 1
        return 0

    def _grad_of_out(self, t: TensorSpec) -> L.Tensor:
        t = self._grad_alias.get(t.name, t)
        if t.kind == "f32":  # logits: the loss' fp32 gradient staged in an 8-channel compute-dtype buffer
            assert t.name == self.eng.prog.logits.name
            return self._logits_grad(False)
        assert self._written.get(t.root.name), f"gradient of {t.name} is consumed before it is produced"
        return self._desc(t, self.grads)

    def _narrow_wgrad(self, Lr: Layer, x: TensorSpec, dy: L.Tensor, dy_compact: Optional[L.Tensor], bias_grad: bool = False) -> bool:
        """One input or one output channel, 3x3x1 / 1x1x1, stride 1: the weight gradient is a bandwidth reduction over the C-channel
        operand (vsseg_wgrad_narrow) instead of an MFMA launch on a zero-extended one (narrow-channel tails off the matrix cores)."""
        if Lr.transposed or tuple(Lr.stride) != (1, 1, 1) or Lr.kernel not in ((3, 3, 1), (1, 1, 1)) or self.lv[Lr.level][1] % 4:
            return False
        lib, es, k3 = self.eng.lib, self.eng.es, Lr.kernel[0]
        scr = self.eng.wgrad_scratch()  # partial-sum slabs (shared with vsseg_wgrad: the weight-gradient launches serialise on one stream)
        if Lr.cin == 1 and Lr.cout in (8, 16, 32, 64) and x.root.name == self.eng.prog.input.name and dy.c == Lr.cout and not dy.ptr2:
            x1 = self._xdesc(x, True)  # the compact one-channel copy of the network input
            assert not bias_grad, "the 1 -> C narrow weight gradient does not reduce a bias gradient (those convolutions sit in front of a BatchNorm)"
            head = [dy, x1.ptr, k3, 1, self._gp(Lr.wkey), k3 * k3, None]  # (the scratch pair follows: _move_late_wgrads retargets it through scratch_at)
            self.bwd.append(Launch(lib.vsseg_wgrad_narrow, head + [scr.data_ptr(), scr.numel()],
                                   dict(name="wgrad_narrow", kind="hbm", flops=0.0, bytes=float(es) * self._vox(Lr.level) * (Lr.cout + 1), tag=f"{Lr.prefix[-40:]} 1->{Lr.cout} k={Lr.kernel}"),
                                   side=True, late_ok=(k3 == 1), scratch_at=len(head)))
            return True
        if Lr.cout == 1 and Lr.cin in (8, 16, 32, 64) and dy_compact is not None and x.parts is None and x.base is None:
            # (the bias gradient of the C -> 1 convolution = sum of its one-channel dY rides in the same slabs: fixed summation order)
            self.bwd.append(Launch(lib.vsseg_wgrad_narrow, [self._desc(x), dy_compact.ptr, k3, -1, self._gp(Lr.wkey), k3 * k3, self._gp(Lr.bkey) if bias_grad else None, scr.data_ptr(), scr.numel()],
                                   dict(name="wgrad_narrow", kind="hbm", flops=0.0, bytes=float(es) * self._vox(Lr.level) * (Lr.cin + 1), tag=f"{Lr.prefix[-40:]} {Lr.cin}->1 k={Lr.kernel}"), side=True))
            return True
        return False

    def _conv_backward(self, Lr: Layer, x: TensorSpec, dy: L.Tensor, bias_grad: bool, relumask: Optional[TensorSpec] = None, dy_compact: Optional[L.Tensor] = None, gate=None, own_dy: bool = False):
        eng, B = self.eng, self.bwd
        wg = self.cplans[Lr.prefix].wgrad
        if self._narrow_wgrad(Lr, x, dy, dy_compact, bias_grad):
            self._conv_backward_data(Lr, x, dy, relumask, dy_compact, gate)
            return
        gl = self.gate_onload.get(x.name)  # the convolution's input is an attention-gated tensor that was never materialised: H = x, gated on load
        xin = self._desc(gl.x if gl is not None else x)
        d = L.WgradDesc()
        if gl is not None:
            d.h_gate = self._alloc(gl.att, self.bufs).data_ptr()
        pc2 = dy_compact is not None and dy_compact.c == 2  # P = the compact two-channel gradient of the logits (marching kernel only, csrc/mwgrad.hip PC2)
        if Lr.transposed:
            d.p, d.h, d.cp_valid, d.ch_valid = xin, dy, Lr.cin, Lr.cout
        else:
            d.p, d.h, d.cp_valid, d.ch_valid = (dy_compact if pc2 else dy), xin, Lr.cout, Lr.cin
        fill_wgrad_desc(d, wg)
        d.dw = self._gp(Lr.wkey)
        if bias_grad and not Lr.transposed:  # bias gradient = sum of dY, reduced inside the weight-gradient kernel (P = dY)
            d.dbias_p = self._gp(Lr.bkey)
        hch = (d.ch_valid + 15) // 16
        tiles = self.n
        for a in range(3):
            tiles *= -(-wg.q[a] // wg.tile[a])
        # few persistent workgroups with many tiles each: the per-workgroup flush is as large as the weight gradient itself
        scr = eng.wgrad_scratch()
        d.scratch, d.scratch_elems = scr.data_ptr(), scr.numel()
        # H-chunk group: one workgroup multiplies the P tile it fetched with `hgroup` 16-channel chunks of H (P is then read
        # ceil(chunks / hgroup) times instead of once per chunk); the library clamps the request to a divisor of the chunk count
        # that fits registers and LDS.  Heuristic: as large as allowed.
        hgs = [g for g in (4, 3, 2, 1) if hch % g == 0]
        d.hgroup = hgs[0]

        def set_blocks(wpc):  # persistent workgroups = wpc per CU over all H-chunk groups (the library clamps to what is resident)
            d.persistent_blocks = max(1, min(tiles, (256 * wpc) // max(1, hch // max(1, d.hgroup))))

        # the marching kernel (csrc/mwgrad.hip: both operands fetched once) where it is instantiated: stride-1 3x3x1 bf16, 16/32/64 input channels
        mtiles = []
        if eng.es == 2 and Lr.stride1_3x3x1 and d.h.c == Lr.cin and (d.p.c in (8, 16, 32) or pc2) and not d.p.ptr2:
            mtiles = P.march_wgrad_tiles(Lr.cin, 8 if pc2 else d.p.c, wg.q, self.n, scr.numel())
        assert mtiles or not pc2
        # the compute kernel (csrc/cwgrad.hip, march = 2) on the MFMA-bound stride-1 3x3x3 layers of levels 2-3: H chunks per workgroup (hgroup) 1 or 2
        cgs = []
        if (eng.compute_wgrad and eng.es == 2 and not Lr.transposed and tuple(Lr.stride) == (1, 1, 1) and Lr.kernel == (3, 3, 3) and gl is None and not pc2 and d.p.c in (48, 64) and d.p.c == Lr.cout
                and d.h.c == Lr.cin and Lr.cin % 16 == 0 and wg.q[1] % 8 == 0 and wg.q[2] % 32 == 0 and not d.p.ptr2):
            cgs = [g for g in ((2, 1) if d.p.c == 48 else (1,)) if hch % g == 0 and hch // g <= 8]
        wpc, live_tile, tuned = 4, L.i3(wg.tile), ""
        if self.tune:  # measured per launch: {double-buffered DMA pipeline | one buffer} x H-chunk group x workgroups per CU, and the marching kernel's tiles
            key = f"wgrad{4 if cgs else 3}|w{tuple(Lr.wshape)}|T{int(Lr.transposed)}|q{wg.q}|n{self.n}|es{eng.es}|two{int(bool(d.h.ptr2))}|pc{d.p.c}" + ("|gin" if gl is not None else "") + ("|c2" if pc2 else "")
            hit, tuned = self._tune_wgrad(key, d, wg, hgs, gl is None and not pc2, mtiles, cgs, set_blocks)
            if hit[0] == "m":
                d.march, live_tile = 1, L.i3(hit[1:4])
            elif hit[0] == "c":
                d.march, d.hgroup = 2, int(hit[1])
            else:
                d.march = 0
                d.single_buffer, d.hgroup, wpc = (int(v) for v in hit)
        elif cgs:  # untuned lowering: the compute kernel wherever it applies, two chunks per workgroup where they divide
            d.march, d.hgroup = 2, cgs[0]
        elif gl is not None or pc2:  # untuned lowering of a gated H operand / a compact P: the marching kernel is the only one that reads them — its first tile
            assert mtiles, "gate-on-load / a compact P was enabled for a layer without a marching weight-gradient tile"
            d.march, live_tile = 1, L.i3(mtiles[0])
        d.tile = live_tile
        set_blocks(wpc)
        nq = self.n * wg.q[0] * wg.q[1] * wg.q[2]
        meta = dict(tag=f"{Lr.prefix[-40:]} q={wg.q} taps={len(wg.taps)} cin={Lr.cin} cout={Lr.cout} " + (f"compute chunks/wg={d.hgroup}" if d.march == 2 else f"march tile={tuple(d.tile)}" if d.march else f"tile={wg.tile} blocks={d.persistent_blocks}x{hch} sb={d.single_buffer} hg={d.hgroup} lds={wg.lds}") + tuned,
                    name=(f"cwgrad<bf16,{wg.ntp}>" if d.march == 2 else f"mwgrad<bf16,{wg.ntp}>" if d.march else f"wgrad<{'bf16' if eng.es == 2 else 'f32'},{wg.ntp}>"), kind="mfma", flops=2.0 * nq * len(wg.taps) * Lr.cin * Lr.cout,
                    bytes=float(eng.es) * (nq * (Lr.cout if not Lr.transposed else Lr.cin) + self._vox(Lr.level if not Lr.transposed else Lr.out_level) * (Lr.cin if not Lr.transposed else Lr.cout)))
        B.append(Launch(eng.lib.vsseg_wgrad, [C.byref(d)], meta, desc=d, side=True, own_dy=own_dy))
        if bias_grad and Lr.transposed:  # (does not occur in this network: transposed convolutions are followed by BatchNorm)
            B.append(Launch(eng.lib.vsseg_channel_sum, [L.Tensor(dy.ptr, dy.dtype, Lr.cout, dy.pitch, dy.n, dy.x, dy.y, dy.z), self._gp(Lr.bkey)]))
        self._conv_backward_data(Lr, x, dy, relumask, dy_compact, gate)

    def _tune_wgrad(self, key: str, d: L.WgradDesc, wg: P.WgradPlan, hgs, tile_kernel: bool, mtiles, cgs, set_blocks):
        """The measured choice of one weight-gradient launch, as the tune cache stores it — ["m", tile] marching, ["c", hgroup] compute, [single_buffer, hgroup,
        workgroups per CU] tile kernel — and its tag.  `tile_kernel` False: a gated H operand / a compact P operand, marching kernel only."""
        cache = _tune_cache()
        if _cache_usable(key):
            return cache[key], " tuned[cache]"
        launch = functools.partial(self.eng.lib.vsseg_wgrad, C.byref(d), torch.cuda.current_stream().cuda_stream)
        delta = self._tune_gflat_delta()  # measured launches accumulate into a scratch copy of the gradient buffer, never into the live one
        live_dw, live_db = d.dw, d.dbias_p
        d.dw = live_dw + delta
        d.dbias_p = (live_db + delta) if live_db else None
        ms = {}
        for hg in (hgs if tile_kernel else []):
            for sb in (0, 1):
                for w in (2, 3, 4):
                    d.march, d.single_buffer, d.hgroup = 0, sb, hg
                    set_blocks(w)
                    ms[(sb, hg, w)] = self._time_launch(launch)
        for mt in mtiles:
            d.march, d.tile = 1, L.i3(mt)
            ms[("m", *mt)] = self._time_launch(launch)
        for g in cgs:
            d.march, d.hgroup, d.tile = 2, g, L.i3(wg.tile)
            set_blocks(4)
            ms[("c", g)] = self._time_launch(launch)
        d.dw, d.dbias_p, d.tile = live_dw, live_db, L.i3(wg.tile)
        bestk = min(ms, key=ms.get)
        cache[key] = list(bestk)
        _tune_cache.dirty = True
        return bestk, f" tuned[best of {len(ms)}: {min(ms.values()):.3f} ms, default {ms.get((0, hgs[0], 4), float('nan')):.3f}]"

    def _conv_backward_data(self, Lr: Layer, x: TensorSpec, dy: L.Tensor, relumask, dy_compact, gate):
        cp, B = self.cplans[Lr.prefix], self.bwd
        if not cp.dgrad:
            return
        acc = self._contribution(x)
        gx = self._desc(x, self.grads)
        if gate is not None:  # d(x) = conv^T(dy) + d(gated) * (1 + att): the attention gate's backward rides in this launch's epilogue
            assert acc == 0 and relumask is None and len(cp.dgrad) == 1
            self._igemm(B, cp.dgrad[0], dy, gx, res=gate[0], res_mode=L.RES_GATE, gate=gate[1])
            return
        mask = dict(res=self._desc(relumask), res_mode=L.RES_RELUMASK) if relumask is not None else dict(res=None, res_mode=L.RES_NONE)
        if len(cp.dgrad) > 1 and not any(ch.fold for ch in cp.dgrad):
            self._igemm_classes(B, cp.dgrad, dy, gx, accumulate=acc, ncls=len(cp.dgrad), **mask)
            return
        for ci, ch in enumerate(cp.dgrad):
            cc1 = self._compact_choice(ch, Lr) if (dy_compact is not None and len(cp.dgrad) == 1) else None
            if cc1 is not None:  # the one-channel gradient read compact by the marching kernel (its 8-channel zero-extension is then never written)
                cp.dgrad[ci] = ch = cc1
            self._igemm(B, ch, dy_compact if (ch.fold or cc1 is not None) else dy, gx, accumulate=acc, ncls=len(cp.dgrad), **mask)

    def _fused_backward(self, op: ConvBnAct, yd: L.Tensor, dA: L.Tensor) -> bool:
        """The layer's vsseg_bn_act_bwd_apply + data gradient + weight gradient as ONE marching launch (csrc/mbwd.hip), where it is instantiated and this
        data gradient is the first contribution to d(x) (the launch overwrites): dy is then never written.  Returns False when the layer is not eligible."""
        eng, prog = self.eng, self.eng.prog
        Lr, pre, x, b = op.layer, op.layer.prefix, op.x, self.bn[op.layer.prefix]
        if (eng.es != 2 or not Lr.stride1_3x3x1 or x.parts is not None or x.base is not None or x.kind != "act"
                or x.root.name == prog.input.name or x.c != Lr.cin or dA.ptr2):
            assert x.name not in self.gate_onload, "a unit behind an attention gate applied on load must run the fused backward"
            return False
        glx = self.gate_onload.get(x.name)  # x is an attention-gated tensor that was never materialised: the launch reads the concat and the attention map
        scr = eng.fused_scratch()  # (its own slabs: the launch runs on the main stream, concurrently with the side stream's weight gradients)
        # The ResidualUnit's 1x1x1 residual convolution of the same input (ref:params/networks/blocks/convolutions.py:241-255) rides along: its output gradient is
        # the gradient of the tensor it is added into — this block's own dA (single-subunit decoder units) or the unit's output gradient (encoder units, where
        # the add sits behind the second convolution; complete long before this launch).  Its own data- and weight-gradient launches are then skipped.
        rc = prog.residual_conv(op)
        if rc is not None and rc.layer.prefix in self.merged:  # (what the plan merged into another convolution is the plan's question, not the graph's)
            rc = None
        sink = next((o for o in prog.ops if rc is not None and isinstance(o, ConvBnAct) and o.res is rc.out), None)
        dres = None
        if rc is not None and sink is not None and (Lr.cout == 32 or Lr.cin > Lr.cout) and rc.layer.prefix in self._folded_bias:
            dres = dA if sink is op else self._grad_of_out(sink.out)
            if dres.ptr2 or dres.dtype != L.BF16 or dres.c != Lr.cout or not P.fused_bwd_tiles(Lr.cout, Lr.cin, self.lv[Lr.level], self.n, scr.numel(), res=True):
                dres = None
        tiles = P.fused_bwd_tiles(Lr.cout, Lr.cin, self.lv[Lr.level], self.n, scr.numel(), res=dres is not None)
        cls = P.lattice_classes("conv_dgrad", Lr.kernel, Lr.stride)[0]
        mps = P.march_plans("conv_dgrad", Lr.wshape, cls, self.lv[Lr.level], eng.es, Lr.cout, Lr.cin, Lr.cout, self.n)  # (the packed-weight layout of the data gradient)
        if not tiles or not mps or self._written.get(x.root.name) or (glx is not None and dres is None):
            assert glx is None, "a unit behind an attention gate applied on load must run the fused backward with its residual convolution"
            return False
        assert self._contribution(x) == 0
        mp = mps[0]
        mp.pack_map = P.pack_map(mp, Lr.wshape)
        ch = _Choice([mp], eng.layout.param_off[Lr.wkey][0], wshape=tuple(Lr.wshape))
        self._register(ch, mp)
        d = L.ConvBwdDesc()
        d.y, d.dout, d.x, d.dx = yd, dA, self._desc(glx.x if glx is not None else x), self._desc(x, self.grads)
        if glx is not None:
            d.x_gate = self._alloc(glx.att, self.bufs).data_ptr()
        d.mean, d.invstd, d.gamma, d.scale, d.shift, d.alpha = b.mean, b.invstd, b.gamma, b.scale, b.shift, b.alpha
        d.mean_dz, d.mean_dzx, d.p_drop, d.keep = b.mean_dz, b.mean_dzx, self.p_drop, b.keep
        d.dw = self._gp(Lr.wkey)
        d.scratch, d.scratch_elems = scr.data_ptr(), scr.numel()
        self._wpack_fixups.append((d, "wpack", ch.map_off))
        res_tag = ""
        if dres is not None:
            rp = P.residual_dgrad_pack_plan(rc.layer.wshape, self.lv[Lr.level])
            rch = _Choice([rp], eng.layout.param_off[rc.layer.wkey][0], wshape=tuple(rc.layer.wshape))
            self._register(rch, rp)
            d.dres, d.dw_res = dres, self._gp(rc.layer.wkey)
            self._wpack_fixups.append((d, "wpack_res", rch.map_off))
            self._absorbed_res.add(rc.layer.prefix)
            res_tag = f" +res[{'dA' if sink is op else 'unit dA'}]"
        tile, tuned = tiles[0], ""
        if self.tune and len(tiles) > 1:
            key = f"fbwd|w{tuple(Lr.wshape)}|q{self.lv[Lr.level]}|n{self.n}" + ("|res" if res_tag else "") + ("|xg" if glx is not None else "")
            tile, tuned = self._tune_fused_backward(key, d, tiles, mp.pack_map.size, bool(res_tag))
        d.tile = L.i3(tile)
        nq = float(self._vox(Lr.level))
        meta = dict(tag=f"{pre[-40:]} q={self.lv[Lr.level]} cin={Lr.cin} cout={Lr.cout} tile={tuple(tile)}{res_tag}{tuned}", name=f"mbwd<bf16,{Lr.cout // 16},{Lr.cin // 16}>", kind="mfma",
                    flops=2.0 * 2.0 * nq * (10 if res_tag else 9) * Lr.cin * Lr.cout, bytes=eng.es * nq * ((3 if res_tag.endswith("[unit dA]") else 2) * Lr.cout + 2 * Lr.cin) + nq * Lr.cout / 8)
        self.bwd.append(Launch(eng.lib.vsseg_conv_bwd_fused, [C.byref(d)], meta, desc=d))
        return True

    def _tune_fused_backward(self, key: str, d: L.ConvBwdDesc, tiles, npack: int, res: bool):
        """The fastest tile of one fused backward launch and its tag: from the tune cache, else measured on the real buffers — packed weights in a
        temporary, the weight gradient(s) accumulating into a scratch copy of the gradient buffer."""
        eng, cache = self.eng, _tune_cache()
        if _cache_usable(key):
            return tuple(cache[key]), " tuned[cache]"
        launch = functools.partial(eng.lib.vsseg_conv_bwd_fused, C.byref(d), torch.cuda.current_stream().cuda_stream)
        delta = self._tune_gflat_delta()
        wp = torch.zeros(npack + 8192, dtype=eng.tdtype, device=eng.device)
        live_dw, live_dw_res = d.dw, d.dw_res
        d.dw, d.wpack = live_dw + delta, wp.data_ptr()
        if res:
            d.dw_res, d.wpack_res = live_dw_res + delta, wp.data_ptr() + eng.es * npack
        ms = {}
        for t in tiles:
            d.tile = L.i3(t)
            ms[t] = self._time_launch(launch)
        d.dw = live_dw
        if res:
            d.dw_res = live_dw_res
        tile = min(ms, key=ms.get)
        cache[key] = list(tile)
        _tune_cache.dirty = True
        return tile, f" tuned[best of {len(ms)}: {ms[tile]:.3f} ms]"

    def _fused_narrow(self, op: ConvBnAct, yd: L.Tensor, dA: L.Tensor) -> bool:
        """The 1 -> C 3x3x1 block on the network input (no data gradient): vsseg_bn_act_bwd_apply is applied on load by the narrow weight-gradient reduction."""
        Lr, pre, b = op.layer, op.layer.prefix, self.bn[op.layer.prefix]
        if (self.eng.es != 2 or not Lr.stride1_3x3x1 or Lr.cin != 1 or Lr.cout not in (8, 16, 32, 64)
                or op.x.root.name != self.eng.prog.input.name or self.lv[Lr.level][1] % 4 or dA.ptr2 or dA.c != Lr.cout):
            return False
        x1 = self._xdesc(op.x, True)  # the compact one-channel copy of the network input
        scr = self.eng.wgrad_scratch()
        self.bwd.append(Launch(self.eng.lib.vsseg_wgrad_narrow_bn, [yd, dA, b.keep, b.mean, b.invstd, b.gamma, b.scale, b.shift, b.alpha, b.mean_dz, b.mean_dzx,
                                                                    self.p_drop, x1.ptr, self._gp(Lr.wkey), 9, scr.data_ptr(), scr.numel()],
                               dict(name="wgrad_narrow", kind="hbm", flops=0.0, bytes=float(self.eng.es) * self._vox(Lr.level) * (2 * Lr.cout + 1) + self._vox(Lr.level) * Lr.cout / 8, tag=f"{pre[-40:]} 1->{Lr.cout} k={Lr.kernel} +bn on load"), side=True))
        return True

    def _bwd_conv_bn_act(self, op: ConvBnAct):
        eng, lib, B = self.eng, self.eng.lib, self.bwd
        Lr, pre, b = op.layer, op.layer.prefix, self.bn[op.layer.prefix]
        seed, written = self.seed_dev.data_ptr(), self._written
        yd = self._tdesc(self.bufs["y:" + pre], Lr.out_level)
        dA = self._grad_of_out(op.out)
        B.append(Launch(lib.vsseg_bn_act_bwd_reduce, [yd, dA, b.mean, b.invstd, b.gamma, b.beta, b.scale, b.shift, b.alpha, self.p_drop, seed, b.salt, b.stats_bwd, b.cpad, b.slope, b.keep],
                        self._ew_meta("bn_act_bwd_reduce", Lr.out_level, 2 * Lr.cout)))
        pr = eng.prog.producer(op.res) if op.res is not None else None  # residual conv: d(out)/d(res) = 1, its bias gradient is sum(dA) (reduced above)
        if pr is not None:
            self._folded_bias.add(pr.layer.prefix)
        B.append(Launch(lib.vsseg_bn_act_bwd_finalize, [b.stats_bwd, b.cpad, b.slope, Lr.cout, float(self._vox(Lr.out_level)), self._gp(pre + ".norm.weight"), self._gp(pre + ".norm.bias"),
                                                        self._gp(pre + ".act.weight"), b.mean_dz, b.mean_dzx, self._gp(pr.layer.bkey) if pr is not None else None]))
        if pr is not None and eng.early_res_wgrad == "1":
            # The 1x1x1 residual convolution of the network input (first ResidualUnit): its weight gradient needs d(out) of the unit only — which exists from here on — but in list
            # order it came LAST, behind the unit's first block, where nothing else is left to run beside it (0.13 ms at the end of the step with the main stream idle,
            # profiles/r06_loss_phase.txt's run).  Issued here it shares the GPU with the unit's own backward instead.
            if pr.layer.cin == 1 and pr.x.root.name == eng.prog.input.name and pr.layer.prefix not in self.merged and pr.act != "sigmoid":
                self._conv_backward(pr.layer, pr.x, dA, bias_grad=pr.layer.prefix not in self._folded_bias)
                self._early_res.add(pr.layer.prefix)
        fused = (op.res is None or op.res.name.endswith(":res")) and (self._fused_backward(op, yd, dA) or self._fused_narrow(op, yd, dA))  # (an identity residual re-uses dA's buffer below: keep those unfused)
        if not fused:
            dyd = self._tdesc(self._raw("dy:" + pre, Lr.out_level, Lr.cout), Lr.out_level)
            B.append(Launch(lib.vsseg_bn_act_bwd_apply, [yd, dA, b.mean, b.invstd, b.gamma, b.beta, b.scale, b.shift, b.alpha, self.p_drop, seed, b.salt, b.mean_dz, b.mean_dzx, dyd, b.keep],
                            self._ew_meta("bn_act_bwd_apply", Lr.out_level, 3 * Lr.cout)))
        if op.res is not None and not op.res.name.endswith(":res"):  # identity residual: d(res) += d(out)
            r, o = op.res, self._grad_alias.get(op.out.name, op.out)
            if (r.parts is None and r.base is None and o.parts is None and o.base is None and r.kind == o.kind == "act" and (r.level, r.c) == (o.level, o.c)
                    and not written.get(r.name) and r.name not in self.grads and o.name in self.grads):
                # first contribution to d(res), and d(out) is dead from here on (reduce / apply above were its last readers): d(res) IS the
                # buffer of d(out) — later contributions accumulate into it in place — instead of a copy of it (one tensor round trip less)
                self.grads[r.name] = self.grads[o.name]
                written[r.name] = True
            elif self._contribution(op.res):
                B.append(Launch(lib.vsseg_add_inplace, [self._desc(op.res, self.grads), dA], self._ew_meta("grad_add/copy", Lr.out_level, 3 * Lr.cout)))
            else:
                B.append(Launch(lib.vsseg_copy_cast, [dA, self._desc(op.res, self.grads)], self._ew_meta("grad_add/copy", Lr.out_level, 2 * Lr.cout)))
        if not fused:
            self._conv_backward(Lr, op.x, dyd, bias_grad=False, own_dy=True)  # a bias in front of a training-mode BatchNorm has zero gradient

    def _bwd_conv_plain(self, op: ConvPlain):
        Lr, prog = op.layer, self.eng.prog
        if Lr.prefix in self.merged:  # gradients of a merged residual conv = centre-tap slice / bias gradient of the absorbing conv
            big = self.merged[Lr.prefix].layer
            kx, ky, kz = big.kernel
            centre = ((kx // 2) * ky + ky // 2) * kz + kz // 2
            self.bwd.append(Launch(self.eng.lib.vsseg_merge_residual_grads, [self._gp(big.wkey), self._gp(big.bkey), self._gp(Lr.wkey), self._gp(Lr.bkey), Lr.cout, Lr.cin, kx * ky * kz, centre],
                                   dict(name="vsseg_merge_residual_grads", kind="hbm", flops=0.0, bytes=0.0), side=True))
            return
        if Lr.prefix in self._early_res:  # issued with the unit's last block (_bwd_conv_bn_act)
            return
        if Lr.prefix in self._absorbed_res:  # data + weight gradient came out of the fused launch of the unit's 3x3x1 block (csrc/mbwd.hip, RES); bias gradient: _folded_bias
            return
        assert op.res is None or op.res.name.endswith(":res"), "identity residual on a plain convolution is not part of this network"
        dyc = self._tdesc(self.bufs["dpre1:" + op.out.name], Lr.level) if (op.act == "sigmoid" and ("dpre1:" + op.out.name) in self.bufs) else None
        if op.act != "sigmoid" and op.out.name == prog.logits.name and self._logits_compact(Lr, op.x):
            dyc = self._logits_grad(True)  # both launches of the logits convolution read the two-channel gradient compact (4 bytes per voxel instead of 16)
        dy = (self._tdesc(self.bufs["dpre:" + op.out.name], Lr.level) if ("dpre:" + op.out.name) in self.bufs else dyc) if op.act == "sigmoid" else (dyc if dyc is not None else self._grad_of_out(op.out))
        relu_in = prog.producer(op.x)  # the convolution + ReLU that wrote this one's input: its output is the mask of the data gradient
        self._conv_backward(Lr, op.x, dy, bias_grad=Lr.prefix not in self._folded_bias, relumask=relu_in.out if (relu_in is not None and relu_in.act == "relu") else None, dy_compact=dyc, gate=self._gate_fuse.get(Lr.prefix))

    def _bwd_att_gate(self, op: AttGate):
        prog, dev = self.eng.prog, self.eng.device
        gout = self._grad_of_out(op.out)
        # The gate's d(x) = d(gated) * (1 + att) and the data gradient of the attention branch's first convolution (relu
        # conv on the same x) both flow into d(x): fused, the gate kernel skips its full-width d(x) store and the igemm
        # launch reads d(gated) where it would have read-modify-written d(x) (one tensor pass less per level).
        c1 = next((o for o in prog.ops if isinstance(o, ConvPlain) and o.act == "relu" and o.x is op.x), None)
        xs = op.x.parts if op.x.parts else (op.x,)
        if c1 is not None and len(self.cplans[c1.layer.prefix].dgrad) == 1 and not any(self._written.get(t.root.name) for t in xs):
            self._gate_fuse[c1.layer.prefix] = (gout, self._alloc(op.att, self.bufs).data_ptr())
            acc = 2  # att_apply_bwd: do not write d(x)
        else:
            acc = self._contribution(op.x)
        sigop = prog.producer(op.att)
        sig = sigop.layer  # the sigmoid convolution (its bias gradient sum(dpre) is reduced by its weight-gradient launch, in a fixed order)
        want_c1 = sig.kernel in ((3, 3, 1), (1, 1, 1)) and sig.cin in (8, 16, 32, 64) and self.lv[sig.level][1] % 4 == 0
        dpre1 = self._raw("dpre1:" + op.att.name, op.att.level, 1).data_ptr() if want_c1 else None  # compact copy of d(pre-sigmoid): z-folded data gradient / narrow weight gradient
        # the 8-channel zero-extension of d(pre-sigmoid) (16 bytes per voxel for 2 real ones) is written only if a launch reads it: not when the sigmoid convolution's
        # weight gradient is the narrow reduction and its data gradient reads the compact copy (marching kernel, csrc/mconv.hip C1)
        cps = self.cplans[sig.prefix]
        all_compact = (want_c1 and not sig.transposed and tuple(sig.stride) == (1, 1, 1) and sigop.x.parts is None and sigop.x.base is None and len(cps.dgrad) == 1
                       and self._compact_choice(cps.dgrad[0], sig) is not None)
        dpre = None if all_compact else self._raw("dpre:" + op.att.name, op.att.level, 16 if sig.prefix in self.wide_dpre else 8)  # (channels 8..15 of the wide rows are never written: zero)
        gbuf = self.gatt_buf[op.att.name] = torch.zeros((self.n, *self.lv[op.att.level]), dtype=torch.float32, device=dev)  # the loss' gradient of this attention map is staged here
        self.bwd.append(Launch(self.eng.lib.vsseg_att_apply_bwd, [self._desc(op.x), self._alloc(op.att, self.bufs).data_ptr(), gout, gbuf.data_ptr(), self._desc(op.x, self.grads), acc, self._dpre_desc(dpre, op.att.level) if dpre is not None else L.Tensor(), None, dpre1],
                               self._ew_meta("att_apply_bwd", op.x.level, (2 if acc == 2 else (4 if acc else 3)) * op.x.c + (8 if dpre is not None else 1) + 4)))

    def _move_late_wgrads(self):
        """The LAST weight-gradient launches of the list leave the side stream for the END of the main stream's list: the step ends with the first block's chain
        (statistics pass -> finalize -> narrow weight gradient, ~0.7 ms) in which the main stream has nothing left to issue and the side stream runs one VALU-bound
        launch; weight gradients that would have shared the GPU with the main stream's last convolutions run beside that launch instead.  Only launches whose operands
        nothing writes again (P = the block's own dy buffer, H = a forward activation); their slabs go to the main stream's scratch (the fused launches are done by then)."""
        eng, lib, B = self.eng, self.eng.lib, self.bwd
        if eng.late_wgrad <= 0:
            return
        late = [la for la in B if la.side and la.own_dy and la.fn is lib.vsseg_wgrad][-eng.late_wgrad:]
        if eng.early_res_wgrad == "late":  # + the first unit's 1x1x1 residual-convolution weight gradient (the last launch of the side stream's list)
            late += [la for la in B if la.late_ok and la.fn is lib.vsseg_wgrad_narrow]
        fs = eng.fused_scratch()
        for la in late:
            if la.fn is lib.vsseg_wgrad:
                la.desc.scratch, la.desc.scratch_elems = fs.data_ptr(), fs.numel()
            else:
                la.args[la.scratch_at:la.scratch_at + 2] = [fs.data_ptr(), fs.numel()]
            la.side, la.late = False, True
        B[:] = [la for la in B if not la.late] + late

    def _index_slots(self):
        self.ext_slots = []
        for lst in (self.fwd, self.bwd, self.bwd_pre):
            for launch in lst:
                for i, a in enumerate(launch.args):
                    if isinstance(a, _Slot):
                        assert lst is self.bwd_pre, "a captured launch list may not depend on caller-owned memory"
                        self.ext_slots.append((launch.args, i, a))

    # ------------------------------------------------------------------ run
    def set_seed(self, seed: int, stream=None):
        stream = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        L.check(self.eng.lib.vsseg_store_u64(self.seed_dev.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, stream), "store_u64")

    def set_external_grads(self, glogits: L.Tensor, gatt: Dict[str, Optional[int]], stream=None):
        """glogits: descriptor of the loss' fp32 gradient of the logits (read by the eager prelude); gatt: device address of the fp32
        gradient of each attention map (or None), copied into the plan-owned buffers the captured backward reads."""
        stream = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        lib = self.eng.lib
        for args, i, slot in self.ext_slots:
            args[i] = glogits
        for name, buf in self.gatt_buf.items():
            src = gatt.get(name)
            nbytes = buf.numel() * 4
            if src is not None:
                L.check(lib.vsseg_copy_bytes(src, buf.data_ptr(), nbytes, stream), "copy_bytes")
                self._gatt_set[name] = True
            elif self._gatt_set.get(name):  # no external gradient this time: back to zeros
                L.check(lib.vsseg_memset_zero(buf.data_ptr(), nbytes, stream), "memset_zero")
                self._gatt_set[name] = False

    def grad_landing(self):
        """Where a loss that runs between this plan's forward and backward may write its gradients itself (the fused train step, vs_seg_amd.parallel):
        the descriptor the eager prelude stages the gradient of the logits in (compute dtype; compact two channels, or the first two of VSSEG_ZERO_PADDED rows
        of 8) and, per attention map in the network's order, the fp32 buffer the captured backward reads (None: that map has no gradient path)."""
        assert self.train and getattr(self, "glogits_dst", None) is not None, "no backward was lowered for this plan"
        return self.glogits_dst, [self.gatt_buf.get(spec.name) for spec in self.eng.prog.att_maps]

    def grads_landed(self, att_written, stream=None):
        """The loss wrote the staged gradient of the logits and the attention-map buffers named in `att_written` in place: what set_external_grads + the
        eager prelude would have copied is already there.  Buffers of maps without a gradient this time go back to zeros."""
        stream = stream if stream is not None else torch.cuda.current_stream().cuda_stream
        for name, buf in self.gatt_buf.items():
            if name in att_written:
                self._gatt_set[name] = True
            elif self._gatt_set.get(name):
                L.check(self.eng.lib.vsseg_memset_zero(buf.data_ptr(), buf.numel() * 4, stream), "memset_zero")
                self._gatt_set[name] = False

    def zero_stats(self, stream, row=None):
        """Zero the sharded fp64 statistics (both rows before a training forward, the backward row before a backward)."""
        t = self.stats if row is None else self.stats[row]
        L.check(self.eng.lib.vsseg_memset_zero(t.data_ptr(), t.numel() * t.element_size(), stream), "memset_zero")

    def pack_weights(self, stream):
        m2 = self.pack_map2.data_ptr() if self.pack_map2 is not None else None
        L.check(self.eng.lib.vsseg_gather_cast(self.eng.flat.data_ptr(), self.pack_map.data_ptr(), m2, self.wpack.data_ptr(), self.pack_map.numel(), L.BF16 if self.eng.es == 2 else L.F32, stream), "gather_cast")

    def run(self, lst, stream, graph_key: Optional[str] = None):
        tm, timed = self.timer, None
        if tm is not None and tm["only"] is None:  # the per-kernel profile: every launch between two events
            timed = "all"
        # tm with a set of names (bench.py's timed region: the dominant kernel's launches measured live): the product's schedule — hipGraph replay of the lists that hold none
        # of those launches, bound forks in the eager ones — with two events around the named launches only
        elif tm is not None and tm.get("active", True) and any(la.name in tm["only"] for la in lst):
            timed = tm["only"]
        if graph_key is not None and self.eng.use_graphs and timed is None and not (self.eng.overlap and any(la.side for la in lst)):
            g = self._graphs.get(graph_key)
            if g is not None:
                g.replay()
                return
            runs = self._graph_runs[graph_key] = self._graph_runs.get(graph_key, 0) + 1
            if runs > 2:  # two eager runs first: plan measurement, tile-descriptor tables, function attributes are all settled
                try:
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g):
                        self._run_eager(lst, torch.cuda.current_stream().cuda_stream)
                    self._graphs[graph_key] = g
                    g.replay()  # the capture recorded the launches without executing them
                    return
                except RuntimeError as e:  # capture is an optimisation of HOW the same kernels are launched: fall back to the eager loop, loudly
                    import warnings

                    self._graphs.pop(graph_key, None)
                    if isinstance(e, L.VssegError) and not e.during_capture:  # the library rejected a launch (bad arguments, a real launch failure): an error of the step,
                        raise                                                  # not of the capture — only calls HIP refuses BECAUSE the stream is capturing fall back
                    torch.cuda.synchronize()
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError(f"vs_seg_amd: hipGraph capture of the {graph_key} launch list failed ({e}) and left the stream capturing") from e
                    warnings.warn(f"vs_seg_amd: hipGraph capture of the {graph_key} launch list failed ({e}); launching eagerly")
                    self.eng.use_graphs = False
        self._run_eager(lst, stream, timed)

    def _run_eager(self, lst, stream, timed=None):
        """Launches in list order on `stream` (torch's current stream).  With Engine.overlap, the launches with Launch.side — the weight
        gradients, which nothing in the backward pass reads (they feed the optimizer) — go to a second HIP stream: each forks from the main
        stream where the list places it (its operands are final there; every gradient tensor has its own buffer, so nothing later on the
        main stream overwrites them), they serialise among themselves (shared partial-sum scratch), and the main stream joins the side
        stream at the end of the list.  Under hipGraph capture the fork / join events become graph edges.
        `timed`: None, or the names of the launches that run between two HIP events (recorded on the stream the launch goes to, appended to
        Plan.timer's events), or "all"."""
        side = None
        every = timed == "all"
        # "all" is the per-kernel profile: it wants each kernel alone on the GPU, not sharing it with a concurrent weight gradient — no side stream, no fork
        overlap = self.eng.overlap and not every
        lib = self.eng.lib
        # A fork = the side stream waits for the main-stream launch in front of it.  With Engine.bound_forks that launch's kernels carry the fork's event as the stop event of
        # their own dispatch (vsseg_fork_arm: no marker packet on the main stream, whose next kernel a hipEventRecord delays by 5-8 us, 42 times per step: DESIGN 3.18)
        bound = overlap and self.eng.bound_forks and not torch.cuda.is_current_stream_capturing()
        is_side = [overlap and la.side for la in lst]
        events = self._fork_events if bound else None
        nfork, ready, n = 0, None, len(lst)  # ready: the event the launch in front of the next side launch carried
        for i, la in enumerate(lst):
            on_side = is_side[i]
            if on_side:
                if side is None:
                    side = self.eng.side_stream()
                if ready is not None:
                    L.check(lib.vsseg_stream_wait_event(side.cuda_stream, ready), "stream_wait_event")
                elif i == 0 or not is_side[i - 1]:  # (consecutive side launches share the fork of the first)
                    side.wait_stream(torch.cuda.current_stream())
                ready = None
            e0 = None
            if timed is not None and (every or la.name in timed):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(side if on_side else None)  # (None: the current stream)
            arm = bound and not on_side and i + 1 < n and is_side[i + 1]
            if arm:
                if nfork == len(events):
                    events.append(lib.vsseg_fork_event_create())
                fork = events[nfork]
                nfork += 1
                L.check(lib.vsseg_fork_arm(fork), "fork_arm")
            try:
                rc = la.fn(*la.args, side.cuda_stream if on_side else stream)
            finally:
                if arm:
                    ready = fork if lib.vsseg_fork_disarm() > 0 else None  # 0: the record launched no kernel of the library (a memset): plain fork
            if e0 is not None:
                e1.record(side if on_side else None)
                self.timer["events"].append((la.name, la.meta, e0, e1))
            if rc:
                L.check(rc, la.name)
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)

    def memory_bytes(self) -> int:
        tot = sum(t.numel() * t.element_size() for t in self.bufs.values()) + sum(t.numel() * t.element_size() for t in self.grads.values())
        return tot + self.wpack.numel() * self.wpack.element_size() + self.pack_map.numel() * 4


class Engine:
    """Owns the per-signature plans over the model's flat parameter / gradient / buffer storage."""

    def __init__(self, attention: bool, dtype: str, flat: torch.Tensor, gflat: torch.Tensor, bflat: torch.Tensor, cflat: torch.Tensor, layout: ParamLayout, hp=HP, dropout_p: Optional[float] = None, dry_run: bool = False):
        self.lib = L.lib()
        if not flat.is_cuda and not dry_run:  # dry_run: build plans on CPU to check the lowering (tests); nothing can be launched
            raise RuntimeError("vs_seg_amd: parameters are not on a GPU — this engine has no CPU path (move the model with .to('cuda'))")
        self.device = flat.device
        self.dry_run = dry_run
        # Lowering features that were environment switches while they were being measured are simply how the engine lowers now; what is left here is read from the
        # environment (A/B switches that tests, tools or measurements still use) or turned off by the CPU dry run.
        self.tune_reps = int(os.environ.get("VSSEG_TUNE_REPS", "5"))  # timed launches per candidate plan (best of)
        self.fuse_classes = not dry_run  # output-parity classes of the stride-(2,2,1) level transitions as one launch (DEPTH_STREAM_SHUFFLE)
        self.compute_wgrad = os.environ.get("VSSEG_COMPUTE_WGRAD", "1") != "0"  # A/B switch of round 6: the compute weight-gradient kernel (csrc/cwgrad.hip) as a candidate for the 3x3x3 layers of levels 2-3
        self.wide_dpre = os.environ.get("VSSEG_WIDE_DPRE", "1") != "0"  # A/B switch of round 6: 16-channel rows for d(pre-sigmoid) of the 3x3x3 sigmoid convolutions (compute-kernel data gradient)
        self.early_res_wgrad = os.environ.get("VSSEG_EARLY_RES_WGRAD", "late")  # round 6, where the first unit's 1x1x1 residual-convolution weight gradient runs: "late" = with the late launches (next line), "1" = with the unit's last block, "0" = last on the side stream
        self.late_wgrad = int(os.environ.get("VSSEG_LATE_WGRAD", "1"))  # the last N tile / marching / compute weight-gradient launches run at the end of the main stream's list (see the end of the backward lowering)
        self.bound_forks = os.environ.get("VSSEG_BOUND_FORKS", "1") != "0"  # round 6: the side stream forks on events bound to the main-stream kernels' own completion (no marker packets); 0: hipEventRecord per fork
        self.transition = os.environ.get("VSSEG_TRANSITION", "1") != "0"  # A/B switch of round 6: the level 2 <-> 3 transition kernel (csrc/tconv.hip, DEPTH_TRANSITION)
        self.narrow_fwd = os.environ.get("VSSEG_NARROW_FWD", "1") != "0"  # A/B switch of round 6: the C -> 1 attention convolutions of levels 0-1 on the vector ALUs (csrc/nconv.hip)
        self.chain = os.environ.get("VSSEG_CHAIN", "1")  # inference: pairs of 3x3x1 convolutions as one launch, the tensor between them in LDS (csrc/chain.hip); "0": off, "l0": level 0 only
        self.compact_c1 = not dry_run  # one-real-channel convolution inputs read compact by the marching kernel (csrc/mconv.hip C1)
        self.resn = not dry_run  # forward: the unit's 1x1x1 residual convolution as extra output tiles of its first 3x3x1 convolution
        # the deep-level kernel (csrc/dconv.hip, DEPTH_DEEP plans) on the small launches of levels 3-5: "1" = a candidate the tuner measures, "0" = off, "force" = every launch
        # it is offered for runs on it (the untuned lowering then too: how the tests send a whole network through it)
        self.deep = os.environ.get("VSSEG_DEEP", "1")
        # weight gradients on a second HIP stream, concurrent with the data-gradient chain: on the deep levels neither chain fills the 256 CUs
        # (145 launches of 20-50 us), together they do: 37.3 -> 36.1 ms per step (tools/time_step.py).  The backward list is then launched
        # eagerly: replayed as ONE hipGraph the two branches ran no faster than serially (measured 37.6 ms)
        self.overlap = os.environ.get("VSSEG_OVERLAP", "1") == "1" and not dry_run
        # (ALL weight gradients go to the side stream: they share one partial-sum scratch and must serialise on one stream; keeping the finest
        # levels on the main stream measured slower anyway, 37.0 / 37.1 / 37.6 / 37.9 ms for side-stream levels >= 0 / 1 / 2 / 3)
        self._side = None
        self.use_graphs = os.environ.get("VSSEG_GRAPHS", "1") != "0" and not dry_run  # replay the launch lists as hipGraphs after two eager runs
        self.attention, self.hp = attention, hp
        self.tdtype = {"bf16": torch.bfloat16, "fp32": torch.float32}[dtype]
        self.es = 2 if dtype == "bf16" else 4
        self.flat, self.gflat, self.bflat, self.cflat, self.layout = flat, gflat, bflat, cflat, layout
        self.prog: Program = build_program(attention, hp)
        self.dropout_p = hp["dropout"] if dropout_p is None else dropout_p
        self.plans: Dict[tuple, Plan] = {}

    def side_stream(self) -> "torch.cuda.Stream":
        if self._side is None:
            from ._streams import side_stream  # the process-wide pool: the sliding-window lanes reuse this stream instead of adding a fifth one (see _streams.py)

            self._side = side_stream(self.device, 0)
        return self._side

    def wgrad_scratch(self) -> torch.Tensor:
        if getattr(self, "_wg_scratch", None) is None:
            self._wg_scratch = torch.zeros(48 * 1024 * 1024, dtype=torch.float32, device=self.device)  # 192 MB of partial-sum slabs, shared by all layers
        return self._wg_scratch

    def fused_scratch(self) -> torch.Tensor:
        if getattr(self, "_fb_scratch", None) is None:
            self._fb_scratch = torch.zeros(48 * 1024 * 1024, dtype=torch.float32, device=self.device)  # partial-sum slabs of the fused backward launches (main stream)
        return self._fb_scratch

    def plan(self, n, dims, train, slot: int = 0) -> Plan:
        """The lowered launch lists + activation buffers for one (batch, size, mode).  `slot` > 0: a further, independent set of buffers for
        the same signature (eval forwards issued on different HIP streams run concurrently: sliding-window windows, inferers.py)."""
        key = (int(n), tuple(int(d) for d in dims), bool(train), int(slot))
        pl = self.plans.get(key)
        if pl is None:
            for d, m in zip(key[1], self.min_multiple()):
                if d % m:
                    raise ValueError(f"spatial size {key[1]} must be a multiple of {self.min_multiple()} (product of the network strides)")
            pl = self._lower_rank0_first(key) if train else Plan(self, *key[:3])
            self.plans[key] = pl
        return pl

    def _lower_rank0_first(self, key) -> Plan:
        """Data parallel: rank 0 lowers the training plan (measuring whatever the shipped / cached plans do not cover), broadcasts its measured
        choices, and the other ranks lower from those — every rank then runs the same kernels with the same memory footprint, and the step stays
        bit-reproducible across ranks and processes.  Training plans only: every rank creates them at the same step (DataParallelTrainer), which an
        eval plan (a rank without test cases never lowers one) does not guarantee.  Single process: plain lowering.

        COLLECTIVE: under data parallel the first train-mode forward of a (batch, size) signature issues a broadcast, so every rank must reach it (they do: the
        trainer steps in lock step).  If rank 0 fails while lowering (out of memory, a rejected launch) it broadcasts the error instead of its plan choices and every
        rank raises — nobody is left waiting in the broadcast until the RCCL timeout; ranks whose VSSEG_AUTOTUNE mode differs from rank 0's are an error, too."""
        import torch.distributed as dist

        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) or self.dry_run:
            return Plan(self, *key[:3])
        mode = os.environ.get("VSSEG_AUTOTUNE", "1")
        if dist.get_rank() == 0:
            msg = dict(mode=mode, error=None, cache=None)
            pl = None
            try:
                pl = Plan(self, *key[:3])
                if mode != "0":
                    msg["cache"] = dict(_tune_cache())
            except BaseException as e:  # (re-raised below, after the other ranks have been told)
                msg["error"] = f"{type(e).__name__}: {e}"
                dist.broadcast_object_list([msg], src=0)
                raise
            dist.broadcast_object_list([msg], src=0)
            return pl
        box = [None]
        dist.broadcast_object_list(box, src=0)
        msg = box[0]
        if msg["error"] is not None:
            raise RuntimeError(f"vs_seg_amd: rank 0 failed while lowering the training plan {key[:3]}: {msg['error']}")
        if msg["mode"] != mode:
            raise RuntimeError(f"vs_seg_amd: VSSEG_AUTOTUNE differs between ranks (rank 0: {msg['mode']!r}, rank {dist.get_rank()}: {mode!r}): the ranks would run different kernels")
        if msg["cache"] is not None:
            _tune_cache().update(msg["cache"])
        return Plan(self, *key[:3])

    def min_multiple(self):
        m = [1, 1, 1]
        for s in self.hp["strides"]:
            m = [a * b for a, b in zip(m, s)]
        return tuple(m)
