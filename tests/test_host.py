"""CPU tests of the host side: the C-ABI library loads and exports every declared symbol, plans lower without a GPU."""
import ctypes
import functools
import os
import re

import pytest
import torch

from vs_seg_amd import _lib as L
from vs_seg_amd.engine import Engine, ParamLayout
from vs_seg_amd.graph import build_program, state_manifest


def test_library_exports_every_declared_symbol():
    lib = L.lib()
    header = open("include/vsseg_hip.h").read()
    header = re.sub(r"static inline[^{]*\{.*?\n\}", "", header, flags=re.S)  # (the inline fixed-point encode / decode helpers are not exports)
    declared = set(re.findall(r"\b(vsseg_[a-z0-9_]+)\s*\(", header))
    assert declared == set(L.SYMBOLS), declared ^ set(L.SYMBOLS)
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.vsseg_version() >= 1


def test_invalid_descriptor_is_rejected_with_message():
    lib = L.lib()
    d = L.IgemmDesc()
    assert lib.vsseg_igemm_lds_bytes(ctypes.byref(d)) < 0
    assert b"vsseg_igemm" in lib.vsseg_last_error()


def test_kernel_selector_names_match_the_header():
    """The VSSEG_DEPTH_* values of include/vsseg_hip.h and the DEPTH_* constants of the binding are the same names with the same values."""
    header = open("include/vsseg_hip.h").read()
    declared = {name: int(val) for name, val in re.findall(r"#define\s+VSSEG_(DEPTH_[A-Z_]+)\s+\((-\d+)\)", header)}
    bound = {name: getattr(L, name) for name in dir(L) if name.startswith("DEPTH_")}
    assert declared == bound and sorted(declared.values()) == list(range(-9, 0)), (declared, bound)


def test_depth_that_selects_no_kernel_is_rejected():
    """A negative depth that is none of the VSSEG_DEPTH_* values is an error that names the value (it used to run the general kernel without prefetch)."""
    from tests import gpu_harness as H
    from vs_seg_amd import planner as P

    lib = L.lib()
    w = (16, 16, 3, 3, 3)
    pl = P.plan_igemm("conv_fwd", w, P.lattice_classes("conv_fwd", w[2:], (1, 1, 1))[0], (8, 8, 8), 2, kc_pad=16)
    d = H.igemm_desc(pl, torch.zeros(1), L.Tensor(4096, L.BF16, 16, 16, 1, 8, 8, 8), L.Tensor(8192, L.BF16, 16, 16, 1, 8, 8, 8))
    for depth in (pl.depth, L.DEPTH_NOPREFETCH):  # the descriptor is valid ...
        d.depth = depth
        assert lib.vsseg_igemm_lds_bytes(ctypes.byref(d)) > 0, lib.vsseg_last_error()
    d.depth = -10
    assert lib.vsseg_igemm_lds_bytes(ctypes.byref(d)) == L.EINVAL
    assert b"-10" in lib.vsseg_last_error()


@functools.lru_cache(maxsize=None)
def _dry_plans(att, dt):
    """The engine and its CPU-lowered train (2, 64x32x16) and eval (1, 64x32x16) plans, lowered once for the tests below."""
    lay = ParamLayout(state_manifest(att))
    flat = torch.zeros(lay.n_param)
    eng = Engine(att, dt, flat, torch.zeros_like(flat), torch.zeros(lay.n_buf), torch.zeros(lay.n_cnt, dtype=torch.int64), lay, dry_run=True)
    return eng, eng.plan(2, (64, 32, 16), True), eng.plan(1, (64, 32, 16), False)


@pytest.mark.parametrize("att", [True, False])
@pytest.mark.parametrize("dt", ["bf16", "fp32"])
def test_plans_lower_on_cpu(att, dt):
    eng, tr, ev = _dry_plans(att, dt)
    prog = build_program(att)
    n_conv = len(prog.layers)
    igemms = [r for r in tr.fwd if r.fn is eng.lib.vsseg_igemm]
    # one igemm launch per convolution: the output-parity classes of the transposed convolutions share one launch (planner.class_split_plans);
    # the merged residual conv has none and the 1-channel attention map convolutions run on the narrow kernel
    assert n_conv - 2 <= len(igemms) <= n_conv
    assert sum(1 for r in igemms if r.desc.class_split == 8) == 3 and sum(1 for r in tr.bwd if r.fn is eng.lib.vsseg_igemm and r.desc.class_split == 8) == 3
    # (bf16: the stride-1 3x3x1 blocks of the finest levels run BatchNorm-backward apply + data gradient + weight gradient as ONE launch, csrc/mbwd.hip)
    n_fused = sum(1 for r in tr.bwd if r.fn in (eng.lib.vsseg_conv_bwd_fused, eng.lib.vsseg_wgrad_narrow_bn))
    assert (n_fused >= 2) == (dt == "bf16")
    assert sum(1 for r in tr.bwd if r.fn in (eng.lib.vsseg_wgrad, eng.lib.vsseg_wgrad_narrow)) + n_fused == n_conv - len(tr.merged)  # the final 1x1x1 residual conv is merged into the final 3x3x1 conv
    assert len(tr.merged) == 1 and sum(1 for r in tr.bwd if r.fn is eng.lib.vsseg_merge_residual_grads) == 1
    assert len(ev.bwd) == 0 and len(ev.fwd) < len(tr.fwd)
    # every dropout launch reads the seed through the plan's device scalar (fixed arguments: the lists can be captured as hipGraphs)
    seeded = [r for lst in (tr.fwd, tr.bwd) for r in lst if tr.seed_dev.data_ptr() in [a for a in r.args if isinstance(a, int)]]
    assert len(seeded) == 3 * sum(1 for L_ in prog.layers if L_.has_bn) - n_fused and len(tr.bwd_pre) == 1 and len(tr.ext_slots) == 1  # (a fused launch reads the stored keep-mask: no seed)
    # the LDS request the C side computes equals the planner's (mirrored formula)
    for r in igemms[:10]:
        assert eng.lib.vsseg_igemm_lds_bytes(ctypes.byref(r.desc)) > 0


def _scratch_of(launch):
    """(pointer, element count) of a weight-gradient launch's partial-sum scratch: the descriptor's fields, or — the narrow entry point — the two arguments
    its prototype in include/vsseg_hip.h calls scratch and scratch_elems."""
    if launch.desc is not None:
        return launch.desc.scratch, launch.desc.scratch_elems
    header = re.sub(r"/\*.*?\*/", "", open("include/vsseg_hip.h").read(), flags=re.S)
    params = [p.split()[-1].lstrip("*") for p in re.search(r"\bint %s\((.*?)\);" % launch.fn.__name__, header, re.S).group(1).split(",")]
    i = params.index("scratch")
    assert params[i + 1] == "scratch_elems" and len(launch.args) == len(params) - 1  # (the runner appends the stream)
    return launch.args[i], launch.args[i + 1]


def test_launch_records_of_the_cpu_plans():
    """What the runner and Plan._move_late_wgrads rely on in a Launch: the descriptor behind the byref argument, side launches in the backward list only, and the weight
    gradients moved to the end of the main stream's list — off the side stream, on the main stream's scratch, while every other one keeps the side stream's."""
    n_late = 0
    for att in (True, False):
        for dt in ("bf16", "fp32"):
            eng, tr, ev = _dry_plans(att, dt)
            lib, fs, ws = eng.lib, eng.fused_scratch(), eng.wgrad_scratch()
            assert fs.data_ptr() != ws.data_ptr()
            for plan in (tr, ev):
                for lst in (plan.fwd_pre, plan.fwd, plan.bwd_pre, plan.bwd):
                    for la in lst:
                        assert la.desc is None or la.args[0]._obj is la.desc, la.name
                        assert not la.side or lst is plan.bwd, la.name
                        assert not la.late or lst is plan.bwd, la.name
            late = [la for la in tr.bwd if la.late]
            n_late += len(late)
            assert late and all(a is b for a, b in zip(tr.bwd[-len(late):], late))  # they are the tail of the list
            for la in tr.bwd:
                if la.fn in (lib.vsseg_wgrad, lib.vsseg_wgrad_narrow):
                    scr = fs if la.late else ws
                    assert _scratch_of(la) == (scr.data_ptr(), scr.numel()), la.name
                    assert not (la.late and la.side), la.name
                else:
                    assert not la.late, la.name
    assert n_late == 8


@pytest.mark.parametrize("att", [True, False])
def test_program_queries_agree_with_the_spelled_out_scans(att):
    """Program.producer / readers / residual_conv and Layer.stride1_3x3x1 against the scans and predicates the engine used to spell out."""
    from vs_seg_amd.graph import AttGate, ConvBnAct, ConvPlain

    prog = build_program(att)
    convs = [o for o in prog.ops if isinstance(o, (ConvBnAct, ConvPlain))]
    for Lr in prog.layers:
        assert Lr.stride1_3x3x1 == (not Lr.transposed and tuple(Lr.stride) == (1, 1, 1) and Lr.kernel == (3, 3, 1)), Lr.prefix
    assert any(Lr.stride1_3x3x1 for Lr in prog.layers) and not all(Lr.stride1_3x3x1 for Lr in prog.layers)
    # producer: every ConvPlain output, and nothing else
    plain = [o for o in prog.ops if isinstance(o, ConvPlain)]
    assert plain and all(prog.producer(o.out) is o for o in plain)
    assert all(prog.producer(o.out) is None for o in prog.ops if not isinstance(o, ConvPlain)) and prog.producer(prog.input) is None
    # residual_conv: every `.residual` convolution is found from the first convolution of its unit (same input, `unit0`) and from no other op
    residuals = [o for o in plain if o.layer.prefix.endswith(".residual")]
    assert len(residuals) == 11 and len({id(o.x) for o in residuals}) == len(residuals)  # (five encoder units, the bottom unit, five decoder units: each changes the channel count)
    found = {id(op): prog.residual_conv(op) for op in convs}
    for rc in residuals:
        unit = rc.layer.prefix[: -len(".residual")]
        first = [op for op in convs if op.layer.prefix == unit + ".conv.unit0"]
        assert len(first) == 1 and first[0].x is rc.x and found[id(first[0])] is rc
        assert [op for op in convs if found[id(op)] is rc] == first
    assert sum(1 for v in found.values() if v is not None) == len(residuals)
    # readers: of every attention-gate output, the two scans of the lowering (with and without the readers as an attention map, which a gated tensor never has)
    gates = [g for g in prog.ops if isinstance(g, AttGate)]
    assert bool(gates) == att
    for g in gates:
        scan1 = [o for o in prog.ops if isinstance(o, (ConvBnAct, ConvPlain)) and (o.x is g.out or (o.x.parts is not None and g.out in o.x.parts) or o.res is g.out)]
        scan1 += [o for o in prog.ops if isinstance(o, AttGate) and (o.x is g.out or (o.x.parts is not None and g.out in o.x.parts))]
        scan2 = [o for o in prog.ops if ((getattr(o, "x", None) is g.out) or (getattr(getattr(o, "x", None), "parts", None) is not None and g.out in o.x.parts)
                                         or getattr(o, "res", None) is g.out or getattr(o, "att", None) is g.out)]
        got = prog.readers(g.out)
        assert got and sorted(map(id, got)) == sorted(map(id, scan1)) == sorted(map(id, scan2))
        assert [o for o in prog.readers(g.att) if isinstance(o, AttGate)] == [g]  # the gate reads its attention map


def test_bad_spatial_size_raises():
    lay = ParamLayout(state_manifest(True))
    flat = torch.zeros(lay.n_param)
    eng = Engine(True, "bf16", flat, torch.zeros_like(flat), torch.zeros(lay.n_buf), torch.zeros(lay.n_cnt, dtype=torch.int64), lay, dry_run=True)
    with pytest.raises(ValueError):
        eng.plan(1, (48, 32, 8), False)


def test_shipped_tuned_plans_still_name_existing_candidates():
    """vs_seg_amd/tuned_gfx950.json (plans measured on an MI355X for the benchmark shapes) is only useful while its entries still
    match what `planner.candidate_plans` generates: a planner / kernel change that invalidates them must be noticed (the engine
    would silently fall back to measuring every launch at start-up)."""
    import ast
    import json
    import os

    from vs_seg_amd import engine as E
    from vs_seg_amd import planner as P

    data = json.load(open(E.TUNED_DEFAULTS))
    ig = {k: v for k, v in data.items() if not k.startswith(("wgrad", "use_cs", "fbwd"))}  # (use_cs|...: per-class or class-split launch, 0 / 1; fbwd|...: tile of a fused backward launch)
    assert len(ig) > 150 and sum(1 for k in data if k.startswith("wgrad")) >= 40
    checked = hits = 0
    for key, choice in list(ig.items())[::5]:
        parts = key.split("|")
        kind, fold = parts[0], int(parts[1][1:])
        wshape = ast.literal_eval(parts[2][1:])
        is_, os_, oo = (ast.literal_eval(t) for t in re.findall(r"\([^)]*\)", parts[3]))
        q = ast.literal_eval(parts[4][1:])
        es, kc = int(parts[6][2:]), int(parts[7][2:])
        acc, res, two = int(parts[8][3:]), int(parts[9][3:]), parts[11][3:]
        kernel = tuple(wshape[2:])
        cls = next((c for s in ((1, 1, 1), (2, 2, 1), (2, 2, 2)) for c in P.lattice_classes(kind, kernel, s) if (c.is_, c.os, c.oo) == (is_, os_, oo)), None)
        assert cls is not None, key
        aux_es = es if (acc or res) else 0
        if key.endswith("|cs"):  # every parity class in one launch
            kreal, nreal = P.gemm_dims(kind, wshape)
            cands = P.class_split_plans(kind, wshape, kernel, os_, q, es, kc, nreal, kreal, aux_es=aux_es)
        elif fold:
            cands = P.folded_candidate_plans(kind, wshape, cls, (q[0], q[1], q[2] * fold), es, aux_es=aux_es)
        else:
            cands = P.candidate_plans(kind, wshape, cls, q, es, kc_pad=kc, aux_es=aux_es, in_split=kc // 2 if two[0] == "1" else 0, n=int(parts[5][1:]))  # (the marching shapes depend on the batch)
        checked += 1
        want = choice if len(choice) > 4 else choice + [1]
        hits += any([list(c.tile), c.nt, c.nsplit, c.ck, c.depth] == want for c in cands)
    assert checked >= 30 and hits >= 0.9 * checked, (hits, checked)


def test_bench_refuses_more_ranks_than_gpus():
    """`python bench.py --gpus 2` outside a launcher environment starts its own ranks (bench.self_launch) — and fails loudly, before anything is
    launched, when the box has fewer GPUs than ranks (there is none in the build container)."""
    import subprocess
    import sys

    import torch

    if torch.cuda.device_count() >= 2:
        import pytest

        pytest.skip("needs a box with fewer than 2 GPUs")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "VSSEG_SHARE_DEVICE")}
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--gpus 2 but only" in p.stderr and not p.stdout.strip()
