"""One line per launch of a plan's four lists (fwd_pre, fwd, bwd_pre, bwd): function, arguments, then in braces the reporting metadata and the scheduling flags that
are set; ctypes descriptors field by field.  Two trees lower the same
launches exactly when their dumps are byte-identical (`diff`): `--dry-run` for the CPU plans of tests/test_host.py::test_plans_lower_on_cpu, else one model on the GPU
(`--shape NxXxYxZ [--dtype fp32] [--eval]`).  Device addresses print as `storage+byte offset` of the plan's / engine's buffer they lie in (`?`: in none of them, e.g. a
temporary; `0`: null), `_Slot` arguments as their kind."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vs_seg_amd.engine import Engine, ParamLayout, _Slot  # noqa: E402
from vs_seg_amd.graph import HP, state_manifest  # noqa: E402

BYREF = type(C.byref(C.c_int()))  # a launch's byref(descriptor) argument: shown as Launch.desc


def storages(plan):
    """(name, first byte, byte count) of every buffer a launch argument may point into."""
    eng, out = plan.eng, []
    for group in ("bufs", "grads", "gatt_buf"):
        out += [(f"{group}[{k}]", t) for k, t in getattr(plan, group).items()]
    out += [(k, getattr(plan, k, None)) for k in ("stats", "vec", "wpack", "pack_map", "seed_dev")]
    out += [(k, getattr(eng, k, None)) for k in ("flat", "gflat", "bflat", "cflat", "_wg_scratch", "_fb_scratch")]
    return [(name, t.data_ptr(), t.numel() * t.element_size()) for name, t in out if t is not None]


def address(v, ranges):
    if not v:
        return "0"
    return next((f"{name}+{v - lo}" for name, lo, nbytes in ranges if lo <= v < lo + nbytes), "?")


def show(v, ranges, ctype=None):
    if isinstance(v, _Slot):
        return f"<slot {v.kind}>"
    if isinstance(v, C.Structure):
        return type(v).__name__ + "{" + ", ".join(f"{f[0]}={show(getattr(v, f[0]), ranges, f[1])}" for f in v._fields_) + "}"
    if isinstance(v, C.Array):
        return "[" + ",".join(show(e, ranges, v._type_) for e in v) + "]"
    if ctype is C.c_void_p or v is None:
        return address(v, ranges)
    if isinstance(v, int) and not isinstance(v, bool) and v >= 1 << 40:  # a bare argument this large is an address, not a count or a salt
        return address(v, ranges)
    return repr(v)


def dump(title, plan, out):
    ranges = storages(plan)
    for lname in ("fwd_pre", "fwd", "bwd_pre", "bwd"):
        for i, launch in enumerate(getattr(plan, lname)):
            braces = dict(launch.meta or {}, **{k: True for k in ("side", "own_dy", "late_ok", "late") if getattr(launch, k)})
            print(f"{title} {lname}[{i}] {launch.fn.__name__}(" + ", ".join(show(launch.desc if isinstance(a, BYREF) else a, ranges) for a in launch.args) + ") {"
                  + ", ".join(f"{k}={braces[k]!r}" for k in sorted(braces)) + "}", file=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dry-run", action="store_true", help="the CPU plans: attention on/off x bf16/fp32, train (2, 64x32x16) and eval (1, 64x32x16)")
    ap.add_argument("--shape", default="2x128x64x32", help="NxXxYxZ of the GPU plan")
    ap.add_argument("--dtype", default="bf16", choices=("bf16", "fp32"))
    ap.add_argument("--eval", action="store_true", help="the inference plan instead of the training plan")
    args = ap.parse_args()
    if args.dry_run:
        for att in (True, False):
            for dt in ("bf16", "fp32"):
                lay = ParamLayout(state_manifest(att))
                flat = torch.zeros(lay.n_param)
                eng = Engine(att, dt, flat, torch.zeros_like(flat), torch.zeros(lay.n_buf), torch.zeros(lay.n_cnt, dtype=torch.int64), lay, dry_run=True)
                dump(f"att{int(att)}/{dt}/train", eng.plan(2, (64, 32, 16), True), sys.stdout)
                dump(f"att{int(att)}/{dt}/eval", eng.plan(1, (64, 32, 16), False), sys.stdout)
        return
    import vs_seg_amd as V

    n, *dims = (int(v) for v in args.shape.split("x"))
    torch.manual_seed(0)
    hp = {k: HP[k] for k in ("channels", "strides", "kernel_sizes", "sample_kernel_sizes")}
    model = V.UNet2d5_spvPA(dimensions=3, in_channels=1, out_channels=2, num_res_units=2, norm="batch", dropout=HP["dropout"], attention_module=True, compute_dtype=args.dtype, **hp).to("cuda:0")
    model._ensure_flat()
    plan = model._engine.plan(n, tuple(dims), not args.eval)
    torch.cuda.synchronize()
    dump(f"{args.shape}/{args.dtype}/{'eval' if args.eval else 'train'}", plan, sys.stdout)


if __name__ == "__main__":
    main()
