"""Recorder of tests/golden/augmentation_replay.json: what commit 2a48986 hands to the library for given augmentation settings, and what its VSparams makes of the
17 --aug_* flags.

It uses only the surface that stays when the plumbing behind it changes (PatchSampler / RandomTail with positional and named ranges, their recorded attributes,
VSparams.get_transforms, the aug_* attributes, the four dict properties, the parser's actions and what parser.error is told), so it runs against a later tree as well
and must then write the same file byte for byte: `python tests/golden/make_augmentation_replay.py` from the repository root.  tests/test_augmentation_replay_host.py
calls `record()` and compares it with the file.

No GPU is needed.  Inside `standin()` `_lib.lib()` returns an object whose every entry point records its arguments and returns 0, `torch.cuda.current_stream()` an
object with `cuda_stream = 0`, and `Tensor.record_stream` does nothing; the cases are CPU tensors, so the staging buffer of a job table is host memory and is read back
through the pointer the launch was given.

"samplers": per configuration the constructor arguments, the tail's four dicts and flags, and per batch every library call as [entry point, arguments in the order of "call_args"] (scalars and
small arrays by value, an output pointer as "out<k>" of call k of the batch, an input pointer as the output it names, an optional scratch pointer as null / nonnull,
the staged copy of a job table as "= jobs" where it holds the bytes of the host table, every field of every job in the order of "job_fields", a job's source address
as [case, key]), `last_draws`, `last_augment` as {key: the value of every sample}, `acquisition_launches`, the shape of `last_tone_stats` and which output `sample`
returned as the image (that the label is the second half of the crop launch's output is asserted here).
Python floats are JSON numbers (exact for a double), numpy scalars "f32:<value>" and the like, arrays {dtype, shape, v}; an fp32 value, a `float` field of a job included,
is written as the shortest decimal that rounds to it, which names it exactly.
"params": per argv the three dicts of get_transforms(), the aug_* attributes and the four properties.  "flags": the parser actions.  "rejected": the text parser.error got."""
import argparse
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd import params as P  # noqa: E402
from vs_seg_amd.data import transforms as T  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "augmentation_replay.json")
BASE = ["--data_root", "/data", "--results_folder_name", "t"]
ROI, SHAPES, BATCHES = (32, 32, 8), ((40, 36, 12), (36, 40, 10), (33, 37, 9)), ((0, 1), (2, 0), (1, 2))
AUG = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.2, intensity_shift=0.3, noise_std=0.05)
FIELD = dict(elastic_mag=3.0, bias_field=0.3, field_spacing=16)
APP = dict(blur_sigma=1.0, lowres=0.5, contrast=0.25, gamma=0.3)
ACQ = dict(thick_slices=3, ghost=0.5, spike=1.0)
FLAG_KEYS = tuple(AUG) + tuple(FIELD) + tuple(APP) + ("appearance_prob",) + tuple(ACQ) + ("acquisition_prob",)

# the arguments of the entry points in the order of include/vsseg_hip.h: (name, kind)
CALLS = dict(
    vsseg_crop_flip=(("jobs_dev", L.CropJob), ("njobs", "value"), ("dst", "out"), ("roi", "i3"), ("stream", "value")),
    vsseg_crop_affine=(("jobs", "jobs"), ("jobs_dev", "staged"), ("njobs", "value"), ("dst", "out"), ("roi", "i3"), ("seed", "value"), ("stream", "value")),
    vsseg_crop_field=(("jobs", "jobs"), ("jobs_dev", "staged"), ("njobs", "value"), ("dst", "out"), ("roi", "i3"), ("spacing", "i3"), ("seed", "value"), ("stream", "value")),
    vsseg_patch_acquisition=(("jobs", "jobs"), ("jobs_dev", "staged"), ("njobs", "value"), ("src", "in"), ("dst", "out"), ("scratch", "optional"), ("roi", "i3"), ("stream", "value")),
    vsseg_patch_filter=(("jobs", "jobs"), ("jobs_dev", "staged"), ("njobs", "value"), ("src", "in"), ("dst", "out"), ("scratch", "optional"), ("roi", "i3"), ("stream", "value")),
    vsseg_patch_tone=(("jobs", "jobs"), ("jobs_dev", "staged"), ("njobs", "value"), ("img", "in"), ("numel", "value"), ("stats", "out"), ("work", "optional"), ("stream", "value")),
)
JOBS = dict(vsseg_crop_flip=L.CropJob, vsseg_crop_affine=L.AffineJob, vsseg_crop_field=L.FieldJob, vsseg_patch_acquisition=L.AcquisitionJob, vsseg_patch_filter=L.FilterJob, vsseg_patch_tone=L.ToneJob)


def f32(v) -> float:
    """The shortest decimal that rounds to the fp32 value v (numpy's own text for a float32): it names that value exactly and is a third as long as its double."""
    return float(str(np.float32(v)))


def enc(v):
    """A value as JSON that keeps its type and its exact value."""
    if isinstance(v, np.ndarray):
        return dict(dtype=str(v.dtype), shape=list(v.shape), v=[f32(x) for x in v.ravel()] if v.dtype == np.float32 else v.ravel().tolist())
    if isinstance(v, (np.floating, np.integer)):
        return f"{v.dtype.kind}{8 * v.dtype.itemsize}:{str(v)}"
    if isinstance(v, (np.bool_, bool)):
        return bool(v)
    if isinstance(v, dict):
        return {k: enc(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return [enc(x) for x in v]
    assert v is None or isinstance(v, (int, float, str)), type(v)
    return v


class Recorder:
    """Stands in for the loaded library: every entry point records what it was called with and returns 0."""

    def __init__(self):
        self.calls, self.named, self.sources = [], {}, {}

    def begin_batch(self):
        self.calls, self.named = [], {}

    def job(self, j):
        out = []  # in the order of "job_fields"
        for name, ctype in j._fields_:
            v = getattr(j, name)
            if name == "src":
                out.append(self.sources.get(v))  # (None: a tensor the recording was not told about)
            elif isinstance(v, C.Array):
                out.append([f32(x) for x in v] if ctype._type_ is C.c_float else list(v))
            else:
                out.append(f32(v) if ctype is C.c_float else v)
        return out

    def __getattr__(self, fn):
        def call(*args):
            spec = CALLS[fn]
            assert len(args) == len(spec), (fn, len(args))
            rec, host = [fn], None  # the name, then the arguments in the order of "call_args"
            for (name, kind), a in zip(spec, args):
                if kind == "jobs":
                    host = bytes(a)
                    rec.append([self.job(j) for j in a])
                elif kind == "staged":  # the device copy of the table the launch was also given by its host address
                    rec.append("= jobs" if C.string_at(a, len(host)) == host else "differs from jobs")
                elif isinstance(kind, type):  # the table exists in the staging buffer only
                    n = args[[s[0] for s in spec].index("njobs")]
                    rec.append([self.job(j) for j in (kind * n).from_buffer_copy(C.string_at(a, n * C.sizeof(kind)))])
                elif kind == "out":
                    assert a
                    self.named[a] = f"out{len(self.calls)}" + ("" if name == "dst" else "." + name)
                    rec.append(self.named[a])
                elif kind == "in":
                    rec.append(self.named[a])
                elif kind == "optional":
                    rec.append("nonnull" if a else "null")
                elif kind == "i3":
                    rec.append(list(a))
                else:
                    rec.append(int(a))
            self.calls.append(rec)
            return 0

        return call


class Rejected(Exception):
    pass


class Parser(argparse.ArgumentParser):
    def error(self, message):
        raise Rejected(message)


@contextlib.contextmanager
def standin():
    """The library, the stream and the device check replaced as the module docstring says; yields the recorder.  Everything is put back on the way out."""
    rec = Recorder()
    saved = (L.lib, torch.cuda.current_stream, torch.Tensor.record_stream, torch.cuda.is_available, P.DP.init_distributed)
    L.lib, torch.cuda.current_stream, torch.Tensor.record_stream = (lambda: rec), (lambda *a: type("Stream", (), {"cuda_stream": 0})()), (lambda self, stream: None)
    torch.cuda.is_available, P.DP.init_distributed = (lambda: True), (lambda: (0, 1, 0))
    try:
        yield rec
    finally:
        L.lib, torch.cuda.current_stream, torch.Tensor.record_stream, torch.cuda.is_available, P.DP.init_distributed = saved


def sampler_configs():
    """(name, flip_prob, seed, positional ranges, named ranges)"""
    one = lambda p: dict(appearance_prob=p, acquisition_prob=p)  # noqa: E731
    cfg = [("off", 0.5, 7, (), {}), ("off, another seed", 0.5, 8, (), {}), ("validation", None, 7, (), {}), ("augment alone, positional", 0.5, 7, tuple(AUG.values()), {}), ("field alone", 0.5, 7, (), FIELD),
           ("appearance alone", 0.5, 7, (), dict(APP, appearance_prob=1.0)), ("acquisition alone, default probability", 0.5, 7, (), ACQ)]
    for fam, rest in ((AUG, {}), (FIELD, dict(field_spacing=16)), (APP, dict(appearance_prob=0.5)), (ACQ, dict(acquisition_prob=0.5))):
        cfg += [(k + " alone", 0.5, 7, (), {k: v, **rest}) for k, v in fam.items() if k not in rest]
    for p, seed in ((0.0, 7), (0.5, 8), (1.0, 7)):
        cfg.append((f"all four, p={p}", 0.5, seed, (), dict(AUG, **FIELD, **APP, **ACQ, **one(p))))
    cfg.append(("zeros given", 0.5, 7, (0.0,) * 5, dict(elastic_mag=0.0, bias_field=0.0, field_spacing=16, blur_sigma=0.0, lowres=0.0, contrast=0.0, gamma=0.0, thick_slices=0, ghost=0.0, spike=0.0, **one(1.0))))
    return cfg


def record_sampler(rec, cases, name, flip_prob, seed, ranges, named):
    s = T.PatchSampler(cases, ROI, flip_prob, seed, *ranges, **named)
    t = s.tail
    out = dict(name=name, flip_prob=flip_prob, seed=seed, ranges=list(ranges), named=dict(named),
               tail=enc(dict(augment=t.augment, field=t.field, appearance=t.appearance, acquisition=t.acquisition, augmenting=t.augmenting, fielding=t.fielding, appearing=t.appearing, acquiring=t.acquiring)),
               appearing=enc(s.appearing), acquiring=enc(s.acquiring), batches=[])
    for idx in BATCHES:
        rec.begin_batch()
        img, lab = s.sample(list(idx))
        first = next(k for k, v in rec.named.items() if v == "out0")
        assert img.shape == lab.shape == (2, 1, *ROI) and lab.data_ptr() - first == 4 * img.numel()  # the label is the second half of the crop launch's output
        assert all(a.keys() == s.last_augment[0].keys() for a in s.last_augment)
        by_key = {k: [a[k] for a in s.last_augment] for k in s.last_augment[0]} if s.last_augment else None  # {key: the value of every sample}
        out["batches"].append(dict(calls=rec.calls, last_draws=enc(s.last_draws), last_augment=enc(by_key), acquisition_launches=s.acquisition_launches,
                                   last_tone_stats=None if s.last_tone_stats is None else list(s.last_tone_stats.shape), image=rec.named[img.data_ptr()]))
    return out


def param_argvs():
    f = lambda **kw: sum((["--aug_" + k, str(v)] for k, v in kw.items()), [])  # noqa: E731
    return [[], f(**AUG), f(**FIELD), f(**APP), f(**ACQ), f(rotate_deg=10), f(intensity_shift=0.3), f(elastic_mag=4), f(bias_field=0.3),
            f(field_spacing=32), f(blur_sigma=1.5), f(lowres=0.25), f(gamma=0.5), f(appearance_prob=0.5), f(thick_slices=2.0, acquisition_prob=1), f(ghost=1), f(spike=2.5), f(**AUG, **FIELD, **APP, **ACQ, appearance_prob=1, acquisition_prob=0.75), ["--debug"] + f(rotate_deg=180, elastic_mag=16, bias_field=0.1, gamma=0.1, spike=1)]


def bad_argvs():
    f = lambda **kw: sum((["--aug_" + k, str(v)] for k, v in kw.items()), [])  # noqa: E731
    return [f(rotate_deg=-1), f(rotate_deg=181), f(scale=1), f(noise_std="nan"), f(elastic_mag=17), f(elastic_mag=3, field_spacing=8), f(field_spacing=0), f(field_spacing=2.5), f(bias_field="inf"),
            f(blur_sigma=2), f(lowres=0.1), f(lowres=1), f(contrast=1), f(gamma=-0.5), f(appearance_prob=1.5), f(thick_slices=5), f(thick_slices=2.5), f(ghost=1.5), f(spike=-2),
            f(acquisition_prob=-0.1), f(ghost=2, gamma=2, bias_field=-1, scale=3), f(acquisition_prob=2, appearance_prob=2)]


def record_params(argv):
    p = P.VSparams(Parser(), BASE + list(argv))
    train, val, test = p.get_transforms()
    return dict(argv=list(argv), train=enc(train), val=enc(val), test=enc(test), attributes=enc({"aug_" + k: getattr(p, "aug_" + k) for k in FLAG_KEYS}),
                properties=enc(dict(augment=p.augment, field_augment=p.field_augment, appearance_augment=p.appearance_augment, acquisition_augment=p.acquisition_augment)))


def record_flags():
    parser = Parser()
    P.VSparams(parser, BASE)
    acts = [parser._option_string_actions["--aug_" + k] for k in FLAG_KEYS]
    return dict(order=[a.option_strings for a in parser._actions], aug=[dict(option_strings=a.option_strings, dest=a.dest, nargs=a.nargs, type=a.type.__name__, default=enc(a.default), metavar=a.metavar, help=a.help) for a in acts])


def record_rejected(argv):
    try:
        P.VSparams(Parser(), BASE + list(argv))
    except Rejected as e:
        return dict(argv=list(argv), error=str(e))
    raise AssertionError(f"{argv} was accepted")


def record():
    with standin() as rec:
        cases = [dict(image=torch.zeros(s), label=torch.zeros(s)) for s in SHAPES]
        rec.sources = {c[k].data_ptr(): [i, k] for i, c in enumerate(cases) for k in ("image", "label")}
        fields = {fn: [name for name, _ in job._fields_] for fn, job in JOBS.items()}
        out = dict(commit="2a48986", job_fields=fields, call_args={fn: [name for name, _ in spec] for fn, spec in CALLS.items()}, samplers=[record_sampler(rec, cases, *cfg) for cfg in sampler_configs()], params=[record_params(a) for a in param_argvs()], flags=record_flags(),
                   rejected=[record_rejected(a) for a in bad_argvs()])
    return json.loads(json.dumps(out))  # tuples become lists, as in the file


def dumps(out) -> str:
    """One line per sampler configuration, argv and flag, so that a difference shows as a short diff."""
    line = lambda v: json.dumps(v, sort_keys=True, separators=(",", ":"))  # noqa: E731
    body = ",\n".join(f'"{k}":[\n' + ",\n".join(line(e) for e in out[k]) + "\n]" for k in ("samplers", "params", "rejected"))
    return '{"commit":' + line(out["commit"]) + ',\n"job_fields":' + line(out["job_fields"]) + ',\n"call_args":' + line(out["call_args"]) +',\n"flags":{"order":' + line(out["flags"]["order"]) + ',\n"aug":[\n' + ",\n".join(line(e) for e in out["flags"]["aug"]) + "\n]},\n" + body + "}\n"


def main():
    out = record()
    text = dumps(out)
    assert json.loads(text) == out
    with open(PATH, "w") as f:
        f.write(text)
    print(PATH, len(text), "bytes,", len(out["samplers"]), "sampler configurations,", len(out["params"]), "argvs,", len(out["rejected"]), "rejected argvs")


if __name__ == "__main__":
    main()
