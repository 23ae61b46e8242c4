"""Host cost of PatchSampler.sample without a GPU: the library is replaced by a stand-in whose every entry point returns 0 and records nothing, the stream by an object
with `cuda_stream = 0`, `Tensor.record_stream` by a no-op, and the cases are CPU tensors.  What is left is what the sampler does on the host per call: the draws, the
job tables, their staging and the argument marshalling.

    python tools/bench_sampler_host.py [--runs 9] [--calls 3000]

times `sample([0, 1, 0, 1])` of the plain sampler as bench.py builds it (two cached 448 x 448 x 128 cases, patch 384 x 128 x 128) and of one with all four augmentation
families on at probability 1, and prints per configuration the microseconds per call of every run, their median and their spread (max - min)."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from vs_seg_amd import _lib as L  # noqa: E402
from vs_seg_amd.data.transforms import PatchSampler  # noqa: E402

PATCH = (384, 128, 128)
ALL_FOUR = dict(rotate_deg=15.0, scale=0.1, intensity_scale=0.2, intensity_shift=0.3, noise_std=0.05, elastic_mag=3.0, bias_field=0.3, field_spacing=16,
                blur_sigma=1.0, lowres=0.5, contrast=0.25, gamma=0.3, appearance_prob=1.0, thick_slices=3, ghost=0.5, spike=1.0, acquisition_prob=1.0)


class Null:
    def __getattr__(self, name):
        return lambda *a: 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=3000)
    args = ap.parse_args()
    null = Null()
    L.lib = lambda: null
    torch.cuda.current_stream = lambda *a: type("Stream", (), {"cuda_stream": 0})()
    torch.Tensor.record_stream = lambda self, stream: None
    cached = [dict(image=torch.zeros((448, 448, 128)), label=torch.zeros((448, 448, 128))) for _ in range(2)]
    for name, ranges in (("plain", {}), ("all four, p=1", ALL_FOUR)):
        sampler = PatchSampler(cached, PATCH, flip_prob=0.5, seed=0, **ranges)
        for _ in range(200):
            sampler.sample([0, 1, 0, 1])
        us = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            for _ in range(args.calls):
                sampler.sample([0, 1, 0, 1])
            us.append(1e6 * (time.perf_counter() - t0) / args.calls)
        print(f"{name:<14s} us/call: " + " ".join(f"{u:.2f}" for u in us) + f" | median {statistics.median(us):.2f} spread {max(us) - min(us):.2f}")


if __name__ == "__main__":
    main()
