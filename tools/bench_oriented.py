#!/usr/bin/env python3
"""tools/bench_oriented.py -- the oriented resample (k_resize_tensor<true, ...>, k_tables_tensor over OrientedAntialiasRecords) against the
kernels without orientations and against the route a caller has today to upright tensors, alternating in one process.

    python tools/bench_oriented.py [--steps 20] [--warmup 3] [--rounds 5] [--ring 2] [--out profiles/oriented.txt]

The method is tools/bench_antialias.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets, host work included, and the report is the median per-call time over the rounds.
Nothing is gated.  The workload is the resample stage of the loader alone, view bytes to tensor: 256 crops of mixed sizes,
(224 f u) x (224 f v) pixels as STORED with u, v seeded in [0.85, 1.15], to a [256, 3, 224, 224] fp16 CHW tensor with the
ImageNet constants, every second image flipped, at residual factors f of 1 and 2 (what jpeg_amd_view_denom leaves), for both
filters.  The sources are packed into one allocation once, outside the timed window (the C ABI is called directly).
  plain      jpeg_amd_resize_filter_tensor_batch: the call without orientations
  ones       (a) jpeg_amd_resize_oriented_tensor_batch, every orientation 1: the same kernels from the same records
  flips      (b) every orientation 3: signed steps, no transpose
  transpose  (c) every orientation 6: neighbouring lanes read bytes one stored row apart
  mix        (d) a seeded mix of the 8 orientations
  torch      (e) today's route to (d): per image torch flip / transpose and a contiguous copy of the view's bytes, then `plain`
             on the oriented copies -- 256 times a few framework launches, then one launch; asserted bit-identical to (d)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeg_amd as J  # noqa: E402
from jpeg_amd import _lib  # noqa: E402

N, TARGET = 256, (224, 224)
FACTORS = (1.0, 2.0)
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
BITS = {1: (0, 0, 0), 2: (0, 1, 0), 3: (0, 1, 1), 4: (0, 0, 1), 5: (1, 0, 0), 6: (1, 0, 1), 7: (1, 1, 1), 8: (1, 1, 0)}   # T, fx, fy


def _timed(torch, fn, steps, warmup):
    for k in range(warmup):
        fn(k)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(steps):
        fn(k)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps * 1e3   # us per call


def _orient(t, o):
    T, fx, fy = BITS[o]
    if fy:
        t = t.flip(0)
    if fx:
        t = t.flip(1)
    return t.transpose(0, 1) if T else t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "oriented.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_oriented: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    lib = _lib.lib()
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    flips = (C.c_uint8 * N)(*[i & 1 for i in range(N)])
    wt, ht = TARGET
    out = torch.empty((N, 3, ht, wt), dtype=torch.float16, device=dev)
    out_stride = 3 * wt * ht
    lines = [f"# tools/bench_oriented.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} "
             f"--ring {args.ring}; times are HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included"]
    for name, code in (("bilinear", _lib.FILTER_BILINEAR), ("antialias", _lib.FILTER_ANTIALIAS)):
        for factor in FACTORS:
            rng = np.random.default_rng(int(1000 * factor))
            ext = [(max(int(round(wt * factor * u)), 1), max(int(round(ht * factor * v)), 1)) for u, v in rng.uniform(0.85, 1.15, (N, 2))]
            mixed = [int(o) for o in rng.integers(1, 9, N)]
            stride = max(3 * w * h for w, h in ext)
            gen = torch.Generator(device=dev).manual_seed(7)
            sets = [torch.randint(0, 256, (N * stride,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(args.ring)]
            c_ext = (_lib.Extent * N)(*[_lib.Extent(w, h) for w, h in ext])
            turned = (_lib.Extent * N)(*[_lib.Extent(h, w) if BITS[o][0] else _lib.Extent(w, h) for (w, h), o in zip(ext, mixed)])
            upright = torch.empty(N * stride, dtype=torch.uint8, device=dev)

            def plain(k, extents=c_ext, src=None):
                src = sets[k % args.ring] if src is None else src
                _lib.check(lib.jpeg_amd_resize_filter_tensor_batch(ctx.handle, N, src.data_ptr(), stride, extents, wt, ht, code,
                                                                   C.byref(spec), flips, out.data_ptr(), out_stride), "plain", ctx.handle)

            def oriented(values):
                h_orient = (C.c_uint8 * N)(*values)

                def call(k):
                    _lib.check(lib.jpeg_amd_resize_oriented_tensor_batch(ctx.handle, N, sets[k % args.ring].data_ptr(), stride, c_ext, wt, ht,
                                                                         code, C.byref(spec), flips, h_orient, out.data_ptr(), out_stride),
                               "oriented", ctx.handle)
                return call

            def by_torch(k):
                src = sets[k % args.ring]
                for i, ((w, h), o) in enumerate(zip(ext, mixed)):
                    t = _orient(src[i * stride:i * stride + 3 * w * h].view(h, w, 3), o)
                    upright[i * stride:i * stride + 3 * w * h].view(t.shape).copy_(t)
                plain(k, turned, upright)

            routes = {"plain": plain, "ones": oriented([1] * N), "flips": oriented([3] * N), "transpose": oriented([6] * N),
                      "mix": oriented(mixed), "torch": by_torch}
            # the new call with ones is the old call, and today's route gives the oriented call's tensor, bit for bit
            plain(0)
            a = out.clone()
            routes["ones"](0)
            assert torch.equal(a.view(torch.int16), out.view(torch.int16))
            routes["mix"](0)
            a = out.clone()
            by_torch(0)
            assert torch.equal(a.view(torch.int16), out.view(torch.int16))
            times = {k: [] for k in routes}
            for _ in range(args.rounds):
                for k, fn in routes.items():
                    times[k].append(_timed(torch, fn, max(args.steps // 4, 2) if k == "torch" else args.steps, args.warmup))
            med = {k: statistics.median(v) for k, v in times.items()}
            res = {"filter": name, "factor": factor, "n": N, "target": [wt, ht], "source_MB": round(sum(3 * w * h for w, h in ext) / 1e6, 1),
                   **{f"t_{k}_us": round(v, 1) for k, v in med.items()},
                   "ones_over_plain": round(med["ones"] / med["plain"], 3), "flips_over_ones": round(med["flips"] / med["ones"], 2),
                   "transpose_over_ones": round(med["transpose"] / med["ones"], 2), "mix_over_ones": round(med["mix"] / med["ones"], 2),
                   "torch_over_mix": round(med["torch"] / med["mix"], 1),
                   "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
            lines += [json.dumps(res),
                      f"{name}, f = {factor}: plain {med['plain']:.0f} us, (a) ones {med['ones']:.0f} us, (b) flips {med['flips']:.0f} us, "
                      f"(c) transpose {med['transpose']:.0f} us = {res['transpose_over_ones']:.2f} x (a), (d) mix {med['mix']:.0f} us, "
                      f"(e) torch {med['torch']:.0f} us = {res['torch_over_mix']:.1f} x (d)"]
            print("\n".join(lines[-2:]), flush=True)
            del sets, upright
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
