#!/usr/bin/env python3
"""tools/bench_bicubic.py -- the bicubic resample (k_tables_tensor<BicubicFilter, ...>) against the antialiased one (<TriangleFilter, ...>) on the
same inputs, against the route a caller has today to a bicubic tensor, and against a device copy, alternating in one process.

    python tools/bench_bicubic.py [--steps 20] [--warmup 3] [--rounds 5] [--ring 4] [--only-bilinear | --only-antialias | --only-bytes]
                                  [--out profiles/bicubic.txt]

The method and the workload are tools/bench_antialias.py's: each round times `steps` calls of each route between two HIP
events on the context's stream over a ring of `ring` input sets, and the report is the median per-call time over the rounds.
Nothing is gated.  256 crops of mixed sizes, (224 f u) x (224 f v) pixels with u, v seeded in [0.85, 1.15], to a 224 x 224
fp16 CHW tensor with the ImageNet constants, every second image flipped, at residual factors f of 1.0, 1.5, 2.0 and 8.  One
difference: a side is cut at 8 x 224 = 1792 pixels, the bicubic filter's limit, which binds at f = 8 only (there about half
of the sides are cut: the sources are 2.3 GB instead of bench_antialias.py's 2.5 GB).  Every route sees the same inputs.
  bicubic    jpeg_amd_resize_filter_tensor_batch with JPEG_AMD_FILTER_BICUBIC: one launch
  antialias  the same call with JPEG_AMD_FILTER_ANTIALIAS: one launch of the kernel the parent commit has
  eager      what a caller does without this filter: per image torch.nn.functional.interpolate(mode="bicubic",
             antialias=True) on the crop's bytes as floats, clamp, round half up to bytes, flip, subtract, multiply, cast,
             into the batch tensor -- 256 times a handful of framework launches
  copy       a device copy (torch copy_) that reads and writes, together, the bytes `bicubic` must move: the sources once
             plus the tensor once
--only-bilinear and --only-antialias time jpeg_amd_resize_tensor_batch or the antialiased call alone and print one JSON line
per factor; they touch nothing the parent commit lacks, so a copy of this file in a checkout of the parent, run in
alternation with this one, shows what this filter's arrival costs the calls that were there.  --only-bytes times
jpeg_amd_resize_filter_batch (bytes out: k_tables_bytes) with the antialiasing and the bicubic filter on the same inputs and
prints one JSON line per factor, for an A/B of two builds of the library (JPEG_AMD_LIBRARY).
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
FACTORS = (1.0, 1.5, 2.0, 8.0)
MAX_SCALE = 8                                               # kBicubicMaxScale
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


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


def _case(torch, ctx, factor, ring):
    """-> (extents [(w, h)], c extents, the ring of packed sources, their stride)."""
    rng = np.random.default_rng(int(1000 * factor))
    ext = [(min(max(int(round(TARGET[0] * factor * u)), 1), MAX_SCALE * TARGET[0]),
            min(max(int(round(TARGET[1] * factor * v)), 1), MAX_SCALE * TARGET[1])) for u, v in rng.uniform(0.85, 1.15, (N, 2))]
    stride = max(3 * w * h for w, h in ext)
    gen = torch.Generator(device=ctx.torch_device).manual_seed(7)
    sets = [torch.randint(0, 256, (N * stride,), dtype=torch.uint8, device=ctx.torch_device, generator=gen) for _ in range(ring)]
    return ext, (_lib.Extent * N)(*[_lib.Extent(w, h) for w, h in ext]), sets, stride


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--only-bilinear", action="store_true")
    ap.add_argument("--only-antialias", action="store_true")
    ap.add_argument("--only-bytes", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bicubic.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_bicubic: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    lib = _lib.lib()
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    flips = (C.c_uint8 * N)(*[i & 1 for i in range(N)])
    mean_b = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(3, 1, 1)
    scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(3, 1, 1)
    wt, ht = TARGET
    out = torch.empty((N, 3, ht, wt), dtype=torch.float16, device=dev)
    out_stride = 3 * wt * ht
    lines = [f"# tools/bench_bicubic.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} "
             f"--ring {args.ring}; times are HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included"]
    for factor in FACTORS:
        ext, c_ext, sets, stride = _case(torch, ctx, factor, args.ring)
        src_bytes = sum(3 * w * h for w, h in ext)
        moved = src_bytes + 2 * N * out_stride

        def bilinear(k):
            _lib.check(lib.jpeg_amd_resize_tensor_batch(ctx.handle, N, sets[k % args.ring].data_ptr(), stride, c_ext, wt, ht,
                                                        C.byref(spec), flips, out.data_ptr(), out_stride), "bilinear", ctx.handle)

        def filtered(code):
            def call(k):
                _lib.check(lib.jpeg_amd_resize_filter_tensor_batch(ctx.handle, N, sets[k % args.ring].data_ptr(), stride, c_ext, wt,
                                                                   ht, code, C.byref(spec), flips, out.data_ptr(), out_stride),
                           "filter %d" % code, ctx.handle)
            return call

        if args.only_bytes:
            d_bytes = torch.empty(N * out_stride, dtype=torch.uint8, device=dev)
            res = {"factor": factor}
            for name, code in (("antialias", _lib.FILTER_ANTIALIAS), ("bicubic", _lib.FILTER_BICUBIC)):
                def to_bytes(k):
                    _lib.check(lib.jpeg_amd_resize_filter_batch(ctx.handle, N, sets[k % args.ring].data_ptr(), stride, c_ext, wt, ht, code,
                                                                d_bytes.data_ptr(), out_stride), "bytes %d" % code, ctx.handle)
                times = [_timed(torch, to_bytes, args.steps, args.warmup) for _ in range(args.rounds)]
                res.update({"t_%s_bytes_us" % name: round(statistics.median(times), 1), "rounds_%s" % name: [round(t, 1) for t in times]})
            print(json.dumps(res), flush=True)
            del sets, d_bytes
            torch.cuda.empty_cache()
            continue
        if args.only_bilinear or args.only_antialias:
            name, fn = ("bilinear", bilinear) if args.only_bilinear else ("antialias", filtered(_lib.FILTER_ANTIALIAS))
            times = [_timed(torch, fn, args.steps, args.warmup) for _ in range(args.rounds)]
            print(json.dumps({"factor": factor, "t_%s_us" % name: round(statistics.median(times), 1),
                              "rounds": [round(t, 1) for t in times]}), flush=True)
            del sets
            torch.cuda.empty_cache()
            continue

        copy_src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
        copy_dst = torch.empty_like(copy_src)
        bicubic, antialias = filtered(_lib.FILTER_BICUBIC), filtered(_lib.FILTER_ANTIALIAS)

        def eager(k):
            src = sets[k % args.ring]
            for i, (w, h) in enumerate(ext):
                im = src[i * stride:i * stride + 3 * w * h].view(h, w, 3).permute(2, 0, 1)[None].float()
                u = torch.nn.functional.interpolate(im, size=(ht, wt), mode="bicubic", align_corners=False, antialias=True)
                u = torch.floor(u.clamp_(0, 255).add_(0.5))[0]
                if i & 1:
                    u = u.flip(2)
                out[i] = u.sub_(mean_b).mul_(scale)

        def copy(k):
            copy_dst.copy_(copy_src)

        # the eager route is this filter up to its operation order: at most one level
        bicubic(0)
        a = out.clone()
        eager(0)
        levels = ((a.float() - out.float()).abs() / scale.abs()).max().item()
        assert levels < 1.5, levels   # one level, and the two fp16 roundings
        routes = {"bicubic": bicubic, "antialias": antialias, "eager": eager, "copy": copy}
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                times[k].append(_timed(torch, fn, max(args.steps // 4, 2) if k == "eager" else args.steps, args.warmup))
        med = {k: statistics.median(v) for k, v in times.items()}
        res = {"factor": factor, "n": N, "target": [wt, ht], "source_MB": round(src_bytes / 1e6, 1), "moved_MB": round(moved / 1e6, 1),
               "t_bicubic_us": round(med["bicubic"], 1), "t_antialias_us": round(med["antialias"], 1),
               "t_eager_us": round(med["eager"], 1), "t_copy_us": round(med["copy"], 1),
               "bicubic_over_antialias": round(med["bicubic"] / med["antialias"], 2),
               "eager_over_bicubic": round(med["eager"] / med["bicubic"], 1),
               "bicubic_GBps": round(moved / med["bicubic"] / 1e3, 0), "copy_GBps": round(moved / med["copy"] / 1e3, 0),
               "bicubic_over_copy": round(med["bicubic"] / med["copy"], 2), "worst_level_vs_eager": round(levels, 3),
               "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
        lines += [json.dumps(res),
                  f"f = {factor}: bicubic {med['bicubic']:.0f} us ({res['bicubic_over_antialias']:.2f} x antialias {med['antialias']:.0f} us), "
                  f"eager {med['eager']:.0f} us ({res['eager_over_bicubic']:.1f} x bicubic), "
                  f"source + tensor bytes at {res['bicubic_GBps']:.0f} GB/s, a copy of them {med['copy']:.0f} us "
                  f"({res['copy_GBps']:.0f} GB/s)"]
        print("\n".join(lines[-2:]), flush=True)
        del sets, copy_src, copy_dst
        torch.cuda.empty_cache()
    if args.out and not (args.only_bilinear or args.only_antialias or args.only_bytes):
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
