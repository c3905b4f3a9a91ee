#!/usr/bin/env python3
"""tools/bench_resized.py -- resized decode (jpeg_amd.decode_crops_resized: the view decode into a context buffer, then one
k_resize_bilinear launch) against what a caller had to do before it, alternating in one process.

    python tools/bench_resized.py [--steps 20] [--warmup 3] [--rounds 5] [--ring 4] [--out profiles/r10_resized.txt]

The method is tools/bench_scaled.py's: each round times `steps` calls of each path between two HIP events on the context's
stream over a ring of `ring` input sets (distinct coefficient buffers, together larger than the 256 MiB Infinity Cache); the
report is the median per-call time over the rounds.  Nothing is gated.  The workload is case A of tools/bench_view.py: 256 x
1920 x 1080 4:2:0 RGB, one seeded RandomResizedCrop rectangle per image (area 0.08 .. 1, aspect 3/4 .. 4/3) -> 224 x 224.
  resized   jpeg_amd.decode_crops_resized: the views picked on the host, one call, one dense [256, 224, 224, 3] tensor
  today     the same views through jpeg_amd.decode_views, then torch.nn.functional.interpolate (bilinear, no antialias) per
            image -- the sizes differ, so it cannot be batched -- rounded into the same dense tensor
  resample  jpeg_amd_resize_batch alone on the decoded views: the k_resize_bilinear launch and its record upload
All three are host-inclusive: the events bracket whatever the Python calls enqueue, and a path that cannot keep the GPU fed is
timed as such.  `today` and `resized` agree to one level (tests/test_resize_cpu.py); that is checked here on the first set.
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
from tools.bench_view import TARGET, _timed, random_resized_crops  # noqa: E402

W, H, N = 1920, 1080, 256


def _inputs(torch, ctx, layout, ring):
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(7)
    sets = [[torch.randint(-256, 256, (N, uy, ux, 64), dtype=torch.int16, device=dev, generator=gen) for ux, uy in layout.units((W, H))]
            for _ in range(ring)]
    q = torch.randint(1, 8, (N, 2, 64), dtype=torch.int16, device=dev, generator=gen)
    return sets, q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_resized.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_resized: no GPU (this tool measures the MI355X; there is no CPU number)")
    F = torch.nn.functional
    ctx = J.Context(0)
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    sets, q = _inputs(torch, ctx, layout, args.ring)
    source = random_resized_crops(np.random.default_rng(20240809), W, H, N)
    dense = torch.empty((N, TARGET[1], TARGET[0], 3), dtype=torch.uint8, device=ctx.torch_device)

    def pick_views():
        return [(d,) + J.view_of_source((W, H), d, s) for d, s in ((J.view_denom(s[2:], TARGET), s) for s in source)]

    def resized(k):
        return J.decode_crops_resized(ctx, (W, H), layout, sets[k % args.ring], q, source, TARGET)[0]

    def today(k):
        views = J.decode_views(ctx, (W, H), layout, sets[k % args.ring], q, pick_views())
        for i, v in enumerate(views):
            f = F.interpolate(v.permute(2, 0, 1)[None].to(torch.float32), size=(TARGET[1], TARGET[0]), mode="bilinear",
                              align_corners=False, antialias=False)
            dense[i] = torch.floor(f[0].permute(1, 2, 0).clamp_(0, 255) + 0.5).to(torch.uint8)
        return dense

    views = pick_views()
    decoded = J.decode_views(ctx, (W, H), layout, sets[0], q, views)
    src_stride = max(3 * v[3] * v[4] for v in views)
    extents = (_lib.Extent * N)(*[_lib.Extent(v[3], v[4]) for v in views])
    alone = torch.empty_like(dense)

    def resample(k):
        st = _lib.lib().jpeg_amd_resize_batch(ctx.handle, N, decoded[0].data_ptr(), src_stride, extents, TARGET[0], TARGET[1],
                                              alone.data_ptr(), alone[0].numel())
        assert st == 0, st

    a, b = resized(0).to(torch.int16), today(0).to(torch.int16)
    differ, worst = int((a != b).sum()), int((a - b).abs().max())
    assert worst <= 1 and differ * 1000 <= a.numel(), (worst, differ)
    resample(0)
    assert bool((alone == resized(0)).all())

    paths = {"resized": resized, "today": today, "resample": resample}
    times = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            times[k].append(_timed(torch, fn, args.steps, args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    view_px = sum(v[3] * v[4] for v in views)
    res = {"case": "A", "size": [W, H], "n": N, "target": list(TARGET),
           "denominators": {d: sum(1 for v in views if v[0] == d) for d in (1, 2, 4, 8)}, "view_pixels": view_px,
           "output_pixels": N * TARGET[0] * TARGET[1], "resized_vs_today_differing": differ, "resized_vs_today_worst": worst,
           "t_resized_us": round(med["resized"], 1), "t_today_us": round(med["today"], 1), "t_resample_us": round(med["resample"], 1),
           "today_over_resized": round(med["today"] / med["resized"], 2),
           "resample_GBps": round(3 * (view_px + N * TARGET[0] * TARGET[1]) / med["resample"] * 1e-3, 1),
           "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
    lines = [f"# tools/bench_resized.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; "
             "times are HIP-event medians per call, host work included",
             json.dumps(res),
             f"A: 256 x 1920x1080 crops -> {TARGET[0]}x{TARGET[1]}, denominators {res['denominators']}, {view_px / 1e6:.1f} Mpx decoded:  "
             f"decode_crops_resized {med['resized']:.0f} us  decode_views + {N} x interpolate {med['today']:.0f} us "
             f"({res['today_over_resized']:.2f} x)  resample alone {med['resample']:.1f} us "
             f"({res['resample_GBps']:.0f} GB/s of source + output bytes)"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
