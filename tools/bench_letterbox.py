#!/usr/bin/env python3
"""tools/bench_letterbox.py -- the placed resample (k_resize_placed_tensor, k_tables_placed_tensor over the Placed* records;
include/jpeg_amd.h, "placed resample") against the oriented call and against the route a caller has today to a letterboxed
tensor, alternating in one process.

    python tools/bench_letterbox.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 2] [--out profiles/placed.txt]

The method is tools/bench_oriented.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets, host work included, and the report is the median per-call time over the rounds.
The workload is the resample stage of a detector's loader alone, view bytes to tensor: 256 crops of mixed aspect ratios --
the long side 640 f u pixels with u seeded in [0.85, 1.15], the aspect ratio seeded log-uniformly in [1/2, 2], f = 1.5 (what
jpeg_amd_view_denom leaves) -- to a [256, 3, 640, 640] fp16 CHW tensor with the ImageNet constants and the fill
(124, 116, 104), for the three filters.  The sources are packed into one allocation once, outside the timed window, sorted by
their window's size (the C ABI is called directly).
  fit        jpeg_amd_resize_placed_tensor_batch, place = FIT, centred: the letterbox, one launch
  stretched  (a) jpeg_amd_resize_oriented_tensor_batch, every orientation 1, on the same sources stretched to 640 x 640
  whole      (b) the placed call with whole-canvas windows: (a)'s pixels through the placed kernels.  The bar for whole over
             stretched is the larger of 3 % and the spread of (a)'s own rounds (max - min over its median); asserted
             bit-identical to (a)
  oriented   (a) again with the last image's orientation 3 instead of 1: every record is then the oriented one and the ORIENTED
             kernels run on what is, but for that image, the same work -- it splits (b)'s distance from (a) into what the
             signed steps cost and what the placement costs
  today      (c) torch.full of the fill's elements, then per distinct window size one jpeg_amd_resize_filter_tensor_batch into a
             scratch tensor and a slice-assign per image; asserted bit-identical to `fit`.  Reported, not gated.
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

N, CANVAS, FACTOR = 256, (640, 640), 1.5
MEAN, STD, FILL = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225), (124, 116, 104)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "placed.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_letterbox: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    lib = _lib.lib()
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    wt, ht = CANVAS
    out = torch.empty((N, 3, ht, wt), dtype=torch.float16, device=dev)
    out_stride = 3 * wt * ht
    # the sources, sorted by their window's size, so that (c)'s groups are runs of the packed allocation
    rng = np.random.default_rng(640)
    ext = []
    for u, a in zip(rng.uniform(0.85, 1.15, N), np.exp(rng.uniform(np.log(0.5), np.log(2.0), N))):
        long_side = wt * FACTOR * u
        w, h = (long_side, long_side / a) if a >= 1 else (long_side * a, long_side)
        ext.append((max(int(round(w)), 1), max(int(round(h)), 1)))
    windows = [J.place_window("fit", e, CANVAS) for e in ext]
    order = sorted(range(N), key=lambda i: windows[i][2:])
    ext, windows = [ext[i] for i in order], [windows[i] for i in order]
    groups = []                                                      # (first image, images, (ww, wh))
    for i, w in enumerate(windows):
        if groups and groups[-1][2] == w[2:]:
            groups[-1] = (groups[-1][0], groups[-1][1] + 1, w[2:])
        else:
            groups.append((i, 1, w[2:]))
    stride = max(3 * w * h for w, h in ext)
    gen = torch.Generator(device=dev).manual_seed(7)
    sets = [torch.randint(0, 256, (N * stride,), dtype=torch.uint8, device=dev, generator=gen) for _ in range(args.ring)]
    c_ext = (_lib.Extent * N)(*[_lib.Extent(w, h) for w, h in ext])
    ones = (C.c_uint8 * N)(*[1] * N)
    signed = (C.c_uint8 * N)(*([1] * (N - 1) + [3]))
    fit = _lib.Placement(_lib.PLACE_FIT, _lib.ANCHOR_CENTRE, None, (C.c_uint8 * 3)(*FILL), 0)
    whole_windows = (_lib.Region * N)(*[_lib.Region(0, 0, wt, ht)] * N)
    whole = _lib.Placement(_lib.PLACE_WINDOWS, _lib.ANCHOR_CENTRE, C.cast(whole_windows, C.c_void_p), (C.c_uint8 * 3)(*FILL), 0)
    pad = J.resize_tensor(ctx, [torch.tensor(FILL, dtype=torch.uint8, device=dev).reshape(1, 1, 3)], (1, 1), spec).reshape(1, 3, 1, 1)
    scratch = torch.empty(max(m * 3 * ww * wh for _, m, (ww, wh) in groups), dtype=torch.float16, device=dev)
    lines = [f"# tools/bench_letterbox.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} "
             f"--ring {args.ring}; times are HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included; "
             f"{len(groups)} distinct window sizes, source {sum(3 * w * h for w, h in ext) / 1e6:.1f} MB"]
    for name, code in (("bilinear", _lib.FILTER_BILINEAR), ("antialias", _lib.FILTER_ANTIALIAS), ("bicubic", _lib.FILTER_BICUBIC)):
        def placed(place):
            def call(k):
                _lib.check(lib.jpeg_amd_resize_placed_tensor_batch(ctx.handle, N, sets[k % args.ring].data_ptr(), stride, c_ext, wt, ht, code,
                                                                   C.byref(spec), None, None, C.byref(place), None, out.data_ptr(),
                                                                   out_stride), "placed", ctx.handle)
            return call

        def stretched(k, h_orient=ones):
            _lib.check(lib.jpeg_amd_resize_oriented_tensor_batch(ctx.handle, N, sets[k % args.ring].data_ptr(), stride, c_ext, wt, ht, code,
                                                                 C.byref(spec), None, h_orient, out.data_ptr(), out_stride), "oriented",
                       ctx.handle)

        def today(k):
            src = sets[k % args.ring]
            out[:] = pad
            for i0, m, (ww, wh) in groups:
                part = scratch[:m * 3 * ww * wh]
                _lib.check(lib.jpeg_amd_resize_filter_tensor_batch(ctx.handle, m, src.data_ptr() + i0 * stride, stride,
                                                                   C.byref(c_ext, i0 * C.sizeof(_lib.Extent)), ww, wh, code, C.byref(spec), None,
                                                                   part.data_ptr(), 3 * ww * wh), "today", ctx.handle)
                part = part.view(m, 3, wh, ww)
                for j in range(m):
                    x0, y0 = windows[i0 + j][:2]
                    out[i0 + j, :, y0:y0 + wh, x0:x0 + ww] = part[j]

        routes = {"fit": placed(fit), "stretched": stretched, "whole": placed(whole), "oriented": lambda k: stretched(k, signed),
                  "today": today}
        # whole-canvas windows are the oriented call, and today's route gives the placed call's tensor, bit for bit
        stretched(0)
        a = out.clone()
        routes["whole"](0)
        assert torch.equal(a.view(torch.int16), out.view(torch.int16))
        routes["fit"](0)
        a = out.clone()
        today(0)
        assert torch.equal(a.view(torch.int16), out.view(torch.int16))
        del a
        times = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, fn in routes.items():
                times[k].append(_timed(torch, fn, max(args.steps // 5, 2) if k == "today" else args.steps, 1 if k == "today" else args.warmup))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = (max(times["stretched"]) - min(times["stretched"])) / med["stretched"]
        bar = max(0.03, spread)
        res = {"filter": name, "n": N, "canvas": [wt, ht], "window_sizes": len(groups),
               **{f"t_{k}_us": round(v, 1) for k, v in med.items()},
               "whole_over_stretched": round(med["whole"] / med["stretched"], 3), "bar": round(1 + bar, 3),
               "oriented_over_stretched": round(med["oriented"] / med["stretched"], 3),
               "whole_over_oriented": round(med["whole"] / med["oriented"], 3),
               "within_bar": bool(med["whole"] <= med["stretched"] * (1 + bar)),
               "fit_over_stretched": round(med["fit"] / med["stretched"], 2), "today_over_fit": round(med["today"] / med["fit"], 1),
               "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
        lines += [json.dumps(res),
                  f"{name}: fit {med['fit']:.0f} us, (a) stretched {med['stretched']:.0f} us, (b) whole {med['whole']:.0f} us = "
                  f"{res['whole_over_stretched']:.3f} x (a) (bar {res['bar']:.3f}) = {res['whole_over_oriented']:.3f} x the oriented kernels "
                  f"({med['oriented']:.0f} us), (c) today {med['today']:.0f} us = {res['today_over_fit']:.1f} x fit"]
        print("\n".join(lines[-2:]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
