#!/usr/bin/env python3
"""tools/bench_view.py -- view decode (jpeg_amd_decode_view_batch: k_view_decode, and the crop fallback) against what a
caller had to do before it, alternating in one process.

    python tools/bench_view.py [--steps 100] [--warmup 10] [--rounds 5] [--ring 4] [--json PATH] [--cases A,B,C]

Each round times `steps` calls of each path between two HIP events on the context's stream over a ring of `ring` input sets
(distinct coefficient buffers, together larger than the 256 MiB Infinity Cache, as bench.py does); the report is the median
per-call time over the rounds.  Nothing is gated.  Cases:
  A  256 x 1920 x 1080 4:2:0 RGB, one seeded RandomResizedCrop rectangle per image (area 0.08 .. 1, aspect 3/4 .. 4/3) headed
     for 224 x 224: the view of that rectangle at the denominator jpeg_amd_view_denom picks for it, against
       (i)  jpeg_amd_decode_region_batch of the same source rectangles (full-size pixels, the caller resizes all of them),
       (ii) jpeg_amd_decode_scaled_batch of the whole images at the batch's smallest denominator (the caller crops)
  B  8192 x 8192 4:2:0 RGB, the centre 4096 x 4096 of the source as a view at denom 2, 4, 8, against the whole-image scaled
     decode at the same denominator
  C  case A's rectangles through a cosited layout (the fallback), report only
Kernel times: run it again under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_view.py --steps 10 --rounds 1`.
"""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeg_amd as J  # noqa: E402
from jpeg_amd import _lib  # noqa: E402

TARGET = (224, 224)


def _layout(w, h):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes, L.scale_x, L.scale_y = w, h, 8, 3, 2, 2
    for p, f in enumerate((2, 1, 1)):
        L.factor_x[p] = L.factor_y[p] = f
        L.qi[p] = min(p, 1)
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def random_resized_crops(rng, W, H, n, area=(0.08, 1.0), aspect=(3 / 4, 4 / 3)):
    """The rectangle rule of RandomResizedCrop: an area share uniform in `area`, a log-uniform aspect ratio, ten attempts,
    then the central crop at the nearest allowed ratio."""
    out = []
    for _ in range(n):
        for _ in range(10):
            a = W * H * rng.uniform(*area)
            r = math.exp(rng.uniform(math.log(aspect[0]), math.log(aspect[1])))
            w, h = int(round(math.sqrt(a * r))), int(round(math.sqrt(a / r)))
            if 0 < w <= W and 0 < h <= H:
                out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
                break
        else:
            r = min(max(W / H, aspect[0]), aspect[1])
            w, h = (W, int(round(W / r))) if W / H < r else (int(round(H * r)), H)
            out.append(((W - w) // 2, (H - h) // 2, w, h))
    return out


def _views(size, source):
    """(denom, region) per source rectangle: the denominator of jpeg_amd_view_denom, the rectangle of jpeg_amd_view_of_source."""
    denoms = [J.view_denom(s[2:], TARGET) for s in source]
    return [(d, J.view_of_source(size, d, s)) for d, s in zip(denoms, source)]


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


def _inputs(torch, ctx, L, n, ring):
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(7)
    sizes = [64 * L.units_x[p] * L.units_y[p] for p in range(3)]
    sets = [[torch.randint(-256, 256, (n * s,), dtype=torch.int16, device=dev, generator=gen) for s in sizes] for _ in range(ring)]
    q = torch.randint(1, 8, (2 * 64,), dtype=torch.int16, device=dev, generator=gen)
    return sets, [_lib.ptr_array([t.data_ptr() for t in s]) for s in sets], _lib.size_array(sizes), q, sizes


def _head_bytes(L, cosited, denom, region):
    """Bytes of the block heads a view reads: jpeg_amd_view_window's blocks, 128 / 64 / 16 / 2 bytes of each."""
    w = (_lib.Region * _lib.MAX_PLANES)()
    assert _lib.lib().jpeg_amd_view_window(C.byref(L), cosited, denom, C.byref(_lib.Region(*region)), w) == 0
    return sum(w[p].width * w[p].height for p in range(L.nplanes)) * {1: 128, 2: 64, 4: 16, 8: 2}[denom]


def _median(xs):
    return round(statistics.median(xs), 2)


def case_crops(torch, ctx, name, cosited, args, steps):
    lib = _lib.lib()
    W, H, n = 1920, 1080, 256
    L = _layout(W, H)
    sets, ptrs, strides, q, sizes = _inputs(torch, ctx, L, n, args.ring)
    source = random_resized_crops(np.random.default_rng(20240809), W, H, n)
    views = _views((W, H), source)
    h_views = (_lib.View * n)(*[_lib.View(d, _lib.Region(*r)) for d, r in views])
    h_regions = (_lib.Region * n)(*[_lib.Region(*s) for s in source])
    dmin = min(d for d, _ in views)
    sw, sh = J.scaled_size((W, H), dmin)
    view_stride = max(3 * r[2] * r[3] for _, r in views)
    region_stride = max(3 * s[2] * s[3] for s in source)
    out = torch.empty(n * max(view_stride, region_stride, 3 * sw * sh), dtype=torch.uint8, device=ctx.torch_device)

    def view(k):
        st = lib.jpeg_amd_decode_view_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, cosited,
                                            _lib.COLOR_RGB8, h_views, out.data_ptr(), view_stride)
        assert st == 0, st

    def region(k):
        st = lib.jpeg_amd_decode_region_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, cosited,
                                              _lib.COLOR_RGB8, h_regions, out.data_ptr(), region_stride)
        assert st == 0, st

    def scaled(k):
        st = lib.jpeg_amd_decode_scaled_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, cosited,
                                              _lib.COLOR_RGB8, dmin, out.data_ptr(), 3 * sw * sh)
        assert st == 0, st

    paths = {"view": view, "region": region, "scaled": scaled}
    times = {k: [] for k in paths}
    for _ in range(args.rounds):
        for k, fn in paths.items():
            times[k].append(_timed(torch, fn, steps, args.warmup))
    tv = statistics.median(times["view"])
    hist = {d: sum(1 for v, _ in views if v == d) for d in (1, 2, 4, 8)}
    view_px = sum(r[2] * r[3] for _, r in views)
    need = sum(_head_bytes(L, cosited, d, r) for d, r in views) + 3 * view_px
    res = {"case": name, "size": [W, H], "n": n, "cosited": cosited, "denominators": hist, "smallest_denom": dmin,
           "view_pixels": view_px, "region_pixels": sum(s[2] * s[3] for s in source), "scaled_pixels": n * sw * sh,
           "t_view_us": _median(times["view"]), "t_region_us": _median(times["region"]), "t_scaled_us": _median(times["scaled"]),
           "view_over_region": round(tv / statistics.median(times["region"]), 4),
           "view_over_scaled": round(tv / statistics.median(times["scaled"]), 4),
           "view_needed_GBps": round(need / tv * 1e-3, 1), "view_Gpx_per_s": round(view_px / tv * 1e-3, 2),
           "rounds": {k: [round(t, 2) for t in v] for k, v in times.items()}}
    print(json.dumps(res), flush=True)
    del sets, out
    torch.cuda.empty_cache()
    return res


def case_centre(torch, ctx, args):
    lib = _lib.lib()
    W = H = 8192
    L = _layout(W, H)
    sets, ptrs, strides, q, sizes = _inputs(torch, ctx, L, 1, args.ring)
    out = torch.empty(3 * (W // 2) * (H // 2), dtype=torch.uint8, device=ctx.torch_device)
    res = {"case": "B", "size": [W, H], "n": 1, "cosited": 0, "denoms": {}}
    times = {}
    fns = []
    for denom in (2, 4, 8):
        region = J.view_of_source((W, H), denom, (W // 4, H // 4, W // 2, H // 2))
        h_view = _lib.View(denom, _lib.Region(*region))
        sw, sh = J.scaled_size((W, H), denom)

        def view(k, h_view=h_view):
            st = lib.jpeg_amd_decode_view_batch(ctx.handle, C.byref(L), 1, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, 0,
                                                _lib.COLOR_RGB8, C.byref(h_view), out.data_ptr(), 0)
            assert st == 0, st

        def scaled(k, denom=denom, sw=sw, sh=sh):
            st = lib.jpeg_amd_decode_scaled_batch(ctx.handle, C.byref(L), 1, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, 0,
                                                  _lib.COLOR_RGB8, denom, out.data_ptr(), 3 * sw * sh)
            assert st == 0, st

        fns += [((denom, "view"), view), ((denom, "scaled"), scaled)]
        res["denoms"][denom] = {"region": list(region), "needed_bytes": _head_bytes(L, 0, denom, region) + 3 * region[2] * region[3]}
    for key, _ in fns:
        times[key] = []
    for _ in range(args.rounds):
        for key, fn in fns:
            times[key].append(_timed(torch, fn, args.steps, args.warmup))
    for denom in (2, 4, 8):
        tv, ts = statistics.median(times[(denom, "view")]), statistics.median(times[(denom, "scaled")])
        d = res["denoms"][denom]
        d.update({"t_view_us": round(tv, 2), "t_scaled_us": round(ts, 2), "view_over_scaled": round(tv / ts, 4),
                  "view_needed_GBps": round(d["needed_bytes"] / tv * 1e-3, 1),
                  "rounds_view": [round(t, 2) for t in times[(denom, "view")]],
                  "rounds_scaled": [round(t, 2) for t in times[(denom, "scaled")]]})
    print(json.dumps(res), flush=True)
    del sets, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--cases", default="A,B,C")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_view: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    cases = set(args.cases.split(","))
    results = []
    if "A" in cases:
        results.append(case_crops(torch, ctx, "A", 0, args, args.steps))
    if "B" in cases:
        results.append(case_centre(torch, ctx, args))
    if "C" in cases:
        results.append(case_crops(torch, ctx, "C", 1, args, max(1, args.steps // 10)))   # whole-image decodes: fewer steps
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    for r in results:
        if r["case"] == "B":
            for d, x in r["denoms"].items():
                print(f"B: 8192x8192 centre 4096x4096 denom {d}:  view {x['t_view_us']:.1f} us  whole scaled {x['t_scaled_us']:.1f} us  "
                      f"view / scaled {x['view_over_scaled']:.3f}  needed bytes at {x['view_needed_GBps']:.0f} GB/s")
        else:
            print(f"{r['case']}: 256 x 1920x1080 {'cosited' if r['cosited'] else 'centred'} crops -> 224x224, denominators {r['denominators']}:  "
                  f"view {r['t_view_us']:.1f} us ({r['view_pixels'] / 1e6:.1f} Mpx)  (i) region {r['t_region_us']:.1f} us "
                  f"({r['region_pixels'] / 1e6:.1f} Mpx)  (ii) scaled at denom {r['smallest_denom']} {r['t_scaled_us']:.1f} us "
                  f"({r['scaled_pixels'] / 1e6:.1f} Mpx)  view / (i) {r['view_over_region']:.3f}  view / (ii) {r['view_over_scaled']:.3f}  "
                  f"{r['view_Gpx_per_s']:.1f} Gpx/s, needed bytes at {r['view_needed_GBps']:.0f} GB/s")


if __name__ == "__main__":
    main()
