#!/usr/bin/env python3
"""tools/bench_scaled.py -- scaled decode (jpeg_amd_decode_scaled_batch: k_scaled_decode, and the k_idct_scaled fallback)
against the full decode of the same inputs (jpeg_amd_decode_batch), alternating in one process.

    python tools/bench_scaled.py [--steps 200] [--warmup 20] [--rounds 5] [--ring 4] [--json PATH] [--cases A,B,C]
                                 [--layout 420|y8] [--color rgb|ycc]

Each round times `steps` calls of each path between two HIP events on the context's stream -- the three denominators, then
the full decode -- over a ring of `ring` input sets (distinct coefficient buffers, together larger than the 256 MiB Infinity
Cache, as bench.py does); the report is the median per-call time over the rounds.  Nothing is gated.  Cases:
  A  8192 x 8192 4:2:0 RGB, denom 2, 4, 8
  B  256 x 1920 x 1080 4:2:0 RGB, denom 2, 4, 8
  C  4096 x 4096 4:2:0 cosited (the fallback: k_idct_scaled planes + the staged interleave kernel), denom 2, 4, 8
--layout y8 and --color ycc run the same cases with grey images and to YCbCr bytes: with the defaults, the four kinds of
k_scaled_decode<N, planes, rgb> at each N.
Kernel times: run it again under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_scaled.py --steps 20 --rounds 1`.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeg_amd as J  # noqa: E402
from jpeg_amd import _lib  # noqa: E402

DENOMS = (2, 4, 8)


def _layout(w, h, grey=False):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes, L.scale_x, L.scale_y = (w, h, 8, 1, 1, 1) if grey else (w, h, 8, 3, 2, 2)
    for p, f in enumerate((1,) if grey else (2, 1, 1)):
        L.factor_x[p] = L.factor_y[p] = f
        L.qi[p] = min(p, 1)
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def _case(torch, ctx, name, W, H, n, cosited, args):
    lib = _lib.lib()
    L = _layout(W, H, args.layout == "y8")
    color = _lib.COLOR_YCC8 if args.color == "ycc" else _lib.COLOR_RGB8
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(7)
    sizes = [64 * L.units_x[p] * L.units_y[p] for p in range(L.nplanes)]
    ring = [[torch.randint(-256, 256, (n * s,), dtype=torch.int16, device=dev, generator=gen) for s in sizes]
            for _ in range(args.ring)]
    q = torch.randint(1, 8, (2 * 64,), dtype=torch.int16, device=dev, generator=gen)
    strides = _lib.size_array(sizes)
    full_stride = 3 * W * H
    full = torch.empty(n * full_stride, dtype=torch.uint8, device=dev)
    out = torch.empty(n * 3 * ((W + 1) // 2) * ((H + 1) // 2), dtype=torch.uint8, device=dev)
    ptrs = [_lib.ptr_array([t.data_ptr() for t in s]) for s in ring]

    def scaled(denom):
        w, h = J.scaled_size((W, H), denom)

        def fn(k):
            st = lib.jpeg_amd_decode_scaled_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2,
                                                  cosited, color, denom, out.data_ptr(), 3 * w * h)
            assert st == 0, st
        return fn

    def whole(k):
        st = lib.jpeg_amd_decode_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, cosited,
                                       color, full.data_ptr(), full_stride)
        assert st == 0, st

    def timed(fn):
        for k in range(args.warmup):
            fn(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(args.steps):
            fn(k)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.steps * 1e3   # us per call

    times = {d: [] for d in DENOMS + (1,)}
    for _ in range(args.rounds):
        for d in DENOMS:
            times[d].append(timed(scaled(d)))
        times[1].append(timed(whole))
    tf = statistics.median(times[1])
    res = {"case": name, "layout": args.layout, "color": args.color, "size": [W, H], "n": n, "cosited": cosited, "t_full_us": round(tf, 2),
           "t_full_rounds": [round(t, 2) for t in times[1]], "denoms": {}}
    px = n * W * H
    for d in DENOMS:
        t = statistics.median(times[d])
        w, h = J.scaled_size((W, H), d)
        # bytes the contract needs: the head of every block (32 / 8 / 1 int16 of 64) and the scaled pixels
        head = {2: 64, 4: 16, 8: 2}[d]
        need = n * sum(sizes) // 64 * head + 3 * n * w * h
        res["denoms"][d] = {"t_us": round(t, 2), "ratio": round(t / tf, 4), "speedup": round(tf / t, 2),
                            "needed_GBps": round(need / t * 1e-3, 1), "rounds": [round(x, 2) for x in times[d]]}
    res["full_GBps"] = round((n * sum(sizes) * 2 + 3 * px) / tf * 1e-3, 1)
    print(json.dumps(res), flush=True)
    del ring, full, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--cases", default="A,B,C")
    ap.add_argument("--json", default=None)
    ap.add_argument("--layout", choices=["420", "y8"], default="420")
    ap.add_argument("--color", choices=["rgb", "ycc"], default="rgb")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_scaled: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    cases = set(args.cases.split(","))
    results = []
    if "A" in cases:
        results.append(_case(torch, ctx, "A", 8192, 8192, 1, 0, args))
    if "B" in cases:
        results.append(_case(torch, ctx, "B", 1920, 1080, 256, 0, args))
    if "C" in cases:
        results.append(_case(torch, ctx, "C", 4096, 4096, 1, 1, args))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    for r in results:
        for d in DENOMS:
            x = r["denoms"][d]
            print(f"{r['case']}: {r['size'][0]}x{r['size'][1]} n={r['n']} {'cosited' if r['cosited'] else 'centred'} denom {d}:  "
                  f"scaled {x['t_us']:.1f} us  full {r['t_full_us']:.1f} us  ratio {x['ratio']:.3f}  speedup {x['speedup']:.2f}x  "
                  f"needed bytes at {x['needed_GBps']:.0f} GB/s (full decode: {r['full_GBps']:.0f} GB/s)")


if __name__ == "__main__":
    main()
