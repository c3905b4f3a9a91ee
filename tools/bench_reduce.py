#!/usr/bin/env python3
"""tools/bench_reduce.py -- spectral reduce (jpeg_amd_spectral_reduce_batch, k_spectral_reduce) against the routes a caller
had before it, alternating in one process (the method of tools/bench_scaled.py).

    python tools/bench_reduce.py [--steps 100] [--slow-steps 3] [--warmup 5] [--rounds 3] [--ring 4] [--json PATH] [--cases A,B]

Each round times the calls of each route between two HIP events on the context's stream, over a ring of `ring` input sets
(distinct coefficient buffers, together larger than the 256 MiB Infinity Cache); the report is the median per-call time
over the rounds.  Nothing is gated.  Routes, each from the same Spectral planes to the reduced Spectral planes:
  reduce  the one launch for every plane of every image
  staged  per image jpeg_amd_spectral_idct_scaled + jpeg_amd_planar_fdct (host tables, a launch per plane and stage, a
          uint16 plane through HBM) -- `slow-steps` steps where the batch makes it hundreds of calls
  pixels  jpeg_amd_decode_scaled_batch + jpeg_amd_encode_batch under the reduced layout (3 B / pixel out and in again;
          not the same coefficients: a second generation of chroma and colour rounding)
  copy    a device copy of the input's bytes (torch copy_), the yardstick of tools/bench_transform.py
Cases:
  A  8192 x 8192 4:2:0, denom 2, 4, 8
  B  256 x 1920 x 1080 4:2:0, denom 2, 4, 8
Kernel times: run it again under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_reduce.py --steps 20 --rounds 1`.
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

DENOMS = (2, 4, 8)
ROUTES = ("reduce", "staged", "pixels", "copy")


def _layout(w, h):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes, L.scale_x, L.scale_y = w, h, 8, 3, 2, 2
    for p, f in enumerate((2, 1, 1)):
        L.factor_x[p] = L.factor_y[p] = f
        L.qi[p] = min(p, 1)
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def _sizes(L):
    return [64 * L.units_x[p] * L.units_y[p] for p in range(L.nplanes)]


def _case(torch, ctx, name, W, H, n, args):
    lib = _lib.lib()
    L = _layout(W, H)
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(7)
    sizes = _sizes(L)
    ring = [[torch.randint(-256, 256, (n * s,), dtype=torch.int16, device=dev, generator=gen) for s in sizes]
            for _ in range(args.ring)]
    q = torch.randint(1, 8, (2 * 64,), dtype=torch.int16, device=dev, generator=gen)
    qh = np.ascontiguousarray(q.cpu().numpy().astype(np.uint16))
    strides = _lib.size_array(sizes)
    ptrs = [_lib.ptr_array([t.data_ptr() for t in s]) for s in ring]
    copy_dst = [torch.empty_like(t) for t in ring[0]]
    slow = args.slow_steps if n > 1 else args.steps
    res = {"case": name, "size": [W, H], "n": n, "input_MB": round(2 * n * sum(sizes) / 1e6, 1), "denoms": {}}

    def timed(fn, steps):
        for k in range(min(args.warmup, steps)):
            fn(k)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for k in range(steps):
            fn(k)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / steps * 1e3   # us per call

    for denom in DENOMS:
        O = _lib.Layout()
        S = _lib.Layout()
        assert lib.jpeg_amd_reduce_layout(C.byref(L), denom, C.byref(O)) == 0
        assert lib.jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(S)) == 0
        osizes = _sizes(O)
        assert osizes == _sizes(S)                           # 4:2:0: the factors divide the scale
        outs = [torch.empty(n * s, dtype=torch.int16, device=dev) for s in osizes]
        optrs = _lib.ptr_array([t.data_ptr() for t in outs])
        ostrides = _lib.size_array(osizes)
        samples = [torch.empty(s, dtype=torch.int16, device=dev) for s in osizes]
        sptrs = _lib.ptr_array([t.data_ptr() for t in samples])
        pixels = torch.empty(n * 3 * O.width * O.height, dtype=torch.uint8, device=dev)

        def reduce(k):
            st = lib.jpeg_amd_spectral_reduce_batch(ctx.handle, C.byref(L), n, denom, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2,
                                                    None, optrs, ostrides)
            assert st == 0, st

        def staged(k):
            src = ring[k % args.ring]
            for i in range(n):
                ip = _lib.ptr_array([t.data_ptr() + 2 * i * s for t, s in zip(src, sizes)])
                op = _lib.ptr_array([t.data_ptr() + 2 * i * s for t, s in zip(outs, osizes)])
                assert lib.jpeg_amd_spectral_idct_scaled(ctx.handle, C.byref(L), ip, qh.ctypes.data, 2, denom, sptrs) == 0
                assert lib.jpeg_amd_planar_fdct(ctx.handle, C.byref(S), sptrs, qh.ctypes.data, 2, op) == 0

        def through_pixels(k):
            st = lib.jpeg_amd_decode_scaled_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, 0,
                                                  _lib.COLOR_YCC8, denom, pixels.data_ptr(), 3 * O.width * O.height)
            assert st == 0, st
            st = lib.jpeg_amd_encode_batch(ctx.handle, C.byref(O), n, pixels.data_ptr(), 3 * O.width * O.height, _lib.COLOR_YCC8,
                                           q.data_ptr(), 0, 2, optrs, ostrides)
            assert st == 0, st

        def copy(k):
            for d, s in zip(copy_dst, ring[k % args.ring]):
                d.copy_(s)

        fns = {"reduce": (reduce, args.steps), "staged": (staged, slow), "pixels": (through_pixels, args.steps), "copy": (copy, args.steps)}
        times = {r: [] for r in ROUTES}
        for _ in range(args.rounds):
            for r in ROUTES:
                times[r].append(timed(*fns[r]))
        med = {r: statistics.median(times[r]) for r in ROUTES}
        head = {2: 64, 4: 16, 8: 2}[denom]
        need = n * sum(sizes) // 64 * head + 2 * n * sum(osizes)      # the block heads read, the coefficients written
        res["denoms"][denom] = {
            **{f"t_{r}_us": round(med[r], 2) for r in ROUTES},
            "staged_over_reduce": round(med["staged"] / med["reduce"], 2),
            "pixels_over_reduce": round(med["pixels"] / med["reduce"], 2),
            "reduce_over_copy": round(med["reduce"] / med["copy"], 3),
            "needed_GBps": round(need / med["reduce"] * 1e-3, 1),
            "rounds": {r: [round(x, 2) for x in times[r]] for r in ROUTES}}
        print(json.dumps({"case": name, "denom": denom, **res["denoms"][denom]}), flush=True)
        del outs, samples, pixels
    del ring, copy_dst
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--slow-steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--cases", default="A,B")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_reduce: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    cases = set(args.cases.split(","))
    results = []
    if "A" in cases:
        results.append(_case(torch, ctx, "A", 8192, 8192, 1, args))
    if "B" in cases:
        results.append(_case(torch, ctx, "B", 1920, 1080, 256, args))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    for r in results:
        for d in DENOMS:
            x = r["denoms"][d]
            print(f"{r['case']}: {r['size'][0]}x{r['size'][1]} n={r['n']} denom {d}:  reduce {x['t_reduce_us']:.1f} us  "
                  f"staged {x['t_staged_us']:.1f} us ({x['staged_over_reduce']:.2f}x)  pixels {x['t_pixels_us']:.1f} us "
                  f"({x['pixels_over_reduce']:.2f}x)  copy of the input {x['t_copy_us']:.1f} us (reduce / copy {x['reduce_over_copy']:.3f})  "
                  f"needed bytes at {x['needed_GBps']:.0f} GB/s")


if __name__ == "__main__":
    main()
