#!/usr/bin/env python3
"""tools/bench_transform.py -- the lossless spectral transforms (kernels_transform.hip) against a device-to-device copy.

    python tools/bench_transform.py [--calls 200] [--rounds 5] [--files 200] [--json PATH]

Each case times `calls` warmed calls of jpeg_amd_spectral_transform_batch between two HIP events, alternating in the same
process with `calls` torch copy_ calls of the same bytes (the yardstick: what moving the planes costs at all), `rounds`
times; it reports the median per-call time of each, TB/s (bytes read + written over the call time) and the fraction of
8 TB/s.  Cases: 8192 x 8192 4:2:0 with NONE, TRANSPOSE, ROT_CCW and ROT_180, each without and with requantisation, and
one batch of 64 1920 x 1080 4:2:0 images.  Then jpeg_amd_transform (file to file, ROT_CCW) on a 1080p 4:2:0 file:
files per second, host-bound (entropy decoding and writing on the host), reported and not gated.

Kernel times from the trace: run it again under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_transform.py
--calls 20 --rounds 1 --files 0`.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeg_amd as J  # noqa: E402
from jpeg_amd import _lib  # noqa: E402

PEAK = 8.0e12
OPS = {"none": 0, "transpose": 1, "rot_ccw": 5, "rot_180": 6}


def _layout(w, h):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes, L.scale_x, L.scale_y = w, h, 8, 3, 2, 2
    for p, f in enumerate((2, 1, 1)):
        L.factor_x[p] = L.factor_y[p] = f
        L.qi[p] = min(p, 1)
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def _case(torch, ctx, name, w, h, n, op, requant, calls, rounds):
    lib = _lib.lib()
    L = _layout(w, h)
    out = _lib.Layout()
    assert lib.jpeg_amd_transform_layout(C.byref(L), op, None, C.byref(out)) == 0
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(7)
    sizes_in = [64 * L.units_x[p] * L.units_y[p] for p in range(3)]
    sizes_out = [64 * out.units_x[p] * out.units_y[p] for p in range(3)]
    src = [torch.randint(-64, 64, (n * s,), dtype=torch.int16, device=dev, generator=gen) for s in sizes_in]
    dst = [torch.empty(n * s, dtype=torch.int16, device=dev) for s in sizes_out]
    q = torch.randint(1, 8, (2 * 64,), dtype=torch.int16, device=dev, generator=gen)
    qo = torch.randint(1, 255, (2 * 64,), dtype=torch.int16, device=dev, generator=gen)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    flat_in = torch.randint(-64, 64, (n * sum(sizes_in),), dtype=torch.int16, device=dev, generator=gen)
    flat_out = torch.empty_like(flat_in)
    args = (ctx.handle, C.byref(L), n, op, None, _lib.ptr_array([t.data_ptr() for t in src]), _lib.size_array(sizes_in),
            q.data_ptr(), 0, 2, qo.data_ptr() if requant else None, _lib.ptr_array([t.data_ptr() for t in dst]),
            _lib.size_array(sizes_out), flag.data_ptr())

    def xform():
        _lib.check(lib.jpeg_amd_spectral_transform_batch(*args), "jpeg_amd_spectral_transform_batch", ctx.handle)

    def copy():
        flat_out.copy_(flat_in)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / calls       # us per call

    for _ in range(20):                               # warm both
        xform(); copy()
    torch.cuda.synchronize()
    tx, tc = [], []
    for _ in range(rounds):
        tx.append(timed(xform))
        tc.append(timed(copy))
    assert int(flag.item()) == 0
    nbytes = 2 * 2 * n * sum(sizes_in)                # read + write, int16
    ux, uc = float(np.median(tx)), float(np.median(tc))
    r = {"case": name, "op": op, "requant": requant, "images": n, "bytes_moved": nbytes,
         "transform_us": round(ux, 2), "copy_us": round(uc, 2), "ratio": round(ux / uc, 3),
         "transform_TBps": round(nbytes / ux / 1e6, 3), "copy_TBps": round(nbytes / uc / 1e6, 3),
         "transform_frac_8TBps": round(nbytes / ux / 1e6 / 8.0, 3), "copy_frac_8TBps": round(nbytes / uc / 1e6 / 8.0, 3),
         "transform_us_rounds": [round(t, 2) for t in tx], "copy_us_rounds": [round(t, 2) for t in tc]}
    print(json.dumps(r), flush=True)
    del src, dst, flat_in, flat_out
    torch.cuda.empty_cache()
    return r


def _files(ctx, nfiles):
    """jpeg_amd_transform, ROT_CCW, on one 1080p 4:2:0 file of photo-like sparsity."""
    rng = np.random.default_rng(3)
    size = (1920, 1080)
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    planes = []
    for ux, uy in layout.units(size):
        p = np.zeros((uy, ux, 64), np.int16)
        p[..., 0] = rng.integers(-200, 200, (uy, ux))
        p[..., 1:6] = rng.integers(-12, 12, (uy, ux, 5))
        planes.append(p)
    quanta = [J.compression_quanta("luminance", 1.0), J.compression_quanta("chrominance", 1.0)]
    sp = J.Spectral.from_host(ctx, size, layout, planes, quanta)
    data = np.frombuffer(sp.compress([[(0, 0, 0)], [(1, 1, 1), (2, 1, 1)]]), np.uint8).copy()
    lib = _lib.lib()
    out = np.empty(4 * data.size + (1 << 20), np.uint8)
    n = C.c_size_t()

    def one():
        _lib.check(lib.jpeg_amd_transform(ctx.handle, data.ctypes.data, data.size, 5, None, None, 0, out.ctypes.data, out.size,
                                          C.byref(n), None), "jpeg_amd_transform", ctx.handle)
    for _ in range(5):
        one()
    t0 = time.perf_counter()
    for _ in range(nfiles):
        one()
    dt = time.perf_counter() - t0
    r = {"case": "jpeg_amd_transform 1920x1080 4:2:0 ROT_CCW (file to file)", "file_bytes": int(data.size),
         "files": nfiles, "files_per_s": round(nfiles / dt, 1), "ms_per_file": round(dt / nfiles * 1e3, 3)}
    print(json.dumps(r), flush=True)
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=40, help="calls per round (rounds x calls >= 200 by default)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--files", type=int, default=200)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_transform: no GPU (there is nothing to measure on the CPU)")
    ctx = J.Context(0)
    results = []
    for requant in (False, True):
        for name, op in OPS.items():
            results.append(_case(torch, ctx, f"8192x8192 4:2:0 {name}", 8192, 8192, 1, op, requant, a.calls, a.rounds))
    for name in ("none", "rot_ccw"):
        results.append(_case(torch, ctx, f"64 x 1920x1080 4:2:0 {name}", 1920, 1080, 64, OPS[name], False, a.calls, a.rounds))
    if a.files:
        results.append(_files(ctx, a.files))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
