#!/usr/bin/env python3
"""Entropy decoding on the GPU against the host threads, files to pixels in device memory:

    tools/bench_entropy_device.py --parent-lib PATH [--files 512] [--threads 16] [--reps 7] [--out profiles/entropy_device.json]

jpeg_amd_decompress_batch_device on N 1080p 4:2:0 files (8 distinct pictures, written by this library) with one restart
interval per MCU row, with one per 8 MCUs and without DRI, with `threads` host threads.  For each, in ALTERNATING runs on the
same box:
  on      a context with JPEG_AMD_CTX_DEVICE_ENTROPY, this tree's library;
  off     a context without the flag, the PARENT commit's library (--parent-lib: its libjpeg_amd.so, built from the parent);
  off_tree  a context without the flag, this tree's library (what the flag's absence costs: nothing should differ from `off`).
Wall time of the whole call (the pixels are in device memory when it returns).  `kernel_ms`: the time k_huffman_intervals
itself took per call of `on` (jpeg_amd_ctx_device_entropy_kernel_ms: HIP events around every launch, summed over the chunks);
`device_files`: how many of the N files took the device route.  The pixels of `on` and `off` are compared."""
import argparse, ctypes as C, json, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import jpeg_amd as J
from jpeg_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--files", type=int, default=512)
ap.add_argument("--threads", type=int, default=16)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()
import torch
lib = _lib.lib()
parent = C.CDLL(os.path.abspath(args.parent_lib))
for name in ("jpeg_amd_ctx_create", "jpeg_amd_decompress_batch_device"):
    getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]
ctx_on, ctx_off = J.Context(0, device_entropy=True), J.Context(0)
h_parent = C.c_void_p()
stream = torch.cuda.current_stream(ctx_off.torch_device).cuda_stream
assert parent.jpeg_amd_ctx_create(0, C.c_void_p(stream), 0, C.byref(h_parent)) == 0
W, H, N = 1920, 1080, args.files
layout = J.Layout("ycc8", {1: ((2, 2), 0), 2: ((1, 1), 1), 3: ((1, 1), 1)})
quanta = {0: J.compression_quanta("luminance", 0.5), 1: J.compression_quanta("chrominance", 0.5)}


def picture(k):
    yy, xx = np.mgrid[0:H, 0:W]
    rng = np.random.default_rng(k)
    img = np.clip(128 + 70 * np.sin(xx / (29.0 + k)) * np.cos(yy / (19.0 + k)) + rng.integers(-10, 11, (H, W)), 0, 255).astype(np.uint8)
    return np.stack([img, np.roll(img, 5, 0), np.roll(img, 9, 1)], -1).reshape(-1, 3)


def kernel_ms():
    ms = C.c_double()
    assert lib.jpeg_amd_ctx_device_entropy_kernel_ms(ctx_on.handle, C.byref(ms)) == 0
    return ms.value


rects = [J.Rectangular.pack(ctx_off, (W, H), layout, picture(k), J.RGB) for k in range(8)]
out = {k: torch.empty(N * W * H * 3, dtype=torch.uint8, device=ctx_off.torch_device) for k in ("on", "off")}
record = {"files": N, "size": [W, H], "threads": args.threads, "reps": args.reps, "device": torch.cuda.get_device_name(0),
          "call": "jpeg_amd_decompress_batch_device", "cases": []}
for label, ri in (("one interval per MCU row", W // 16), ("one interval per 8 MCUs", 8), ("no DRI", 0)):
    distinct = [np.frombuffer(r.compress(quanta, [[(0, 0, 0), (1, 1, 1), (2, 1, 1)]], restart_interval=ri), np.uint8).copy() for r in rects]
    files = [distinct[i % 8].copy() for i in range(N)]
    ptrs, sizes = (C.c_void_p * N)(*[f.ctypes.data for f in files]), (C.c_size_t * N)(*[f.size for f in files])

    def call(which, handle, into):
        st = which.jpeg_amd_decompress_batch_device(handle, ptrs, sizes, N, args.threads, 0, J.RGB.code, C.c_void_p(into.data_ptr()), 0, None)
        assert st == 0, st

    runs = (("on", lambda: call(lib, ctx_on.handle, out["on"])), ("off", lambda: call(parent, h_parent, out["off"])),
            ("off_tree", lambda: call(lib, ctx_off.handle, out["off"])))
    for _, fn in runs:                                  # warm-up: staging grown, threads started, pages touched
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(out["on"], out["off"]))
    times, k0, f0 = {name: [] for name, _ in runs}, kernel_ms(), ctx_on.device_entropy_files
    for _ in range(args.reps):
        for name, fn in runs:
            t0 = time.perf_counter()
            fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    case = {"case": label, "restart_interval": ri, "intervals_per_file": J.plan_intervals(files[0])[2], "file_bytes": int(files[0].size),
            "same_pixels": same, "device_files": (ctx_on.device_entropy_files - f0) // args.reps,
            "kernel_ms": round((kernel_ms() - k0) / args.reps, 3)}
    for name, ts in times.items():
        case[name + "_ms"] = {"min": round(min(ts), 3), "median": round(statistics.median(ts), 3), "max": round(max(ts), 3)}
    record["cases"].append(case)
    print(json.dumps(case), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)
