#!/usr/bin/env python3
"""tools/bench_tensor_encode.py -- the tensor sources of the encoder (jpeg_amd_encode_tensor_batch: one k_tensor_pixels launch
into a context buffer, then the fused encoder) against what a caller runs today in framework ops in front of the byte call,
alternating in one process.

    python tools/bench_tensor_encode.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 3] [--out profiles/tensor_encode.txt]

The method is tools/bench_tensor.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input tensors; the report is the median per-call time over the rounds.  Nothing is gated.  Every
case is 4:2:0, RGB, the ImageNet constants (elements in normalised units):
  256 x [3, 224, 224] fp16 CHW;  64 x [3, 1080, 1920] fp16 CHW;  1 x [3, 4096, 4096] fp16 CHW;  1 x [4096, 4096, 3] fp32 HWC
  a  tensor   jpeg_amd_encode_tensor_batch: the one call
  b  today    float, mul, add, clamp, round, to(uint8), permute, contiguous in torch, then jpeg_amd_encode_batch
  c  bytes    jpeg_amd_encode_batch alone on ready bytes
  d  front    jpeg_amd_tensor_pixels_batch alone
  e  copy     a device-to-device copy that moves what the front moves: (elements in + bytes out) / 2 bytes read and written
a - c is what the intermediate costs (the front launch and the bytes' trip through memory); d against e says how far the front
is from a plain copy of the same traffic.  All are host-inclusive: the events bracket whatever the calls enqueue.  torch's
round is half-to-even and the contract's is half-up, so b's bytes may differ from a's on exact ties; the count is reported.
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
from tools.bench_view import _timed  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
CASES = [("256 x 224x224 fp16 chw", 256, 224, 224, "float16", "chw"), ("64 x 1920x1080 fp16 chw", 64, 1920, 1080, "float16", "chw"),
         ("1 x 4096x4096 fp16 chw", 1, 4096, 4096, "float16", "chw"), ("1 x 4096x4096 fp32 hwc", 1, 4096, 4096, "float32", "hwc")]


def run_case(torch, ctx, args, name, n, w, h, dtype_name, layout_name):
    lib = _lib.lib()
    dev = ctx.torch_device
    dtype = getattr(torch, dtype_name)
    chw = layout_name == "chw"
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    units = layout.units((w, h))
    L = layout.c_layout((w, h), units, [0, 1, 1])
    tables = np.stack([J.compression_quanta("luminance", 1.0), J.compression_quanta("chrominance", 1.0)]).astype(np.uint16)
    dq = ctx.upload(tables)
    source = J.tensor_source(MEAN, STD, dtype=dtype, layout=layout_name)
    scale = torch.tensor(list(source.scale), dtype=torch.float32, device=dev).view((1, 3, 1, 1) if chw else (1, 1, 1, 3))
    offset = torch.tensor(list(source.offset), dtype=torch.float32, device=dev).view((1, 3, 1, 1) if chw else (1, 1, 1, 3))
    gen = torch.Generator(device=dev).manual_seed(20240809)
    npx = 3 * w * h
    ring = []
    for _ in range(args.ring):          # bytes a little beyond both ends of the clamp, as normalised elements
        t = torch.rand((n, 3, h, w) if chw else (n, h, w, 3), dtype=torch.float32, device=dev, generator=gen).mul_(275.0).sub_(10.0)
        ring.append(t.sub_(offset).div_(scale).to(dtype))
        del t
    planes = [ctx.empty(n * 64 * ux * uy, torch.int16) for ux, uy in units]
    ptrs, strides = J.api._ptrs(planes), _lib.size_array([64 * ux * uy for ux, uy in units])
    pixels = ctx.empty(n * npx, torch.uint8)
    elem = ring[0].element_size()
    half = ctx.empty((n * npx * elem + n * npx) // 2, torch.uint8)
    half_dst = torch.empty_like(half)

    def check(st):
        assert st == 0, st

    def tensor(k):
        check(lib.jpeg_amd_encode_tensor_batch(ctx.handle, C.byref(L), n, ring[k % args.ring].data_ptr(), npx, C.byref(source), J.RGB.code,
                                               dq.data_ptr(), 0, 2, ptrs, strides))

    def chain(t):
        u = t.float().mul_(scale).add_(offset).clamp_(0.0, 255.0).round_().to(torch.uint8)
        return u.permute(0, 2, 3, 1).contiguous() if chw else u.contiguous()

    def today(k):
        u = chain(ring[k % args.ring])
        check(lib.jpeg_amd_encode_batch(ctx.handle, C.byref(L), n, u.data_ptr(), npx, J.RGB.code, dq.data_ptr(), 0, 2, ptrs, strides))

    def bytes_only(k):
        check(lib.jpeg_amd_encode_batch(ctx.handle, C.byref(L), n, pixels.data_ptr(), npx, J.RGB.code, dq.data_ptr(), 0, 2, ptrs, strides))

    def front(k):
        check(lib.jpeg_amd_tensor_pixels_batch(ctx.handle, n, ring[k % args.ring].data_ptr(), npx, w, h, C.byref(source), pixels.data_ptr(), npx))

    def copy(k):
        half_dst.copy_(half)

    front(0)
    differ = int((pixels.view(n, h, w, 3) != chain(ring[0])).sum())
    routes = {"tensor": tensor, "today": today, "bytes": bytes_only, "front": front, "copy": copy}
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(_timed(torch, fn, args.steps, args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    moved = n * npx * (elem + 1)
    res = {"case": name, "n": n, "size": [w, h], "dtype": dtype_name, "layout": layout_name, "t_tensor_us": round(med["tensor"], 1),
           "t_today_us": round(med["today"], 1), "t_bytes_us": round(med["bytes"], 1), "t_front_us": round(med["front"], 1),
           "t_copy_us": round(med["copy"], 1), "intermediate_us": round(med["tensor"] - med["bytes"], 1),
           "today_over_tensor": round(med["today"] / med["tensor"], 2), "front_over_copy": round(med["front"] / med["copy"], 2),
           "front_GBps": round(moved / med["front"] / 1e3, 1), "today_bytes_differing_from_contract": differ,
           "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
    line = (f"{name}:  a tensor {med['tensor']:.0f} us  b today {med['today']:.0f} us ({res['today_over_tensor']:.2f} x)  c bytes "
            f"{med['bytes']:.0f} us  a - c {res['intermediate_us']:.0f} us  d front {med['front']:.0f} us ({res['front_GBps']:.0f} GB/s)  "
            f"e copy {med['copy']:.0f} us (d / e {res['front_over_copy']:.2f})")
    return res, line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_encode.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensor_encode: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    lines = [f"# tools/bench_tensor_encode.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; "
             "times are HIP-event medians per call, host work included; 4:2:0, RGB, ImageNet constants"]
    tail = []
    for case in CASES:
        res, line = run_case(torch, ctx, args, *case)
        lines.append(json.dumps(res))
        tail.append(line)
        torch.cuda.empty_cache()
    lines += tail
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
