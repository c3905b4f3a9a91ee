#!/usr/bin/env python3
"""tools/bench_colour.py -- the colour stage (include/jpeg_amd.h, "colour stage") against the same calls without it and against
the route a caller has today to a colour-jittered tensor, alternating in one process.

    python tools/bench_colour.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 2] [--out profiles/colour.txt]

The method is tools/bench_warp.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets, host work included, and the report is the median per-call time over the rounds.
Nothing is gated.  The workload is tools/bench_mixed.py's case M: 256 images, one seeded RandomResizedCrop rectangle per image,
to a [256, 3, 224, 224] fp16 CHW tensor with the ImageNet constants, every second image flipped.
  a          jpeg_amd.decode_tensors_mixed with a seeded colour_matrix per image and the clamp (0, 255)
  b          the same call without colour
  c          today's route: (b), then per image un-normalise, a 3 x 4 matrix product, clamp, normalise and cast in torch
and the resample launch alone, on the views decoded once and packed outside the timed window (the C ABI called directly), with
and without colour: k_placed / k_placed_colour (the bilinear placed kernel: whole-canvas windows) and k_warp / k_warp_colour
(the warp kernel, the crop's matrix at angle 0).  These windows hold the whole C call: the copy of the records (64-byte placed or
48-byte warp records per image, and with colour 48 bytes more per image, from pageable memory) as well as the kernel.
--kernels-only runs those four launches `steps` times each and nothing else, for runs of their own that look at the kernels alone:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_colour.py --kernels-only --steps 5
    rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_VMEM_RD SQ_WAVES --output-format csv -d DIR -- python tools/bench_colour.py --kernels-only --steps 3"""
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
from tools.bench_mixed import MEAN, STD, _mixed_inputs  # noqa: E402
from tools.bench_resized import N  # noqa: E402
from tools.bench_view import TARGET, _timed, random_resized_crops  # noqa: E402
from tools.bench_warp import _packed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colour.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="no timing: the four launches `steps` times each, for rocprofv3")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_colour: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    lib = _lib.lib()
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    flips = [i & 1 for i in range(N)]
    rng = np.random.default_rng(20241020)
    names, sizes, sets, tables = _mixed_inputs(torch, ctx, rng, args.ring)
    crops = [random_resized_crops(rng, w, h, 1)[0] for w, h in sizes]
    k = np.stack([J.colour_matrix(*rng.uniform(0.6, 1.4, 3), rng.uniform(-0.1, 0.1)) for _ in range(N)])
    wt, ht = TARGET
    mean = torch.tensor([spec.mean[c] for c in range(3)], device=dev).reshape(3, 1, 1)
    scale = torch.tensor([spec.scale[c] for c in range(3)], device=dev).reshape(3, 1, 1)
    kd = torch.from_numpy(k).to(dev)

    _, views = J.decode_crops_tensor_mixed(ctx, sets[0], crops, TARGET, spec, flips=flips)

    def a(i):
        return J.decode_tensors_mixed(ctx, sets[i % args.ring], views, TARGET, spec, flips=flips, colour=k, colour_clamp=(0, 255))

    def b(i):
        return J.decode_tensors_mixed(ctx, sets[i % args.ring], views, TARGET, spec, flips=flips)

    def c(i):
        t = b(i)
        for j in range(N):
            u = t[j].float() / scale + mean
            q = torch.clamp(torch.einsum("cd,dhw->chw", kd[j, :, :3], u) + kd[j, :, 3].reshape(3, 1, 1), 0.0, 255.0)
            t[j] = ((q - mean) * scale).half()
        return t

    worst = float(((c(0).float() - a(0).float()).abs() / scale.reshape(1, 3, 1, 1)).max())      # in levels; (c) is not bit exact

    pixels = J.decode_views_mixed(ctx, sets[0], views)
    src, stride, ext = _packed(torch, ctx, pixels)
    h_flip = (C.c_uint8 * N)(*flips)
    out = torch.empty(N * 3 * wt * ht, dtype=torch.float16, device=dev)
    kc = np.ascontiguousarray(k, np.float32).reshape(N, 12)
    col = _lib.Colour()
    col.h_matrices, col.lo, col.hi = kc.ctypes.data, 0.0, 255.0
    m0 = np.ascontiguousarray([[v[3] / wt, 0, 0, 0, v[4] / ht, 0] for v in views], np.float32)
    replicate = _lib.Warp(_lib.EDGE_REPLICATE, (C.c_uint8 * 3)(0, 0, 0))
    whole = (_lib.Region * N)(*[_lib.Region(0, 0, wt, ht)] * N)
    place = _lib.Placement()
    place.mode, place.h_windows = _lib.PLACE_WINDOWS, C.cast(whole, C.c_void_p)

    def placed(colour):
        def run(i):
            _lib.check(lib.jpeg_amd_resize_colour_tensor_batch(ctx.handle, N, src.data_ptr(), stride, ext, wt, ht, _lib.FILTER_BILINEAR,
                                                               C.byref(spec), h_flip, None, C.byref(place), None, colour, out.data_ptr(),
                                                               3 * wt * ht), "resize", ctx.handle)
        return run

    def warped(colour):
        def run(i):
            _lib.check(lib.jpeg_amd_warp_colour_tensor_batch(ctx.handle, N, src.data_ptr(), stride, ext, m0.ctypes.data, C.byref(replicate), wt,
                                                             ht, C.byref(spec), h_flip, colour, out.data_ptr(), 3 * wt * ht), "warp", ctx.handle)
        return run

    if args.kernels_only:                     # for a counter or a kernel-trace run: the four launches alone, `steps` times each
        for fn in (placed(None), placed(C.byref(col)), warped(None), warped(C.byref(col))):
            for i in range(args.steps):
                fn(i)
        ctx.synchronize()
        return
    routes = {"a": a, "b": b, "c": c, "k_placed": placed(None), "k_placed_colour": placed(C.byref(col)), "k_warp": warped(None),
              "k_warp_colour": warped(C.byref(col))}
    times = {r: [] for r in routes}
    for _ in range(args.rounds):
        for r, fn in routes.items():
            times[r].append(_timed(torch, fn, max(args.steps // 5, 2) if r == "c" else args.steps, 1 if r == "c" else args.warmup))
    med = {r: statistics.median(v) for r, v in times.items()}
    spread = {r: round((max(v) - min(v)) / statistics.median(v), 3) for r, v in times.items()}
    res = {"n": N, "target": list(TARGET), **{f"t_{r}_us": round(v, 1) for r, v in med.items()}, "a_over_b": round(med["a"] / med["b"], 3),
           "c_over_a": round(med["c"] / med["a"], 1), "k_placed_colour_over_plain": round(med["k_placed_colour"] / med["k_placed"], 3),
           "k_warp_colour_over_plain": round(med["k_warp_colour"] / med["k_warp"], 3), "spread": spread, "c_worst_level": round(worst, 3),
           "rounds": {r: [round(t, 1) for t in v] for r, v in times.items()}}
    lines = [f"# tools/bench_colour.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; times are "
             f"HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included; spread = (max - min) / median over the rounds",
             json.dumps(res),
             f"whole call: (a) with colour {med['a']:.0f} us = {res['a_over_b']:.3f} x (b) without {med['b']:.0f} us; (c) today {med['c']:.0f} us = "
             f"{res['c_over_a']:.1f} x (a), within {worst:.2f} level",
             f"resample launch alone: placed bilinear {med['k_placed']:.0f} us, with colour {med['k_placed_colour']:.0f} us "
             f"({res['k_placed_colour_over_plain']:.3f} x); warp {med['k_warp']:.0f} us, with colour {med['k_warp_colour']:.0f} us "
             f"({res['k_warp_colour_over_plain']:.3f} x)"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
