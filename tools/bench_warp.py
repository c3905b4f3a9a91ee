#!/usr/bin/env python3
"""tools/bench_warp.py -- the warped resample (k_mapped_tensor<AffineMap, TwoTaps> over WarpRecords; include/jpeg_amd.h, "warped resample") against
the bilinear kernels on the same views and against the route a caller has today to a rotated crop, alternating in one process.

    python tools/bench_warp.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 2] [--out profiles/warp.txt]

The method is tools/bench_letterbox.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets, host work included, and the report is the median per-call time over the rounds.
Nothing is gated.  The workload is tools/bench_mixed.py's case M: 256 images of seeded sizes (sides 160 ... 1200) and a seeded
mix of 4:2:0, 4:4:4, 4:2:2 and grey, one seeded RandomResizedCrop rectangle per image, to a [256, 3, 224, 224] fp16 CHW tensor
with the ImageNet constants, every second image flipped.
  a          jpeg_amd.decode_tensors_warped_mixed, angle 0: affine_matrix of the crop rectangle, edge "replicate" -- the warp
             kernel does the bilinear kernel's work
  a_tables   jpeg_amd.decode_tensors_mixed on the views (a) decoded: the same decode, the bilinear kernel with its LDS tables.
             a / a_tables is the price of per-pixel coordinates against tables, through the whole call
  b          (a) with a seeded angle in +-30 degrees per image, edge "fill": larger views, and a fetch that is not along rows
  c          today's route to (b): jpeg_amd.decode_views_mixed, then per image affine_grid + grid_sample on the GPU, the flip,
             normalise and cast.  Its values agree with (b) within one level, not bit for bit
and the resample launch alone, on the views of (a) and of (b) decoded once and packed outside the timed window (the C ABI
called directly):
  k_tables   jpeg_amd_resize_tensor_batch on (a)'s views
  k_warp0    jpeg_amd_warp_tensor_batch on (a)'s views, angle 0
  k_warp30   jpeg_amd_warp_tensor_batch on (b)'s views, the seeded angles, edge "fill"; k_warp30_replicate: with "replicate"
--kernels-only runs those three launches `steps` times each and nothing else, for a counter run of its own:
    rocprofv3 --pmc TCP_TCC_READ_REQ_sum --output-format csv -d DIR -- python tools/bench_warp.py --kernels-only --steps 3
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
from tools.bench_mixed import MEAN, STD, _mixed_inputs  # noqa: E402
from tools.bench_resized import N  # noqa: E402
from tools.bench_view import TARGET, _timed, random_resized_crops  # noqa: E402


def _packed(torch, ctx, pixels):
    """Decoded views [h, w, 3] in one allocation -> (it, its stride, the c extents)."""
    stride = max(int(p.numel()) for p in pixels)
    src = torch.zeros(len(pixels) * stride, dtype=torch.uint8, device=ctx.torch_device)
    ext = (_lib.Extent * len(pixels))()
    for i, p in enumerate(pixels):
        src[i * stride:i * stride + p.numel()] = p.reshape(-1)
        ext[i].width, ext[i].height = int(p.shape[1]), int(p.shape[0])
    return src, stride, ext


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="no timing: k_tables, k_warp0 and k_warp30 `steps` times each, for rocprofv3 --pmc")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    lib = _lib.lib()
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    flips = [i & 1 for i in range(N)]
    rng = np.random.default_rng(20241019)
    names, sizes, sets, tables = _mixed_inputs(torch, ctx, rng, args.ring)
    crops = [random_resized_crops(rng, w, h, 1)[0] for w, h in sizes]
    angles = rng.uniform(-30.0, 30.0, N)
    m0 = np.stack([J.affine_matrix(s, TARGET, source_region=c) for s, c in zip(sizes, crops)])
    m30 = np.stack([J.affine_matrix(s, TARGET, angle=float(a), source_region=c) for s, c, a in zip(sizes, crops, angles)])
    wt, ht = TARGET
    mean = torch.tensor([spec.mean[c] for c in range(3)], device=dev).reshape(1, 3, 1, 1)
    scale = torch.tensor([spec.scale[c] for c in range(3)], device=dev).reshape(1, 3, 1, 1)
    batch = torch.empty((N, 3, ht, wt), dtype=torch.float16, device=dev)

    def a(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m0, TARGET, spec, flips=flips, edge="replicate")

    def b(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m30, TARGET, spec, flips=flips, edge="fill")

    _, views0, mv0 = a(0)
    want, views30, mv30 = b(0)

    def a_tables(k):
        return J.decode_tensors_mixed(ctx, sets[k % args.ring], views0, TARGET, spec, flips=flips)

    # theta of grid_sample for each of (b)'s views: the pixel matrix between the two normalisations, in double
    thetas = []
    for v, m in zip(views30, mv30.astype(np.float64)):
        pix = np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0, 0, 1]])
        to_src = np.array([[2.0 / v[3], 0, -1], [0, 2.0 / v[4], -1], [0, 0, 1]])
        from_out = np.array([[wt / 2.0, 0, wt / 2.0], [0, ht / 2.0, ht / 2.0], [0, 0, 1]])
        thetas.append(torch.from_numpy((to_src @ pix @ from_out)[:2].astype(np.float32))[None].to(dev))

    def c(k):
        pixels = J.decode_views_mixed(ctx, sets[k % args.ring], views30)
        for i, p in enumerate(pixels):
            grid = torch.nn.functional.affine_grid(thetas[i], (1, 3, ht, wt), align_corners=False)
            x = torch.nn.functional.grid_sample(p.permute(2, 0, 1)[None].float(), grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            x = torch.floor(torch.clamp(x, 0.0, 255.0) + 0.5)
            if flips[i]:
                x = x.flip(3)
            batch[i] = ((x - mean) * scale).half()[0]
        return batch

    # (c) gives (b)'s bytes within one level: compared as bytes, through the inverse of the normalisation
    back = lambda t: torch.round(t.float() / scale + mean)   # noqa: E731
    worst = float((back(c(0)) - back(want)).abs().max())          # (reported; tests/test_warp_cpu.py holds the bound)

    pixels0, pixels30 = J.decode_views_mixed(ctx, sets[0], views0), J.decode_views_mixed(ctx, sets[0], views30)
    src0, stride0, ext0 = _packed(torch, ctx, pixels0)
    src30, stride30, ext30 = _packed(torch, ctx, pixels30)
    h_flip = (C.c_uint8 * N)(*flips)
    replicate, fill = _lib.Warp(_lib.EDGE_REPLICATE, (C.c_uint8 * 3)(0, 0, 0)), _lib.Warp(_lib.EDGE_FILL, (C.c_uint8 * 3)(0, 0, 0))
    out = torch.empty(N * 3 * wt * ht, dtype=torch.float16, device=dev)
    mv0c, mv30c = np.ascontiguousarray(mv0, np.float32), np.ascontiguousarray(mv30, np.float32)

    def k_tables(k):
        _lib.check(lib.jpeg_amd_resize_tensor_batch(ctx.handle, N, src0.data_ptr(), stride0, ext0, wt, ht, C.byref(spec), h_flip, out.data_ptr(),
                                                    3 * wt * ht), "resize", ctx.handle)

    def k_warp0(k):
        _lib.check(lib.jpeg_amd_warp_tensor_batch(ctx.handle, N, src0.data_ptr(), stride0, ext0, mv0c.ctypes.data, C.byref(replicate), wt, ht,
                                                  C.byref(spec), h_flip, out.data_ptr(), 3 * wt * ht), "warp", ctx.handle)

    def k_warp30(k):
        _lib.check(lib.jpeg_amd_warp_tensor_batch(ctx.handle, N, src30.data_ptr(), stride30, ext30, mv30c.ctypes.data, C.byref(fill), wt, ht,
                                                  C.byref(spec), h_flip, out.data_ptr(), 3 * wt * ht), "warp", ctx.handle)

    def k_warp30_replicate(k):                 # the same matrices with the other edge mode: what of k_warp30 is the fill's
        _lib.check(lib.jpeg_amd_warp_tensor_batch(ctx.handle, N, src30.data_ptr(), stride30, ext30, mv30c.ctypes.data, C.byref(replicate), wt,
                                                  ht, C.byref(spec), h_flip, out.data_ptr(), 3 * wt * ht), "warp", ctx.handle)

    if args.kernels_only:                     # for a counter run: the three launches alone, `steps` times each
        for fn in (k_tables, k_warp0, k_warp30):
            for k in range(args.steps):
                fn(k)
        ctx.synchronize()
        return
    routes = {"a": a, "a_tables": a_tables, "b": b, "c": c, "k_tables": k_tables, "k_warp0": k_warp0, "k_warp30": k_warp30,
              "k_warp30_replicate": k_warp30_replicate}
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(_timed(torch, fn, max(args.steps // 5, 2) if k == "c" else args.steps, 1 if k == "c" else args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    mpx = lambda v: round(float((v[:, 3].astype(np.int64) * v[:, 4]).sum()) / 1e6, 1)   # noqa: E731
    res = {"n": N, "target": list(TARGET), "view_mpx_a": mpx(views0), "view_mpx_b": mpx(views30),
           "denoms_a": {d: int((views0[:, 0] == d).sum()) for d in (1, 2, 4, 8)}, "denoms_b": {d: int((views30[:, 0] == d).sum()) for d in (1, 2, 4, 8)},
           **{f"t_{k}_us": round(v, 1) for k, v in med.items()},
           "a_over_tables": round(med["a"] / med["a_tables"], 3), "b_over_a": round(med["b"] / med["a"], 3), "c_over_b": round(med["c"] / med["b"], 1),
           "k_warp0_over_tables": round(med["k_warp0"] / med["k_tables"], 3), "k_warp30_over_warp0": round(med["k_warp30"] / med["k_warp0"], 3),
           "c_worst_level": worst, "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
    lines = [f"# tools/bench_warp.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; times are "
             f"HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included",
             json.dumps(res),
             f"whole call: (a) angle 0 {med['a']:.0f} us = {res['a_over_tables']:.3f} x the bilinear kernels on the same views ({med['a_tables']:.0f} us, "
             f"{res['view_mpx_a']} Mpx); (b) +-30 degrees {med['b']:.0f} us = {res['b_over_a']:.3f} x (a) ({res['view_mpx_b']} Mpx); (c) today "
             f"{med['c']:.0f} us = {res['c_over_b']:.1f} x (b), within {worst:.0f} level",
             f"resample launch alone: tables {med['k_tables']:.0f} us, warp angle 0 {med['k_warp0']:.0f} us ({res['k_warp0_over_tables']:.3f} x), "
             f"warp +-30 degrees {med['k_warp30']:.0f} us ({res['k_warp30_over_warp0']:.3f} x angle 0; with edge \"replicate\" "
             f"{med['k_warp30_replicate']:.0f} us)"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
