#!/usr/bin/env python3
"""tools/bench_warp_cubic.py -- the bicubic warp (k_mapped_tensor<ProjectiveMap, CubicTaps> over ProjectRecords; include/jpeg_amd.h, "bicubic warp")
against the bilinear warp on the same views and matrices and against the route a caller has today to a bicubic rotation,
alternating in one process.

    python tools/bench_warp_cubic.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 2] [--out profiles/warp_cubic.txt]

The method and the workload are tools/bench_warp.py's: each round times `steps` calls of each route between two HIP events on
the context's stream over a ring of `ring` input sets, host work included, and the report is the median per-call time over the
rounds.  Nothing is gated.  Case M of tools/bench_mixed.py: 256 images of seeded sizes and layouts, one seeded
RandomResizedCrop rectangle per image, to a [256, 3, 224, 224] fp16 CHW tensor with the ImageNet constants, every second image
flipped.  Whole calls, at angle 0 (edge "replicate") and at a seeded angle in +-30 degrees per image (edge "fill"):
  cubic0, cubic30    jpeg_amd.decode_tensors_warped_mixed(filter="bicubic")
  linear0, linear30  the same call with the bilinear filter: the parent's code, on views one pixel narrower on each side
  today30            decode_views_mixed, then per image affine_grid + grid_sample(mode="bicubic"), the flip, normalise and cast.
                     torch's cubic has a = -0.75: another filter, so the TIME is compared and the values are not
and the resample launch alone, on those views decoded once and packed outside the timed window (the C ABI called directly), in
both edge modes:
  k_cubic0, k_cubic30_fill, k_cubic30_replicate     jpeg_amd_project_filter_tensor_batch with JPEG_AMD_FILTER_BICUBIC
  k_linear0, k_linear30_fill, k_linear30_replicate  jpeg_amd_warp_tensor_batch on the same views and matrices
--kernels-only runs k_linear30_fill and k_cubic30_fill `steps` times each and nothing else, for a counter run of its own:
    rocprofv3 --pmc TCP_TCC_READ_REQ_sum --output-format csv -d DIR -- python tools/bench_warp_cubic.py --kernels-only --steps 3
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
from tools.bench_warp import _packed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_cubic.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="no timing: k_linear30_fill and k_cubic30_fill `steps` times each, for rocprofv3 --pmc")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_warp_cubic: no GPU (this tool measures the MI355X; there is no CPU number)")
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

    def cubic0(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m0, TARGET, spec, flips=flips, edge="replicate", filter="bicubic")

    def cubic30(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m30, TARGET, spec, flips=flips, edge="fill", filter="bicubic")

    _, views0, mv0 = cubic0(0)
    _, views30, mv30 = cubic30(0)

    def linear0(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m0, TARGET, spec, flips=flips, edge="replicate")

    def linear30(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m30, TARGET, spec, flips=flips, edge="fill")

    # theta of grid_sample for each of the rotated views: the pixel matrix between the two normalisations, in double
    thetas = []
    for v, m in zip(views30, mv30.astype(np.float64)):
        pix = np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0, 0, 1]])
        to_src = np.array([[2.0 / v[3], 0, -1], [0, 2.0 / v[4], -1], [0, 0, 1]])
        from_out = np.array([[wt / 2.0, 0, wt / 2.0], [0, ht / 2.0, ht / 2.0], [0, 0, 1]])
        thetas.append(torch.from_numpy((to_src @ pix @ from_out)[:2].astype(np.float32))[None].to(dev))

    def today30(k):
        pixels = J.decode_views_mixed(ctx, sets[k % args.ring], views30)
        for i, p in enumerate(pixels):
            grid = torch.nn.functional.affine_grid(thetas[i], (1, 3, ht, wt), align_corners=False)
            x = torch.nn.functional.grid_sample(p.permute(2, 0, 1)[None].float(), grid, mode="bicubic", padding_mode="zeros", align_corners=False)
            x = torch.floor(torch.clamp(x, 0.0, 255.0) + 0.5)
            if flips[i]:
                x = x.flip(3)
            batch[i] = ((x - mean) * scale).half()[0]
        return batch

    pixels0, pixels30 = J.decode_views_mixed(ctx, sets[0], views0), J.decode_views_mixed(ctx, sets[0], views30)
    src0, stride0, ext0 = _packed(torch, ctx, pixels0)
    src30, stride30, ext30 = _packed(torch, ctx, pixels30)
    h_flip = (C.c_uint8 * N)(*flips)
    replicate, fill = _lib.Warp(_lib.EDGE_REPLICATE, (C.c_uint8 * 3)(0, 0, 0)), _lib.Warp(_lib.EDGE_FILL, (C.c_uint8 * 3)(0, 0, 0))
    out = torch.empty(N * 3 * wt * ht, dtype=torch.float16, device=dev)
    pad = lambda m: np.ascontiguousarray(np.concatenate([m, np.tile(np.array([0, 0, 1], np.float32), (N, 1))], axis=1), np.float32)   # noqa: E731
    six = {0: np.ascontiguousarray(mv0, np.float32), 30: np.ascontiguousarray(mv30, np.float32)}
    nine = {0: pad(six[0]), 30: pad(six[30])}
    packed = {0: (src0, stride0, ext0), 30: (src30, stride30, ext30)}

    def k_cubic(angle, warp):
        src, stride, ext = packed[angle]
        return lambda k: _lib.check(lib.jpeg_amd_project_filter_tensor_batch(
            ctx.handle, N, src.data_ptr(), stride, ext, nine[angle].ctypes.data, C.byref(warp), _lib.FILTER_BICUBIC, wt, ht, C.byref(spec), h_flip,
            None, out.data_ptr(), 3 * wt * ht), "project_filter", ctx.handle)

    def k_linear(angle, warp):
        src, stride, ext = packed[angle]
        return lambda k: _lib.check(lib.jpeg_amd_warp_tensor_batch(
            ctx.handle, N, src.data_ptr(), stride, ext, six[angle].ctypes.data, C.byref(warp), wt, ht, C.byref(spec), h_flip, out.data_ptr(),
            3 * wt * ht), "warp", ctx.handle)

    launches = {"k_cubic0": k_cubic(0, replicate), "k_linear0": k_linear(0, replicate),
                "k_cubic30_fill": k_cubic(30, fill), "k_linear30_fill": k_linear(30, fill),
                "k_cubic30_replicate": k_cubic(30, replicate), "k_linear30_replicate": k_linear(30, replicate)}
    if args.kernels_only:                     # for a counter run: the two rotated launches alone, `steps` times each
        for name in ("k_linear30_fill", "k_cubic30_fill"):
            for k in range(args.steps):
                launches[name](k)
        ctx.synchronize()
        return
    routes = {"cubic0": cubic0, "linear0": linear0, "cubic30": cubic30, "linear30": linear30, "today30": today30, **launches}
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            slow = k == "today30"
            times[k].append(_timed(torch, fn, max(args.steps // 5, 2) if slow else args.steps, 1 if slow else args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    mpx = lambda v: round(float((v[:, 3].astype(np.int64) * v[:, 4]).sum()) / 1e6, 1)   # noqa: E731
    ratio = lambda a, b: round(med[a] / med[b], 3)   # noqa: E731
    res = {"n": N, "target": list(TARGET), "view_mpx_0": mpx(views0), "view_mpx_30": mpx(views30),
           **{f"t_{k}_us": round(v, 1) for k, v in med.items()},
           "cubic0_over_linear0": ratio("cubic0", "linear0"), "cubic30_over_linear30": ratio("cubic30", "linear30"),
           "today30_over_cubic30": round(med["today30"] / med["cubic30"], 1),
           "k_cubic0_over_linear0": ratio("k_cubic0", "k_linear0"), "k_cubic30_fill_over_linear": ratio("k_cubic30_fill", "k_linear30_fill"),
           "k_cubic30_replicate_over_linear": ratio("k_cubic30_replicate", "k_linear30_replicate"),
           "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
    lines = [f"# tools/bench_warp_cubic.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; times "
             f"are HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included",
             json.dumps(res),
             f"whole call: angle 0 bicubic {med['cubic0']:.0f} us = {res['cubic0_over_linear0']:.3f} x the bilinear warp "
             f"({med['linear0']:.0f} us, {res['view_mpx_0']} Mpx); +-30 degrees bicubic {med['cubic30']:.0f} us = "
             f"{res['cubic30_over_linear30']:.3f} x bilinear ({med['linear30']:.0f} us, {res['view_mpx_30']} Mpx); today (grid_sample bicubic, "
             f"a = -0.75: another filter, time only) {med['today30']:.0f} us = {res['today30_over_cubic30']:.1f} x",
             f"resample launch alone: angle 0 bicubic {med['k_cubic0']:.0f} us = {res['k_cubic0_over_linear0']:.3f} x bilinear "
             f"({med['k_linear0']:.0f} us); +-30 degrees fill {med['k_cubic30_fill']:.0f} us = {res['k_cubic30_fill_over_linear']:.3f} x "
             f"({med['k_linear30_fill']:.0f} us); replicate {med['k_cubic30_replicate']:.0f} us = {res['k_cubic30_replicate_over_linear']:.3f} x "
             f"({med['k_linear30_replicate']:.0f} us)"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
