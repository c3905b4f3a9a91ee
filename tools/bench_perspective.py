#!/usr/bin/env python3
"""tools/bench_perspective.py -- the projective resample (k_mapped_tensor<ProjectiveMap, TwoTaps> over ProjectRecords; include/jpeg_amd.h, "projective
resample") against the affine warp on identical matrices and against the route a caller has today to a perspective crop,
alternating in one process.

    python tools/bench_perspective.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 2] [--out profiles/perspective.txt]

The method is tools/bench_warp.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets, host work included, and the report is the median per-call time over the rounds.
Nothing is gated.  The workload is tools/bench_mixed.py's case M: 256 images of seeded sizes (sides 160 ... 1200) and a seeded
mix of 4:2:0, 4:4:4, 4:2:2 and grey, one seeded RandomResizedCrop rectangle per image, to a [256, 3, 224, 224] fp16 CHW tensor
with the ImageNet constants, every second image flipped, edge "fill".
  a_warp     jpeg_amd.decode_tensors_warped_mixed on affine_matrix of the crop rectangle (angle 0): the existing kernel
  a          jpeg_amd.decode_tensors_projected_mixed on the same matrices with the last row (0, 0, 1): the same views, the same
             bytes; a / a_warp is the price of the division and the wider record through the whole call
  a_warp2    a_warp once more, behind (a): the first route of a round runs behind (c), today's torch route, and its host work
             measures slower for it; a / a_warp2 is the comparison in like position
  b          (a) with a seeded four-corner distortion of the crop rectangle per image (distortion_scale = 0.5: each corner
             pulled in by up to a quarter of the side)
  c          today's route to (b): jpeg_amd.decode_views_mixed of the WHOLE images (nothing tells which part the canvas reads),
             then per image a grid from the homography + grid_sample on the GPU, the flip, normalise and cast.  Its values agree
             with (b) within one level, not bit for bit
and the resample launch alone, on the views of (a) and of (b) decoded once and packed outside the timed window (the C ABI
called directly):
  k_warp     jpeg_amd_warp_tensor_batch on (a)'s views
  k_project  jpeg_amd_project_tensor_batch on (a)'s views, the same matrices with the last row (0, 0, 1)
  k_persp    jpeg_amd_project_tensor_batch on (b)'s views, the seeded distortions
--kernels-only runs those three launches `steps` times each and nothing else, for a counter run of its own:
    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVE_CYCLES SQ_WAIT_INST_ANY --output-format csv -d DIR -- python tools/bench_perspective.py --kernels-only --steps 3
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


def distorted_crop(rng, crop, target, scale=0.5):
    """The canvas's corners onto the corners of `crop` (x, y, width, height), each pulled inwards by up to scale / 2 of the side:
    torchvision's RandomPerspective on the crop.  float64 [3, 3]"""
    x, y, w, h = crop
    d = [(rng.uniform(0, scale / 2) * w, rng.uniform(0, scale / 2) * h) for _ in range(4)]
    src = [(x + d[0][0], y + d[0][1]), (x + w - d[1][0], y + d[1][1]), (x + w - d[2][0], y + h - d[2][1]), (x + d[3][0], y + h - d[3][1])]
    return J.perspective_matrix(src, [(0, 0), (target[0], 0), (target[0], target[1]), (0, target[1])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "perspective.txt"))
    ap.add_argument("--kernels-only", action="store_true", help="no timing: k_warp, k_project and k_persp `steps` times each, for rocprofv3 --pmc")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_perspective: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    lib = _lib.lib()
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    flips = [i & 1 for i in range(N)]
    rng = np.random.default_rng(20241020)
    names, sizes, sets, tables = _mixed_inputs(torch, ctx, rng, args.ring)
    crops = [random_resized_crops(rng, w, h, 1)[0] for w, h in sizes]
    m6 = np.stack([J.affine_matrix(s, TARGET, source_region=c) for s, c in zip(sizes, crops)])
    m9 = np.concatenate([m6, np.tile(np.array([0, 0, 1], np.float32), (N, 1))], axis=1)
    mp = np.stack([distorted_crop(rng, c, TARGET).reshape(9) for c in crops]).astype(np.float32)
    wt, ht = TARGET
    mean = torch.tensor([spec.mean[c] for c in range(3)], device=dev).reshape(1, 3, 1, 1)
    scale = torch.tensor([spec.scale[c] for c in range(3)], device=dev).reshape(1, 3, 1, 1)
    batch = torch.empty((N, 3, ht, wt), dtype=torch.float16, device=dev)

    def a_warp(k):
        return J.decode_tensors_warped_mixed(ctx, sets[k % args.ring], m6, TARGET, spec, flips=flips, edge="fill")

    def a(k):
        return J.decode_tensors_projected_mixed(ctx, sets[k % args.ring], m9, TARGET, spec, flips=flips, edge="fill")

    def b(k):
        return J.decode_tensors_projected_mixed(ctx, sets[k % args.ring], mp, TARGET, spec, flips=flips, edge="fill")

    ref, views_w, mv6 = a_warp(0)
    same, views_a, mv9 = a(0)
    assert views_w.tolist() == views_a.tolist() and torch.equal(ref.view(torch.int16), same.view(torch.int16))   # (a) is (a_warp), bit for bit
    want, views_b, mvb = b(0)

    # today's route: the whole images, and per image the homography's grid in normalised coordinates
    whole = np.array([(1, 0, 0, w, h) for w, h in sizes], np.int32)
    xc = (torch.arange(wt, device=dev, dtype=torch.float32) + 0.5).reshape(1, wt).expand(ht, wt)
    yc = (torch.arange(ht, device=dev, dtype=torch.float32) + 0.5).reshape(ht, 1).expand(ht, wt)
    hom = [[float(v) for v in m] for m in mp]

    def c(k):
        pixels = J.decode_views_mixed(ctx, sets[k % args.ring], whole)
        for i, p in enumerate(pixels):
            m = hom[i]
            den = m[6] * xc + m[7] * yc + m[8]
            gx = (m[0] * xc + m[1] * yc + m[2]) / den * (2.0 / sizes[i][0]) - 1.0
            gy = (m[3] * xc + m[4] * yc + m[5]) / den * (2.0 / sizes[i][1]) - 1.0
            x = torch.nn.functional.grid_sample(p.permute(2, 0, 1)[None].float(), torch.stack([gx, gy], -1)[None], mode="bilinear",
                                                padding_mode="zeros", align_corners=False)
            x = torch.floor(torch.clamp(x, 0.0, 255.0) + 0.5)
            if flips[i]:
                x = x.flip(3)
            batch[i] = ((x - mean) * scale).half()[0]
        return batch

    # (c) gives (b)'s bytes within a level or two (another denominator, float32 grid): compared as bytes, through the inverse of
    # the normalisation, on the images both routes take at full size
    back = lambda t: torch.round(t.float() / scale + mean)   # noqa: E731
    full = [i for i in range(N) if views_b[i][0] == 1]
    worst = float((back(c(0))[full] - back(want)[full]).abs().max()) if full else -1.0   # (reported; tests/test_project_cpu.py holds the bound)

    pixels_a, pixels_b = J.decode_views_mixed(ctx, sets[0], views_a), J.decode_views_mixed(ctx, sets[0], views_b)
    src_a, stride_a, ext_a = _packed(torch, ctx, pixels_a)
    src_b, stride_b, ext_b = _packed(torch, ctx, pixels_b)
    h_flip = (C.c_uint8 * N)(*flips)
    fill = _lib.Warp(_lib.EDGE_FILL, (C.c_uint8 * 3)(0, 0, 0))
    out = torch.empty(N * 3 * wt * ht, dtype=torch.float16, device=dev)
    mv6c, mv9c, mvbc = (np.ascontiguousarray(m, np.float32) for m in (mv6, mv9, mvb))

    def k_warp(k):
        _lib.check(lib.jpeg_amd_warp_tensor_batch(ctx.handle, N, src_a.data_ptr(), stride_a, ext_a, mv6c.ctypes.data, C.byref(fill), wt, ht,
                                                  C.byref(spec), h_flip, out.data_ptr(), 3 * wt * ht), "warp", ctx.handle)

    def k_project(k):
        _lib.check(lib.jpeg_amd_project_tensor_batch(ctx.handle, N, src_a.data_ptr(), stride_a, ext_a, mv9c.ctypes.data, C.byref(fill), wt, ht,
                                                     C.byref(spec), h_flip, None, out.data_ptr(), 3 * wt * ht), "project", ctx.handle)

    def k_persp(k):
        _lib.check(lib.jpeg_amd_project_tensor_batch(ctx.handle, N, src_b.data_ptr(), stride_b, ext_b, mvbc.ctypes.data, C.byref(fill), wt, ht,
                                                     C.byref(spec), h_flip, None, out.data_ptr(), 3 * wt * ht), "project", ctx.handle)

    if args.kernels_only:                     # for a counter run: the three launches alone, `steps` times each
        for fn in (k_warp, k_project, k_persp):
            for k in range(args.steps):
                fn(k)
        ctx.synchronize()
        return
    routes = {"a_warp": a_warp, "a": a, "a_warp2": a_warp, "b": b, "c": c, "k_warp": k_warp, "k_project": k_project, "k_persp": k_persp}
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(_timed(torch, fn, max(args.steps // 5, 2) if k == "c" else args.steps, 1 if k == "c" else args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    mpx = lambda v: round(float((v[:, 3].astype(np.int64) * v[:, 4]).sum()) / 1e6, 1)   # noqa: E731
    res = {"n": N, "target": list(TARGET), "view_mpx_a": mpx(views_a), "view_mpx_b": mpx(views_b), "whole_mpx": mpx(whole),
           "denoms_a": {d: int((views_a[:, 0] == d).sum()) for d in (1, 2, 4, 8)}, "denoms_b": {d: int((views_b[:, 0] == d).sum()) for d in (1, 2, 4, 8)},
           **{f"t_{k}_us": round(v, 1) for k, v in med.items()},
           "a_over_warp": round(med["a"] / med["a_warp"], 3), "a_over_warp2": round(med["a"] / med["a_warp2"], 3), "b_over_a": round(med["b"] / med["a"], 3), "c_over_b": round(med["c"] / med["b"], 1),
           "k_project_over_warp": round(med["k_project"] / med["k_warp"], 3), "k_persp_over_project": round(med["k_persp"] / med["k_project"], 3),
           "c_worst_level": worst, "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
    lines = [f"# tools/bench_perspective.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; times "
             f"are HIP-event medians per call of {N} images -> {wt}x{ht} fp16 CHW, host work included",
             json.dumps(res),
             f"whole call: (a) last row (0, 0, 1) {med['a']:.0f} us = {res['a_over_warp']:.3f} x the affine warp on the same matrices "
             f"({med['a_warp']:.0f} us first in the round, {med['a_warp2']:.0f} us behind (a): {res['a_over_warp2']:.3f} x; {res['view_mpx_a']} Mpx); (b) distortion 0.5 {med['b']:.0f} us = {res['b_over_a']:.3f} x (a) "
             f"({res['view_mpx_b']} Mpx); (c) today {med['c']:.0f} us = {res['c_over_b']:.1f} x (b) ({res['whole_mpx']} Mpx decoded), within "
             f"{worst:.0f} level on the full-size views",
             f"resample launch alone: affine warp {med['k_warp']:.0f} us, project on the same matrices {med['k_project']:.0f} us "
             f"({res['k_project_over_warp']:.3f} x), project with distortion 0.5 {med['k_persp']:.0f} us ({res['k_persp_over_project']:.3f} x)"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
