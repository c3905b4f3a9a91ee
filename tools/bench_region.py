#!/usr/bin/env python3
"""tools/bench_region.py -- region decode (jpeg_amd_decode_region_batch, k_region_decode) against the full decode of the same
inputs (jpeg_amd_decode_batch), alternating in one process.

    python tools/bench_region.py [--steps 200] [--warmup 20] [--rounds 5] [--ring 4] [--json PATH] [--cases A,B,C,D]

Each round times `steps` calls of each path between two HIP events on the context's stream -- region first, then full --
over a ring of `ring` input sets (distinct coefficient buffers, together larger than the 256 MiB Infinity Cache, as bench.py
does); the report is the median per-call time over the rounds.  Cases:
  A  8192 x 8192 4:2:0 RGB, one region of 4096 x 4096 at (1237, 901)           target t_region <= 0.33 t_full
  B  256 x 1920 x 1080 4:2:0 RGB, seeded RandomResizedCrop regions (scale 0.08-1, ratio 3/4-4/3)
                                       target area-normalised efficiency area_fraction * t_full / t_region >= 0.70
  C  256 x 1920 x 1080 4:2:0 RGB, 224 x 224 centre crops                      target t_full / t_region >= 8
  D  4096 x 4096 4:2:0 CENTRED -> cosited (the fallback: whole decode + crop), region 2048 x 2048 at (1237, 901): report only
Kernel times: run it again under `rocprofv3 --kernel-trace --stats -d DIR -- python tools/bench_region.py --steps 20 --rounds 1`.
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


def _layout(w, h):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes, L.scale_x, L.scale_y = w, h, 8, 3, 2, 2
    for p, f in enumerate((2, 1, 1)):
        L.factor_x[p] = L.factor_y[p] = f
        L.qi[p] = min(p, 1)
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def random_resized_crops(rng, W, H, n, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3)):
    """torchvision's RandomResizedCrop.get_params, seeded: 10 draws, then the centre crop at the clamped ratio."""
    out = []
    area = W * H
    for _ in range(n):
        for _ in range(10):
            a = area * rng.uniform(*scale)
            r = math.exp(rng.uniform(math.log(ratio[0]), math.log(ratio[1])))
            w, h = int(round(math.sqrt(a * r))), int(round(math.sqrt(a / r)))
            if 0 < w <= W and 0 < h <= H:
                out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
                break
        else:
            r0 = W / H
            w, h = (W, int(round(W / ratio[0]))) if r0 < ratio[0] else ((int(round(H * ratio[1])), H) if r0 > ratio[1] else (W, H))
            w, h = min(w, W), min(h, H)
            out.append(((W - w) // 2, (H - h) // 2, w, h))
    return out


def _case(torch, ctx, name, W, H, n, regions, cosited, args):
    lib = _lib.lib()
    L = _layout(W, H)
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(7)
    sizes = [64 * L.units_x[p] * L.units_y[p] for p in range(3)]
    ring = [[torch.randint(-256, 256, (n * s,), dtype=torch.int16, device=dev, generator=gen) for s in sizes]
            for _ in range(args.ring)]
    q = torch.randint(1, 8, (2 * 64,), dtype=torch.int16, device=dev, generator=gen)
    strides = _lib.size_array(sizes)
    full_stride = 3 * W * H
    full = torch.empty(n * full_stride, dtype=torch.uint8, device=dev)
    reg_stride = max(3 * w * h for _, _, w, h in regions)
    out = torch.empty(n * reg_stride, dtype=torch.uint8, device=dev)
    h_regions = (_lib.Region * n)()
    for i, (x, y, w, h) in enumerate(regions):
        h_regions[i].x, h_regions[i].y, h_regions[i].width, h_regions[i].height = x, y, w, h
    ptrs = [_lib.ptr_array([t.data_ptr() for t in s]) for s in ring]

    def region(k):
        st = lib.jpeg_amd_decode_region_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2,
                                              cosited, _lib.COLOR_RGB8, h_regions, out.data_ptr(), reg_stride)
        assert st == 0, st

    def whole(k):
        st = lib.jpeg_amd_decode_batch(ctx.handle, C.byref(L), n, ptrs[k % args.ring], strides, q.data_ptr(), 0, 2, cosited,
                                       _lib.COLOR_RGB8, full.data_ptr(), full_stride)
        assert st == 0, st

    # bit-exact on the first ring set before timing anything
    region(0)
    whole(0)
    full_v = full.view(n, H, W, 3)
    for i, (x, y, w, h) in enumerate(regions):
        assert torch.equal(out[i * reg_stride:i * reg_stride + 3 * w * h].view(h, w, 3), full_v[i, y:y + h, x:x + w]), i

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

    t_region, t_full = [], []
    for _ in range(args.rounds):
        t_region.append(timed(region))
        t_full.append(timed(whole))
    tr, tf = statistics.median(t_region), statistics.median(t_full)
    area = sum(w * h for _, _, w, h in regions) / (n * W * H)
    res = {"case": name, "size": [W, H], "n": n, "cosited": cosited, "area_fraction": round(area, 5),
           "t_region_us": round(tr, 2), "t_full_us": round(tf, 2), "ratio": round(tr / tf, 4),
           "speedup": round(tf / tr, 2), "efficiency": round(area * tf / tr, 3),
           "t_region_rounds": [round(t, 2) for t in t_region], "t_full_rounds": [round(t, 2) for t in t_full]}
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
    ap.add_argument("--cases", default="A,B,C,D")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_region: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    cases = set(args.cases.split(","))
    results = []
    if "A" in cases:
        results.append(_case(torch, ctx, "A", 8192, 8192, 1, [(1237, 901, 4096, 4096)], 0, args))
    if "B" in cases:
        regs = random_resized_crops(np.random.default_rng(20240807), 1920, 1080, 256)
        results.append(_case(torch, ctx, "B", 1920, 1080, 256, regs, 0, args))
    if "C" in cases:
        results.append(_case(torch, ctx, "C", 1920, 1080, 256, [((1920 - 224) // 2, (1080 - 224) // 2, 224, 224)] * 256, 0,
                             args))
    if "D" in cases:
        results.append(_case(torch, ctx, "D", 4096, 4096, 1, [(1237, 901, 2048, 2048)], 1, args))
    targets = {"A": ("ratio", "<=", 0.33), "B": ("efficiency", ">=", 0.70), "C": ("speedup", ">=", 8.0)}
    for r in results:
        if r["case"] in targets:
            key, op, v = targets[r["case"]]
            r["target"] = f"{key} {op} {v}"
            r["met"] = r[key] <= v if op == "<=" else r[key] >= v
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    for r in results:
        print(f"{r['case']}: {r['size'][0]}x{r['size'][1]} n={r['n']} area {r['area_fraction']:.4f}  region {r['t_region_us']:.1f} us"
              f"  full {r['t_full_us']:.1f} us  ratio {r['ratio']:.3f}  speedup {r['speedup']:.2f}x  efficiency "
              f"{r['efficiency']:.3f}  {r.get('target', 'report only')} {'' if 'met' not in r else ('MET' if r['met'] else 'MISSED')}")


if __name__ == "__main__":
    main()
