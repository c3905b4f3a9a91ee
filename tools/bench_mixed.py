#!/usr/bin/env python3
"""tools/bench_mixed.py -- the mixed calls (jpeg_amd.decode_crops_tensor_mixed: k_view_decode_mixed over per-image records,
then one k_resize_tensor launch) against what a caller of files of different sizes does without them, and against the uniform
call on a batch that did not need them, alternating in one process.

    python tools/bench_mixed.py [--steps 10] [--warmup 2] [--rounds 5] [--ring 4] [--out profiles/r11_mixed.txt]

The method is tools/bench_scaled.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets (distinct coefficient buffers); the report is the median per-call time over the
rounds.  Nothing is gated.  Every route ends in one [256, 3, 224, 224] fp16 CHW tensor, ImageNet constants, every second
image flipped, from one seeded RandomResizedCrop rectangle per image.
  M  256 images of seeded sizes (sides 160 ... 1200) and a seeded mix of 4:2:0, 4:4:4, 4:2:2 and grey:
       mixed    jpeg_amd.decode_crops_tensor_mixed, one call
       today    one jpeg_amd.decode_crops_tensor per image, each result copied into its row of the batch tensor
  A  case A of DESIGN.md 8d, 256 x 1920 x 1080 4:2:0 -- one geometry, the batch the uniform call was written for; the C calls
     with their arguments built once, so that what differs is the per-image records and the tile kernel without shortcuts:
       uniform  jpeg_amd_decode_tensor_batch
       mixed    jpeg_amd_decode_tensor_mixed, the same views
The routes of a case agree bit for bit (tests/test_gpu_mixed.py); that is checked here on the first set.  M is
host-inclusive: the events bracket whatever the Python calls enqueue.
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
from tools.bench_resized import H, N, W, _inputs  # noqa: E402
from tools.bench_view import TARGET, _timed, random_resized_crops  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
YCC = {name: J.Layout("ycc8", {1: J.Component(f, 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
       for name, f in (("420", (2, 2)), ("444", (1, 1)), ("422", (2, 1)))}
LAYOUTS = dict(YCC, grey=J.Layout("y8", {1: J.Component((1, 1), 0)}))


def _mixed_inputs(torch, ctx, rng, ring):
    """-> (names, sizes, per ring set the 256 Spectral objects, per image its tables on the device [1, ntables, 64])."""
    dev = ctx.torch_device
    gen = torch.Generator(device=dev).manual_seed(11)
    names = [("420", "444", "422", "grey")[int(k)] for k in rng.choice(4, N, p=(0.55, 0.2, 0.15, 0.1))]
    sizes = [(int(rng.integers(160, 1201)), int(rng.integers(160, 1201))) for _ in range(N)]
    tables = [torch.randint(1, 8, (1, 1 if name == "grey" else 2, 64), dtype=torch.int16, device=dev, generator=gen) for name in names]
    host = [t.cpu().numpy().astype(np.uint16) for t in tables]
    sets = []
    for _ in range(ring):
        one = []
        for name, size, qh in zip(names, sizes, host):
            layout = LAYOUTS[name]
            planes = [torch.randint(-256, 256, (uy, ux, 64), dtype=torch.int16, device=dev, generator=gen)
                      for ux, uy in layout.units(size)]
            one.append(J.Spectral(ctx, size, layout, planes, list(qh[0]), [0, 1, 1][:layout.count]))
        sets.append(one)
    return names, sizes, sets, tables


def case_mixed(torch, ctx, args, spec, flips):
    rng = np.random.default_rng(20241019)
    names, sizes, sets, tables = _mixed_inputs(torch, ctx, rng, args.ring)
    source = [random_resized_crops(rng, w, h, 1)[0] for w, h in sizes]
    batch = torch.empty((N, 3, TARGET[1], TARGET[0]), dtype=torch.float16, device=ctx.torch_device)

    def mixed(k):
        return J.decode_crops_tensor_mixed(ctx, sets[k % args.ring], source, TARGET, spec, flips=flips)[0]

    def today(k):
        for i, sp in enumerate(sets[k % args.ring]):
            batch[i] = J.decode_crops_tensor(ctx, sp.size, sp.layout, [p.unsqueeze(0) for p in sp.planes], tables[i], source[i:i + 1],
                                             TARGET, spec, flips=flips[i:i + 1], q=sp.q)[0][0]
        return batch

    differ = int((mixed(0).view(torch.int16) != today(0).view(torch.int16)).sum())
    assert differ == 0, differ
    views = J.decode_crops_tensor_mixed(ctx, sets[0], source, TARGET, spec, flips=flips)[1]
    times = {"mixed": [], "today": []}
    for _ in range(args.rounds):
        times["mixed"].append(_timed(torch, mixed, args.steps, args.warmup))
        times["today"].append(_timed(torch, today, max(1, args.steps // 4), 1))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"case": "M", "n": N, "layouts": {k: names.count(k) for k in LAYOUTS}, "denoms": {d: int((views[:, 0] == d).sum()) for d in (1, 2, 4, 8)},
            "view_mpx": round(float((views[:, 3].astype(np.int64) * views[:, 4]).sum()) / 1e6, 1),
            "mixed_vs_today_differing": differ, "t_mixed_us": round(med["mixed"], 1), "t_today_us": round(med["today"], 1),
            "today_over_mixed": round(med["today"] / med["mixed"], 2), "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}


def case_a(torch, ctx, args, spec, flips):
    lib = _lib.lib()
    layout = YCC["420"]
    sets, q = _inputs(torch, ctx, layout, args.ring)
    source = random_resized_crops(np.random.default_rng(20240809), W, H, N)
    L = layout.c_layout((W, H), layout.units((W, H)), [0, 1, 1])
    h_views = (_lib.View * N)()
    for i, s in enumerate(source):
        denom = J.view_denom(s[2:], TARGET)
        h_views[i] = _lib.View(denom, _lib.Region(*J.view_of_source((W, H), denom, s)))
    h_flip = (C.c_uint8 * N)(*flips)
    stride = 3 * TARGET[0] * TARGET[1]
    outs = [torch.empty(N * stride, dtype=torch.float16, device=ctx.torch_device) for _ in range(2)]
    ptrs = [_lib.ptr_array([p.data_ptr() for p in s]) for s in sets]
    strides = _lib.size_array([p[0].numel() for p in sets[0]])
    images = []
    for s in sets:
        arr = (_lib.Image * N)()
        for i in range(N):
            arr[i].layout = L
            for p, plane in enumerate(s):
                arr[i].d_coef[p] = plane[i].data_ptr()
            arr[i].d_quanta, arr[i].ntables = q[i].data_ptr(), 2
        images.append(arr)

    def uniform(k):
        st = lib.jpeg_amd_decode_tensor_batch(ctx.handle, C.byref(L), N, ptrs[k % args.ring], strides, q.data_ptr(), 128, 2, 0,
                                              _lib.COLOR_RGB8, h_views, TARGET[0], TARGET[1], C.byref(spec), h_flip, outs[0].data_ptr(),
                                              stride)
        assert st == 0, st

    def mixed(k):
        st = lib.jpeg_amd_decode_tensor_mixed(ctx.handle, N, images[k % args.ring], 0, _lib.COLOR_RGB8, h_views, TARGET[0], TARGET[1],
                                              C.byref(spec), h_flip, outs[1].data_ptr(), stride)
        assert st == 0, st

    uniform(0), mixed(0)
    differ = int((outs[0].view(torch.int16) != outs[1].view(torch.int16)).sum())
    assert differ == 0, differ
    times = {"uniform": [], "mixed": []}
    for _ in range(args.rounds):
        for name, fn in (("uniform", uniform), ("mixed", mixed)):
            times[name].append(_timed(torch, fn, args.steps, args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"case": "A", "size": [W, H], "n": N, "uniform_vs_mixed_differing": differ, "t_uniform_us": round(med["uniform"], 1),
            "t_mixed_us": round(med["mixed"], 1), "mixed_over_uniform": round(med["mixed"] / med["uniform"], 3),
            "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--cases", default="M,A")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_mixed.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_mixed: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    flips = [i & 1 for i in range(N)]
    lines = [f"# tools/bench_mixed.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; "
             "times are HIP-event medians per call, host work included"]
    for name in args.cases.split(","):
        if name == "M":
            r = case_mixed(torch, ctx, args, spec, flips)
            lines += [json.dumps(r),
                      f"M: 256 images of mixed sizes and layouts {r['layouts']} -> {TARGET[0]}x{TARGET[1]} fp16 CHW, denominators {r['denoms']}, "
                      f"{r['view_mpx']} Mpx of views:  decode_crops_tensor_mixed {r['t_mixed_us']:.0f} us  one decode_crops_tensor per image "
                      f"{r['t_today_us']:.0f} us ({r['today_over_mixed']:.2f} x)"]
        elif name == "A":
            r = case_a(torch, ctx, args, spec, flips)
            lines += [json.dumps(r),
                      f"A: 256 x {W}x{H} 4:2:0 -> {TARGET[0]}x{TARGET[1]} fp16 CHW:  jpeg_amd_decode_tensor_batch {r['t_uniform_us']:.0f} us  "
                      f"jpeg_amd_decode_tensor_mixed {r['t_mixed_us']:.0f} us ({r['mixed_over_uniform']:.3f} of the uniform call)"]
        torch.cuda.empty_cache()
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
