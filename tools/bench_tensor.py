#!/usr/bin/env python3
"""tools/bench_tensor.py -- the tensor output (jpeg_amd.decode_crops_tensor: the view decode into a context buffer, then one
k_resize_tensor launch that resamples, flips, normalises, converts and stores CHW) against the tail a caller runs today in
framework ops behind the byte call, alternating in one process.

    python tools/bench_tensor.py [--steps 20] [--warmup 3] [--rounds 5] [--ring 4] [--out profiles/r12_tensor.txt]

The method is tools/bench_scaled.py's: each round times `steps` calls of each route between two HIP events on the context's
stream over a ring of `ring` input sets (distinct coefficient buffers, together larger than the 256 MiB Infinity Cache); the
report is the median per-call time over the rounds.  Nothing is gated.  The workload is case A of DESIGN.md 8d: 256 x 1920 x
1080 4:2:0 RGB, one seeded RandomResizedCrop rectangle per image -> 224 x 224, every second image flipped, fp16, CHW, the
ImageNet constants.
  tensor   jpeg_amd.decode_crops_tensor: one call, one [256, 3, 224, 224] fp16 tensor
  today    jpeg_amd.decode_crops_resized, then the flip of the selected images, permute, .float(), sub, mul, .half()
  bytes    jpeg_amd.decode_crops_resized alone: what both routes share
All three are host-inclusive: the events bracket whatever the Python calls enqueue.  `tensor` and `today` agree bit for bit
(tests/test_tensor_cpu.py, tests/test_gpu_tensor.py); that is checked here on the first set.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeg_amd as J  # noqa: E402
from tools.bench_resized import H, N, W, _inputs  # noqa: E402
from tools.bench_view import TARGET, _timed, random_resized_crops  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ring", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_tensor.txt"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tensor: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    dev = ctx.torch_device
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    sets, q = _inputs(torch, ctx, layout, args.ring)
    source = random_resized_crops(np.random.default_rng(20240809), W, H, N)
    flips = [i & 1 for i in range(N)]
    flipped = torch.tensor([i for i in range(N) if flips[i]], device=dev)
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    mean_b = torch.tensor(list(spec.mean), dtype=torch.float32, device=dev).view(1, 3, 1, 1)
    scale = torch.tensor(list(spec.scale), dtype=torch.float32, device=dev).view(1, 3, 1, 1)

    def tensor(k):
        return J.decode_crops_tensor(ctx, (W, H), layout, sets[k % args.ring], q, source, TARGET, spec, flips=flips)[0]

    def today(k):
        u = J.decode_crops_resized(ctx, (W, H), layout, sets[k % args.ring], q, source, TARGET)[0]
        u[flipped] = u[flipped].flip(2)
        return u.permute(0, 3, 1, 2).float().sub_(mean_b).mul_(scale).half()

    def bytes_only(k):
        return J.decode_crops_resized(ctx, (W, H), layout, sets[k % args.ring], q, source, TARGET)[0]

    a, b = tensor(0), today(0)
    assert a.shape == b.shape and a.dtype == b.dtype
    differ = int((a.view(torch.int16) != b.contiguous().view(torch.int16)).sum())
    assert differ == 0, differ

    routes = {"tensor": tensor, "today": today, "bytes": bytes_only}
    times = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, fn in routes.items():
            times[k].append(_timed(torch, fn, args.steps, args.warmup))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"case": "A", "size": [W, H], "n": N, "target": list(TARGET), "dtype": "float16", "layout": "chw", "flipped": sum(flips),
           "tensor_vs_today_differing": differ, "t_tensor_us": round(med["tensor"], 1), "t_today_us": round(med["today"], 1),
           "t_bytes_us": round(med["bytes"], 1), "today_over_tensor": round(med["today"] / med["tensor"], 2),
           "tail_today_us": round(med["today"] - med["bytes"], 1), "tail_tensor_us": round(med["tensor"] - med["bytes"], 1),
           "rounds": {k: [round(t, 1) for t in v] for k, v in times.items()}}
    lines = [f"# tools/bench_tensor.py, one MI355X, --steps {args.steps} --warmup {args.warmup} --rounds {args.rounds} --ring {args.ring}; "
             "times are HIP-event medians per call, host work included",
             json.dumps(res),
             f"A: 256 x 1920x1080 crops -> {TARGET[0]}x{TARGET[1]} fp16 CHW, {sum(flips)} flipped:  decode_crops_tensor {med['tensor']:.0f} us  "
             f"decode_crops_resized + flip/permute/float/sub/mul/half {med['today']:.0f} us ({res['today_over_tensor']:.2f} x)  "
             f"decode_crops_resized alone {med['bytes']:.0f} us"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
