#!/usr/bin/env python3
"""tools/bench_files_tensor.py -- JPEG FILES of mixed sizes and layouts to one training tensor in one call
(jpeg_amd.decompress_tensors: host threads entropy-decode into the sparse form, k_expand_mixed rebuilds the heads of the
blocks of the views' windows, then the mixed tensor call) against today's route on the same files, in one process.

    python tools/bench_files_tensor.py [--files 256] [--rounds 5] [--threads 0] [--out profiles/files_tensor.json]

Workload: `files` synthetic files, sides seeded in 160 ... 1200, a seeded mix of 4:2:0, 4:4:4, 4:2:2 and grey, every fifth
with a restart interval, one seeded RandomResizedCrop rectangle per file, to a [files, 3, 224, 224] fp16 CHW tensor with the
ImageNet constants, every second image flipped.  The files are written on the host from coefficients as sparse as a
photograph's (about a dozen per block), so their entropy decoding costs what a real file's does.
  leg 1  new     jpeg_amd.decompress_tensors, one call
  leg 2  today   one Spectral.decompress per file (serial host decode into dense planes, an upload per plane), then ONE
                 jpeg_amd.decode_crops_tensor_mixed -- the ratio today / new is the figure to report
  leg 3  uniform on `--uniform` files of ONE geometry (500 x 375 4:2:0), whole images: jpeg_amd_decompress_batch_device and
                 jpeg_amd.resize_tensor, against the new call on the same files
  leg 4  expand  jpeg_amd_spectral_expand_mixed over all the files' records, resident on the device: the views' windows at
                 their heads against whole-plane windows at head 8, in all and for the files at denominator 1 alone
Legs 1 to 3 are HOST-INCLUSIVE wall times (each call ends with the device idle; the median of `rounds` calls after one
warm-up call); leg 4 is timed between two HIP events on the context's stream, 20 launches per reading.  Legs 1 and 2 agree
bit for bit (tests/test_gpu_file_tensor.py); that is checked here too.  Nothing is gated: the record is the result."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import jpeg_amd as J  # noqa: E402
from jpeg_amd import _lib  # noqa: E402
from jpeg_amd.api import _scan_array  # noqa: E402
from tools.bench_view import TARGET, random_resized_crops  # noqa: E402

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
FACTORS = {"420": [(2, 2), (1, 1), (1, 1)], "444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "grey": [(1, 1)]}
POOL = 1 << 16                                               # blocks of seeded coefficients that the files draw from


def c_layout(w, h, factors):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes = w, h, 8, len(factors)
    L.scale_x, L.scale_y = max(f[0] for f in factors), max(f[1] for f in factors)
    for p, (fx, fy) in enumerate(factors):
        L.factor_x[p], L.factor_y[p], L.qi[p] = fx, fy, p
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def block_pool(rng):
    """int16 [POOL, 64]: every DC, AC coefficients that thin out towards the high frequencies (about a dozen per block)."""
    scale = (400.0 / (1.0 + np.arange(64)) ** 2.5).astype(np.float32)
    v = np.rint(rng.laplace(0.0, 1.0, (POOL, 64)).astype(np.float32) * scale)
    v[:, 0] = rng.integers(-1000, 1000, POOL)
    return np.clip(v, -1000, 1000).astype(np.int16)


def write_file(L, pool, first, quanta, restart):
    """The baseline file of layout L whose planes are the pool's blocks from `first` on (one interleaved scan)."""
    n = L.nplanes
    planes = []
    for p in range(n):
        blocks = L.units_x[p] * L.units_y[p]
        idx = (first + np.arange(blocks)) % POOL
        planes.append(np.ascontiguousarray(pool[idx]))
        first += blocks
    info = _lib.FrameInfo()
    info.width, info.height, info.precision, info.ncomponents = L.width, L.height, 8, n
    info.process, info.scale_x, info.scale_y, info.restart_interval = 0, L.scale_x, L.scale_y, restart
    for p in range(n):
        info.id[p], info.factor_x[p], info.factor_y[p] = p + 1, L.factor_x[p], L.factor_y[p]
        info.units_x[p], info.units_y[p] = L.units_x[p], L.units_y[p]
    keys, tkeys = (C.c_int32 * n)(*[min(c, 1) for c in range(n)]), (C.c_int32 * 2)(0, 1)
    scans = [[(c, min(c, 1), min(c, 1)) for c in range(n)]]
    size = C.c_size_t()
    args = [C.byref(info), keys, _lib.ptr_array([p.ctypes.data for p in planes]), quanta.ctypes.data, tkeys, min(n, 2),
            _scan_array(scans), 1, None, 0]
    lib = _lib.lib()
    assert lib.jpeg_amd_jpeg_encode_spectral(*args, None, 0, C.byref(size)) == 0
    out = np.empty(size.value, np.uint8)
    assert lib.jpeg_amd_jpeg_encode_spectral(*args, out.ctypes.data, out.size, C.byref(size)) == 0
    return out[:size.value].copy()


def make_files(n, rng, uniform=None):
    """-> (the files' bytes, their layouts, their names)."""
    pool = block_pool(rng)
    quanta = rng.integers(1, 8, (2, 64)).astype(np.uint16)
    names = [uniform[0] if uniform else ("420", "444", "422", "grey")[int(k)] for k in rng.choice(4, n, p=(0.55, 0.2, 0.15, 0.1))]
    sizes = [uniform[1] if uniform else (int(rng.integers(160, 1201)), int(rng.integers(160, 1201))) for _ in range(n)]
    layouts = [c_layout(w, h, FACTORS[name]) for name, (w, h) in zip(names, sizes)]
    files = [write_file(L, pool, int(rng.integers(POOL)), quanta, 8 if i % 5 == 4 else 0) for i, L in enumerate(layouts)]
    return files, layouts, names


def wall(ctx, fn, rounds):
    """Median wall time of fn() in ms, the device idle before and after; one warm-up call."""
    fn()
    ctx.synchronize()
    times = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        ctx.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), [round(t, 2) for t in times]


def legs_files(torch, ctx, args, spec):
    rng = np.random.default_rng(20241019)
    files, layouts, names = make_files(args.files, rng)
    n = len(files)
    flips = [i & 1 for i in range(n)]
    source = [random_resized_crops(rng, L.width, L.height, 1)[0] for L in layouts]

    def new():
        return J.decompress_tensors(ctx, files, TARGET, spec, source_regions=source, flips=flips, threads=args.threads)

    def today():
        spectrals = [J.Spectral.decompress(ctx, f) for f in files]
        return J.decode_crops_tensor_mixed(ctx, spectrals, source, TARGET, spec, flips=flips)

    (a, views, infos), (b, views_b) = new(), today()
    differ = int((a.view(torch.int16) != b.view(torch.int16)).sum())
    assert differ == 0 and (views == views_b).all(), differ
    t_new, r_new = wall(ctx, new, args.rounds)
    t_today, r_today = wall(ctx, today, max(2, args.rounds // 2))
    plane_mb = sum(128 * L.units_x[p] * L.units_y[p] for L in layouts for p in range(L.nplanes)) / 1e6
    record = {"legs": "1,2", "files": n, "file_mb": round(sum(f.size for f in files) / 1e6, 1), "plane_mb": round(plane_mb, 1),
              "layouts": {k: names.count(k) for k in FACTORS}, "denoms": {str(d): int((views[:, 0] == d).sum()) for d in (1, 2, 4, 8)},
              "threads": args.threads, "new_vs_today_differing": differ, "t_new_ms": round(t_new, 2), "t_today_ms": round(t_today, 2),
              "today_over_new": round(t_today / t_new, 2), "new_files_per_s": round(n / t_new * 1e3), "rounds": {"new": r_new, "today": r_today}}
    return record, files, layouts, views


def leg_uniform(torch, ctx, args, spec):
    rng = np.random.default_rng(7)
    size = (500, 375)
    files, layouts, _ = make_files(args.uniform, rng, uniform=("420", size))
    n = len(files)
    ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in files])
    sizes = (C.c_size_t * n)(*[f.size for f in files])
    npx = 3 * size[0] * size[1]
    pixels = torch.empty(n * npx, dtype=torch.uint8, device=ctx.torch_device)

    def batch():
        _lib.check(_lib.lib().jpeg_amd_decompress_batch_device(ctx.handle, ptrs, sizes, n, args.threads, 0, _lib.COLOR_RGB8,
                                                               pixels.data_ptr(), npx, None), "jpeg_amd_decompress_batch_device", ctx.handle)
        return J.resize_tensor(ctx, list(pixels.view(n, size[1], size[0], 3)), TARGET, spec)

    def new():
        return J.decompress_tensors(ctx, files, TARGET, spec, threads=args.threads)[0]

    differ = int((batch().view(torch.int16) != new().view(torch.int16)).sum())   # whole images at denominator 1, both ways
    t_batch, r_batch = wall(ctx, batch, args.rounds)
    t_new, r_new = wall(ctx, new, args.rounds)
    return {"leg": "3", "files": n, "size": list(size), "batch_vs_new_differing": differ, "t_batch_resize_ms": round(t_batch, 2), "t_new_ms": round(t_new, 2),
            "batch_over_new": round(t_batch / t_new, 2), "rounds": {"batch_resize": r_batch, "new": r_new}}


def leg_expand(torch, ctx, args, files, layouts, views):
    lib = _lib.lib()
    n = len(files)
    records, at, where = [], 0, []
    for f, L in zip(files, layouts):
        blocks = sum(L.units_x[p] * L.units_y[p] for p in range(L.nplanes))
        rec = np.zeros(25 * blocks + 72, np.uint32)
        count = C.c_size_t()
        quanta = np.zeros((4, 64), np.uint16)
        st = lib.jpeg_amd_jpeg_decode_sparse(f.ctypes.data, f.size, rec.ctypes.data, blocks, rec[blocks:].ctypes.data, 24 * blocks + 72,
                                             C.byref(count), quanta.ctypes.data, None)
        assert st == 0, st
        records.append(rec[:blocks + count.value])
        where.append((at, at + blocks))
        at += blocks + count.value
    d_records = torch.from_numpy(np.concatenate(records).view(np.int32)).to(ctx.torch_device)
    planes = [[torch.empty(64 * L.units_x[p] * L.units_y[p], dtype=torch.int16, device=ctx.torch_device) for p in range(L.nplanes)]
              for L in layouts]

    def items(which, windowed):
        arr = (_lib.ExpandItem * len(which))()
        octets = 0
        for it, i in zip(arr, which):
            L, denom = layouts[i], int(views[i, 0])
            it.layout, it.head = L, ((1 if denom >= 4 else 4 if denom == 2 else 8) if windowed else 8)
            w = (_lib.Region * 4)()
            if windowed:
                _lib.check(lib.jpeg_amd_view_window(C.byref(L), 0, denom, C.byref(_lib.Region(*[int(v) for v in views[i, 1:]])), w), "window")
            for p in range(L.nplanes):
                it.d_coef[p] = planes[i][p].data_ptr()
                it.window[p] = w[p] if windowed else _lib.Region(0, 0, L.units_x[p], L.units_y[p])
                octets += it.window[p].width * it.window[p].height * it.head
            it.desc_at, it.entries_at = where[i]
        return arr, octets

    def timed(arr):
        def launch():
            _lib.check(lib.jpeg_amd_spectral_expand_mixed(ctx.handle, len(arr), arr, d_records.data_ptr()), "expand", ctx.handle)
        for _ in range(3):
            launch()
        readings = []
        for _ in range(args.rounds):
            ctx.timer_begin()
            for _ in range(20):
                launch()
            readings.append(ctx.timer_end() / 20 * 1e3)
        return statistics.median(readings), [round(t, 1) for t in readings]

    out = {"leg": "4", "files": n, "record_mb": round(4 * at / 1e6, 1)}
    ones = [i for i in range(n) if int(views[i, 0]) == 1]
    for name, which in (("all", list(range(n))), ("denominator_1", ones)):
        if not which:
            continue
        r = {"files": len(which)}
        for kind, windowed in (("windowed", True), ("whole_head8", False), ("windowed_again", True)):
            arr, octets = items(which, windowed)
            t, rounds = timed(arr)
            r[kind] = {"t_us": round(t, 1), "written_mb": round(16 * octets / 1e6, 1), "rounds": rounds}
        r["whole_over_windowed"] = round(r["whole_head8"]["t_us"] / r["windowed"]["t_us"], 2)
        out[name] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=256)
    ap.add_argument("--uniform", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--threads", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "files_tensor.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_files_tensor: no GPU (this tool measures the MI355X; there is no CPU number)")
    ctx = J.Context(0)
    spec = J.tensor_spec(MEAN, STD, dtype=torch.float16, layout="chw")
    record = {"tool": "tools/bench_files_tensor.py", "args": {k: v for k, v in vars(args).items() if k != "out"}, "target": list(TARGET),
              "timing": "legs 1-3: host wall time per call, device idle before and after, median; leg 4: HIP events, 20 launches per reading"}
    files_record, files, layouts, views = legs_files(torch, ctx, args, spec)
    record["files_to_tensor"] = files_record
    record["uniform"] = leg_uniform(torch, ctx, args, spec)
    record["expand"] = leg_expand(torch, ctx, args, files, layouts, views)
    text = json.dumps(record, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
