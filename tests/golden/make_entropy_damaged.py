#!/usr/bin/env python3
"""Records tests/golden/entropy_damaged.json: status and SHA-256 of what the host entropy decoder (csrc/entropy.cpp) writes for
every *.jpg under tests/golden/decode -- the intact file and 16 damaged copies of each, progressive files included -- through the
plane call on one thread, the careful reader (max_scans 1000; on the intact file also the previews after 1 and 2 scans) and the
sparse call.  tests/test_entropy_damaged_cpu.py imports this file, makes the same copies and holds the library to the record.

    python tests/golden/make_entropy_damaged.py ["which build this is"]    (JPEG_AMD_LIBRARY=<library> to record with another)

The digests are this project's own output.  Record with a library whose decoder is trusted: the file says which one it was."""
import ctypes as C
import glob
import hashlib
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
from jpeg_amd import _lib          # noqa: E402
from _sparse import sparse_decode  # noqa: E402

FIXTURE = os.path.join(HERE, "entropy_damaged.json")
SEED, COPIES = 20240921, 16
KINDS = ["intact", "flipped bits", "a run without 0xFF", "stray 0xFF bytes", "a marker in the data", "truncation",
         "a removed restart marker", "all ones to the end"]
REMOVED_MARKER = KINDS.index("a removed restart marker")


class Lcg:
    """Knuth's MMIX generator, the high bits: the positions do not depend on any library's bit generator."""

    def __init__(self, seed):
        self.x = seed & (2 ** 64 - 1)
        self.below(1)

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % max(1, n)

    def between(self, lo, hi):              # lo <= value < hi; lo where the range is empty
        return lo + self.below(hi - lo) if hi > lo else lo


def files():
    return sorted(glob.glob(os.path.join(HERE, "decode", "*.jpg")))


def scans(data):
    """[start, end) of the entropy-coded bytes of every scan (a marker walk; the data ends at the next marker that is
    neither stuffing nor RSTn)."""
    out, pos = [], 2
    while pos + 3 < len(data):
        if data[pos] != 0xff:
            break
        m = data[pos + 1]
        if m == 0xff:
            pos += 1
            continue
        if m == 0xd9:
            break
        if m == 0x01 or 0xd0 <= m <= 0xd7:
            pos += 2
            continue
        pos += 2 + int.from_bytes(data[pos + 2:pos + 4], "big")
        if m == 0xda:
            e = pos
            while e + 1 < len(data) and not (data[e] == 0xff and data[e + 1] != 0 and not 0xd0 <= data[e + 1] <= 0xd7):
                e += 1
            if e + 1 >= len(data):
                e = len(data)
            out.append((pos, e))
            pos = e
    return out


def damaged(data, kind, rng):
    """One copy of `data` with damage of `kind` (an index into KINDS) inside one of its scans."""
    d = bytearray(data)
    if kind == 0:
        return d
    all_scans = scans(data)
    roomy = [s for s in all_scans if s[1] - s[0] >= 64] or all_scans
    start, end = roomy[rng.below(len(roomy))]
    if kind == 1:
        for _ in range(1 + rng.below(5)):
            d[rng.between(start, end)] ^= 1 << rng.below(8)
    elif kind == 2:
        lo = rng.between(start, end - 48)
        for i in range(lo, min(lo + 48, end)):
            d[i] = rng.below(0xff)
    elif kind == 3:
        lo = rng.between(start, end - 3)
        d[lo:lo + 3] = [b"\xff\x00\xff", b"\xff\xff\x00", b"\xff\x01\x02"][rng.below(3)]
    elif kind == 4:
        lo = rng.between(start, end - 2)
        d[lo:lo + 2] = bytes([0xff, [0xd0, 0xd3, 0xd7, 0xc4, 0xfe][rng.below(5)]])
    elif kind == 5:
        d = d[:rng.between(start + 1, end)]
    elif kind == 6:
        marks = [i for i in range(start, end - 1) if d[i] == 0xff and 0xd0 <= d[i + 1] <= 0xd7]
        if marks:
            i = marks[rng.below(len(marks))]
            d[i:i + 2] = b"\x12\x34"
    elif kind == 7:
        lo = rng.between(start, end)
        d[lo:end] = b"\xfe" * (end - lo)
    return d


def copies(data, name, seed=SEED, count=COPIES):
    """(kind, bytes): the intact file, then `count` damaged copies, the kinds in turn."""
    rng = Lcg(seed ^ zlib.crc32(name.encode()))
    yield 0, bytearray(data)
    for i in range(count):
        kind = 1 + i % (len(KINDS) - 1)
        yield kind, damaged(data, kind, rng)


def inspect(lib, data):
    info = _lib.FrameInfo()
    buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    assert lib.jpeg_amd_jpeg_inspect(buf, len(data), C.byref(info)) == 0
    return info


def decode_planes(lib, data, info, threads=1, max_scans=0):
    """Status, planes (filled with 7 before the call) and tables of jpeg_amd_jpeg_decode_spectral_partial."""
    planes = [np.full((info.units_y[c], info.units_x[c], 64), 7, np.int16) for c in range(info.ncomponents)]
    quanta = np.zeros((4, 64), np.uint16)
    buf = (C.c_uint8 * len(data)).from_buffer_copy(bytes(data))
    ptrs = _lib.ptr_array([p.ctypes.data for p in planes])
    if threads == 1 and max_scans == 0:
        st = lib.jpeg_amd_jpeg_decode_spectral(buf, len(data), ptrs, quanta.ctypes.data, None)
    else:
        st = lib.jpeg_amd_jpeg_decode_spectral_partial(buf, len(data), ptrs, quanta.ctypes.data, None, threads, max_scans)
    return st, planes, quanta


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record(lib, data, info, intact):
    """What the fixture holds for one copy: [status, digest] per call."""
    out = {}
    st, planes, quanta = decode_planes(lib, data, info)
    out["spectral"] = [st, digest(*planes, quanta)]
    for n in (1000, 1, 2) if intact else (1000,):
        st, planes, quanta = decode_planes(lib, data, info, max_scans=n)
        out["partial%d" % n] = [st, digest(*planes, quanta)]
    st, desc, entries, _ = sparse_decode(lib, data, info)
    out["sparse"] = [st, digest(desc, entries)]
    return out


def main():
    lib = _lib.lib()
    out = {"seed": SEED, "copies": COPIES, "kinds": KINDS,
           "recorded_with": sys.argv[1] if len(sys.argv) > 1 else os.environ.get("JPEG_AMD_LIBRARY", "the product build"),
           "files": {}}
    for path in files():
        name = os.path.basename(path)
        data = open(path, "rb").read()
        info = inspect(lib, data)
        out["files"][name] = [dict(kind=kind, **record(lib, d, info, kind == 0)) for kind, d in copies(data, name)]
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(FIXTURE, os.path.getsize(FIXTURE), "bytes,", sum(len(v) for v in out["files"].values()), "copies")


if __name__ == "__main__":
    main()
