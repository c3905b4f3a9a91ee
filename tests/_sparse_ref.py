"""The sparse coefficient record (jpeg_amd/csrc/sparse_format.hpp) stated in numpy, for the tests of its writers and readers:
the writer's contract (sparsify_rows), a reader that follows descriptors (rows_of), records constructed with the rows in any
order and poison between them (record), and planes whose blocks cycle through the shapes a writer or reader can get wrong
(pattern_planes).  A row is a block's entries, a uint32 array: value | zigzag index << 16, bit 31 on the last.
Importing this needs no GPU and no torch."""
import ctypes as C

import numpy as np

import _files as F
from _calls import FUSED, c_layout, plane_units
from jpeg_amd import _lib
from jpeg_amd.api import _scan_array

ABSENT = F.ABSENT
LAST = 0x80000000
POISON = 63 << 16 | 0x7FFF                                   # index 63, value 32767, no flag: a reader that strays shows it
SENTINEL32 = 0xA5A5A5A5
WG, WAVE = 256, 64                                           # blocks per k_sparsify workgroup, and per wave of it
PATTERNS = 10

# name -> (width, height, factors).  Blocks: 1; 256 = exactly one k_sparsify workgroup; 17 x 33 = 561; 38 x 18 + 2 * 19 x 9 =
# 684 + 171 + 171, so that planes meet at blocks 684 and 855, inside a workgroup of 256 and a k_expand_sparse group of 32; four
# planes of 3 x 5 = 15, all four inside one workgroup.
LAYOUTS = {
    "one block": (1, 1, FUSED["y8"]),
    "one workgroup": (128, 128, FUSED["y8"]),
    "y8 131x257": (131, 257, FUSED["y8"]),
    "420 300x140": (300, 140, FUSED["420"]),
    "four planes 17x33": (17, 33, [(1, 1)] * 4),
}


def layout(name):
    w, h, factors = LAYOUTS[name]
    return c_layout(w, h, factors, qi=list(range(len(factors))))


def blocks_of(L):
    return sum(ux * uy for ux, uy in plane_units(L))


# ---- the writer's contract, and a reader --------------------------------------------------------------------------------------

def sparsify_rows(planes):
    """The rows a writer owes for `planes` (int16 [uy, ux, 64] each, in frame order): per block an entry for index 0 always,
    one for every nonzero index behind it, ascending, the last one flagged.  -> a row per block of the frame"""
    rows = []
    for plane in planes:
        for block in plane.reshape(-1, 64):
            keep = np.flatnonzero(block)
            if keep.size == 0 or keep[0] != 0:
                keep = np.concatenate([[0], keep])
            row = block[keep].view(np.uint16).astype(np.uint32) | keep.astype(np.uint32) << 16
            row[-1] |= LAST
            rows.append(row)
    return rows


def rows_of(desc, entries):
    """Follow each descriptor to its last-entry flag.  -> a row per descriptor, None for ABSENT.  A descriptor that points
    outside `entries`, or a row that reaches its end without a flag, is an AssertionError."""
    rows = []
    flagged = np.flatnonzero(entries >> 31)
    for b, at in enumerate(desc):
        if at == ABSENT:
            rows.append(None)
            continue
        assert at < entries.size, (b, int(at), entries.size)
        k = np.searchsorted(flagged, at)
        assert k < flagged.size, ("no flag behind", b, int(at))
        rows.append(entries[at:flagged[k] + 1])
    return rows


def same_rows(got, want):
    return len(got) == len(want) and all((g is None and w is None) or (g is not None and w is not None and np.array_equal(g, w))
                                         for g, w in zip(got, want))


def assert_tiles(desc, rows, count):
    """The rows lie pairwise disjoint in [0, count) and leave no hole in it."""
    live = [b for b, r in enumerate(rows) if r is not None]
    order = sorted(live, key=lambda b: int(desc[b]))
    at = 0
    for b in order:
        assert int(desc[b]) == at, ("a hole or an overlap in front of block", b, int(desc[b]), at)
        at += rows[b].size
    assert at == count, (at, count)


def record(rows, order, gap):
    """Descriptors and an arena with rows[b] placed in the order of `order` (a permutation of the blocks), `gap` POISON words in
    front of, between and behind them.  rows[b] None: ABSENT, and nothing in the arena.  -> (desc, arena)"""
    assert sorted(order) == list(range(len(rows)))
    desc = np.full(len(rows), ABSENT, np.uint32)
    parts, at = [np.full(gap, POISON, np.uint32)], gap
    for b in order:
        if rows[b] is None:
            continue
        desc[b] = at
        parts += [rows[b], np.full(gap, POISON, np.uint32)]
        at += rows[b].size + gap
    return desc, np.concatenate(parts).astype(np.uint32)


def group_shuffled(nblocks, seed, group=WG):
    """The order k_sparsify's arena has: the blocks in runs of `group`, the runs in the order their workgroups arrived."""
    runs = [list(range(a, min(a + group, nblocks))) for a in range(0, nblocks, group)]
    np.random.Generator(np.random.PCG64(seed)).shuffle(runs)
    return [b for run in runs for b in run]


# ---- planes -------------------------------------------------------------------------------------------------------------------

def pattern_planes(units, seed, safe=False):
    """Planes [uy, ux, 64] in which block b of the frame (planes in frame order) takes pattern b % 10:
       0 all zero                      1 the DC only, -32768 (the value 0x8000)       2 index 63 only, 32767
       3 index 1 only                  4 all 64 nonzero, signs alternating             5 the even indices only
       6 the odd indices only          7 exactly 24 nonzero, anywhere                  8 the last slot of each octet: 7, 15 .. 63
       9 what _files.sparse_planes has there
    safe: every value within +-1000, what baseline Huffman coding holds (patterns 1 and 2 take -1000 and 1000)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    lo, hi = (-1000, 1000) if safe else (-32768, 32767)
    nb = sum(ux * uy for ux, uy in units)
    frame = np.zeros((nb, 64), np.int16)
    like_a_file = np.concatenate([p.reshape(-1, 64) for p in F.sparse_planes(units, seed + 7)])
    k = np.arange(64)

    def nonzero(n):
        v = rng.integers(1, hi + 1, n) * rng.choice([-1, 1], n)
        return v.astype(np.int16)

    for b in range(nb):
        pat = b % PATTERNS
        if pat == 1:
            frame[b, 0] = lo
        elif pat == 2:
            frame[b, 63] = hi
        elif pat == 3:
            frame[b, 1] = nonzero(1)[0]
        elif pat == 4:
            frame[b] = np.abs(nonzero(64)) * np.where(k % 2 == 0, 1, -1)
        elif pat == 5:
            frame[b, 0::2] = nonzero(32)
        elif pat == 6:
            frame[b, 1::2] = nonzero(32)
        elif pat == 7:
            frame[b, rng.permutation(rng.integers(24, 65))[:24]] = nonzero(24)   # (among the first 24 .. 64: the last one in any octet)
        elif pat == 8:
            frame[b, 7::8] = nonzero(8)
        elif pat == 9:
            frame[b] = like_a_file[b]
    planes, first = [], 0
    for ux, uy in units:
        planes.append(frame[first:first + ux * uy].reshape(uy, ux, 64).copy())
        first += ux * uy
    return planes


def entry_count(planes):
    return sum(r.size for r in sparsify_rows(planes))


def top_up(planes, extra):
    """`extra` more nonzero coefficients (the value 5), in place: into the zero AC slots of the frame's blocks, first block
    first.  The count of entries grows by exactly `extra`."""
    for plane in planes:
        for block in plane.reshape(-1, 64):                   # (a view: the planes are contiguous)
            for z in range(1, 64):
                if extra == 0:
                    return planes
                if block[z] == 0:
                    block[z] = 5
                    extra -= 1
    assert extra == 0, "no room"
    return planes


def three_images(name, seed, safe=False, equal=False):
    """The planes of the three images of one call on LAYOUTS[name]; equal: topped up to the same count of entries."""
    units = plane_units(layout(name))
    images = [pattern_planes(units, seed + 100 * i, safe) for i in range(3)]
    if equal:
        counts = [entry_count(p) for p in images]
        for p, c in zip(images, counts):
            top_up(p, max(counts) - c)
    return images


# ---- the host writers -----------------------------------------------------------------------------------------------------------

def write_files(L, planes, desc, entries, interleaved, restart):
    """`planes` through jpeg_amd_jpeg_encode_spectral and the record (desc, entries) through jpeg_amd_jpeg_encode_sparse, one
    interleaved scan or a scan per component, extended sequential (four table slots, any component count).  -> (bytes, bytes)"""
    n = L.nplanes
    scans = [[(c, min(c, 1), min(c, 1)) for c in range(n)]] if interleaved else [[(c, min(c, 1), min(c, 1))] for c in range(n)]
    info = F.frame_info(L, 1, restart)
    keys, tkeys = (C.c_int32 * n)(*[min(c, 1) for c in range(n)]), (C.c_int32 * 2)(0, 1)
    q = F.tables(n, 3)
    sarr = _scan_array(scans)
    planes = [np.ascontiguousarray(p) for p in planes]
    desc, entries = np.ascontiguousarray(desc, np.uint32), np.ascontiguousarray(entries, np.uint32)
    lib = _lib.lib()
    out = [np.zeros(512 * blocks_of(L) + 4096, np.uint8) for _ in range(2)]
    size = [C.c_size_t(), C.c_size_t()]
    assert lib.jpeg_amd_jpeg_encode_spectral(C.byref(info), keys, _lib.ptr_array([p.ctypes.data for p in planes]), q.ctypes.data, tkeys,
                                             q.shape[0], sarr, len(scans), None, 0, out[0].ctypes.data, out[0].size, C.byref(size[0])) == 0
    assert lib.jpeg_amd_jpeg_encode_sparse(C.byref(info), keys, desc.ctypes.data, entries.ctypes.data, entries.size, q.ctypes.data, tkeys,
                                           q.shape[0], sarr, len(scans), None, 0, out[1].ctypes.data, out[1].size, C.byref(size[1])) == 0
    return out[0][:size[0].value].tobytes(), out[1][:size[1].value].tobytes()
