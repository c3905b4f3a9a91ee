"""What the tests of the file-to-tensor calls (jpeg_amd_spectral_expand_mixed, jpeg_amd_decompress_tensor_mixed,
jpeg_amd_decompress_resized_mixed) share, each stated once: JPEG files made on the host from synthetic coefficient planes
(jpeg_amd_jpeg_encode_spectral: sequential, with a restart interval, progressive), their sparse records, and a numpy mirror of
the windowed expand's contract.  Importing this needs no GPU and no torch."""
import ctypes as C

import numpy as np

import _golden as G
from _calls import FUSED, c_layout, plane_units
from jpeg_amd import _lib
from jpeg_amd.api import Scan, _scan_array

ABSENT = 0xFFFFFFFF
SENTINEL16 = np.int16(-23131)                              # 0xA5A5: two sentinel bytes


# ---- files ----------------------------------------------------------------------------------------------------------------------

def sparse_planes(units, seed):
    """Coefficient planes [uy, ux, 64] as a sequential file of a photograph has them: every DC, about a dozen AC coefficients
    per block that thin out towards the high frequencies -- few enough for the sparse decoder's arena (24 entries per block),
    with entries in every octet of some block.  Magnitudes stay inside what baseline Huffman coding holds (10 bits)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    planes = []
    scale = (400.0 / (1.0 + np.arange(64)) ** 2.5).astype(np.float32)
    for ux, uy in units:
        v = np.rint(rng.laplace(0.0, 1.0, (uy, ux, 64)).astype(np.float32) * scale)
        for z in (9, 26, 33, 47, 63):                         # a few in the later octets too, the last coefficient included
            v[..., z] = np.where(rng.random((uy, ux)) < 0.1, rng.integers(-9, 10, (uy, ux)), v[..., z])
        v[..., 0] = rng.integers(-1000, 1000, (uy, ux))
        planes.append(np.clip(v, -1000, 1000).astype(np.int16))
    return planes


def dense_planes(units, seed):
    """Planes with most of the 64 coefficients of every block set: more than the sparse decoder's arena holds."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return [np.clip(rng.integers(-40, 41, (uy, ux, 64)), -1000, 1000).astype(np.int16) for ux, uy in units]


def tables(nplanes, seed):
    """uint16 [min(nplanes, 2), 64]: a table for the first component and one for the others (baseline has two slots)."""
    return np.random.Generator(np.random.PCG64(seed + 1)).integers(1, 24, (min(nplanes, 2), 64)).astype(np.uint16)


def frame_info(L, process=0, restart=0):
    info = _lib.FrameInfo()
    info.width, info.height, info.precision, info.ncomponents = L.width, L.height, L.precision, L.nplanes
    info.process, info.scale_x, info.scale_y, info.restart_interval = process, L.scale_x, L.scale_y, restart
    for p in range(L.nplanes):
        info.id[p] = p + 1
        info.factor_x[p], info.factor_y[p] = L.factor_x[p], L.factor_y[p]
        info.units_x[p], info.units_y[p] = L.units_x[p], L.units_y[p]
    return info


def progressive_script(nplanes):
    """Spectral selection and successive approximation: DC with a point transform, its refinement, two AC bands per
    component and the refinement of the first."""
    scans = [Scan.progressive_dc(*[(c, min(c, 1)) for c in range(nplanes)], bits=1),
             Scan.progressive_dc_refine(*range(nplanes), bit=0)]
    for c in range(nplanes):
        scans += [Scan.progressive_ac((c, min(c, 1)), (1, 6), 1), Scan.progressive_ac((c, min(c, 1)), (6, 64), 0),
                  Scan.progressive_ac_refine((c, min(c, 1)), (1, 6), 0)]
    return scans


def write_file(L, planes, quanta, kind="sequential", restart=0):
    """The file of `planes` (jpeg_amd_jpeg_encode_spectral) -> uint8 array.  kind: "sequential" (one interleaved scan),
    "scans" (a scan per component), "progressive"."""
    n = L.nplanes
    if kind == "progressive":
        scans, process = progressive_script(n), 2
    elif kind == "scans":
        scans, process = [[(c, min(c, 1), min(c, 1))] for c in range(n)], 0
    else:
        scans, process = [[(c, min(c, 1), min(c, 1)) for c in range(n)]], 0
    if L.precision != 8:
        process = max(process, 1)                              # baseline is 8-bit
    info = frame_info(L, process, restart)
    keys, tkeys = (C.c_int32 * n)(*[min(c, 1) for c in range(n)]), (C.c_int32 * 2)(0, 1)
    q = np.ascontiguousarray(quanta, np.uint16)
    size = C.c_size_t()
    args = [C.byref(info), keys, _lib.ptr_array([p.ctypes.data for p in planes]), q.ctypes.data, tkeys, q.shape[0], _scan_array(scans),
            len(scans), None, 0]
    lib = _lib.lib()
    assert lib.jpeg_amd_jpeg_encode_spectral(*args, None, 0, C.byref(size)) == 0
    out = np.empty(size.value, np.uint8)
    assert lib.jpeg_amd_jpeg_encode_spectral(*args, out.ctypes.data, out.size, C.byref(size)) == 0
    return out[:size.value].copy()


def synthetic_file(name, size, seed, kind="sequential", restart=0, precision=8, factors=None):
    """A file of layout FUSED[name] (or `factors`) and `size` -> (bytes, its C layout).  kind "dense": a sequential file too
    dense for the sparse decoder."""
    L = c_layout(size[0], size[1], factors or FUSED[name], precision=precision, qi=list(range(len(factors or FUSED[name]))))
    planes = dense_planes(plane_units(L), seed) if kind == "dense" else sparse_planes(plane_units(L), seed)
    return write_file(L, planes, tables(L.nplanes, seed), "sequential" if kind == "dense" else kind, restart), L


def undefined_tables(data):
    """A copy whose first scan header names Huffman tables the file does not define: it passes jpeg_amd_jpeg_inspect and fails
    in the entropy decoder, sparse or not."""
    bad = data.copy()
    sos = bytes(bad).index(b"\xff\xda")
    assert bad[sos + 6] in (0, 0x11)
    bad[sos + 6] = 0x33
    return bad


def lossless_marker(data):
    """A copy whose frame header is marked lossless (SOF3): ENOSUP from every reader, jpeg_amd_jpeg_inspect included."""
    bad = data.copy()
    bad[bytes(bad).index(b"\xff\xc0") + 1] = 0xC3
    return bad


def golden_file(name):
    return np.fromfile(G.path("decode/" + name), np.uint8)


def inspect(data):
    info = _lib.FrameInfo()
    assert _lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) == 0
    return info


def layout_of(info):
    """The layout the file calls give a frame: component c's table is table c."""
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes = info.width, info.height, info.precision, info.ncomponents
    L.scale_x, L.scale_y = info.scale_x, info.scale_y
    for c in range(info.ncomponents):
        L.factor_x[c], L.factor_y[c], L.units_x[c], L.units_y[c], L.qi[c] = (info.factor_x[c], info.factor_y[c], info.units_x[c],
                                                                             info.units_y[c], c)
    return L


def decode_planes(data):
    """jpeg_amd_jpeg_decode_spectral -> (info, planes [uy, ux, 64], quanta [4, 64])."""
    info = inspect(data)
    planes = [np.full((info.units_y[c], info.units_x[c], 64), 77, np.int16) for c in range(info.ncomponents)]
    quanta = np.zeros((4, 64), np.uint16)
    assert _lib.lib().jpeg_amd_jpeg_decode_spectral(data.ctypes.data, data.size, _lib.ptr_array([p.ctypes.data for p in planes]),
                                                    quanta.ctypes.data, None) == 0
    return info, planes, quanta


def decode_sparse(data):
    """jpeg_amd_jpeg_decode_sparse -> (status, info, record uint32 [blocks + entries]: the descriptors, then the entries)."""
    info = inspect(data)
    blocks = sum(info.units_x[c] * info.units_y[c] for c in range(info.ncomponents))
    record = np.zeros(25 * blocks + 72, np.uint32)              # (the decoder wants room for a whole block in front of it)
    n = C.c_size_t()
    quanta = np.zeros((4, 64), np.uint16)
    st = _lib.lib().jpeg_amd_jpeg_decode_sparse(data.ctypes.data, data.size, record.ctypes.data, blocks, record[blocks:].ctypes.data,
                                                24 * blocks + 72, C.byref(n), quanta.ctypes.data, None)
    return st, info, record[:blocks + n.value].copy()


# ---- the contract of the windowed expand ---------------------------------------------------------------------------------------

def whole_windows(L):
    return [(0, 0, ux, uy) for ux, uy in plane_units(L)]


def expand_mirror(L, record, windows, head, into=None):
    """What jpeg_amd_spectral_expand_mixed leaves in planes that held SENTINEL16 everywhere (or `into`, changed in place): inside
    every window the first 8 * head coefficients of each block as jpeg_amd_spectral_expand_batch rebuilds them from `record`
    (zeros, then every entry of the block up to its last-entry flag, a later one over an earlier one), everything else as it
    was.  record: the image's descriptors, then its entries.  -> planes int16 [uy, ux, 64]"""
    units = plane_units(L)
    blocks = sum(ux * uy for ux, uy in units)
    desc, entries = record[:blocks], record[blocks:]
    planes = into if into is not None else [np.full((uy, ux, 64), SENTINEL16, np.int16) for ux, uy in units]
    first = 0
    for (ux, uy), plane, (x0, y0, w, h) in zip(units, planes, windows):
        for y in range(y0, y0 + h):
            for x in range(x0, x0 + w):
                block = np.zeros(64, np.int16)
                at = int(desc[first + y * ux + x])
                while at != ABSENT:
                    v = int(entries[at])
                    block[(v >> 16) & 63] = np.uint16(v & 0xFFFF).astype(np.int16)
                    if v >> 31:
                        break
                    at += 1
                plane[y, x, :8 * head] = block[:8 * head]
        first += ux * uy
    return planes
