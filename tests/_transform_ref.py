"""numpy restatement of the lossless spectral transforms (include/jpeg_amd.h, JPEG_AMD_XFORM_*), written from the reference's
examples/rotate/main.swift (Block.transform with its procedural transpose / reflectHorizontal / reflectVertical, the
block-index `matrix` / `offset`, Spectral.set(width:) / set(height:)) and examples/recompress/main.swift:52-56 -- independent of
the library's own tables."""
import ctypes as C
import os

import numpy as np

from jpeg_amd import _lib
from jpeg_amd.zigzag import z as zz

ROOT = os.path.dirname(os.path.abspath(__file__))
XFORM_DIR = os.path.join(ROOT, "golden", "transform")
OPS = {"none": 0, "transpose": 1, "flip_h": 2, "rot_cw": 3, "flip_v": 4, "rot_ccw": 5, "rot_180": 6, "transverse": 7}


def xpath(name):
    return os.path.join(XFORM_DIR, name)


# ---- Block.transform (examples/rotate/main.swift) ---------------------------------------------
def _transpose(a):
    return [a[8 * x + y] for y in range(8) for x in range(8)]


def _reflect_vertical(a):
    return [(a[8 * y + x][0], a[8 * y + x][1] * (1 - 2 * (y & 1))) for y in range(8) for x in range(8)]


def _reflect_horizontal(a):
    return [(a[8 * y + x][0], a[8 * y + x][1] * (1 - 2 * (x & 1))) for y in range(8) for x in range(8)]


def block_mapping(op):
    """[(m(z), sign(z))] for z in 0..63: transpose, then reflectHorizontal, then reflectVertical as the op's bits say."""
    blank = [(zz(x, y), 1) for y in range(8) for x in range(8)]
    r = blank
    if op & 1:
        r = _transpose(r)
    if op & 2:
        r = _reflect_horizontal(r)
    if op & 4:
        r = _reflect_vertical(r)
    out = [None] * 64
    for h in range(8):
        for k in range(8):
            out[zz(k, h)] = r[8 * h + k]
    return out


def mapping_arrays(op):
    m = block_mapping(op)
    return np.array([a for a, _ in m]), np.array([b for _, b in m], np.int32)


# ---- geometry ----------------------------------------------------------------------------------
def _units(n, s):
    return -(-n // s)


def layout_ref(width, height, factors, op, region=None):
    """-> (out_width, out_height, out_factors, out_units, cropped_units, origin_blocks) or None for EINVAL.
    factors: [(fx, fy)] of every plane; scale = the max over them."""
    sx, sy = max(f[0] for f in factors), max(f[1] for f in factors)
    x, y, w, h = region if region is not None else (0, 0, width, height)
    if x < 0 or y < 0 or x >= width or y >= height or x % (8 * sx) or y % (8 * sy) or w <= 0 or h <= 0:
        return None
    T = op & 1
    mirror_x = (op & 4) if T else (op & 2)
    mirror_y = (op & 2) if T else (op & 4)
    if mirror_x:
        w -= w % (8 * sx)
    if mirror_y:
        h -= h % (8 * sy)
    if w <= 0 or h <= 0:
        return None
    cropped = [(_units(w * fx, 8 * sx), _units(h * fy, 8 * sy)) for fx, fy in factors]
    origin = [(x // (8 * sx) * fx, y // (8 * sy) * fy) for fx, fy in factors]
    if T:
        ow, oh, ofac, osx, osy = h, w, [(fy, fx) for fx, fy in factors], sy, sx
    else:
        ow, oh, ofac, osx, osy = w, h, list(factors), sx, sy
    units = [(_units(ow * fx, 8 * osx), _units(oh * fy, 8 * osy)) for fx, fy in ofac]
    return ow, oh, ofac, units, cropped, origin


def transform_plane(plane, op, cropped_units, origin):
    """plane int16 [uy, ux, 64] -> the transformed plane: Spectral.set(width:/height:) from the origin (new blocks zero), the
    block grid transposed / mirrored (the example's matrix + offset), the coefficients permuted and sign-flipped."""
    cux, cuy = cropped_units
    ox, oy = origin
    c = np.zeros((cuy, cux, 64), np.int32)
    src = plane[oy:oy + cuy, ox:ox + cux].astype(np.int32)
    c[:src.shape[0], :src.shape[1]] = src
    if op & 1:
        c = c.transpose(1, 0, 2)
    if op & 2:
        c = c[:, ::-1]
    if op & 4:
        c = c[::-1, :]
    m, sign = mapping_arrays(op)
    return c[..., m] * sign


def requantize_ref(plane_t, q_in_t, q_out):
    """examples/recompress/main.swift:52-56 on an already transformed plane (sign applied) and the transformed input table:
    Int16 product, float64 quotient, + 0.3 * sign, truncation.  Returns (values, trapped)."""
    v = plane_t.astype(np.int64) * np.asarray(q_in_t, np.int64)
    q_out = np.asarray(q_out, np.int64)
    trapped = bool((v < -32768).any() or (v > 32767).any() or (q_out == 0).any() or (np.asarray(q_in_t) > 32767).any())
    r = v.astype(np.float64) / np.where(q_out == 0, 1, q_out).astype(np.float64)
    r = r + 0.3 * np.where(r < 0, -1.0, 1.0)
    return np.trunc(r).astype(np.int64), trapped


# ---- the shapes of the seam tests (test_gpu_transform_shapes, test_transform_cpu) ---------------
# A workgroup of k_spectral_transform covers 256 x 1 output blocks (ops that keep the axes) or 32 x 8 (transposing ops).
LAYOUTS = {"y8": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)],
           "440": [(1, 2), (1, 1), (1, 1)], "411": [(4, 1), (1, 1), (1, 1)], "4p": [(2, 2), (2, 2), (2, 2), (1, 1)]}
# (4133, 37): luma 517 x 5 blocks, split 256 / 256 / 5 by the 256-block workgroups, 4:2:0 chroma 259 x 3 behind it;
# (150, 600): luma 19 x 75, 4:2:0 chroma 10 x 38: transposed, past 32 blocks in x and 8 in y in every plane;
# (1, 1), (9, 15): planes of one block and of 2 x 2
SEAM_SIZES = [(4133, 37), (150, 600), (1, 1), (9, 15)]
# luma 257 x 33: one block past a seam of either workgroup shape, where a rounded-down count of workgroups per row shows
# (none of the sizes above has a plane of 256 k + 1 or 32 k + 1 blocks other than 1)
SEAM_PLUS_ONE = {"y8": [(2049, 257)], "420": [(2049, 257)]}


def seam_sizes(name):
    return SEAM_SIZES + SEAM_PLUS_ONE.get(name, [])


def layout_tables(name):
    """-> (qi per plane, number of tables) of a LAYOUTS entry."""
    n = len(LAYOUTS[name])
    qi = [0, 1, 1, 2] if n == 4 else [min(p, 1) for p in range(n)]
    return qi, max(qi) + 1


def seam_regions(w, h, factors):
    """None, an interior region (where there is room for one), a region that grows from the origin past a workgroup seam of
    either tile shape, and one that grows from the last MCU column, so that almost every output block is new."""
    sx, sy = max(f[0] for f in factors), max(f[1] for f in factors)
    regions = [None]
    if w - 8 * sx - 5 > 0 and h - 8 * sy - 3 > 0:
        regions.append((8 * sx, 8 * sy, w - 8 * sx - 5, h - 8 * sy - 3))
    regions.append((0, 0, w + 320 * sx + 3, h + 72 * sy + 1))
    regions.append(((w - 1) // (8 * sx) * 8 * sx, 0, 320 * sx + 3, h + 72 * sy + 1))
    return regions


# ---- the C entry points ------------------------------------------------------------------------
def c_layout(width, height, factors, precision=8):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes = width, height, precision, len(factors)
    L.scale_x, L.scale_y = max(f[0] for f in factors), max(f[1] for f in factors)
    for p, (fx, fy) in enumerate(factors):
        L.factor_x[p], L.factor_y[p], L.qi[p] = fx, fy, p
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def c_transform_layout(L, op, region=None):
    out = _lib.Layout()
    reg = None
    if region is not None:
        r = _lib.Region(*region)
        reg = C.byref(r)
    st = _lib.lib().jpeg_amd_transform_layout(C.byref(L), op, reg, C.byref(out))
    return st, out


def c_script(data):
    """jpeg_amd_jpeg_script -> (scans as tuples, keys, metadata as (kind, app, bytes))."""
    lib = _lib.lib()
    data = np.ascontiguousarray(data, np.uint8)
    ns, nm = C.c_int(), C.c_int()
    keys = (C.c_int32 * 4)()
    st = lib.jpeg_amd_jpeg_script(data.ctypes.data, data.size, None, 0, C.byref(ns), keys, None, 0, C.byref(nm))
    if st != 0:
        return st, None, None, None
    scans = (_lib.Scan * max(ns.value, 1))()
    meta = (_lib.Metadata * max(nm.value, 1))()
    st = lib.jpeg_amd_jpeg_script(data.ctypes.data, data.size, scans, ns.value, C.byref(ns), keys, meta, nm.value, C.byref(nm))
    if st != 0:
        return st, None, None, None
    base = data.ctypes.data
    out_scans = [(s.ncomponents, tuple((s.component[j], s.dc[j], s.ac[j]) for j in range(s.ncomponents)),
                  s.band_lo, s.band_hi, s.bit, s.refine) for s in scans[:ns.value]]
    out_meta = []
    for m in meta[:nm.value]:
        off = m.data - base
        assert 0 <= off and off + m.size <= data.size          # points into the input buffer
        out_meta.append((m.kind, m.app, bytes(data[off:off + m.size])))
    return 0, out_scans, list(keys), out_meta


def decode_file(data):
    """Host entropy decoding: (info, planes, per-component tables)."""
    lib = _lib.lib()
    data = np.ascontiguousarray(data, np.uint8)
    info = _lib.FrameInfo()
    assert lib.jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) == 0
    planes = [np.zeros((info.units_y[c], info.units_x[c], 64), np.int16) for c in range(info.ncomponents)]
    quanta = np.zeros((4, 64), np.uint16)
    assert lib.jpeg_amd_jpeg_decode_spectral(data.ctypes.data, data.size, _lib.ptr_array([p.ctypes.data for p in planes]),
                                             quanta.ctypes.data, C.byref(info)) == 0
    return info, planes, quanta[:info.ncomponents]
