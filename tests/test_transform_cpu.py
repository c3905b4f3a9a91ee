"""The host halves of the lossless spectral transforms -- no GPU: jpeg_amd_transform_layout (geometry, trim, region),
jpeg_amd_transform_quanta (the example's Block.transform restated in _transform_ref) and jpeg_amd_jpeg_script (the scan
script, table keys and metadata segments of a file, against a Python marker walk)."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _transform_ref as R
from _golden import GOLDEN
from jpeg_amd import _lib
from test_entropy_encode_cpu import _script

JPEGS = sorted(glob.glob(os.path.join(GOLDEN, "**", "*.jpg"), recursive=True))


def _frame(path):
    info = _lib.FrameInfo()
    data = np.fromfile(path, np.uint8)
    assert _lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) == 0
    factors = [(info.factor_x[c], info.factor_y[c]) for c in range(info.ncomponents)]
    return info, factors


def _check(L, factors, op, region):
    st, out = R.c_transform_layout(L, op, region)
    want = R.layout_ref(L.width, L.height, factors, op, region)
    if want is None:
        assert st == _lib.EINVAL
        return None
    assert st == 0
    ow, oh, ofac, units, cropped, _ = want
    assert (out.width, out.height) == (ow, oh)
    assert (out.scale_x, out.scale_y) == (max(f[0] for f in ofac), max(f[1] for f in ofac))
    for p in range(len(factors)):
        assert (out.factor_x[p], out.factor_y[p]) == ofac[p]
        assert (out.units_x[p], out.units_y[p]) == units[p]
        assert units[p] == (cropped[p][::-1] if op & 1 else cropped[p])   # the block grid is transposed, not resized
        assert out.qi[p] == L.qi[p]
    return out


@pytest.mark.parametrize("path", JPEGS, ids=lambda p: os.path.relpath(p, GOLDEN))
def test_layout_of_every_op_on_every_fixture_frame(path):
    info, factors = _frame(path)
    L = R.c_layout(info.width, info.height, factors, info.precision)
    sx, sy = L.scale_x, L.scale_y
    for op in range(8):
        out = _check(L, factors, op, None)
        T = op & 1
        # the example's trim: ROT_CCW / ROT_180 / FLIP_H / TRANSVERSE cut the width, ROT_CW / ROT_180 / FLIP_V / TRANSVERSE
        # the height, to whole MCUs; other edges are kept
        trims_w = op in (2, 5, 6, 7)
        trims_h = op in (3, 4, 6, 7)
        w = info.width - info.width % (8 * sx) if trims_w else info.width
        h = info.height - info.height % (8 * sy) if trims_h else info.height
        assert (out.width, out.height) == ((h, w) if T else (w, h))
        # one MCU-aligned region inside the image, one reaching past it
        _check(L, factors, op, (8 * sx, 8 * sy, max(info.width // 2, 1), max(info.height // 3, 1)))
        _check(L, factors, op, (0, 8 * sy, info.width + 37, info.height + 3))


@pytest.mark.parametrize("name", sorted(R.LAYOUTS))
def test_layout_of_every_op_at_the_seam_shapes(name):
    """The layouts, sizes and regions of test_gpu_transform_shapes: the library's geometry against the restatement's, EINVAL
    exactly where a mirror trims the image to nothing."""
    factors = R.LAYOUTS[name]
    qi, _ = R.layout_tables(name)
    refused = 0
    for w, h in R.seam_sizes(name):
        L = R.c_layout(w, h, factors)
        for p, t in enumerate(qi):
            L.qi[p] = t
        for op in range(8):
            for region in R.seam_regions(w, h, factors):
                refused += _check(L, factors, op, region) is None
    assert refused                                        # (1, 1) under a mirror, at the least
    # the unit counts the seam tests are built on
    units = lambda size, op=0: R.layout_ref(*size, factors, op)[3]
    assert units((4133, 37))[0] == (517, 5) and units((150, 600))[0] == (19, 75)
    assert units((150, 600), 1)[0] == (75, 19)
    assert all(units(size)[0] == (257, 33) for size in R.SEAM_PLUS_ONE.get(name, []))
    if name == "420":
        assert units((4133, 37))[1] == (259, 3) and units((150, 600))[1] == (10, 38)
    if name == "411":
        assert units((4133, 37))[1] == (130, 5)


def test_every_op_of_the_restatement_is_the_geometric_transform_in_pixel_space():
    """The float64 inverse cosine transform of R.transform_plane(plane, op) is that of the plane, transposed and / or mirrored
    as op's bits say.  In real arithmetic the identity is exact (a mirror of cos((2x+1)k pi/16) in x is its negation for odd
    k), so the bound is float64 rounding alone: 1e-12 of the largest source sample (the worst of the 8 ops is 1.1e-15 of it).
    This anchors the restatement's TRANSPOSE, FLIP_H, FLIP_V and TRANSVERSE, which no file of the reference covers."""
    from jpeg_amd.zigzag import z as zz
    ux, uy = 5, 7
    rng = np.random.default_rng(23)
    plane = rng.integers(-32767, 32768, (uy, ux, 64)).astype(np.int16)
    k = np.arange(8)
    basis = np.cos((2 * k[:, None] + 1) * k[None, :] * np.pi / 16)         # [x, k]
    basis[:, 0] = 1 / np.sqrt(2)
    unzig = np.array([[zz(kk, hh) for kk in range(8)] for hh in range(8)])  # [h, k]

    def samples(p):
        f = p.astype(np.float64)[..., unzig]                                # [by, bx, h, k]
        s = np.einsum("yh,xk,abhk->aybx", basis, basis, f)
        return s.reshape(8 * p.shape[0], 8 * p.shape[1])

    source = samples(plane)
    bound = 1e-12 * np.abs(source).max()
    for op in range(8):
        want = source
        if op & 1:
            want = want.T
        if op & 2:
            want = want[:, ::-1]
        if op & 4:
            want = want[::-1, :]
        got = samples(R.transform_plane(plane, op, (ux, uy), (0, 0)))
        assert got.shape == want.shape
        err = np.abs(got - want).max()
        print(f"op {op}: {err / np.abs(source).max():.2e} of the largest sample")
        assert err <= bound, (op, err, bound)


def test_transposing_ops_swap_the_sampling_layout():
    for factors, want in (([(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)]),     # 4:2:2 -> 4:4:0
                          ([(2, 2), (1, 1), (1, 1)], [(2, 2), (1, 1), (1, 1)]),     # 4:2:0 stays
                          ([(1, 1)] * 3, [(1, 1)] * 3)):
        L = R.c_layout(333, 201, factors)
        for op in (1, 3, 5, 7):
            st, out = R.c_transform_layout(L, op)
            assert st == 0
            assert [(out.factor_x[p], out.factor_y[p]) for p in range(3)] == want
            assert (out.scale_x, out.scale_y) == (L.scale_y, L.scale_x)
        for op in (0, 2, 4, 6):
            st, out = R.c_transform_layout(L, op)
            assert [(out.factor_x[p], out.factor_y[p]) for p in range(3)] == factors


def test_region_growth_and_set_width_height():
    L = R.c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    st, out = R.c_transform_layout(L, 0, (0, 0, 250, 61))     # Spectral.set(width: 250), set(height: 61)
    assert st == 0 and (out.width, out.height) == (250, 61)
    assert [(out.units_x[p], out.units_y[p]) for p in range(3)] == [(32, 8), (16, 4), (16, 4)]
    st, out = R.c_transform_layout(L, 0, (16, 32, 8, 8))       # a single partial MCU
    assert st == 0 and (out.width, out.height) == (8, 8)
    assert [(out.units_x[p], out.units_y[p]) for p in range(3)] == [(1, 1), (1, 1), (1, 1)]
    st, out = R.c_transform_layout(L, 6, (16, 32, 8, 8))       # ... which ROT_180 trims to nothing
    assert st == _lib.EINVAL


def test_invalid_regions():
    L = R.c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    for region in ((8, 0, 16, 16),     # x not a multiple of 8 * scale_x
                   (0, 24, 16, 16),    # y not a multiple of 8 * scale_y
                   (112, 0, 16, 16),   # origin outside the image
                   (0, 64, 16, 16),
                   (0, 0, 0, 16),      # zero size
                   (0, 0, 16, 0),
                   (-16, 0, 16, 16)):
        assert R.c_transform_layout(L, 0, region)[0] == _lib.EINVAL, region
    assert R.c_transform_layout(L, 8)[0] == _lib.EINVAL
    assert R.c_transform_layout(L, -1)[0] == _lib.EINVAL
    L1 = R.c_layout(100, 60, [(1, 1)])
    assert R.c_transform_layout(L1, 0, (8, 8, 16, 16))[0] == 0


def test_quanta_follow_the_examples_block_transform():
    lib = _lib.lib()
    rng = np.random.default_rng(7)
    tables = [np.arange(64, dtype=np.uint16), rng.integers(1, 65535, 64).astype(np.uint16)]
    for op in range(8):
        m, _ = R.mapping_arrays(op)
        for t in tables:
            out = np.zeros(64, np.uint16)
            assert lib.jpeg_amd_transform_quanta(op, t.ctypes.data, out.ctypes.data) == 0
            assert (out == t[m]).all()
    assert lib.jpeg_amd_transform_quanta(8, tables[0].ctypes.data, np.zeros(64, np.uint16).ctypes.data) == _lib.EINVAL


def test_block_mapping_of_the_examples_rotations():
    """The example's three rotations are the named ops: 'ii' = reflectVertical(transpose) = ROT_CCW, 'iii' =
    reflectVertical(reflectHorizontal) = ROT_180, 'iv' = reflectHorizontal(transpose) = ROT_CW."""
    assert _lib.XFORM["ii"] == R.OPS["rot_ccw"] == 5
    assert _lib.XFORM["iii"] == R.OPS["rot_180"] == 6
    assert _lib.XFORM["iv"] == R.OPS["rot_cw"] == 3
    # a rotation by 90 degrees four times is the identity, in the block as well
    m, s = R.mapping_arrays(5)
    idx, sign = np.arange(64), np.ones(64, np.int32)
    for _ in range(4):
        idx, sign = idx[m], sign[m] * s
    assert (idx == np.arange(64)).all() and (sign == 1).all()


def _python_script(data):
    process, metadata, scans, keys, tkeys, _ = _script(data)
    meta = [(2, 0, bytes(m[1])) if m[0] == "comment" else (1, m[1], bytes(m[2])) for m in metadata]
    sc = []
    for s in scans:
        sc.append((len(s.components), tuple(tuple(c) for c in s.components), s.band[0], s.band[1], s.bit, s.refine))
    return sc, keys, meta


@pytest.mark.parametrize("path", JPEGS, ids=lambda p: os.path.relpath(p, GOLDEN))
def test_script_matches_a_marker_walk(path):
    data = np.fromfile(path, np.uint8)
    st, scans, keys, meta = R.c_script(data)
    assert st == 0
    want_scans, want_keys, want_meta = _python_script(data)
    assert scans == want_scans
    assert keys[:len(want_keys)] == want_keys
    assert meta == want_meta


def test_script_refuses_too_small_arrays_and_garbage():
    lib = _lib.lib()
    data = np.fromfile(R.xpath("karlie-kwk-wwdc-2017.jpg"), np.uint8)
    ns, nm = C.c_int(), C.c_int()
    keys = (C.c_int32 * 4)()
    assert lib.jpeg_amd_jpeg_script(data.ctypes.data, data.size, None, 0, C.byref(ns), keys, None, 0, C.byref(nm)) == 0
    assert ns.value >= 1
    if ns.value > 1:
        scans = (_lib.Scan * 1)()
        assert lib.jpeg_amd_jpeg_script(data.ctypes.data, data.size, scans, 1, C.byref(ns), keys, None, 0,
                                        C.byref(nm)) == _lib.EINVAL
    junk = np.zeros(64, np.uint8)
    assert lib.jpeg_amd_jpeg_script(junk.ctypes.data, junk.size, None, 0, C.byref(ns), keys, None, 0,
                                    C.byref(nm)) == _lib.EINVAL
