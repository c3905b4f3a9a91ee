"""The host half of region decode -- no GPU: jpeg_amd_region_window (which blocks of each plane the pixels of a rectangle
read) against a brute-force restatement of the interleave index formula (decode.swift:4182-4276, oracle/jpeg_oracle.c
orc_interleave_rows), and the region checks of the three entry points."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import jpeg_amd as J
from _calls import c_layout
from _golden import GOLDEN
from jpeg_amd import _lib

DECODE = sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg")))


def _window(L, cosited, region):
    r = _lib.Region(*region)
    w = (_lib.Region * _lib.MAX_PLANES)()
    st = _lib.lib().jpeg_amd_region_window(C.byref(L), cosited, C.byref(r), w)
    return st, [(w[p].x, w[p].y, w[p].width, w[p].height) for p in range(_lib.MAX_PLANES)]


def _samples(t, f, s, units, direct, cosited):
    """Every sample index pixels t read along one axis: the oracle's formula, C truncation, jx = min(ix + 1, 8 units - 1)."""
    if direct:
        return t
    a, b, c = (0, f, s) if cosited else (f - s, 2 * f, 2 * s)
    n = a + b * t.astype(np.int64)
    i = np.sign(n) * (np.abs(n) // c)                  # truncation toward zero, like C's / and quotientAndRemainder
    j = np.minimum(i + 1, 8 * units - 1)
    return np.concatenate([i, j])


def _brute(L, cosited, region):
    """Bounding box, in blocks, of the samples every pixel of `region` reads.  The sample a pixel (x, y) reads is
    (sample_x(x), sample_y(y)) for each of the (up to) 2 x 2 neighbours, so the samples touched by all pixels of the
    rectangle are the product of the per-column and the per-row sets; their bounding box is the product of the ranges."""
    x, y, w, h = region
    out = []
    for p in range(L.nplanes):
        direct = L.nplanes == 1 or (L.factor_x[p] == L.scale_x and L.factor_y[p] == L.scale_y)
        sx = _samples(np.arange(x, x + w), L.factor_x[p], L.scale_x, L.units_x[p], direct, cosited)
        sy = _samples(np.arange(y, y + h), L.factor_y[p], L.scale_y, L.units_y[p], direct, cosited)
        assert sx.min() >= 0 and sx.max() < 8 * L.units_x[p] and sy.min() >= 0 and sy.max() < 8 * L.units_y[p]
        bx0, bx1, by0, by1 = sx.min() // 8, sx.max() // 8, sy.min() // 8, sy.max() // 8
        out.append((int(bx0), int(by0), int(bx1 - bx0 + 1), int(by1 - by0 + 1)))
    return out + [(0, 0, 0, 0)] * (_lib.MAX_PLANES - L.nplanes)


def _regions(rng, W, H, k):
    """Corners (1 x 1), the whole image, the right / bottom edge strips, a few odd ones, and k random regions."""
    out = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, W, H),
           (W - 1, 0, 1, H), (0, H - 1, W, 1), (W // 2, H // 2, W - W // 2, H - H // 2)]
    for _ in range(k):
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        out.append((x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))))
    return out


def _check_all(L, rng, k):
    for cosited in (0, 1):
        for region in _regions(rng, L.width, L.height, k):
            st, got = _window(L, cosited, region)
            assert st == 0, (region, cosited)
            assert got == _brute(L, cosited, region), (region, cosited, L.width, L.height)


def _frame_layout(path):
    data = np.fromfile(path, np.uint8)
    info = _lib.FrameInfo()
    assert _lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) == 0
    L = _lib.Layout()
    L.width, L.height, L.precision = info.width, info.height, info.precision
    L.nplanes = info.ncomponents
    L.scale_x, L.scale_y = info.scale_x, info.scale_y
    for c in range(info.ncomponents):
        L.factor_x[c], L.factor_y[c] = info.factor_x[c], info.factor_y[c]
        L.units_x[c], L.units_y[c] = info.units_x[c], info.units_y[c]
    return L


@pytest.mark.parametrize("path", DECODE, ids=[os.path.basename(p) for p in DECODE])
def test_window_of_every_decode_fixture(path):
    L = _frame_layout(path)
    if L.precision != 8:
        pytest.skip("not an 8-bit frame")
    _check_all(L, np.random.default_rng(len(path)), 40)


def test_window_of_random_layouts():
    rng = np.random.default_rng(20240807)
    for it in range(2000):
        n = 1 if rng.random() < 0.3 else 3
        factors = [(int(rng.integers(1, 5)), int(rng.integers(1, 5))) for _ in range(n)]
        scale = None
        if n == 3 and rng.random() < 0.2:   # a component the format does not recognise sets the scale
            scale = (max(max(f[0] for f in factors), int(rng.integers(1, 5))),
                     max(max(f[1] for f in factors), int(rng.integers(1, 5))))
        W, H = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        L = c_layout(W, H, factors, scale)
        _check_all(L, rng, 3)


def test_window_at_edges_of_sizes_off_the_mcu_grid():
    rng = np.random.default_rng(7)
    for W, H in ((17, 33), (31, 15), (47, 1), (1, 47), (161, 97)):
        for factors in ([(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(1, 1)] * 3,
                        [(4, 2), (1, 1), (2, 1)], [(1, 1)]):
            L = c_layout(W, H, factors)
            for cosited in (0, 1):
                for x in range(max(0, W - 18), W):
                    for y in (0, H - 1, max(0, H - 9)):
                        region = (x, y, W - x, H - y)
                        assert _window(L, cosited, region) == (0, _brute(L, cosited, region))
            _check_all(L, rng, 10)


def test_window_of_a_420_region_holds_the_chroma_halo():
    L = c_layout(1920, 1080, [(2, 2), (1, 1), (1, 1)])
    st, w = _window(L, 0, (1237 % 1920, 901 % 1080, 64, 64))
    assert st == 0
    # luma: the blocks under the pixels; chroma: one sample beyond on each side of 32 x 32 samples
    assert w[0] == (1237 // 8, 901 // 8, (1237 + 63) // 8 - 1237 // 8 + 1, (901 + 63) // 8 - 901 // 8 + 1)
    assert w[1] == w[2] == _brute(L, 0, (1237, 901, 64, 64))[1]


def _planes_cover_image(L):
    """The rule Planar.interleaved puts on the planes (decode.swift:4190-4246), restated: a direct plane is copied up to the
    image size; any other plane is read at the last pixel's sample, whose cosited index factor (size - 1) / scale is the
    larger of the two maps' (the neighbour is clamped to the plane, the sample itself is not)."""
    for p in range(L.nplanes):
        fx, fy, ux, uy = L.factor_x[p], L.factor_y[p], L.units_x[p], L.units_y[p]
        if L.nplanes == 1 or (fx == L.scale_x and fy == L.scale_y):
            ok = 8 * ux >= L.width and 8 * uy >= L.height
        else:
            ok = ux >= 1 and uy >= 1 and fx * (L.width - 1) // L.scale_x < 8 * ux and fy * (L.height - 1) // L.scale_y < 8 * uy
        if not ok:
            return False
    return True


def _check_cover(L):
    """Every plane's units as computed, one fewer and one more, per axis: accept / reject as the rule says."""
    lib, r, w = _lib.lib(), _lib.Region(0, 0, 1, 1), (_lib.Region * _lib.MAX_PLANES)()
    accepted = 0
    for p in range(L.nplanes):
        ux, uy = L.units_x[p], L.units_y[p]
        try:
            for dx in (-1, 0, 1):
                for dy in (-1, 0, 1):
                    L.units_x[p], L.units_y[p] = ux + dx, uy + dy
                    want = 0 if _planes_cover_image(L) else _lib.EINVAL
                    for cosited in (0, 1):
                        st = lib.jpeg_amd_region_window(C.byref(L), cosited, C.byref(r), w)
                        assert st == want, (L.width, L.height, p, dx, dy, cosited, list(L.factor_x), list(L.factor_y),
                                            L.scale_x, L.scale_y)
                    accepted += want == 0
        finally:
            L.units_x[p], L.units_y[p] = ux, uy
    return accepted


def test_planes_must_cover_the_image():
    rng = np.random.default_rng(4190)
    accepted = total = 0
    layouts = []
    for it in range(600):                     # the layouts of test_window_of_random_layouts
        n = 1 if rng.random() < 0.3 else 3
        factors = [(int(rng.integers(1, 5)), int(rng.integers(1, 5))) for _ in range(n)]
        scale = None
        if n == 3 and rng.random() < 0.2:
            scale = (max(max(f[0] for f in factors), int(rng.integers(1, 5))),
                     max(max(f[1] for f in factors), int(rng.integers(1, 5))))
        layouts.append(c_layout(int(rng.integers(1, 301)), int(rng.integers(1, 301)), factors, scale))
    for W, H in ((17, 33), (31, 15), (47, 1), (1, 47), (161, 97), (8, 8), (16, 16), (9, 9)):   # ... and of the edge test
        for factors in ([(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(1, 1)] * 3,
                        [(4, 2), (1, 1), (2, 1)], [(1, 1)]):
            layouts.append(c_layout(W, H, factors))
    for L in layouts:
        accepted += _check_cover(L)
        total += 9 * L.nplanes
    assert 0 < accepted < total               # the sweep sees both answers


def test_python_wrapper():
    layout = J.Layout("ycc8", {1: ((2, 2), 0), 2: ((1, 1), 1), 3: ((1, 1), 1)})
    got = J.region_window((100, 60), layout, (17, 9, 30, 20))
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    assert got == _brute(L, 0, (17, 9, 30, 20))[:3]
    assert J.region_window((100, 60), layout, (17, 9, 30, 20), cosite=True) == _brute(L, 1, (17, 9, 30, 20))[:3]
    with pytest.raises(J.JpegAmdError):
        J.region_window((100, 60), layout, (90, 0, 11, 1))


@pytest.mark.parametrize("region", [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (0, 0, -3, 4),
                                    (97, 0, 4, 4), (0, 57, 4, 4), (0, 0, 101, 60), (0, 0, 100, 61),
                                    (5, 0, 2 ** 31 - 1, 4), (0, 5, 4, 2 ** 31 - 1), (2 ** 31 - 1, 0, 1, 1)])
def test_window_rejects_regions_outside_the_image(region):
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    for cosited in (0, 1):
        assert _window(L, cosited, region)[0] == _lib.EINVAL


def test_window_rejects_null_arguments():
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    r = _lib.Region(0, 0, 1, 1)
    w = (_lib.Region * _lib.MAX_PLANES)()
    lib = _lib.lib()
    assert lib.jpeg_amd_region_window(C.byref(L), 0, None, w) == _lib.EINVAL
    assert lib.jpeg_amd_region_window(C.byref(L), 0, C.byref(r), None) == _lib.EINVAL
    assert lib.jpeg_amd_region_window(None, 0, C.byref(r), w) == _lib.EINVAL


def test_region_entry_points_check_their_arguments_before_the_device():
    """A NULL context is EINVAL before anything else (the device entry points need one; here there is no GPU)."""
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    r = _lib.Region(0, 0, 1, 1)
    lib = _lib.lib()
    assert lib.jpeg_amd_decode_region(None, C.byref(L), None, None, 2, 0, 1, C.byref(r), None) == _lib.EINVAL
    assert lib.jpeg_amd_decode_region_batch(None, C.byref(L), 1, None, None, None, 0, 2, 0, 1, C.byref(r), None, 0) == \
        _lib.EINVAL
