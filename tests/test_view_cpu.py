"""The host half of view decode -- no GPU: jpeg_amd_view_window (which blocks of each scaled plane the pixels of a view
read) against a brute-force restatement of the interleave index formula with N in the place of 8, jpeg_amd_view_of_source
and jpeg_amd_view_denom against their definitions, and the argument checks of the entry points, which come before the
device is touched."""
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
DENOMS = (1, 2, 4, 8)


def _ceil(a, b):
    return -(-a // b)


def _scaled_size(W, H, denom):
    N = 8 // denom
    return _ceil(W * N, 8), _ceil(H * N, 8)


def _window(L, cosited, denom, region):
    r = _lib.Region(*region)
    w = (_lib.Region * _lib.MAX_PLANES)()
    st = _lib.lib().jpeg_amd_view_window(C.byref(L), cosited, denom, C.byref(r), w)
    return st, [(w[p].x, w[p].y, w[p].width, w[p].height) for p in range(_lib.MAX_PLANES)]


def _region_window(L, cosited, region):
    r = _lib.Region(*region)
    w = (_lib.Region * _lib.MAX_PLANES)()
    st = _lib.lib().jpeg_amd_region_window(C.byref(L), cosited, C.byref(r), w)
    return st, [(w[p].x, w[p].y, w[p].width, w[p].height) for p in range(_lib.MAX_PLANES)]


def _samples(t, f, s, units, direct, cosited, N):
    """Every sample index pixels t read along one axis: the interleave formula, C truncation, j = min(i + 1, N units - 1)."""
    if direct:
        return t
    a, b, c = (0, f, s) if cosited else (f - s, 2 * f, 2 * s)
    n = a + b * t.astype(np.int64)
    i = np.sign(n) * (np.abs(n) // c)                  # truncation toward zero, like C's / and quotientAndRemainder
    j = np.minimum(i + 1, N * units - 1)
    return np.concatenate([i, j])


def _brute(L, cosited, denom, region):
    """Bounding box, in blocks of N x N samples, of the samples every pixel of `region` reads: the samples touched by all
    pixels of the rectangle are the product of the per-column and the per-row sets."""
    N = 8 // denom
    x, y, w, h = region
    out = []
    for p in range(L.nplanes):
        direct = L.nplanes == 1 or (L.factor_x[p] == L.scale_x and L.factor_y[p] == L.scale_y)
        sx = _samples(np.arange(x, x + w), L.factor_x[p], L.scale_x, L.units_x[p], direct, cosited, N)
        sy = _samples(np.arange(y, y + h), L.factor_y[p], L.scale_y, L.units_y[p], direct, cosited, N)
        assert sx.min() >= 0 and sx.max() < N * L.units_x[p] and sy.min() >= 0 and sy.max() < N * L.units_y[p]
        bx0, bx1, by0, by1 = sx.min() // N, sx.max() // N, sy.min() // N, sy.max() // N
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
    for denom in DENOMS:
        W, H = _scaled_size(L.width, L.height, denom)
        for cosited in (0, 1):
            for region in _regions(rng, W, H, k):
                st, got = _window(L, cosited, denom, region)
                assert st == 0, (region, cosited, denom)
                assert got == _brute(L, cosited, denom, region), (region, cosited, denom, L.width, L.height)
                if denom == 1:
                    assert (st, got) == _region_window(L, cosited, region)


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
    _check_all(_frame_layout(path), np.random.default_rng(len(path)), 20)


def test_window_of_random_layouts():
    rng = np.random.default_rng(20240809)
    for it in range(2000):
        n = 1 if rng.random() < 0.3 else 3
        factors = [(int(rng.integers(1, 5)), int(rng.integers(1, 5))) for _ in range(n)]
        scale = None
        if n == 3 and rng.random() < 0.2:   # a component the format does not recognise sets the scale
            scale = (max(max(f[0] for f in factors), int(rng.integers(1, 5))),
                     max(max(f[1] for f in factors), int(rng.integers(1, 5))))
        W, H = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        _check_all(c_layout(W, H, factors, scale), rng, 2)


def test_window_at_edges_of_sizes_off_the_mcu_grid():
    """Rectangles that end on the last column and row of (W', H'), where the neighbour clamps at N units - 1."""
    rng = np.random.default_rng(7)
    for W, H in ((17, 33), (31, 15), (47, 1), (1, 47), (161, 97)):
        for factors in ([(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 2), (1, 1), (1, 1)], [(1, 1)] * 3,
                        [(4, 2), (1, 1), (2, 1)], [(1, 1)]):
            L = c_layout(W, H, factors)
            for denom in DENOMS:
                W1, H1 = _scaled_size(W, H, denom)
                for cosited in (0, 1):
                    for x in range(max(0, W1 - 18), W1):
                        for y in (0, H1 - 1, max(0, H1 - 9)):
                            region = (x, y, W1 - x, H1 - y)
                            assert _window(L, cosited, denom, region) == (0, _brute(L, cosited, denom, region))
            _check_all(L, rng, 6)


def test_window_of_a_420_view_holds_the_chroma_halo():
    L = c_layout(1920, 1080, [(2, 2), (1, 1), (1, 1)])
    st, w = _window(L, 0, 4, (237, 101, 64, 64))          # N = 2: blocks of 2 x 2 samples
    assert st == 0
    assert w[0] == (237 // 2, 101 // 2, (237 + 63) // 2 - 237 // 2 + 1, (101 + 63) // 2 - 101 // 2 + 1)
    # chroma: samples (2 x - 1) / 4 = 118 .. 149 and the neighbour 150 across, 50 .. 81 and 82 down
    assert w[1] == w[2] == (59, 25, 17, 17) == _brute(L, 0, 4, (237, 101, 64, 64))[1]


def test_view_of_source_sizes_1_to_70():
    """Scaled pixel x' stands for the source pixels [8 x' / N, 8 (x' + 1) / N): the result holds exactly the scaled pixels
    whose footprint meets the source rectangle -- so it covers, and it is minimal -- clipped to (W', H')."""
    lib = _lib.lib()
    out = _lib.Region()
    for denom in DENOMS:
        N = 8 // denom
        for size in range(1, 71):
            L = c_layout(size, 71 - size, [(1, 1)])
            W1, H1 = _scaled_size(size, 71 - size, denom)
            ys, hs = (71 - size) // 3, max(1, (71 - size) // 2)
            hs = min(hs, 71 - size - ys)
            for x in range(size):
                for w in range(1, size - x + 1):
                    src = _lib.Region(x, ys, w, hs)
                    assert lib.jpeg_amd_view_of_source(C.byref(L), denom, C.byref(src), C.byref(out)) == 0
                    for lo, n, full, got0, got_n in ((x, w, W1, out.x, out.width), (ys, hs, H1, out.y, out.height)):
                        # footprints as integers: 8 t <= N s < 8 (t + 1) for a source pixel s of scaled pixel t
                        meets = [t for t in range(full) if 8 * t < N * (lo + n) and 8 * (t + 1) > N * lo]
                        assert meets and (got0, got_n) == (meets[0], len(meets)), (denom, size, x, w)
                        assert meets == list(range(meets[0], meets[-1] + 1)) and got0 + got_n <= full
    assert J.view_of_source((70, 40), 4, (9, 3, 17, 30)) == (2, 0, 5, 9)


@pytest.mark.parametrize("src", [(-1, 0, 4, 4), (0, -1, 4, 4), (0, 0, 0, 4), (0, 0, 4, 0), (97, 0, 4, 4), (0, 57, 4, 4),
                                 (0, 0, 101, 60), (5, 0, 2 ** 31 - 1, 4), (2 ** 31 - 1, 0, 1, 1)])
def test_view_of_source_rejects_rectangles_outside_the_image(src):
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    out = _lib.Region()
    r = _lib.Region(*src)
    for denom in DENOMS:
        assert _lib.lib().jpeg_amd_view_of_source(C.byref(L), denom, C.byref(r), C.byref(out)) == _lib.EINVAL


def _denom(src_w, src_h, want_w, want_h):
    for denom in (8, 4, 2):
        if src_w * (8 // denom) // 8 >= want_w and src_h * (8 // denom) // 8 >= want_h:
            return denom
    return 1


def test_view_denom_over_a_grid_of_sizes():
    lib = _lib.lib()
    sizes = list(range(0, 40)) + [63, 64, 65, 223, 224, 225, 447, 448, 449, 895, 896, 897, 1791, 1792, 1793, 4096, 65535]
    seen = set()
    for sw in sizes:
        for sh in (1, 9, 224, 448, 1080, 1793):
            for ww in (1, 2, 7, 8, 9, 56, 112, 224, 225):
                for wh in (1, 8, 224):
                    got = lib.jpeg_amd_view_denom(sw, sh, ww, wh)
                    assert got == _denom(sw, sh, ww, wh), (sw, sh, ww, wh)
                    seen.add(got)
    assert seen == {1, 2, 4, 8}
    assert J.view_denom((1792, 1792), (224, 224)) == 8 and J.view_denom((1791, 1792), (224, 224)) == 4
    assert J.view_denom((100, 100), (224, 224)) == 1


def test_python_wrapper():
    layout = J.Layout("ycc8", {1: ((2, 2), 0), 2: ((1, 1), 1), 3: ((1, 1), 1)})
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    for denom in DENOMS:
        W1, H1 = _scaled_size(100, 60, denom)
        region = (W1 // 3, H1 // 4, W1 - W1 // 3, H1 // 2)
        assert J.view_window((100, 60), layout, denom, region) == _brute(L, 0, denom, region)[:3]
        assert J.view_window((100, 60), layout, denom, region, cosite=True) == _brute(L, 1, denom, region)[:3]
    assert J.view_window((100, 60), layout, 1, (17, 9, 30, 20)) == J.region_window((100, 60), layout, (17, 9, 30, 20))
    with pytest.raises(J.JpegAmdError):
        J.view_window((100, 60), layout, 2, (45, 0, 6, 1))        # W' = 50


# (denom, region): outside the scaled image of a 100 x 60 source -- (50, 30), (25, 15), (13, 8)
OUTSIDE = [(2, (-1, 0, 4, 4)), (2, (0, -1, 4, 4)), (2, (0, 0, 0, 4)), (2, (0, 0, 4, 0)), (4, (0, 0, -3, 4)),
           (2, (47, 0, 4, 4)), (2, (0, 27, 4, 4)), (2, (0, 0, 51, 30)), (4, (0, 0, 25, 16)), (8, (13, 0, 1, 1)),
           (8, (0, 0, 14, 8)), (2, (0, 0, 100, 60)),              # fits the source size, not (W', H')
           (4, (5, 0, 2 ** 31 - 1, 4)), (8, (2 ** 31 - 1, 0, 1, 1)), (1, (97, 0, 4, 4))]


@pytest.mark.parametrize("denom,region", OUTSIDE)
def test_window_rejects_regions_outside_the_scaled_image(denom, region):
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    for cosited in (0, 1):
        assert _window(L, cosited, denom, region)[0] == _lib.EINVAL


@pytest.mark.parametrize("denom", [0, 3, 16, -1, -8])
def test_other_denoms_are_einval(denom):
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    lib = _lib.lib()
    r, out = _lib.Region(0, 0, 1, 1), _lib.Region()
    assert _window(L, 0, denom, (0, 0, 1, 1))[0] == _lib.EINVAL
    assert lib.jpeg_amd_view_of_source(C.byref(L), denom, C.byref(r), C.byref(out)) == _lib.EINVAL


def test_host_calls_reject_null_arguments():
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    r, out = _lib.Region(0, 0, 1, 1), _lib.Region()
    w = (_lib.Region * _lib.MAX_PLANES)()
    lib = _lib.lib()
    assert lib.jpeg_amd_view_window(C.byref(L), 0, 2, None, w) == _lib.EINVAL
    assert lib.jpeg_amd_view_window(C.byref(L), 0, 2, C.byref(r), None) == _lib.EINVAL
    assert lib.jpeg_amd_view_window(None, 0, 2, C.byref(r), w) == _lib.EINVAL
    assert lib.jpeg_amd_view_of_source(None, 2, C.byref(r), C.byref(out)) == _lib.EINVAL
    assert lib.jpeg_amd_view_of_source(C.byref(L), 2, None, C.byref(out)) == _lib.EINVAL
    assert lib.jpeg_amd_view_of_source(C.byref(L), 2, C.byref(r), None) == _lib.EINVAL


def _decode_view(ctx, L, view, coef=None, quanta=None, pixels=None):
    return _lib.lib().jpeg_amd_decode_view(ctx, C.byref(L) if L is not None else None, coef, quanta, 2, 0, _lib.COLOR_RGB8,
                                           C.byref(view) if view is not None else None, pixels)


def _decode_view_batch(ctx, L, n, views, coef=None, strides=None, quanta=None, pixels=None, stride=0):
    return _lib.lib().jpeg_amd_decode_view_batch(ctx, C.byref(L) if L is not None else None, n, coef, strides, quanta, 128, 2, 0,
                                                 _lib.COLOR_RGB8, views, pixels, stride)


def test_view_entry_points_check_their_arguments_before_the_device():
    """There is no GPU here and the context is NULL: a status other than EINVAL shows that the arguments are judged before
    the context is looked at, and a valid call with a NULL context is EINVAL."""
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    L12 = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)], precision=12)
    ok = _lib.View(2, _lib.Region(0, 0, 1, 1))
    assert _decode_view(None, L12, ok) == _lib.ENOSUP
    assert _decode_view_batch(None, L12, 1, C.byref(ok)) == _lib.ENOSUP
    assert _decode_view_batch(None, L12, 0, None) == _lib.ENOSUP
    # ... and every refusal is a refusal with a NULL context as well
    assert _decode_view(None, L, ok) == _lib.EINVAL
    assert _decode_view(None, L, None) == _lib.EINVAL
    assert _decode_view(None, None, ok) == _lib.EINVAL
    assert _decode_view_batch(None, L, 1, C.byref(ok)) == _lib.EINVAL
    assert _decode_view_batch(None, L, 0, None) == _lib.EINVAL
    assert _decode_view_batch(None, None, 1, C.byref(ok)) == _lib.EINVAL
    assert _decode_view_batch(None, L, -1, C.byref(ok)) == _lib.EINVAL
    assert _decode_view_batch(None, L, 65536, C.byref(ok)) == _lib.EINVAL
    for denom in (0, 3, 16, -1):
        bad = _lib.View(denom, _lib.Region(0, 0, 1, 1))
        assert _decode_view(None, L, bad) == _lib.EINVAL
        assert _decode_view_batch(None, L, 1, C.byref(bad)) == _lib.EINVAL
    for denom, region in OUTSIDE:
        bad = _lib.View(denom, _lib.Region(*region))
        assert _decode_view(None, L, bad) == _lib.EINVAL
        assert _decode_view_batch(None, L, 1, C.byref(bad)) == _lib.EINVAL


def test_batch_checks_every_view_and_the_stride_before_the_device():
    """Host pointers stand in for the device's: with a NULL context a call is refused before anything could read them."""
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    n = 5
    views = (_lib.View * n)(*[_lib.View(d, _lib.Region(1, 2, 5, 3)) for d in (1, 2, 8, 4, 2)])
    buf = np.zeros(64, np.int16)
    coef = _lib.ptr_array([buf.ctypes.data] * 3)
    strides = _lib.size_array([0, 0, 0, 0])

    def call(stride=45):
        return _decode_view_batch(None, L, n, views, coef, strides, buf.ctypes.data, buf.ctypes.data, stride)

    assert call() == _lib.EINVAL                           # the NULL context, after everything else passed
    views[2].denom = 3                                     # a bad denominator in the middle of the batch
    assert call() == _lib.EINVAL
    views[2].denom = 8
    views[3].region.x = 25 - 5 + 1                         # one pixel past W' = 25
    assert call() == _lib.EINVAL
    views[3].region.x = 1
    assert call(stride=44) == _lib.EINVAL                  # smaller than 3 * 5 * 3
