"""The host half of scaled decode -- no GPU: jpeg_amd_scaled_layout against the contract's formulas (include/jpeg_amd.h,
"scaled decode"), the bound that keeps every pixel's sample index inside the scaled plane, the argument checks, and the
test-side reference (_scaled_ref) against the float64 textbook form of the reduced transform."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _scaled_ref as S
import jpeg_amd as J
from _calls import c_layout
from _golden import GOLDEN
from jpeg_amd import _lib

DECODE = sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg")))
DENOMS = (1, 2, 4, 8)


def _scaled(L, denom):
    out = _lib.Layout()
    return _lib.lib().jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(out)), out


def _ceil(a, b):
    return -(-a // b)


_INDEX_CACHE = {}


def _max_index(size, f, s, cosited):
    """The largest sample index any pixel t < size reads before the neighbour clamp: i = (a + b t) / c, truncating."""
    key = (size, f, s, cosited)
    if key not in _INDEX_CACHE:
        a, b, c = (0, f, s) if cosited else (f - s, 2 * f, 2 * s)
        n = a + b * np.arange(size, dtype=np.int64)
        _INDEX_CACHE[key] = int((np.sign(n) * (np.abs(n) // c)).max())
    return _INDEX_CACHE[key]


def _check(L):
    for denom in DENOMS:
        N = 8 // denom
        st, out = _scaled(L, denom)
        assert st == 0
        assert (out.width, out.height) == (_ceil(L.width * N, 8), _ceil(L.height * N, 8)) == S.scaled_size((L.width, L.height), denom)
        assert (out.precision, out.nplanes, out.scale_x, out.scale_y) == (L.precision, L.nplanes, L.scale_x, L.scale_y)
        for p in range(_lib.MAX_PLANES):
            assert (out.factor_x[p], out.factor_y[p], out.qi[p]) == (L.factor_x[p], L.factor_y[p], L.qi[p])
            if p >= L.nplanes:
                continue
            assert out.units_x[p] == _ceil(N * L.units_x[p], 8) and out.units_y[p] == _ceil(N * L.units_y[p], 8)
            # every pixel of the scaled image indexes inside the N units samples of the scaled plane
            direct = L.nplanes == 1 or (L.factor_x[p] == L.scale_x and L.factor_y[p] == L.scale_y)
            for size, f, s, units in ((out.width, L.factor_x[p], L.scale_x, L.units_x[p]),
                                      (out.height, L.factor_y[p], L.scale_y, L.units_y[p])):
                if direct:
                    assert size - 1 <= N * units - 1
                else:
                    for cosited in (False, True):
                        assert 0 <= _max_index(size, f, s, cosited) <= N * units - 1, (size, f, s, units, N, cosited)


def _fixture_layouts():
    """The distinct (factors, scale) of the decode fixtures."""
    seen = {}
    for path in DECODE:
        data = np.fromfile(path, np.uint8)
        info = _lib.FrameInfo()
        if _lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) != 0:
            continue
        n = min(info.ncomponents, 3)
        factors = tuple((info.factor_x[c], info.factor_y[c]) for c in range(n))
        seen[(factors, (info.scale_x, info.scale_y))] = True
    return sorted(seen)


def test_scaled_layout_of_every_fixture_layout_at_sizes_1_to_70():
    layouts = _fixture_layouts()
    assert layouts
    for factors, scale in layouts:
        for W in range(1, 71):
            for H in range(1, 71):
                _check(c_layout(W, H, list(factors), scale))


def test_scaled_layout_of_random_layouts():
    rng = np.random.default_rng(20240807)
    for it in range(2000):
        n = 1 if rng.random() < 0.3 else 3
        factors = [(int(rng.integers(1, 5)), int(rng.integers(1, 5))) for _ in range(n)]
        scale = None
        if n == 3 and rng.random() < 0.2:   # a component the format does not recognise sets the scale
            scale = (max(max(f[0] for f in factors), int(rng.integers(1, 5))),
                     max(max(f[1] for f in factors), int(rng.integers(1, 5))))
        _check(c_layout(int(rng.integers(1, 5000)), int(rng.integers(1, 5000)), factors, scale))


def test_denom_1_is_the_same_layout():
    L = c_layout(319, 480, [(2, 2), (1, 1), (1, 1)])
    st, out = _scaled(L, 1)
    assert st == 0 and bytes(out) == bytes(L)


@pytest.mark.parametrize("denom", [0, 3, 16, -1])
def test_other_denoms_are_einval(denom):
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    lib = _lib.lib()
    assert _scaled(L, denom)[0] == _lib.EINVAL
    with pytest.raises(ValueError):
        J.scaled_size((100, 60), denom)
    # the device entry points: a NULL context is EINVAL before anything else (here there is no GPU)
    assert lib.jpeg_amd_decode_scaled(None, C.byref(L), None, None, 2, 0, 1, denom, None) == _lib.EINVAL
    assert lib.jpeg_amd_decode_scaled_batch(None, C.byref(L), 1, None, None, None, 0, 2, 0, 1, denom, None, 0) == _lib.EINVAL
    assert lib.jpeg_amd_spectral_idct_scaled(None, C.byref(L), None, None, 2, denom, None) == _lib.EINVAL


def test_scaled_layout_rejects_null_and_bad_layouts():
    L = c_layout(100, 60, [(2, 2), (1, 1), (1, 1)])
    out = _lib.Layout()
    lib = _lib.lib()
    assert lib.jpeg_amd_scaled_layout(None, 2, C.byref(out)) == _lib.EINVAL
    assert lib.jpeg_amd_scaled_layout(C.byref(L), 2, None) == _lib.EINVAL
    L.width = 0
    assert lib.jpeg_amd_scaled_layout(C.byref(L), 2, C.byref(out)) == _lib.EINVAL


def test_python_scaled_size():
    for size in ((1, 1), (7, 9), (319, 480), (1920, 1080)):
        for denom in DENOMS:
            st, out = _scaled(c_layout(size[0], size[1], [(1, 1)]), denom)
            assert st == 0 and J.scaled_size(size, denom) == (out.width, out.height)


@pytest.mark.parametrize("N", [4, 2, 1])
def test_reference_planes_are_within_one_level_of_the_textbook_transform(N):
    """(N / 8) x the orthonormal N-point 2-D IDCT in float64, plus level, clamped, truncated.  The butterflies' float error
    is orders of magnitude below 1, so a sample can differ from the textbook one only where the value lies at an integer
    boundary, and then by one level.  The share of samples that differ at all is printed, not gated."""
    rng = np.random.default_rng(8 + N)
    uy, ux = 48, 64
    q = rng.integers(1, 256, 64).astype(np.uint16)
    bound = (4096 // q.astype(np.int64))                # |c Q| <= 4096
    coef = (rng.integers(-(1 << 20), 1 << 20, (uy, ux, 64)) % (2 * bound + 1) - bound).astype(np.int16)
    coef[uy // 2:] //= 64                               # half of the blocks at amplitudes that stay off the clamp
    assert (np.abs(coef.astype(np.int64) * q) <= 4096).all()
    coef[0, 0] = bound.astype(np.int16)                 # the extremes, both signs
    coef[0, 1] = -bound.astype(np.int16)
    got = S.idct_plane_scaled(coef, q, N).astype(np.int64)
    want, _ = S.textbook_plane(coef, q, N)
    diff = np.abs(got - want.astype(np.int64))
    print("N = %d: %.4f %% of %d samples differ from the float64 textbook transform, by at most %d level"
          % (N, 100.0 * (diff != 0).mean(), diff.size, diff.max()))
    assert diff.max() <= 1
