"""The host half of spectral reduce -- no GPU: jpeg_amd_reduce_layout against the contract's formula (include/jpeg_amd.h,
"spectral reduce"), and the properties of the test-side reference (_reduce_ref) that pin the contract."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _reduce_ref as R
import _scaled_ref as S
from _calls import c_layout, plane_factors, plane_units
from _golden import GOLDEN
from jpeg_amd import _lib
from oracle import oracle as O

DECODE = sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg")))
DENOMS = (2, 4, 8)


def _reduced(L, denom):
    out = _lib.Layout()
    return _lib.lib().jpeg_amd_reduce_layout(C.byref(L), denom, C.byref(out)), out


def _scaled(L, denom):
    out = _lib.Layout()
    assert _lib.lib().jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(out)) == 0
    return out


def _check(L):
    factors = plane_factors(L)
    for denom in DENOMS:
        st, out = _reduced(L, denom)
        assert st == 0
        size, units = R.reduce_geometry((L.width, L.height), factors, (L.scale_x, L.scale_y), denom)
        assert (out.width, out.height) == size == S.scaled_size((L.width, L.height), denom)
        assert (out.precision, out.nplanes, out.scale_x, out.scale_y) == (L.precision, L.nplanes, L.scale_x, L.scale_y)
        for p in range(_lib.MAX_PLANES):
            assert (out.factor_x[p], out.factor_y[p], out.qi[p]) == (L.factor_x[p], L.factor_y[p], L.qi[p])
        assert plane_units(out) == units
        # what a reader of the output file derives from its header
        again = c_layout(out.width, out.height, factors, (L.scale_x, L.scale_y), L.precision)
        assert plane_units(again) == units
        # against jpeg_amd_scaled_layout: equal where every factor divides the scale, never smaller, at most one larger
        sc = _scaled(L, denom)
        for p in range(L.nplanes):
            for u, su, f, s in ((out.units_x[p], sc.units_x[p], L.factor_x[p], L.scale_x),
                                (out.units_y[p], sc.units_y[p], L.factor_y[p], L.scale_y)):
                assert su <= u <= su + 1
                if s % f == 0:
                    assert u == su


def _fixture_layouts():
    """The distinct (factors, scale, precision) of the decode fixtures."""
    seen = {}
    for path in DECODE:
        data = np.fromfile(path, np.uint8)
        info = _lib.FrameInfo()
        if _lib.lib().jpeg_amd_jpeg_inspect(data.ctypes.data, data.size, C.byref(info)) != 0:
            continue
        n = min(info.ncomponents, _lib.MAX_PLANES)
        factors = tuple((info.factor_x[c], info.factor_y[c]) for c in range(n))
        seen[(factors, (info.scale_x, info.scale_y), info.precision)] = True
    return sorted(seen)


def test_reduce_layout_of_every_fixture_layout():
    layouts = _fixture_layouts()
    assert len(layouts) >= 3
    for factors, scale, precision in layouts:
        for w, h in ((1, 1), (7, 9), (8, 16), (17, 33), (131, 257), (1920, 1080)):
            _check(c_layout(w, h, list(factors), scale, precision))


def test_reduce_layout_of_2000_random_sizes_and_layouts():
    rng = np.random.Generator(np.random.PCG64(11))
    for _ in range(2000):
        n = int(rng.integers(1, 5))
        sx, sy = int(rng.integers(1, 5)), int(rng.integers(1, 5))
        factors = [(int(rng.integers(1, sx + 1)), int(rng.integers(1, sy + 1))) for _ in range(n)]
        factors[0] = (sx, sy)
        w, h = int(rng.integers(1, 700)), int(rng.integers(1, 700))
        _check(c_layout(w, h, factors, (sx, sy), int(rng.integers(1, 17))))


@pytest.mark.parametrize("width", [21, 41, 85])
def test_a_factor_that_does_not_divide_the_scale_can_take_one_more_unit(width):
    """3 in 4: the units recomputed from (W', H') exceed jpeg_amd_scaled_layout's ceil(N units / 8) at some denominator."""
    L = c_layout(width, 16, [(4, 1), (3, 1), (1, 1)])
    _check(L)
    larger = []
    for denom in DENOMS:
        st, out = _reduced(L, denom)
        assert st == 0
        if out.units_x[1] > _scaled(L, denom).units_x[1]:
            larger.append(denom)
    assert larger, width
    if width == 21:                                      # the contract's own example: N = 4 gives 2 against 1
        st, out = _reduced(L, 2)
        assert (out.units_x[1], _scaled(L, 2).units_x[1]) == (2, 1)


def test_reduce_layout_refuses_other_denominators_and_bad_layouts():
    L = c_layout(33, 17, [(2, 2), (1, 1), (1, 1)])
    for denom in (1, 3, 16, 0, -2):
        out = _lib.Layout()
        out.width = 12345
        assert _lib.lib().jpeg_amd_reduce_layout(C.byref(L), denom, C.byref(out)) == _lib.EINVAL
        assert out.width == 12345
    assert _lib.lib().jpeg_amd_reduce_layout(C.byref(L), 2, None) == _lib.EINVAL
    assert _lib.lib().jpeg_amd_reduce_layout(None, 2, C.byref(_lib.Layout())) == _lib.EINVAL
    bad = c_layout(33, 17, [(2, 2), (1, 1), (1, 1)])
    bad.precision = 17
    assert _reduced(bad, 2)[0] == _lib.EINVAL


# ---- properties of the reference that pin the contract ------------------------------------------------------------------

LUMA_HALF = O.compression_quanta("luminance", 0.5)


@pytest.mark.parametrize("denom", DENOMS)
def test_a_flat_plane_stays_flat(denom):
    """Every block DC = 13, AC = 0, luminance table at level 0.5 (samples 143 throughout), Q_out = Q_in: DC = 13 and AC = 0
    in every output block."""
    coef = np.zeros((5, 7, 64), np.int16)
    coef[..., 0] = 13
    assert (S.idct_plane_scaled(coef, LUMA_HALF, 8 // denom) == 143).all()
    for units in ((1, 1), (2, 1), (7, 5)):
        out = R.reduce_plane(coef, LUMA_HALF, denom, units)
        assert out.shape == (units[1], units[0], 64)
        assert (out[..., 0] == 13).all() and (out[..., 1:] == 0).all()


@pytest.mark.parametrize("denom", DENOMS)
def test_with_unit_output_tables_the_result_decodes_to_the_replicated_samples_within_one_level(denom):
    """Q_out all ones: oracle.idct_plane of the result against the replicated scaled samples.  Bound 1 (one level: the
    forward transform's quotient is rounded to an integer, the inverse truncates).  Measured maximum: 1 at N = 4, 2 and 1."""
    from jpeg_amd.synth import blocks_natural
    uy, ux = 9, 11
    coef = blocks_natural(uy * ux, seed=denom).reshape(uy, ux, 64)
    N = 8 // denom
    units = (-(-N * ux // 8) + 1, -(-N * uy // 8))           # one replicated block column more
    ones = np.ones(64, np.uint16)
    want = R.reduced_samples(coef, LUMA_HALF, denom, units)
    got = O.idct_plane(R.reduce_plane(coef, LUMA_HALF, denom, units, ones), ones)
    err = int(np.abs(got.astype(np.int64) - want.astype(np.int64)).max())
    print("denom", denom, "max |error|", err)
    assert err <= 1


@pytest.mark.parametrize("denom", DENOMS)
def test_coefficients_outside_the_head_do_not_change_the_result(denom):
    from jpeg_amd.synth import blocks_natural
    N = 8 // denom
    coef = blocks_natural(6 * 5, seed=3).reshape(6, 5, 64)
    head = sorted(int(S.Z[h][k]) for h in range(N) for k in range(N))
    noisy = np.full_like(coef, 32767)
    noisy[1::2] = -32767
    noisy[..., head] = coef[..., head]
    zeroed = np.zeros_like(coef)
    zeroed[..., head] = coef[..., head]
    units = (-(-N * 5 // 8), -(-N * 6 // 8))
    a = R.reduce_plane(zeroed, LUMA_HALF, denom, units)
    assert (a == R.reduce_plane(noisy, LUMA_HALF, denom, units)).all()
    assert (a == R.reduce_plane(coef, LUMA_HALF, denom, units)).all()


def test_replication_repeats_the_last_sample():
    s = np.arange(12, dtype=np.uint16).reshape(3, 4)
    r = R.replicate(s, (1, 1))
    assert r.shape == (8, 8)
    assert (r[:3, :4] == s).all() and (r[:3, 4:] == s[:, 3:4]).all() and (r[3:, :] == r[2:3, :]).all()
