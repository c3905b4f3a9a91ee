"""The bicubic warp (include/jpeg_amd.h, "bicubic warp") without a GPU: the numpy mirror of the contract (_project_cubic_ref)
against the contract's consequences, against a float64 evaluation of the same filter written out here, and against the
bicubic resize's mirror where the two filters meet; jpeg_amd_project_filter_view against its Python restatement and the wider
margin of its views; what the new calls refuse with a NULL context; and the Python keywords, through a recorder in the
library's place."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import _bicubic_ref as B
import _files as FI
import _orient as E
import _project_cubic_ref as Q
import _project_ref as P
import _warp_ref as W
import jpeg_amd as J
from _calls import FUSED, c_layout
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, -1, -5
F = np.float32
RGB = _lib.COLOR_RGB8
EDGES = (Q.FILL, Q.REPLICATE)
FILLB = (7, 130, 255)
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def image(w, h, seed, checker=False):
    if checker:                       # 0 / 255 in squares of 1 .. 3 pixels: the cubic overshoots, so the clamp is live
        s = 1 + seed % 3
        y, x = np.mgrid[0:h, 0:w]
        return np.repeat(((((x // s) + (y // s)) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- the mirror against the contract's consequences ---------------------------------------------------------------------------------

def test_the_identity_gives_the_source_bytes():
    for w, h in ((1, 1), (1, 7), (6, 1), (13, 9), (64, 33)):
        src = image(w, h, 10 * w + h)
        for edge in EDGES:
            assert np.array_equal(Q.project(src, IDENT, w, h, edge, FILLB), src), (w, h, edge)


def test_an_integer_translation_gives_the_shifted_bytes():
    w, h = 23, 17
    src = image(w, h, 3)
    for tx, ty in ((1, 0), (0, 1), (-3, 2), (5, -4), (-30, 0), (0, 25), (2, 2), (-2, -2)):
        m = [1, 0, tx, 0, 1, ty, 0, 0, 1]
        ys, xs = np.mgrid[0:h, 0:w]
        sy, sx = ys + ty, xs + tx
        inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
        clamped = src[np.clip(sy, 0, h - 1), np.clip(sx, 0, w - 1)]
        assert np.array_equal(Q.project(src, m, w, h, Q.REPLICATE, FILLB), clamped), (tx, ty)
        want = np.where(inside[..., None], clamped, np.asarray(FILLB, np.uint8))
        assert np.array_equal(Q.project(src, m, w, h, Q.FILL, FILLB), want), (tx, ty)


def test_the_four_quarter_turns_are_permutations_of_bytes():
    w, h = 19, 11
    src = image(w, h, 5)
    turns = [(IDENT, (w, h), src),
             ([0, 1, 0, -1, 0, h, 0, 0, 1], (h, w), src[::-1].transpose(1, 0, 2)),        # out[y][x] = src[h - 1 - x][y]
             ([-1, 0, w, 0, -1, h, 0, 0, 1], (w, h), src[::-1, ::-1]),
             ([0, -1, w, 1, 0, 0, 0, 0, 1], (h, w), src[:, ::-1].transpose(1, 0, 2))]     # out[y][x] = src[x][w - 1 - y]
    for m, out, want in turns:
        for edge in EDGES:
            assert np.array_equal(Q.project(src, m, out[0], out[1], edge, FILLB), want), (m, edge)


def test_far_outside_under_fill_is_the_fill_byte_for_all_256_fills():
    """A 23 x 19 canvas mapped well outside a 5 x 4 source.  A pixel has no tap inside only where the clamp binds on one axis
    (columns w .. w + 3, or rows h .. h + 3); the other axis then runs through fractions of every kind, whose weights sum to 1
    only up to a few ulp.  Also both axes bound, and the bound at -2, where the one tap that counts is column or row -2."""
    src = image(5, 4, 7)
    cases = [[0.37, 0.011, -2.1, 0.0, 0.01, 60.0], [0.0, 0.01, 60.0, 0.013, 0.29, -2.2], [1, 0, 1e6, 0, 1, 1e6],
             [0.37, 0.011, -2.1, 0.0, 0.01, -60.0], [0.0, 0.01, -60.0, 0.013, 0.29, -2.2]]
    for k, six in enumerate(cases):
        m = np.array(six + [0, 0, 1], F)
        sx, sy = Q.coordinates(m, 5, 4, 23, 19)
        free = (sx, sy, None, sx, sy)[k]
        assert free is None or len(np.unique(free - np.floor(free))) > 200
        assert ((sx == F(6.0)) | (sx == F(-2.0)) | (sy == F(5.0)) | (sy == F(-2.0))).all()
        for f in range(256):
            fill = (f, 255 - f, (f * 7) % 256)
            assert (Q.project(src, m, 23, 19, Q.FILL, fill) == np.asarray(fill, np.uint8)).all(), (k, f)


def test_a_coordinate_that_the_clamp_binds_has_the_weights_0_1_0_0():
    """What the kernels' early exit rests on: at sx == -2 or w + 1 the fraction is 0 and only the column x0 counts."""
    for f in (F(0.0), F(1.0)):
        w = Q.axis_weights(np.array([f], F))
        assert [float(v[0]) for v in w] == ([0.0, 1.0, 0.0, 0.0] if f == 0 else [0.0, 0.0, 1.0, 0.0])
    sx, _ = Q.coordinates([1, 0, -50, 0, 1, 0, 0, 0, 1], 8, 8, 4, 4)
    assert (sx == F(-2.0)).all()
    sx, _ = Q.coordinates([1, 0, 50, 0, 1, 0, 0, 0, 1], 8, 8, 4, 4)
    assert (sx == F(9.0)).all()


# ---- against a float64 evaluation of the same filter --------------------------------------------------------------------------------

def keys64(x):
    """The Keys cubic with a = -0.5 of a distance x >= 0, float64, in its textbook form."""
    a = -0.5
    return np.where(x <= 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, a * (((x - 5.0) * x + 8.0) * x - 4.0), 0.0))


def cubic64(src, m, out_w, out_h, edge, fill):
    """The filter in float64: 16 products per channel, the coordinate clamped as the contract clamps it -> int32 levels."""
    h, w = src.shape[:2]
    m = np.asarray(m, F).astype(np.float64).reshape(3, 3)
    xc, yc = np.meshgrid(np.arange(out_w) + 0.5, np.arange(out_h) + 0.5)
    den = m[2, 0] * xc + m[2, 1] * yc + m[2, 2]
    sx = np.clip((m[0, 0] * xc + m[0, 1] * yc + m[0, 2]) / den - 0.5, -2.0, w + 1.0)
    sy = np.clip((m[1, 0] * xc + m[1, 1] * yc + m[1, 2]) / den - 0.5, -2.0, h + 1.0)
    x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    img = src.astype(np.float64)
    acc = np.zeros((out_h, out_w, 3), np.float64)
    for j in range(-1, 3):
        for i in range(-1, 3):
            xi, yi = x0 + i, y0 + j
            t = img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)]
            if edge == Q.FILL:
                inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
                t = np.where(inside[..., None], t, np.asarray(fill, np.float64))
            acc += (keys64(np.abs(sx - xi)) * keys64(np.abs(sy - yi)))[..., None] * t
    return np.floor(np.clip(acc, 0.0, 255.0) + 0.5).astype(np.int32)


def seeded_case(rng, case):
    """Sources of 1 x 1 up to 140 x 140 (every fifth narrower than the four taps), a rotation of any angle about the centres,
    a scale of 0.5 .. 2 and a mild perspective row; every third source a checkerboard."""
    w, h = (int(v) for v in (rng.integers(1, 4, 2) if case % 5 == 0 else rng.integers(1, 141, 2)))
    out_w, out_h = (int(v) for v in rng.integers(4, 97, 2))
    angle, scale = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 2.0)
    lin = scale * np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]])
    t = np.array([w / 2.0, h / 2.0]) - lin @ np.array([out_w / 2.0, out_h / 2.0])
    aff = np.array([[lin[0, 0], lin[0, 1], t[0]], [lin[1, 0], lin[1, 1], t[1]], [0, 0, 1.0]])
    g, k = rng.uniform(-0.25, 0.25, 2) / np.array([out_w, out_h])
    persp = np.array([[1, 0, 0], [0, 1, 0], [g, k, 1.0]])
    m = (aff @ persp).reshape(9).astype(F)
    assert P.accepted(m, out_w, out_h), (case, list(m))
    return image(w, h, 7000 + case, checker=case % 3 == 0), m, out_w, out_h


def test_the_mirror_is_within_one_level_of_a_float64_evaluation():
    """60 seeded cases per edge mode; every byte within one level, at most 1 % of them different at all (the cap of the
    bilinear test: the one-level allowance cannot hide a wrong tap).  Measured here: 0.0130 % (fill) and 0.0225 % (replicate)
    of the bytes differ."""
    for edge in EDGES:
        rng = np.random.default_rng(211)
        differ = total = 0
        for case in range(60):
            src, m, out_w, out_h = seeded_case(rng, case)
            got = Q.project(src, m, out_w, out_h, edge, FILLB).astype(np.int32)
            ref = cubic64(src, m, out_w, out_h, edge, FILLB)
            assert np.abs(got - ref).max() <= 1, (edge, case, src.shape, out_w, out_h)
            differ += int((got != ref).sum())
            total += got.size
        print(f"edge {edge}: {differ} of {total} bytes differ from the float64 evaluation ({100.0 * differ / total:.4f} %)")
        assert differ <= 0.01 * total, (edge, differ, total)


def test_an_enlarging_axis_aligned_matrix_is_within_one_level_of_the_bicubic_resize():
    """(w / out_w, 0, 0, 0, h / out_h, 0, 0, 0, 1) with out >= the source is the map of the resize; where the 4 x 4 taps lie inside
    the image the resize clips nothing, and differs only by its renormalisation.  Within one level, at most 1 % of the bytes
    different.  Measured here: 0.0977 % of the compared bytes differ."""
    rng = np.random.default_rng(223)
    differ = total = 0
    for case in range(40):
        w, h = (int(v) for v in rng.integers(5, 60, 2))
        out_w, out_h = int(w * rng.uniform(1.0, 3.0)) + 1, int(h * rng.uniform(1.0, 3.0)) + 1
        src = image(w, h, 8000 + case, checker=case % 3 == 0)
        m = np.array([w / out_w, 0, 0, 0, h / out_h, 0, 0, 0, 1], np.float64).astype(F)
        inside = Q.taps_inside(m, w, h, out_w, out_h)
        got = Q.project(src, m, out_w, out_h, Q.REPLICATE).astype(np.int32)[inside]
        ref = B.resize(src, out_w, out_h).astype(np.int32)[inside]
        assert np.abs(got - ref).max(initial=0) <= 1, (case, w, h, out_w, out_h)
        differ += int((got != ref).sum())
        total += got.size
    print(f"{differ} of {total} bytes differ from the bicubic resize ({100.0 * differ / total:.4f} %)")
    assert total > 100000 and differ <= 0.01 * total


def test_bilinear_through_the_mirror_is_the_projective_and_the_affine_mirror():
    rng = np.random.default_rng(227)
    for case in range(20):
        w, h, out_w, out_h = (int(v) for v in rng.integers(1, 60, 4))
        src = image(w, h, 9000 + case)
        a = rng.uniform(-math.pi, math.pi)
        m6 = np.array([math.cos(a), -math.sin(a), w / 2.0, math.sin(a), math.cos(a), h / 2.0], np.float64).astype(F)
        m9 = np.concatenate([m6, np.array([0, 0, 1], F)])
        for edge in EDGES:
            got = Q.project_filter(src, m9, Q.BILINEAR, out_w, out_h, edge, FILLB)
            assert np.array_equal(got, P.project(src, m9, out_w, out_h, edge, FILLB)), (case, edge)
            assert np.array_equal(got, W.warp(src, m6, out_w, out_h, edge, FILLB)), (case, edge)


# ---- jpeg_amd_project_filter_view ---------------------------------------------------------------------------------------------------

def c_filter_view(L, o, m, filter, out_w, out_h):
    m = np.ascontiguousarray(m, F)
    v = _lib.View(-7, _lib.Region(-7, -7, -7, -7))
    mv = np.full(9, -7, F)
    st = _lib.lib().jpeg_amd_project_filter_view(C.byref(L), o, m.ctypes.data, filter, out_w, out_h, C.byref(v), mv.ctypes.data)
    return st, (v.denom, v.region.x, v.region.y, v.region.width, v.region.height), mv


def c_plain_view(L, o, m, out_w, out_h):
    m = np.ascontiguousarray(m, F)
    v = _lib.View(-7, _lib.Region(-7, -7, -7, -7))
    mv = np.full(9, -7, F)
    st = _lib.lib().jpeg_amd_project_view(C.byref(L), o, m.ctypes.data, out_w, out_h, C.byref(v), mv.ctypes.data)
    return st, (v.denom, v.region.x, v.region.y, v.region.width, v.region.height), mv


def check_view(w, h, o, m, out, what):
    """Both filters against the restatement, and the bilinear one against jpeg_amd_project_view -> the bicubic view."""
    L = c_layout(w, h, FUSED["420"])
    for filter in (Q.BILINEAR, Q.BICUBIC):
        st, view, mv = c_filter_view(L, o, m, filter, *out)
        want_view, want_mv = Q.project_filter_view(w, h, o, m, filter, *out)
        assert st == OK and view == want_view and np.array_equal(mv, want_mv), (what, filter, w, h, o, list(m), out, view, want_view)
        ws, hs = P.scaled_size(w, h, view[0])
        assert view[3] >= 1 and view[4] >= 1 and view[1] >= 0 and view[2] >= 0 and view[1] + view[3] <= ws and view[2] + view[4] <= hs, what
        assert P.accepted(mv, *out), what
        if filter == Q.BILINEAR:
            plain = c_plain_view(L, o, m, *out)
            assert plain[0] == OK and plain[1] == view and np.array_equal(plain[2], mv), what
            assert view == P.project_view(w, h, o, m, *out)[0]
            narrow = view
    # the bicubic view holds the bilinear one and is at most one pixel wider on each side
    assert view[0] == narrow[0] and narrow[1] - 1 <= view[1] <= narrow[1] and narrow[2] - 1 <= view[2] <= narrow[2], what
    assert 0 <= view[1] + view[3] - (narrow[1] + narrow[3]) <= 1 and 0 <= view[2] + view[4] - (narrow[2] + narrow[4]) <= 1, what
    return view, mv


def test_project_filter_view_is_the_python_restatement():
    rng = np.random.default_rng(229)
    denoms, last = set(), 0
    for case in range(2000):
        w, h = (int(v) for v in (rng.integers(1, 65536, 2) if case % 4 == 0 else rng.integers(1, 700, 2)))
        out = tuple(int(v) for v in (rng.integers(1, 300, 2) if case % 2 else rng.integers(1, 40, 2)))
        for o in range(1, 9):
            uw, uh = E.oriented_size(o, w, h)
            m = P.distortion(rng, uw, uh, out[0], out[1], 0.5, 0.2)
            if not P.accepted(m, *out):
                continue
            view, _ = check_view(w, h, o, m, out, case)
            denoms.add(view[0])
            last += view[1] + view[3] == P.scaled_size(w, h, view[0])[0]
    assert denoms == {1, 2, 4, 8} and last > 1000           # (views that end at the column W' - 1)


def test_project_filter_view_edges():
    w, h, out = 100, 60, (16, 16)
    row2 = [0.001, 0.002, 1]
    # a footprint that misses the image entirely: a one-pixel view at the nearest corner or edge, with either filter
    for t, want in (((-500, -500), (1, 0, 0, 1, 1)), ((500, 500), (1, 99, 59, 1, 1)), ((500, -500), (1, 99, 0, 1, 1)),
                    ((-500, 500), (1, 0, 59, 1, 1))):
        assert check_view(w, h, 1, np.array([1, 0, t[0], 0, 1, t[1]] + row2, F), out, "missed")[0] == want
    # both sides of the denominator rule, which the filter does not move
    for d in (2, 4, 8):
        below = np.nextafter(F(d), F(0))
        assert check_view(800, 800, 1, np.array([d, 0, 0, 0, d, 0, 0, 0, 1], F), out, d)[0][0] == d
        assert check_view(800, 800, 1, np.array([below, 0, 0, 0, d, 0, 0, 0, 1], F), out, d)[0][0] == d // 2
    # the identity on a canvas of the image's size: columns -2 .. W + 2 clamped are the whole image; a corner at W' - 1
    assert check_view(40, 30, 1, np.array(IDENT, F), (40, 30), "whole")[0] == (1, 0, 0, 40, 30)
    assert check_view(40, 30, 1, np.array([1, 0, 20, 0, 1, 10, 0, 0, 1], F), (8, 8), "inner")[0] == (1, 17, 7, 14, 14)
    assert check_view(40, 30, 1, np.array([1, 0, 32, 0, 1, 22, 0, 0, 1], F), (8, 8), "corner")[0] == (1, 29, 19, 11, 11)


def test_project_filter_view_refuses():
    L = c_layout(100, 60, FUSED["420"])
    good = np.array([1, 0, 0, 0, 1, 0, 0.001, 0.002, 1], F)
    unset = (-7, -7, -7, -7, -7)
    assert c_filter_view(L, 1, good, Q.BICUBIC, 16, 16)[0] == OK
    for filter in (1, 2, 4, -1):
        st, view, mv = c_filter_view(L, 1, good, filter, 16, 16)
        assert (st, view) == (EINVAL, unset) and (mv == -7).all(), filter
    for o in (0, 9):
        assert c_filter_view(L, o, good, Q.BICUBIC, 16, 16)[:2] == (EINVAL, unset)
    bad = good.copy()
    bad[6] = -1.0 / 16
    assert c_filter_view(L, 1, bad, Q.BICUBIC, 16, 16)[:2] == (EINVAL, unset)
    assert c_filter_view(L, 1, good, Q.BICUBIC, 0, 16)[:2] == (EINVAL, unset)
    lib = _lib.lib()
    v, mv = _lib.View(), np.zeros(9, F)
    assert lib.jpeg_amd_project_filter_view(None, 1, good.ctypes.data, 3, 16, 16, C.byref(v), mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_project_filter_view(C.byref(L), 1, None, 3, 16, 16, C.byref(v), mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_project_filter_view(C.byref(L), 1, good.ctypes.data, 3, 16, 16, None, mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_project_filter_view(C.byref(L), 1, good.ctypes.data, 3, 16, 16, C.byref(v), None) == EINVAL


def test_the_wider_margin_is_enough():
    """Dyadic affine matrices (multiples of 1 / 256 on sources below 2^7 a side: every coordinate operation is exact in
    binary32, and so are the orientation composed into the matrix and m_view): the mirror on the view's pixels with m_view IS
    the mirror on the whole STORED image with the matrix against it -- a tap the view lacked would show.  100 cases x 8
    orientations x both edge modes; the columns' norms stay below 2, so every view is taken at denominator 1.
    Against the ORIENTED whole image with the caller's matrix the same holds bit for bit in orientation 1 only: a flip
    reverses the ascending order of a row's four products and a transposition exchanges the row sums with the column sum, so
    the same sixteen products are added in another order.  There the two are within one level, and (measured here) 0.0003 %
    of the bytes differ."""
    rng = np.random.default_rng(233)
    cropped = differ = total = 0
    for case in range(100):
        w, h = (int(v) for v in rng.integers(6, 100, 2))
        out_w, out_h = (int(v) for v in rng.integers(3, 40, 2))
        stored = image(w, h, 9500 + case)
        for o in range(1, 9):
            uw, uh = E.oriented_size(o, w, h)
            a, s = rng.uniform(-math.pi, math.pi), rng.uniform(0.3, 1.3)
            lin = np.round(256 * s * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])) / 256
            t = np.round(256 * (rng.uniform(0.2, 0.8, 2) * np.array([uw, uh]) - lin @ np.array([out_w / 2.0, out_h / 2.0]))) / 256
            m = np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1], 0, 0, 1], np.float64)
            assert np.array_equal(m.astype(F).astype(np.float64), m)
            st, view, mv = c_filter_view(c_layout(w, h, FUSED["444"]), o, m, Q.BICUBIC, out_w, out_h)
            assert st == OK and view[0] == 1, (case, o, view)
            # the matrix against the whole stored image: the orientation composed into it, exactly
            T, fx, fy = E.BITS[o]
            r0, r1 = (m[3:6], m[0:3]) if T else (m[0:3], m[3:6])
            r0 = np.array([0, 0, w]) - r0 if fx else r0
            r1 = np.array([0, 0, h]) - r1 if fy else r1
            whole = np.concatenate([r0, r1, [0, 0, 1]])
            assert np.array_equal(whole.astype(F).astype(np.float64), whole)
            assert np.array_equal(mv.astype(np.float64), whole - np.array([0, 0, view[1], 0, 0, view[2], 0, 0, 0]))
            crop = np.ascontiguousarray(stored[view[2]:view[2] + view[4], view[1]:view[1] + view[3]])
            cropped += crop.size < stored.size
            upright = E.orient(stored, o)
            for edge in EDGES:
                got = Q.project(crop, mv, out_w, out_h, edge, FILLB)
                assert np.array_equal(got, Q.project(stored, whole, out_w, out_h, edge, FILLB)), (case, o, edge, view)
                seen = Q.project(upright, m, out_w, out_h, edge, FILLB)
                if o == 1:
                    assert np.array_equal(got, seen), (case, edge, view)
                assert np.abs(got.astype(np.int32) - seen).max() <= 1, (case, o, edge, view)
                differ += int((got != seen).sum())
                total += got.size
    print(f"{differ} of {total} bytes differ between the stored and the oriented image's sums ({100.0 * differ / total:.4f} %)")
    assert cropped > 400 and differ <= 0.01 * total


# ---- what the calls refuse, and in which order, with a NULL context -----------------------------------------------------------------

SPEC = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
BUF = np.zeros(16, np.uint16)
PTR = BUF.ctypes.data
N = 2


def c_warp(edge=Q.FILL, fill=FILLB):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = fill
    return w


def batch_call(form, filter, matrices=(IDENT, IDENT), edge=Q.FILL, n=N, size=(20, 10), out=(8, 8), dst=PTR, spec=True, plain=False):
    ext = (_lib.Extent * N)(*[_lib.Extent(*size)] * N)
    m = np.ascontiguousarray(matrices, F)
    wp = c_warp(edge)
    head = (None, n, PTR, 3 * size[0] * size[1], ext, m.ctypes.data, C.byref(wp)) + (() if plain else (filter,)) + (out[0], out[1])
    lib = _lib.lib()
    if form == "bytes":
        return (lib.jpeg_amd_project_batch if plain else lib.jpeg_amd_project_filter_batch)(*head, dst, 3 * out[0] * out[1])
    call = lib.jpeg_amd_project_tensor_batch if plain else lib.jpeg_amd_project_filter_tensor_batch
    return call(*head, C.byref(SPEC) if spec else None, None, None, dst, 3 * out[0] * out[1])


def mixed_call(form, filter, matrices=(IDENT, IDENT), edge=Q.FILL, n=N, size=(20, 10), out=(8, 8), dst=PTR, precisions=(8, 8), plain=False):
    """-> (status, the views written, the matrices written)"""
    images = (_lib.Image * N)()
    for i in range(N):
        images[i].layout = c_layout(size[0], size[1], [(1, 1)] * 3, precision=precisions[i])
        for c in range(3):
            images[i].d_coef[c] = PTR
        images[i].d_quanta, images[i].ntables = PTR, 2
    m = np.ascontiguousarray(matrices, F)
    wp = c_warp(edge)
    views = (_lib.View * N)(*[_lib.View(-7, _lib.Region(-7, -7, -7, -7))] * N)
    mout = np.full((N, 9), -7, F)
    head = (None, n, images, 0, RGB, None, m.ctypes.data, C.byref(wp)) + (() if plain else (filter,)) + (out[0], out[1])
    lib = _lib.lib()
    if form == "bytes":
        call = lib.jpeg_amd_decode_projected_mixed if plain else lib.jpeg_amd_decode_projected_filter_mixed
        st = call(*head, views, mout.ctypes.data, dst, 3 * out[0] * out[1])
    else:
        call = lib.jpeg_amd_decode_tensor_projected_mixed if plain else lib.jpeg_amd_decode_tensor_projected_filter_mixed
        st = call(*head, C.byref(SPEC), None, views, mout.ctypes.data, None, dst, 3 * out[0] * out[1])
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views], mout


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_batch_calls_refuse(form):
    """The batch calls look at the context in front of n_images == 0, so with a NULL context every call is EINVAL, a right one
    included: the mixed calls (below), which run the same check, tell the verdicts apart, and tests/test_gpu_project_cubic.py
    repeats these with a context."""
    assert batch_call(form, Q.BICUBIC) == EINVAL and batch_call(form, Q.BICUBIC, n=0) == EINVAL
    for filter in (1, 2, 4, -1):
        assert batch_call(form, filter) == EINVAL, filter
    assert batch_call(form, Q.BICUBIC, edge=2) == EINVAL and batch_call(form, Q.BICUBIC, out=(0, 8)) == EINVAL
    assert batch_call(form, Q.BICUBIC, size=(2 ** 24 + 1, 1)) == EINVAL
    bad = np.array([IDENT, IDENT], F)
    bad[1, 6:] = [-1.0 / 8, 0, 1]
    assert batch_call(form, Q.BICUBIC, bad) == EINVAL


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_mixed_calls_judge_the_filter_where_the_edge_mode_is_judged(form):
    """12-bit images are ENOSUP, in front of the target and behind every image's matrix; the edge mode is judged with the target,
    so an image 0 of 12 bits hides a wrong edge mode and an image 1 of 12 bits does not -- and the same holds of the filter."""
    wide = (1, 0, 0, 11, 10)                # an 8 x 8 canvas through the identity: columns 0 .. 10 and rows 0 .. 9 of 20 x 10
    narrow = (1, 0, 0, 10, 10)
    assert mixed_call(form, Q.BICUBIC, n=0)[0] == OK
    st, views, mout = mixed_call(form, Q.BICUBIC)
    assert st == EINVAL and views == [wide, wide] and np.array_equal(mout, np.array([IDENT, IDENT], F))      # (the context)
    st, views, _ = mixed_call(form, Q.BILINEAR)
    assert st == EINVAL and views == [narrow, narrow]
    for filter in (1, 2, 4):
        assert mixed_call(form, filter, n=0)[0] == EINVAL, filter
        assert mixed_call(form, filter, precisions=(8, 12))[0] == mixed_call(form, Q.BICUBIC, precisions=(8, 12), edge=2)[0] == EINVAL
        assert mixed_call(form, filter, precisions=(12, 8))[0] == mixed_call(form, Q.BICUBIC, precisions=(12, 8), edge=2)[0] == ENOSUP
        # a filter that is refused has the two-tap footprint: the views written are the bilinear call's
        assert mixed_call(form, filter)[1] == [narrow, narrow]
    assert mixed_call(form, Q.BICUBIC, precisions=(8, 12))[0] == ENOSUP
    # with BILINEAR: the existing call, status for status and view for view
    for kw in (dict(), dict(edge=2), dict(precisions=(8, 12)), dict(out=(0, 8)), dict(n=0), dict(matrices=[IDENT, [1, 0, 0, 0, 1, 0, -1, 0, 1]])):
        a, b = mixed_call(form, Q.BILINEAR, **kw), mixed_call(form, None, plain=True, **kw)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), kw
        assert batch_call(form, Q.BILINEAR, **{k: v for k, v in kw.items() if k != "precisions"}) == \
            batch_call(form, None, plain=True, **{k: v for k, v in kw.items() if k != "precisions"})


def test_the_file_calls_take_each_view_from_project_filter_view():
    """Pass 0 of the file calls needs no device: with a NULL context a call that is right gets as far as the context, and the
    views, matrices and orientations written by then are jpeg_amd_project_filter_view's for each file's own size and tag."""
    datas = [FI.synthetic_file("420", (160, 120), 61)[0], E.insert(FI.synthetic_file("444", (53, 37), 62)[0], E.exif_segment(6, big=True)),
             FI.synthetic_file("y8", (37, 83), 63)[0]]
    sizes, tags = [(160, 120), (53, 37), (37, 83)], [1, 6, 1]
    out = (24, 16)
    rng = np.random.default_rng(239)
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    nbytes = (C.c_size_t * n)(*[d.size for d in datas])
    lib = _lib.lib()
    orient = (C.c_uint8 * n)(0, 0, 0)
    mats = np.array([P.distortion(rng, *E.oriented_size(o, *s), out[0], out[1], 0.5, 0.1) for s, o in zip(sizes, tags)], F)
    for filter in (Q.BILINEAR, Q.BICUBIC, 1, 4):
        for tensor in (False, True):
            infos, views = (_lib.FrameInfo * n)(), (_lib.View * n)()
            mout, oout = np.full((n, 9), -7, F), (C.c_int32 * n)(-7, -7, -7)
            wp = c_warp()
            head = (None, ptrs, nbytes, n, 1, 0, RGB, orient, mats.ctypes.data, C.byref(wp), filter, out[0], out[1])
            if tensor:
                st = lib.jpeg_amd_decompress_tensor_projected_filter_mixed(*head, C.byref(SPEC), None, None, PTR, 3 * out[0] * out[1], infos,
                                                                           views, mout.ctypes.data, oout)
            else:
                st = lib.jpeg_amd_decompress_resized_projected_filter_mixed(*head, PTR, 3 * out[0] * out[1], infos, views, mout.ctypes.data,
                                                                            oout)
            assert st == EINVAL                                      # the context, last -- or the filter, judged behind pass 0
            assert list(oout) == tags
            for i in range(n):
                want_view, want_m = Q.project_filter_view(sizes[i][0], sizes[i][1], tags[i], mats[i], Q.BICUBIC if filter == Q.BICUBIC else 0,
                                                          *out)
                v = views[i]
                assert (v.denom, v.region.x, v.region.y, v.region.width, v.region.height) == want_view, (filter, i)
                assert np.array_equal(mout[i], want_m) and (infos[i].width, infos[i].height) == sizes[i]
    wp = c_warp()
    for filter, want in ((Q.BICUBIC, OK), (Q.BILINEAR, OK), (1, EINVAL), (4, EINVAL)):      # no files need no context
        assert lib.jpeg_amd_decompress_resized_projected_filter_mixed(None, ptrs, nbytes, 0, 1, 0, RGB, None, None, C.byref(wp), filter, out[0],
                                                                      out[1], None, 0, None, None, None, None) == want


# ---- the Python keywords --------------------------------------------------------------------------------------------------------------

class Recorder:
    """In the library's place: every call of a symbol whose name holds warp, project, warped or projected is noted with its
    arguments and answers 0; every other symbol is the library's own."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        if any(part in name for part in ("_warp", "_project")) and not name.endswith("_view"):
            return functools.partial(self.note, name)
        return getattr(self.real, name)

    def note(self, name, *values):
        # (the matrices now: what the pointers point at lives as long as the call)  The warp, and the n x k floats in front of it
        at = next(i for i, v in enumerate(values) if hasattr(v, "_obj") and isinstance(v._obj, _lib.Warp))
        k = 9 if "project" in name else 6
        sent = np.frombuffer(C.string_at(values[at - 1], 4 * 2 * k), F).reshape(2, k).copy()
        self.calls.append((name, values, at, sent))
        return 0


class StandIn:
    """A context without a device: a handle, host tensors, uploads that stay on the host."""
    handle = C.c_void_p(0x5A5A)

    def empty(self, n, dtype):
        return torch.zeros(max(int(n), 0), dtype=dtype)

    def upload(self, a):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


CTX = StandIn()
OUT = (10, 6)
M6 = np.array([[1.5, 0.25, 1.0, -0.125, 1.25, 0.5], [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]], F)
M9 = np.concatenate([M6, np.array([[0.001, 0.002, 1.0], [0.0, 0.0, 1.0]], F)], axis=1)
PADDED = np.concatenate([M6, np.array([[0, 0, 1.0], [0, 0, 1.0]], F)], axis=1)


def pictures():
    rng = np.random.default_rng(5)
    return [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for w, h in ((7, 5), (4, 9))]


def spectrals():
    out = []
    for seed, (size, factors) in enumerate((((24, 16), [(2, 2), (1, 1), (1, 1)]), ((16, 16), [(1, 1)] * 3))):
        layout = J.Layout("ycc8", {c + 1: J.Component(f, min(c, 1)) for c, f in enumerate(factors)})
        rng = np.random.default_rng(seed)
        planes = [rng.integers(-64, 64, (uy, ux, 64)).astype(np.int16) for ux, uy in layout.units(size)]
        quanta = [rng.integers(1, 24, 64).astype(np.uint16) for _ in range(2)]
        out.append(J.Spectral.from_host(CTX, size, layout, planes, quanta))
    return out


def files():
    return [FI.synthetic_file("420", (24, 16), 3)[0], FI.synthetic_file("444", (16, 16), 4)[0]]


@pytest.fixture
def recorder(monkeypatch):
    rec = Recorder(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: rec)
    return rec


def spec():
    return J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")


def calls(kw):
    """Every public function through a map, called with the keywords kw (`filter`, or for the file calls `warp_filter`) ->
    [(function, affine?, what it returned)]."""
    fkw = {("warp_" + k if k == "filter" else k): v for k, v in kw.items()}
    return [("warp", True, J.warp(CTX, pictures(), M6, OUT, **kw)),
            ("warp_tensor", True, J.warp_tensor(CTX, pictures(), M6, OUT, spec(), **kw)),
            ("project", False, J.project(CTX, pictures(), M9, OUT, **kw)),
            ("project_tensor", False, J.project_tensor(CTX, pictures(), M9, OUT, spec(), **kw)),
            ("decode_warped_mixed", True, J.decode_warped_mixed(CTX, spectrals(), M6, OUT, **kw)),
            ("decode_tensors_warped_mixed", True, J.decode_tensors_warped_mixed(CTX, spectrals(), M6, OUT, spec(), **kw)),
            ("decode_projected_mixed", False, J.decode_projected_mixed(CTX, spectrals(), M9, OUT, **kw)),
            ("decode_tensors_projected_mixed", False, J.decode_tensors_projected_mixed(CTX, spectrals(), M9, OUT, spec(), **kw)),
            ("decompress_resized/6", True, J.decompress_resized(CTX, files(), OUT, warp=M6, **fkw)),
            ("decompress_resized/9", False, J.decompress_resized(CTX, files(), OUT, warp=M9, **fkw)),
            ("decompress_tensors/6", True, J.decompress_tensors(CTX, files(), OUT, spec(), warp=M6, **fkw)),
            ("decompress_tensors/9", False, J.decompress_tensors(CTX, files(), OUT, spec(), warp=M9, **fkw))]


PLAIN = ["jpeg_amd_warp_batch", "jpeg_amd_warp_colour_tensor_batch", "jpeg_amd_project_batch", "jpeg_amd_project_tensor_batch",
         "jpeg_amd_decode_warped_mixed", "jpeg_amd_decode_tensor_warped_colour_mixed", "jpeg_amd_decode_projected_mixed",
         "jpeg_amd_decode_tensor_projected_mixed", "jpeg_amd_decompress_resized_warped_mixed", "jpeg_amd_decompress_resized_projected_mixed",
         "jpeg_amd_decompress_tensor_warped_colour_mixed", "jpeg_amd_decompress_tensor_projected_mixed"]
CUBIC = ["jpeg_amd_project_filter_batch", "jpeg_amd_project_filter_tensor_batch"] * 2 + \
        ["jpeg_amd_decode_projected_filter_mixed", "jpeg_amd_decode_tensor_projected_filter_mixed"] * 2 + \
        ["jpeg_amd_decompress_resized_projected_filter_mixed"] * 2 + ["jpeg_amd_decompress_tensor_projected_filter_mixed"] * 2


def test_the_default_and_bilinear_make_the_call_they_made(recorder):
    """Without the keyword and with "bilinear": the same symbols with the same number of arguments, no filter among them, and
    the same matrices (tests/test_resample_routes_cpu.py holds every argument of the default to its record)."""
    calls({})
    first = recorder.calls[:]
    del recorder.calls[:]
    calls(dict(filter="bilinear"))
    assert [c[0] for c in first] == PLAIN and [c[0] for c in recorder.calls] == PLAIN
    for (name, a, _, sent_a), (_, b, _, sent_b) in zip(first, recorder.calls):
        assert len(a) == len(_lib.SIGNATURES[name][1]) == len(b), name
        assert np.array_equal(sent_a, sent_b) and np.array_equal(sent_a, M9 if "project" in name else M6), name
        small = lambda vs: [v for v in vs if isinstance(v, int) and abs(v) < 2 ** 20]          # noqa: E731  (not the pointers)
        assert small(a) == small(b) and _lib.FILTER_BICUBIC not in small(a), name


def test_bicubic_calls_the_forms_with_a_filter(recorder):
    results = calls(dict(filter="bicubic"))
    assert [c[0] for c in recorder.calls] == CUBIC
    for (name, values, at, sent), (what, affine, got) in zip(recorder.calls, results):
        proto = _lib.SIGNATURES[name][1]
        assert len(values) == len(proto), name
        # the filter stands behind the warp, and the matrices in front of the warp are [n, 9]: an affine map padded with (0, 0, 1)
        assert values[at + 1] == _lib.FILTER_BICUBIC and values[at + 2:at + 4] == OUT, name
        assert np.array_equal(sent, PADDED if affine else M9), what
        if isinstance(got, tuple) and "mixed" in what or "decompress" in what:
            mats = got[-1]
            assert mats.shape == (2, 6 if affine else 9) and mats.dtype == F, what


def test_the_keyword_rules(recorder):
    for call in (lambda f: J.warp(CTX, pictures(), M6, OUT, filter=f), lambda f: J.project_tensor(CTX, pictures(), M9, OUT, spec(), filter=f),
                 lambda f: J.decode_warped_mixed(CTX, spectrals(), M6, OUT, filter=f),
                 lambda f: J.decompress_tensors(CTX, files(), OUT, spec(), warp=M9, warp_filter=f),
                 lambda f: J.decompress_resized(CTX, files(), OUT, warp=M6, warp_filter=f)):
        for bad in ("antialias", "nearest", 3):
            with pytest.raises(ValueError):
                call(bad)
    # warp_filter only together with warp; the resize's filter stays bilinear with a warp, as it did
    for f in ("bicubic", "bilinear"):
        with pytest.raises(ValueError, match="warp_filter"):
            J.decompress_tensors(CTX, files(), OUT, spec(), warp_filter=f)
        with pytest.raises(ValueError, match="warp_filter"):
            J.decompress_resized(CTX, files(), OUT, warp_filter=f)
    with pytest.raises(ValueError, match="not together"):
        J.decompress_tensors(CTX, files(), OUT, spec(), warp=M6, filter="bicubic", warp_filter="bicubic")
    assert recorder.calls == []


def test_the_views_of_python():
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    m6 = np.array([1, 0, 20, 0, 1, 10], F)
    m9 = np.concatenate([m6, np.array([0, 0, 1], F)])
    narrow, mv = J.warp_view((40, 30), layout, m6, (8, 8))
    assert narrow == (1, 18, 8, 12, 12) and J.warp_view((40, 30), layout, m6, (8, 8), filter="bilinear")[0] == narrow
    wide, mw = J.warp_view((40, 30), layout, m6, (8, 8), filter="bicubic")
    assert wide == (1, 17, 7, 14, 14) and mw.shape == (6,) and mw.tolist() == [1, 0, 3, 0, 1, 3]
    view9, m9v = J.project_view((40, 30), layout, m9, (8, 8), filter="bicubic")
    assert view9 == wide and m9v.shape == (9,) and m9v.tolist() == [1, 0, 3, 0, 1, 3, 0, 0, 1]
    assert J.project_view((40, 30), layout, m9, (8, 8))[0] == narrow
    with pytest.raises(ValueError):
        J.warp_view((40, 30), layout, m6, (8, 8), filter="antialias")
