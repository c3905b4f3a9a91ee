"""The projective resample (include/jpeg_amd.h, "projective resample") without a GPU: the numpy mirror of the contract
(_project_ref) against the points where the contract ties into what exists -- the affine warp's mirror, bit for bit, and
torch's grid_sample on a float64 homography grid, within one level -- jpeg_amd_project_view against its Python restatement,
the one-pixel margin of its views, what the calls refuse with a NULL context, and perspective_matrix."""
import ctypes as C
import math

import numpy as np
import pytest

import _files as FI
import _orient as E
import _project_ref as P
import _warp_ref as W
from _calls import FUSED, c_layout
from jpeg_amd import _lib
from jpeg_amd.api import perspective_matrix

OK, EINVAL, ENOSUP = 0, -1, -5
F = np.float32
RGB = _lib.COLOR_RGB8
EDGES = (P.FILL, P.REPLICATE)
FILLB = (7, 130, 255)


def image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def random_affine(rng, w, h, out_w, out_h):
    """A rotate / scale / shear matrix that takes the canvas centre to the source centre, as float32 [6]."""
    angle, scale, shear = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 2.0), rng.uniform(-0.3, 0.3)
    lin = scale * np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]]) @ np.array([[1.0, shear], [0.0, 1.0]])
    t = np.array([w / 2.0, h / 2.0]) - lin @ np.array([out_w / 2.0, out_h / 2.0])
    return np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1]], np.float64).astype(F)


def seeded_distortion(rng, case):
    """The seeded four-corner cases of this file: sources of 8 .. 200 a side, canvases of 8 .. 120, distortion_scale 0.5, and
    every third one with corners up to 20 % outside the source."""
    w, h = (int(v) for v in rng.integers(8, 201, 2))
    out_w, out_h = (int(v) for v in rng.integers(8, 121, 2))
    m = P.distortion(rng, w, h, out_w, out_h, 0.5, 0.2 if case % 3 == 2 else 0.0)
    assert P.accepted(m, out_w, out_h), (case, list(m))
    return w, h, out_w, out_h, m


# ---- the mirror against the contract's consequences ---------------------------------------------------------------------------------

def test_a_last_row_001_is_the_affine_warp():
    rng = np.random.default_rng(101)
    for case in range(50):
        w, h, out_w, out_h = (int(v) for v in rng.integers(1, 91, 4))
        src = image(w, h, 4000 + case)
        m6 = random_affine(rng, w, h, out_w, out_h)
        m9 = np.concatenate([m6, np.array([0, 0, 1], F)])
        for edge in EDGES:
            for flip in (False, True):
                assert np.array_equal(P.project(src, m9, out_w, out_h, edge, FILLB, flip), W.warp(src, m6, out_w, out_h, edge, FILLB, flip)), \
                    (case, edge, flip)


def test_the_mirror_is_within_one_level_of_grid_sample():
    """grid_sample(bilinear, align_corners=False) on a grid made from the same homography in float64.  Measured here: never more
    than one level; 0.0267 % (zeros) and 0.0280 % (border) of the bytes differ; the float32 coordinates are within 3.5e-5 px
    of the float64 ones wherever these lie inside the clamp's range."""
    torch = pytest.importorskip("torch")
    worst = 0.0
    for mode, edge in (("zeros", P.FILL), ("border", P.REPLICATE)):
        rng = np.random.default_rng(103)
        differ = total = 0
        for case in range(60):
            w, h, out_w, out_h, m = seeded_distortion(rng, case)
            src = image(w, h, 5000 + case)
            m64 = m.astype(np.float64).reshape(3, 3)
            xc, yc = np.meshgrid(np.arange(out_w) + 0.5, np.arange(out_h) + 0.5)
            den = m64[2, 0] * xc + m64[2, 1] * yc + m64[2, 2]
            X, Y = (m64[0, 0] * xc + m64[0, 1] * yc + m64[0, 2]) / den, (m64[1, 0] * xc + m64[1, 1] * yc + m64[1, 2]) / den
            grid = torch.from_numpy(np.stack([2.0 * X / w - 1.0, 2.0 * Y / h - 1.0], -1))[None]
            ref = torch.nn.functional.grid_sample(torch.from_numpy(src.astype(np.float64).transpose(2, 0, 1))[None], grid, mode="bilinear",
                                                  padding_mode=mode, align_corners=False)[0].numpy().transpose(1, 2, 0)
            ref = np.floor(np.clip(ref, 0.0, 255.0) + 0.5).astype(np.int32)
            got = P.project(src, m, out_w, out_h, edge, (0, 0, 0)).astype(np.int32)
            assert np.abs(got - ref).max() <= 1, (mode, case, w, h, out_w, out_h)
            differ += int((got != ref).sum())
            total += got.size
            sx, sy = P.coordinates(m, w, h, out_w, out_h)
            inside = (X - 0.5 > -1) & (X - 0.5 < w) & (Y - 0.5 > -1) & (Y - 0.5 < h)
            worst = max(worst, float(np.abs(sx - (X - 0.5))[inside].max(initial=0.0)), float(np.abs(sy - (Y - 0.5))[inside].max(initial=0.0)))
        print(f"{mode}: {differ} of {total} bytes differ from torch's rounded value ({100.0 * differ / total:.4f} %)")
        assert differ <= 0.01 * total, (mode, differ, total)
    print(f"float32 coordinates within {worst:.3g} px of float64")
    assert worst < 1e-3           # (2^-24 (67 |X| + 4 A) of the header with |X| <= 240 and A <= 1000)


# ---- jpeg_amd_project_view ----------------------------------------------------------------------------------------------------------

def c_project_view(L, o, m, out_w, out_h):
    m = np.ascontiguousarray(m, F)
    v = _lib.View(-7, _lib.Region(-7, -7, -7, -7))
    mv = np.full(9, -7, F)
    st = _lib.lib().jpeg_amd_project_view(C.byref(L), o, m.ctypes.data, out_w, out_h, C.byref(v), mv.ctypes.data)
    return st, (v.denom, v.region.x, v.region.y, v.region.width, v.region.height), mv


def check_view(w, h, o, m, out, what):
    L = c_layout(w, h, FUSED["420"])
    st, view, mv = c_project_view(L, o, m, *out)
    want_view, want_mv = P.project_view(w, h, o, m, *out)
    assert st == OK and view == want_view and np.array_equal(mv, want_mv), (what, w, h, o, list(m), out, view, want_view, mv, want_mv)
    ws, hs = P.scaled_size(w, h, view[0])
    assert view[3] >= 1 and view[4] >= 1 and view[1] >= 0 and view[2] >= 0 and view[1] + view[3] <= ws and view[2] + view[4] <= hs, what
    assert P.accepted(mv, *out), what            # m_view passes the contract's own check
    return view, mv


def test_project_view_is_the_python_restatement():
    rng = np.random.default_rng(107)
    denoms = set()
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
    assert denoms == {1, 2, 4, 8}


def test_project_view_with_a_last_row_001_is_warp_view():
    rng = np.random.default_rng(109)
    lib = _lib.lib()
    for case in range(300):
        w, h = (int(v) for v in rng.integers(1, 700, 2))
        out = tuple(int(v) for v in rng.integers(1, 300, 2))
        m6 = random_affine(rng, w, h, *out)
        m6[:2] *= F(rng.choice([0.5, 1, 3, 9]))
        m9 = np.concatenate([m6, np.array([0, 0, 1], F)])
        for o in range(1, 9):
            L = c_layout(w, h, FUSED["420"])
            st, view, mv = c_project_view(L, o, m9, *out)
            v6, mv6 = _lib.View(), np.zeros(6, F)
            assert lib.jpeg_amd_warp_view(C.byref(L), o, m6.ctypes.data, out[0], out[1], C.byref(v6), mv6.ctypes.data) == OK
            assert st == OK and view == (v6.denom, v6.region.x, v6.region.y, v6.region.width, v6.region.height), (case, o)
            assert np.array_equal(mv[:6], mv6) and mv[6:].tolist() == [0, 0, 1], (case, o, mv, mv6)


def test_project_view_edges():
    w, h, out = 100, 60, (16, 16)
    row2 = [0.001, 0.002, 1]
    # a footprint that misses the image entirely: a one-pixel view at the nearest corner or edge
    for t, want in (((-500, -500), (1, 0, 0, 1, 1)), ((500, 500), (1, 99, 59, 1, 1)), ((500, -500), (1, 99, 0, 1, 1)),
                    ((-500, 500), (1, 0, 59, 1, 1))):
        assert check_view(w, h, 1, np.array([1, 0, t[0], 0, 1, t[1]] + row2, F), out, "missed")[0] == want
    # the denominator on both sides of d * d == the smallest squared column norm; with the last row (0, 0, w22) the map is the
    # affine one divided by w22, and the columns' norms are (d / w22) at every point
    for d in (2, 4, 8):
        below = np.nextafter(F(d), F(0))
        for w22 in (1.0, 2.0, 0.5):
            s = F(w22)
            assert check_view(800, 800, 1, np.array([d * s, 0, 0, 0, d * s, 0, 0, 0, s], F), out, d)[0][0] == d
            assert check_view(800, 800, 1, np.array([below * s, 0, 0, 0, d * s, 0, 0, 0, s], F), out, d)[0][0] == d // 2
            assert check_view(800, 800, 1, np.array([d * s, 0, 0, 0, below * s, 0, 0, 0, s], F), out, d)[0][0] == d // 2
        # a true keystone: the step is d at the canvas's left edge and falls towards the right; the corner's column decides
        key = np.array([d, 0, 0, 0, d, 0, 1.0 / 64, 0, 1], F)
        view, _ = check_view(800, 800, 1, key, out, ("keystone", d))
        assert view[0] < d
    assert check_view(800, 800, 1, np.array([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1], F), out, "enlarging")[0][0] == 1
    # the whole image is never exceeded by a canvas far larger than it
    assert check_view(5, 3, 1, np.array([1, 0, -50, 0, 1, -50, 0, 0, 1], F), (200, 200), "larger")[0] == (1, 0, 0, 5, 3)


def test_project_view_refuses():
    L = c_layout(100, 60, FUSED["420"])
    good = np.array([1, 0, 0, 0, 1, 0, 0.001, 0.002, 1], F)
    unset = (-7, -7, -7, -7, -7)
    assert c_project_view(L, 1, good, 16, 16)[0] == OK
    for o in (0, 9, -1):
        assert c_project_view(L, o, good, 16, 16)[:2] == (EINVAL, unset)
    for k in range(9):
        for bad in (np.nan, np.inf, -np.inf, F(2.0 ** 30) * F(1.0000002), -F(2.0 ** 31)):
            m = good.copy()
            m[k] = bad
            st, view, mv = c_project_view(L, 1, m, 16, 16)
            assert (st, view) == (EINVAL, unset) and (mv == -7).all(), (k, bad)
    for k in range(6):
        m = good.copy()
        m[k] = F(2.0 ** 30)                                                     # the limit itself is inside
        assert c_project_view(L, 1, m, 16, 16)[0] == OK
    for out in ((0, 16), (16, 0), (2 ** 30 + 1, 16), (16, 2 ** 30 + 1)):
        assert c_project_view(L, 1, good, *out)[:2] == (EINVAL, unset)
    assert c_project_view(L, 1, np.array(IDENT, F), 2 ** 30, 2 ** 30)[0] == OK
    lib = _lib.lib()
    v, mv = _lib.View(), np.zeros(9, F)
    assert lib.jpeg_amd_project_view(None, 1, good.ctypes.data, 16, 16, C.byref(v), mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_project_view(C.byref(L), 1, None, 16, 16, C.byref(v), mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_project_view(C.byref(L), 1, good.ctypes.data, 16, 16, None, mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_project_view(C.byref(L), 1, good.ctypes.data, 16, 16, C.byref(v), None) == EINVAL


def test_the_views_margin_holds_and_the_view_route_is_within_one_level():
    """Over the seeded cases: every tap index of the float32 mirror on the WHOLE scaled image that lies inside the image lies
    inside the view, and the mirror on the view with m_view is within one level of the mirror on the whole image, at most
    1 % of the bytes different.  Measured here: 0.0374 % of the bytes differ (the two matrices round differently)."""
    rng = np.random.default_rng(113)
    differ = total = cropped = 0
    for case in range(60):
        w, h, out_w, out_h, m = seeded_distortion(rng, case)
        if case % 2:                                  # a reduction, so that the views are taken at 1/2, 1/4, 1/8 as well
            k = float(rng.choice([2.5, 5.0, 9.0]))
            w, h = int(w * k), int(h * k)
            m[:6] *= F(k)
        for o in (1, 3, 6, 8) if case % 4 else range(1, 9):
            st, view, mv = c_project_view(c_layout(w, h, FUSED["444"]), o, m, out_w, out_h)
            assert st == OK
            d = view[0]
            ws, hs = P.scaled_size(w, h, d)
            # the matrix against the whole STORED scaled image, in float32: the restatement's with a view at the origin
            T, fx, fy = E.BITS[o]
            m64 = [float(v) for v in m]
            r0, r1, r2 = (m64[3:6], m64[0:3], m64[6:9]) if T else (m64[0:3], m64[3:6], m64[6:9])
            if fx:
                r0 = [float(w) * r2[k] - r0[k] for k in range(3)]
            if fy:
                r1 = [float(h) * r2[k] - r1[k] for k in range(3)]
            whole = np.array([v / d for v in r0] + [v / d for v in r1] + r2, np.float64).astype(F)
            sx, sy = P.coordinates(whole, ws, hs, out_w, out_h)
            x0, y0, _, _ = P.taps(sx, sy)
            for idx, lo, n, size in ((x0, view[1], view[3], ws), (y0, view[2], view[4], hs)):
                for tap in (idx, idx + 1):
                    inside = (tap >= 0) & (tap <= size - 1)
                    assert ((tap[inside] >= lo) & (tap[inside] <= lo + n - 1)).all(), (case, o, view)
            src = image(ws, hs, 6000 + case)
            crop = np.ascontiguousarray(src[view[2]:view[2] + view[4], view[1]:view[1] + view[3]])
            cropped += crop.size < src.size
            for edge in EDGES:
                a = P.project(src, whole, out_w, out_h, edge, FILLB).astype(np.int32)
                b = P.project(crop, mv, out_w, out_h, edge, FILLB).astype(np.int32)
                assert np.abs(a - b).max() <= 1, (case, o, edge, view)
                differ += int((a != b).sum())
                total += a.size
    print(f"{differ} of {total} bytes differ between the view route and the whole image ({100.0 * differ / total:.4f} %)")
    assert differ <= 0.01 * total and cropped > 100


# ---- what the calls refuse, and in which order, with a NULL context -----------------------------------------------------------------

SPEC = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
BUF = np.zeros(16, np.uint16)
PTR = BUF.ctypes.data
N = 2
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def c_warp(edge=P.FILL, fill=FILLB):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = fill
    return w


def batch_call(form, matrices=(IDENT, IDENT), warp=True, edge=P.FILL, n=N, size=(20, 10), out=(8, 8), dst=PTR, spec=True, src_stride=None,
               colour=None):
    ext = (_lib.Extent * N)(*[_lib.Extent(*size)] * N)
    m = None if matrices is None else np.ascontiguousarray(matrices, F)
    wp = c_warp(edge)
    head = (None, n, PTR, 3 * size[0] * size[1] if src_stride is None else src_stride, ext, None if m is None else m.ctypes.data,
            C.byref(wp) if warp else None, out[0], out[1])
    if form == "bytes":
        return _lib.lib().jpeg_amd_project_batch(*head, dst, 3 * out[0] * out[1])
    return _lib.lib().jpeg_amd_project_tensor_batch(*head, C.byref(SPEC) if spec else None, None, colour, dst, 3 * out[0] * out[1])


def mixed_call(form, matrices=(IDENT, IDENT), warp=True, edge=P.FILL, n=N, size=(20, 10), out=(8, 8), dst=PTR, spec=True, orient=None,
               precisions=(8, 8)):
    """-> (status, the views written, the matrices written)"""
    images = (_lib.Image * N)()
    for i in range(N):
        images[i].layout = c_layout(size[0], size[1], [(1, 1)] * 3, precision=precisions[i])
        for c in range(3):
            images[i].d_coef[c] = PTR
        images[i].d_quanta, images[i].ntables = PTR, 2
    m = None if matrices is None else np.ascontiguousarray(matrices, F)
    wp = c_warp(edge)
    views = (_lib.View * N)(*[_lib.View(-7, _lib.Region(-7, -7, -7, -7))] * N)
    mout = np.full((N, 9), -7, F)
    o = None if orient is None else (C.c_uint8 * N)(*orient)
    head = (None, n, images, 0, RGB, o, None if m is None else m.ctypes.data, C.byref(wp) if warp else None, out[0], out[1])
    if form == "bytes":
        st = _lib.lib().jpeg_amd_decode_projected_mixed(*head, views, mout.ctypes.data, dst, 3 * out[0] * out[1])
    else:
        st = _lib.lib().jpeg_amd_decode_tensor_projected_mixed(*head, C.byref(SPEC) if spec else None, None, views, mout.ctypes.data, None,
                                                               dst, 3 * out[0] * out[1])
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views], mout


def with_entry(k, value, image=1):
    m = np.array([IDENT, IDENT], F)
    m[image, k] = value
    return m


def with_row2(row2, image=1):
    m = np.array([IDENT, IDENT], F)
    m[image, 6:] = row2
    return m


def row2_cases(out_w, out_h):
    """[(row 2, accepted)] around the contract's limits on a canvas of out_w x out_h (powers of two, so that the sums are exact)."""
    up, down = lambda v: float(np.nextafter(F(v), F(np.inf))), lambda v: float(np.nextafter(F(v), F(-np.inf)))
    cases = []
    # W falls from m22 = 1 to 1 - a out_w at the right-hand corners; S = a out_w + 1: min W = S / 16 at a out_w = 15 / 17
    a = 15.0 / 17.0 / out_w
    cases += [((-down(a), 0, 1), True), ((-up(a) * 1.000001, 0, 1), False), ((0, -down(a * out_w / out_h), 1), True),
              ((0, -up(a * out_w / out_h) * 1.000001, 1), False)]
    # ... rising instead: the minimum is m22 at (0, 0), S = 16 m22 at a out_w = 15 m22
    cases += [((15.0 / out_w, 0, 1), True), ((up(15.0 / out_w), 0, 1), False)]
    # S = 2^-30 on either side (a constant denominator: min W = S)
    cases += [((0, 0, 2.0 ** -30), True), ((0, 0, down(2.0 ** -30)), False), ((0, 0, 0), False), ((0, 0, 2.0 ** 30), True)]
    # a corner with W <= 0: the horizon on the canvas, or the whole canvas behind it
    cases += [((-1.0 / out_w, 0, 1), False), ((-2.0 / out_w, -2.0 / out_h, 1), False), ((0, 0, -1), False), ((0.01, 0.01, -0.001), False)]
    return cases


def test_the_conditioning_check_on_either_side_of_its_limits():
    L = c_layout(100, 60, FUSED["420"])
    for out in ((16, 16), (64, 32)):
        for row2, ok in row2_cases(*out):
            m = np.array(IDENT[:6] + list(row2), F)
            assert P.accepted(m, *out) == ok, (out, row2)                      # the restatement agrees on which side each lies
            assert (c_project_view(L, 1, m, *out)[0] == OK) == ok, (out, row2)


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_batch_calls_refuse(form):
    # a call that is right reaches the context, which is NULL -- so that every EINVAL below is told from it by the mixed calls'
    # views (below) and by jpeg_amd_project_view (above), which run the same check
    assert batch_call(form) == EINVAL
    for k in range(9):
        for bad in (np.nan, np.inf, F(2.0 ** 30) * F(1.0000002)):
            assert batch_call(form, with_entry(k, bad)) == EINVAL
    for row2, ok in row2_cases(8, 8):
        assert batch_call(form, with_row2(row2)) == EINVAL
    assert batch_call(form, edge=2) == EINVAL and batch_call(form, edge=-1) == EINVAL
    assert batch_call(form, matrices=None) == EINVAL and batch_call(form, warp=False) == EINVAL
    assert batch_call(form, size=(2 ** 24 + 1, 1), src_stride=2 ** 40) == EINVAL            # (float)w would not be exact
    for out in ((0, 8), (8, 0), (2 ** 30 + 1, 8)):
        assert batch_call(form, out=out) == EINVAL
    assert batch_call(form, dst=None) == EINVAL and batch_call(form, n=-1) == EINVAL and batch_call(form, n=65536) == EINVAL
    assert batch_call(form, src_stride=5) == EINVAL
    if form == "tensor":
        assert batch_call(form, spec=False) == EINVAL and batch_call(form, dst=PTR + 2) == EINVAL
        k = np.zeros((N, 12), F)
        bad = _lib.Colour()
        bad.h_matrices, bad.lo, bad.hi = k.ctypes.data, 1.0, 0.0
        assert batch_call(form, colour=C.byref(bad)) == EINVAL


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_mixed_calls_judge_everything_before_the_context(form):
    unset = (-7, -7, -7, -7, -7)
    whole = (1, 0, 0, 10, 10)               # an 8 x 8 canvas through the identity: columns and rows 0 .. 9 of 20 x 10
    assert mixed_call(form, n=0)[0] == OK
    st, views, mout = mixed_call(form)
    assert st == EINVAL and views == [whole, whole] and np.array_equal(mout, np.array([IDENT, IDENT], F))
    assert mixed_call(form, n=0, edge=2)[0] == EINVAL and mixed_call(form, n=0, warp=False)[0] == EINVAL
    assert mixed_call(form, n=0, out=(0, 8))[0] == EINVAL
    if form == "tensor":
        assert mixed_call(form, n=0, spec=False)[0] == EINVAL
    assert mixed_call(form, n=0, matrices=None)[0] == OK and mixed_call(form, matrices=None)[0] == EINVAL
    # a matrix the contract refuses, in image 1: image 0's view is written, image 1's is not (h_views_out shows how far)
    for k in range(9):
        for bad in (np.nan, -np.inf, -F(2.0 ** 30) * F(1.0000002)):
            st, views, _ = mixed_call(form, with_entry(k, bad))
            assert st == EINVAL and views == [whole, unset], (k, bad)
    for row2, ok in row2_cases(8, 8):
        st, views, _ = mixed_call(form, with_row2(row2))
        assert st == EINVAL and (views[1] != unset) == ok and views[0] == whole, row2
    st, views, _ = mixed_call(form, orient=[6, 9])
    assert st == EINVAL and views[1] == unset and views[0] == (1, 0, 0, 10, 10)
    assert mixed_call(form, n=-1)[0] == EINVAL and mixed_call(form, n=65536)[0] == EINVAL
    assert mixed_call(form, dst=None)[0] == EINVAL
    # what the mixed view decode refuses of an image (12 bits: ENOSUP) comes behind every image's matrix and in front of the target
    assert mixed_call(form, precisions=(8, 12))[0] == ENOSUP and mixed_call(form, precisions=(12, 8), out=(0, 8))[0] == EINVAL
    assert mixed_call(form, with_entry(0, np.nan), precisions=(8, 12))[0] == EINVAL
    assert mixed_call(form, precisions=(8, 12), edge=2)[0] == EINVAL and mixed_call(form, precisions=(12, 8), edge=2)[0] == ENOSUP
    # a reduction by 8 takes the view at denominator 8; a denominator row of (0, 0, 2) halves every step
    st, views, mout = mixed_call(form, [[8, 0, 0, 0, 8, 0, 0, 0, 1], [8, 0, 0, 0, 18, 0, 0, 0, 2]], size=(640, 640))
    assert st == EINVAL and views == [(8, 0, 0, 10, 10), (4, 0, 0, 10, 20)]
    assert np.array_equal(mout, np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], [2, 0, 0, 0, 4.5, 0, 0, 0, 2]], F))


def test_the_file_calls_take_each_view_from_project_view():
    """Pass 0 of the file calls needs no device: with a NULL context a call that is right gets as far as the context, and the
    views, matrices and orientations it has written by then are jpeg_amd_project_view's for each file's own size and tag."""
    datas = [FI.synthetic_file("420", (160, 120), 61)[0], E.insert(FI.synthetic_file("444", (53, 37), 62)[0], E.exif_segment(6, big=True)),
             FI.synthetic_file("y8", (37, 83), 63)[0]]
    sizes, tags = [(160, 120), (53, 37), (37, 83)], [1, 6, 1]
    out = (24, 16)
    rng = np.random.default_rng(127)
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    nbytes = (C.c_size_t * n)(*[d.size for d in datas])
    lib = _lib.lib()
    for orient, applied in (((C.c_uint8 * n)(0, 0, 0), tags), (None, [1, 1, 1]), ((C.c_uint8 * n)(3, 0, 8), [3, 6, 8])):
        mats = np.array([P.distortion(rng, *E.oriented_size(o, *s), out[0], out[1], 0.5, 0.1) for s, o in zip(sizes, applied)], F)
        for tensor in (False, True):
            infos, views = (_lib.FrameInfo * n)(), (_lib.View * n)()
            mout, oout = np.full((n, 9), -7, F), (C.c_int32 * n)(-7, -7, -7)
            wp = c_warp()
            head = (None, ptrs, nbytes, n, 1, 0, RGB, orient, mats.ctypes.data, C.byref(wp), out[0], out[1])
            if tensor:
                st = lib.jpeg_amd_decompress_tensor_projected_mixed(*head, C.byref(SPEC), None, None, PTR, 3 * out[0] * out[1], infos, views,
                                                                    mout.ctypes.data, oout)
            else:
                st = lib.jpeg_amd_decompress_resized_projected_mixed(*head, PTR, 3 * out[0] * out[1], infos, views, mout.ctypes.data, oout)
            assert st == EINVAL                                      # the context, last
            assert list(oout) == applied
            for i in range(n):
                want_view, want_m = P.project_view(sizes[i][0], sizes[i][1], applied[i], mats[i], *out)
                v = views[i]
                assert (v.denom, v.region.x, v.region.y, v.region.width, v.region.height) == want_view, (i, applied[i])
                assert np.array_equal(mout[i], want_m) and (infos[i].width, infos[i].height) == sizes[i]
    # a matrix that is refused in file 1: file 0 is written, the others are not; no files need no context
    bad = mats.copy()
    bad[1, 6:] = [-1.0 / out[0], 0, 1]
    views, wp = (_lib.View * n)(*[_lib.View(-7, _lib.Region(-7, -7, -7, -7))] * n), c_warp()
    st = lib.jpeg_amd_decompress_resized_projected_mixed(None, ptrs, nbytes, n, 1, 0, RGB, None, bad.ctypes.data, C.byref(wp), out[0], out[1],
                                                         PTR, 3 * out[0] * out[1], None, views, None, None)
    assert st == EINVAL and views[0].denom > 0 and views[1].denom == -7 and views[2].denom == -7
    assert lib.jpeg_amd_decompress_resized_projected_mixed(None, ptrs, nbytes, 0, 1, 0, RGB, None, None, C.byref(wp), out[0], out[1], None, 0,
                                                           None, None, None, None) == OK
    assert lib.jpeg_amd_decompress_resized_projected_mixed(None, ptrs, nbytes, n, 1, 0, RGB, None, None, C.byref(wp), out[0], out[1], PTR,
                                                           3 * out[0] * out[1], None, None, None, None) == EINVAL


# ---- perspective_matrix -------------------------------------------------------------------------------------------------------------

def test_perspective_matrix():
    rng = np.random.default_rng(131)
    for case in range(200):
        w, h, out_w, out_h = (float(v) for v in rng.integers(8, 3000, 4))
        src = [(rng.uniform(-0.2, 0.25) * w, rng.uniform(-0.2, 0.25) * h), (w - rng.uniform(-0.2, 0.25) * w, rng.uniform(-0.2, 0.25) * h),
               (w - rng.uniform(-0.2, 0.25) * w, h - rng.uniform(-0.2, 0.25) * h), (rng.uniform(-0.2, 0.25) * w, h - rng.uniform(-0.2, 0.25) * h)]
        out = [(0, 0), (out_w, 0), (out_w, out_h), (0, out_h)]
        m = perspective_matrix(src, out)
        assert m.dtype == np.float64 and m.shape == (3, 3) and m[2, 2] == 1.0
        for (x, y), (u, v) in zip(out, src):
            p = m @ np.array([x, y, 1.0])
            assert abs(p[0] / p[2] - u) <= 1e-9 * max(w, h) and abs(p[1] / p[2] - v) <= 1e-9 * max(w, h), (case, x, y)
    # two axis-aligned rectangles: exactly (sx, 0, x0, 0, sy, y0, 0, 0, 1), in either corner order
    for case in range(100):
        x0, y0, rw, rh, out_w, out_h = (int(v) for v in rng.integers(1, 3000, 6))
        want = [rw / out_w, 0, x0, 0, rh / out_h, y0, 0, 0, 1]
        src = [(x0, y0), (x0 + rw, y0), (x0 + rw, y0 + rh), (x0, y0 + rh)]
        out = [(0, 0), (out_w, 0), (out_w, out_h), (0, out_h)]
        assert perspective_matrix(src, out).reshape(9).tolist() == want
        swap = [0, 1, 3, 2]
        assert perspective_matrix([src[k] for k in swap], [out[k] for k in swap]).reshape(9).tolist() == want
    for bad in ([(0, 0), (1, 1), (2, 2), (0, 5)], [(0, 0), (0, 0), (4, 4), (0, 4)]):      # three on a line; a repeated point
        with pytest.raises(ValueError):
            perspective_matrix([(0, 0), (9, 1), (8, 7), (1, 9)], bad)
    with pytest.raises(ValueError):
        perspective_matrix([(0, 0), (1, 0), (1, 1)], [(0, 0), (1, 0), (1, 1)])
