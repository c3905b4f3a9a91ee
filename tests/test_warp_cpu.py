"""The warped resample (include/jpeg_amd.h, "warped resample") without a GPU: the numpy mirror of the contract (_warp_ref)
against the points where the contract ties into what exists -- the bilinear resize, bit for bit, and torch's grid_sample,
within one level -- jpeg_amd_warp_view against its Python restatement, the view route on matrices whose arithmetic is exact,
what the calls refuse with a NULL context, and affine_matrix."""
import ctypes as C
import math

import numpy as np
import pytest

import _files as FI
import _orient as E
import _resize_ref as R
import _warp_ref as W
from _calls import FUSED, c_layout
from jpeg_amd import _lib
from jpeg_amd.api import affine_matrix

OK, EINVAL, ENOSUP = 0, -1, -5
F = np.float32
RGB = _lib.COLOR_RGB8
EDGES = (W.FILL, W.REPLICATE)
FILLB = (7, 130, 255)


def image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def scale_matrix(w, h, out_w, out_h):
    return np.array([F(w) / F(out_w), 0, 0, 0, F(h) / F(out_h), 0], F)


# ---- the mirror against the contract's consequences ---------------------------------------------------------------------------------

def test_scale_matrix_with_replicate_is_the_bilinear_resize():
    rng = np.random.default_rng(11)
    for case in range(200):
        w, h, out_w, out_h = (int(v) for v in rng.integers(1, 91, 4))
        src = image(w, h, 1000 + case)
        got = W.warp(src, scale_matrix(w, h, out_w, out_h), out_w, out_h, W.REPLICATE)
        assert np.array_equal(got, R.resize(src, out_w, out_h)), (w, h, out_w, out_h)


def test_identity_integer_shifts_and_the_quarter_turn():
    src = image(23, 17, 5)
    h, w = src.shape[:2]
    for edge in EDGES:
        assert np.array_equal(W.warp(src, [1, 0, 0, 0, 1, 0], w, h, edge, FILLB), src)
    for dx, dy in ((3, 0), (0, -2), (-5, 4), (30, 0), (0, -20)):
        # output pixel (x, y) shows source pixel (x + dx, y + dy): shifted bytes, and the fill where that lies outside
        want = np.empty_like(src)
        want[:, :] = np.asarray(FILLB, np.uint8)
        ys, xs = np.mgrid[0:h, 0:w]
        ok = (xs + dx >= 0) & (xs + dx < w) & (ys + dy >= 0) & (ys + dy < h)
        want[ok] = src[(ys + dy)[ok], (xs + dx)[ok]]
        assert np.array_equal(W.warp(src, [1, 0, dx, 0, 1, dy], w, h, W.FILL, FILLB), want), (dx, dy)
        rep = src[np.clip(ys + dy, 0, h - 1), np.clip(xs + dx, 0, w - 1)]
        assert np.array_equal(W.warp(src, [1, 0, dx, 0, 1, dy], w, h, W.REPLICATE), rep), (dx, dy)
    for edge in EDGES:   # clockwise by 90 degrees: np.rot90 with k = -1
        assert np.array_equal(W.warp(src, [0, 1, 0, -1, 0, h], h, w, edge, FILLB), np.rot90(src, -1))
        assert np.array_equal(W.warp(src, [0, -1, w, 1, 0, 0], h, w, edge, FILLB), np.rot90(src, 1))


def random_affine(rng, w, h, out_w, out_h):
    """A rotate / scale / shear matrix that takes the canvas centre to the source centre, as float32 [6]."""
    angle, scale, shear = rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 2.0), rng.uniform(-0.3, 0.3)
    lin = scale * np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]]) @ np.array([[1.0, shear], [0.0, 1.0]])
    t = np.array([w / 2.0, h / 2.0]) - lin @ np.array([out_w / 2.0, out_h / 2.0])
    return np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1]], np.float64).astype(F)


def test_the_mirror_is_within_one_level_of_grid_sample():
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(23)
    for mode, edge in (("zeros", W.FILL), ("border", W.REPLICATE)):
        differ = total = 0
        for case in range(60):
            w, h, out_w, out_h = (int(v) for v in rng.integers(3, 91, 4))
            src = image(w, h, 2000 + case)
            m = random_affine(rng, w, h, out_w, out_h)
            # theta: the pixel matrix between the two normalisations (X -> 2 X / n - 1), in double
            pix = np.array([[m[0], m[1], m[2]], [m[3], m[4], m[5]], [0, 0, 1]], np.float64)
            to_src = np.array([[2.0 / w, 0, -1], [0, 2.0 / h, -1], [0, 0, 1]])
            from_out = np.array([[out_w / 2.0, 0, out_w / 2.0], [0, out_h / 2.0, out_h / 2.0], [0, 0, 1]])
            theta = torch.from_numpy((to_src @ pix @ from_out)[:2].astype(np.float32))[None]
            grid = torch.nn.functional.affine_grid(theta, (1, 3, out_h, out_w), align_corners=False)
            ref = torch.nn.functional.grid_sample(torch.from_numpy(src.astype(np.float32).transpose(2, 0, 1))[None], grid, mode="bilinear",
                                                  padding_mode=mode, align_corners=False)[0].numpy().transpose(1, 2, 0)
            ref = np.floor(np.clip(ref, 0.0, 255.0) + 0.5).astype(np.int32)
            got = W.warp(src, m, out_w, out_h, edge, (0, 0, 0)).astype(np.int32)
            assert np.abs(got - ref).max() <= 1, (mode, case, w, h, out_w, out_h)
            differ += int((got != ref).sum())
            total += got.size
        print(f"{mode}: {differ} of {total} bytes differ from torch's rounded value ({100.0 * differ / total:.4f} %)")
        assert differ <= 0.01 * total, (mode, differ, total)


# ---- jpeg_amd_warp_view -------------------------------------------------------------------------------------------------------------

def c_warp_view(L, o, m, out_w, out_h):
    m = np.ascontiguousarray(m, F)
    v = _lib.View(-7, _lib.Region(-7, -7, -7, -7))
    mv = np.full(6, -7, F)
    st = _lib.lib().jpeg_amd_warp_view(C.byref(L), o, m.ctypes.data, out_w, out_h, C.byref(v), mv.ctypes.data)
    return st, (v.denom, v.region.x, v.region.y, v.region.width, v.region.height), mv


def check_view(w, h, o, m, out, what):
    L = c_layout(w, h, FUSED["420"])
    st, view, mv = c_warp_view(L, o, m, *out)
    want_view, want_mv = W.warp_view(w, h, o, m, *out)
    assert st == OK and view == want_view and np.array_equal(mv, want_mv), (what, w, h, o, list(m), out, view, want_view, mv, want_mv)
    ws, hs = W.scaled_size(w, h, view[0])
    assert view[3] >= 1 and view[4] >= 1 and view[1] >= 0 and view[2] >= 0 and view[1] + view[3] <= ws and view[2] + view[4] <= hs, what
    return view, mv


def test_warp_view_is_the_python_restatement():
    rng = np.random.default_rng(31)
    denoms = set()
    for case in range(2000):
        w, h = (int(v) for v in (rng.integers(1, 65536, 2) if case % 4 == 0 else rng.integers(1, 700, 2)))
        out = tuple(int(v) for v in rng.integers(1, 300, 2))
        angle, scale = rng.uniform(-math.pi, math.pi), math.exp(rng.uniform(math.log(0.2), math.log(20.0)))
        sq = rng.uniform(0.7, 1.4)
        lin = np.array([[math.cos(angle), -math.sin(angle)], [math.sin(angle), math.cos(angle)]]) @ np.diag([scale * sq, scale / sq])
        centre = np.array([rng.uniform(-0.3, 1.3) * w, rng.uniform(-0.3, 1.3) * h])     # of the upright image, more or less
        t = centre - lin @ np.array([out[0] / 2.0, out[1] / 2.0])
        m = np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1]], np.float64).astype(F)
        for o in range(1, 9):
            uw, uh = E.oriented_size(o, w, h)
            mo = m.copy()
            mo[2], mo[5] = F(m[2] * uw / w), F(m[5] * uh / h)
            view, _ = check_view(w, h, o, mo, out, case)
            denoms.add(view[0])
    assert denoms == {1, 2, 4, 8}


def test_warp_view_edges():
    w, h, out = 100, 60, (16, 16)
    # a footprint that misses the image entirely: a one-pixel view at the nearest corner or edge
    for m, want in (([1, 0, -500, 0, 1, -500], (1, 0, 0, 1, 1)), ([1, 0, 500, 0, 1, 500], (1, 99, 59, 1, 1)),
                    ([1, 0, 500, 0, 1, -500], (1, 99, 0, 1, 1)), ([1, 0, -500, 0, 1, 500], (1, 0, 59, 1, 1))):
        assert check_view(w, h, 1, np.array(m, F), out, "missed")[0] == want
    view, _ = check_view(w, h, 1, np.array([1, 0, 40, 0, 1, 500], F), out, "missed below")
    assert view == (1, 38, 59, 20, 1)
    # the denominator on both sides of d * d == min(...)
    for d in (2, 4, 8):
        below = np.nextafter(F(d), F(0))
        assert check_view(800, 800, 1, np.array([d, 0, 0, 0, d, 0], F), out, d)[0][0] == d
        assert check_view(800, 800, 1, np.array([below, 0, 0, 0, d, 0], F), out, d)[0][0] == d // 2
        assert check_view(800, 800, 1, np.array([d, 0, 0, 0, below, 0], F), out, d)[0][0] == d // 2
        assert check_view(800, 800, 1, np.array([0, d, 0, -d, 0, 800], F), out, d)[0][0] == d       # a quarter turn: the columns' norms
        assert check_view(800, 800, 1, np.array([d, 0, 0, 0, 100, 0], F), out, d)[0][0] == d         # the smaller column decides
    assert check_view(800, 800, 1, np.array([0.5, 0, 0, 0, 0.5, 0], F), out, "enlarging")[0][0] == 1
    # the view's corner at W' - 1, H' - 1, at every denominator (801 x 803: the scaled sizes round up)
    for d in (1, 2, 4, 8):
        ws, hs = W.scaled_size(801, 803, d)
        view, _ = check_view(801, 803, 1, np.array([d, 0, 801 - 16 * d, 0, d, 803 - 16 * d], F), out, ("corner", d))
        assert view[0] == d and view[1] + view[3] == ws and view[2] + view[4] == hs
    # the whole image is never exceeded by a canvas far larger than it
    assert check_view(5, 3, 1, np.array([1, 0, -50, 0, 1, -50], F), (200, 200), "larger")[0] == (1, 0, 0, 5, 3)


def test_warp_view_refuses():
    L = c_layout(100, 60, FUSED["420"])
    good = np.array([1, 0, 0, 0, 1, 0], F)
    unset = (-7, -7, -7, -7, -7)
    assert c_warp_view(L, 1, good, 16, 16)[0] == OK
    for o in (0, 9, -1):
        assert c_warp_view(L, o, good, 16, 16)[:2] == (EINVAL, unset)
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf, F(2.0 ** 30) * F(1.0000002), -F(2.0 ** 31)):
            m = good.copy()
            m[k] = bad
            assert c_warp_view(L, 1, m, 16, 16)[:2] == (EINVAL, unset), (k, bad)
        m = good.copy()
        m[k] = F(2.0 ** 30)                                                     # the limit itself is inside
        assert c_warp_view(L, 1, m, 16, 16)[0] == OK
    for out in ((0, 16), (16, 0), (2 ** 30 + 1, 16), (16, 2 ** 30 + 1)):
        assert c_warp_view(L, 1, good, *out)[:2] == (EINVAL, unset)
    assert c_warp_view(L, 1, good, 2 ** 30, 2 ** 30)[0] == OK
    lib = _lib.lib()
    v, mv = _lib.View(), np.zeros(6, F)
    assert lib.jpeg_amd_warp_view(None, 1, good.ctypes.data, 16, 16, C.byref(v), mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_warp_view(C.byref(L), 1, None, 16, 16, C.byref(v), mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_warp_view(C.byref(L), 1, good.ctypes.data, 16, 16, None, mv.ctypes.data) == EINVAL
    assert lib.jpeg_amd_warp_view(C.byref(L), 1, good.ctypes.data, 16, 16, C.byref(v), None) == EINVAL


# ---- the view route where every coordinate operation is exact -----------------------------------------------------------------------

def dyadic_case(rng):
    """A stored image of at most 200 a side, a canvas and an upright matrix of multiples of 1 / 256 whose linear part is at most 2
    in magnitude and which jpeg_amd_warp_view gives denominator 1."""
    w, h = (int(v) for v in rng.integers(1, 201, 2))
    out = tuple(int(v) for v in rng.integers(1, 60, 2))
    while True:
        lin = rng.integers(-512, 513, 4) / 256.0
        if min(lin[0] ** 2 + lin[2] ** 2, lin[1] ** 2 + lin[3] ** 2) < 4.0:
            break
    return w, h, out, lin


def test_the_view_route_is_the_whole_image_for_dyadic_matrices():
    rng = np.random.default_rng(41)
    cropped = 0
    for case in range(100):
        w, h, out, lin = dyadic_case(rng)
        src = image(w, h, 3000 + case)
        for o in range(1, 9):
            up = E.orient(src, o)
            uh, uw = up.shape[:2]
            # the canvas centre to a point inside or just outside the upright image
            t = np.rint(256 * (np.array([rng.uniform(-0.2, 1.2) * uw, rng.uniform(-0.2, 1.2) * uh])
                               - lin.reshape(2, 2) @ np.array([out[0] / 2.0, out[1] / 2.0]))) / 256.0
            m = np.array([lin[0], lin[1], t[0], lin[2], lin[3], t[1]], F)
            assert np.array_equal(m.astype(np.float64) * 256, np.rint(m.astype(np.float64) * 256))
            st, view, mv = c_warp_view(c_layout(w, h, FUSED["444"]), o, m, *out)
            assert st == OK and view[0] == 1, (case, o, view)
            crop = np.ascontiguousarray(src[view[2]:view[2] + view[4], view[1]:view[1] + view[3]])
            cropped += crop.size < src.size
            for edge in EDGES:
                want = W.warp(up, m, out[0], out[1], edge, FILLB)
                assert np.array_equal(W.warp(crop, mv, out[0], out[1], edge, FILLB), want), (case, o, edge, view, list(m))
                if o == 1:
                    assert np.array_equal(W.warp(src, m, out[0], out[1], edge, FILLB), want)
    assert cropped > 300           # most views are a part of their image


# ---- what the calls refuse, and in which order, with a NULL context -----------------------------------------------------------------

SPEC = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
BUF = np.zeros(16, np.uint16)
PTR = BUF.ctypes.data
N = 2
IDENT = [1, 0, 0, 0, 1, 0]


def c_warp(edge=W.FILL, fill=FILLB):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = fill
    return w


def batch_call(form, matrices=(IDENT, IDENT), warp=True, edge=W.FILL, n=N, size=(20, 10), out=(8, 8), dst=PTR, spec=True, src_stride=None):
    ext = (_lib.Extent * N)(*[_lib.Extent(*size)] * N)
    m = None if matrices is None else np.ascontiguousarray(matrices, F)
    wp = c_warp(edge)
    head = (None, n, PTR, 3 * size[0] * size[1] if src_stride is None else src_stride, ext, None if m is None else m.ctypes.data,
            C.byref(wp) if warp else None, out[0], out[1])
    if form == "bytes":
        return _lib.lib().jpeg_amd_warp_batch(*head, dst, 3 * out[0] * out[1])
    return _lib.lib().jpeg_amd_warp_tensor_batch(*head, C.byref(SPEC) if spec else None, None, dst, 3 * out[0] * out[1])


def mixed_call(form, matrices=(IDENT, IDENT), warp=True, edge=W.FILL, n=N, size=(20, 10), out=(8, 8), dst=PTR, spec=True, orient=None,
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
    mout = np.full((N, 6), -7, F)
    o = None if orient is None else (C.c_uint8 * N)(*orient)
    head = (None, n, images, 0, RGB, o, None if m is None else m.ctypes.data, C.byref(wp) if warp else None, out[0], out[1])
    if form == "bytes":
        st = _lib.lib().jpeg_amd_decode_warped_mixed(*head, views, mout.ctypes.data, dst, 3 * out[0] * out[1])
    else:
        st = _lib.lib().jpeg_amd_decode_tensor_warped_mixed(*head, C.byref(SPEC) if spec else None, None, views, mout.ctypes.data, dst,
                                                            3 * out[0] * out[1])
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views], mout


def with_entry(k, value, image=1):
    m = np.array([IDENT, IDENT], F)
    m[image, k] = value
    return m


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_batch_calls_refuse(form):
    # a call that is right reaches the context, which is NULL
    assert batch_call(form) == EINVAL
    for k in range(6):
        for bad in (np.nan, np.inf, F(2.0 ** 30) * F(1.0000002)):
            assert batch_call(form, with_entry(k, bad)) == EINVAL
    assert batch_call(form, edge=2) == EINVAL and batch_call(form, edge=-1) == EINVAL
    assert batch_call(form, matrices=None) == EINVAL and batch_call(form, warp=False) == EINVAL
    assert batch_call(form, size=(2 ** 24 + 1, 1), src_stride=2 ** 40) == EINVAL            # (float)w would not be exact
    # what the resize and the tensor checks refuse
    for out in ((0, 8), (8, 0), (2 ** 30 + 1, 8)):
        assert batch_call(form, out=out) == EINVAL
    assert batch_call(form, dst=None) == EINVAL and batch_call(form, n=-1) == EINVAL and batch_call(form, n=65536) == EINVAL
    assert batch_call(form, src_stride=5) == EINVAL
    if form == "tensor":
        assert batch_call(form, spec=False) == EINVAL and batch_call(form, dst=PTR + 2) == EINVAL


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_mixed_calls_judge_everything_before_the_context(form):
    unset = (-7, -7, -7, -7, -7)
    whole = (1, 0, 0, 10, 10)               # an 8 x 8 canvas through the identity: columns and rows 0 .. 9 of 20 x 10
    # nothing to do needs no context; a call with images that is right reaches it (NULL), its views written on the way
    assert mixed_call(form, n=0)[0] == OK
    st, views, mout = mixed_call(form)
    assert st == EINVAL and views == [whole, whole] and np.array_equal(mout, np.array([IDENT, IDENT], F))
    # ... so what is wrong with a call of no images is judged without one
    assert mixed_call(form, n=0, edge=2)[0] == EINVAL and mixed_call(form, n=0, warp=False)[0] == EINVAL
    assert mixed_call(form, n=0, out=(0, 8))[0] == EINVAL
    if form == "tensor":
        assert mixed_call(form, n=0, spec=False)[0] == EINVAL
    assert mixed_call(form, n=0, matrices=None)[0] == OK and mixed_call(form, matrices=None)[0] == EINVAL
    # a matrix the contract refuses, in image 1: image 0's view is written, image 1's is not
    for k in range(6):
        for bad in (np.nan, -np.inf, -F(2.0 ** 30) * F(1.0000002)):
            st, views, _ = mixed_call(form, with_entry(k, bad))
            assert st == EINVAL and views == [whole, unset], (k, bad)
    st, views, _ = mixed_call(form, orient=[6, 9])
    assert st == EINVAL and views[1] == unset and views[0] == (1, 0, 0, 10, 10)
    assert mixed_call(form, n=-1)[0] == EINVAL and mixed_call(form, n=65536)[0] == EINVAL
    assert mixed_call(form, dst=None)[0] == EINVAL
    # what the mixed view decode refuses of an image (12 bits: ENOSUP) comes behind every image's matrix and in front of the target
    assert mixed_call(form, precisions=(8, 12))[0] == ENOSUP and mixed_call(form, precisions=(12, 8), out=(0, 8))[0] == EINVAL
    assert mixed_call(form, with_entry(0, np.nan), precisions=(8, 12))[0] == EINVAL
    assert mixed_call(form, precisions=(8, 12), edge=2)[0] == EINVAL and mixed_call(form, precisions=(12, 8), edge=2)[0] == ENOSUP
    # a reduction by 8 takes the view at denominator 8
    st, views, mout = mixed_call(form, [[8, 0, 0, 0, 8, 0], [4, 0, 0, 0, 9, 0]], size=(640, 640))
    assert st == EINVAL and views == [(8, 0, 0, 10, 10), (4, 0, 0, 10, 20)]
    assert np.array_equal(mout, np.array([[1, 0, 0, 0, 1, 0], [1, 0, 0, 0, 2.25, 0]], F))


def test_the_file_calls_take_each_view_from_warp_view():
    """Pass 0 of the file calls needs no device: with a NULL context a call that is right gets as far as the context, and the
    views, matrices and orientations it has written by then are jpeg_amd_warp_view's for each file's own size and tag."""
    datas = [FI.synthetic_file("420", (160, 120), 61)[0], E.insert(FI.synthetic_file("444", (53, 37), 62)[0], E.exif_segment(6, big=True)),
             FI.synthetic_file("y8", (37, 83), 63)[0]]
    sizes, tags = [(160, 120), (53, 37), (37, 83)], [1, 6, 1]
    out = (24, 16)
    mats = np.array([affine_matrix(E.oriented_size(o, *s), out, angle=a, scale=sc) for s, o, a, sc in zip(sizes, tags, (20, -35, 90), (1.0, 0.9, 0.5))], F)
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    nbytes = (C.c_size_t * n)(*[d.size for d in datas])
    lib = _lib.lib()
    for orient, applied in (((C.c_uint8 * n)(0, 0, 0), tags), (None, [1, 1, 1]), ((C.c_uint8 * n)(3, 0, 8), [3, 6, 8])):
        for tensor in (False, True):
            infos, views = (_lib.FrameInfo * n)(), (_lib.View * n)()
            mout, oout = np.full((n, 6), -7, F), (C.c_int32 * n)(-7, -7, -7)
            wp = c_warp()
            head = (None, ptrs, nbytes, n, 1, 0, RGB, orient, mats.ctypes.data, C.byref(wp), out[0], out[1])
            if tensor:
                st = lib.jpeg_amd_decompress_tensor_warped_mixed(*head, C.byref(SPEC), None, PTR, 3 * out[0] * out[1], infos, views,
                                                                 mout.ctypes.data, oout)
            else:
                st = lib.jpeg_amd_decompress_resized_warped_mixed(*head, PTR, 3 * out[0] * out[1], infos, views, mout.ctypes.data, oout)
            assert st == EINVAL                                      # the context, last
            assert list(oout) == applied
            for i in range(n):
                want_view, want_m = W.warp_view(sizes[i][0], sizes[i][1], applied[i], mats[i], *out)
                v = views[i]
                assert (v.denom, v.region.x, v.region.y, v.region.width, v.region.height) == want_view, (i, applied[i])
                assert np.array_equal(mout[i], want_m) and (infos[i].width, infos[i].height) == sizes[i]
    # a matrix that is refused in file 1: file 0 is written, the others are not; no files need no context
    bad = mats.copy()
    bad[1, 2] = np.nan
    views, wp = (_lib.View * n)(*[_lib.View(-7, _lib.Region(-7, -7, -7, -7))] * n), c_warp()
    st = lib.jpeg_amd_decompress_resized_warped_mixed(None, ptrs, nbytes, n, 1, 0, RGB, None, bad.ctypes.data, C.byref(wp), out[0], out[1], PTR,
                                                      3 * out[0] * out[1], None, views, None, None)
    assert st == EINVAL and views[0].denom == 4 and views[1].denom == -7 and views[2].denom == -7      # (160 x 120 to 24 x 16: 1/4)
    assert lib.jpeg_amd_decompress_resized_warped_mixed(None, ptrs, nbytes, 0, 1, 0, RGB, None, None, C.byref(wp), out[0], out[1], None, 0,
                                                        None, None, None, None) == OK
    assert lib.jpeg_amd_decompress_resized_warped_mixed(None, ptrs, nbytes, n, 1, 0, RGB, None, None, C.byref(wp), out[0], out[1], PTR,
                                                        3 * out[0] * out[1], None, None, None, None) == EINVAL


# ---- affine_matrix ------------------------------------------------------------------------------------------------------------------

def test_affine_matrix():
    rng = np.random.default_rng(53)
    for case in range(200):
        w, h, out_w, out_h = (int(v) for v in rng.integers(1, 3000, 4))
        m = affine_matrix((w, h), (out_w, out_h))
        assert m.dtype == F and m.tolist() == scale_matrix(w, h, out_w, out_h).tolist(), (w, h, out_w, out_h)
        x0, y0 = int(rng.integers(0, w)), int(rng.integers(0, h))
        rw, rh = int(rng.integers(1, w - x0 + 1)), int(rng.integers(1, h - y0 + 1))
        m = affine_matrix((w, h), (out_w, out_h), source_region=(x0, y0, rw, rh))
        assert m.tolist() == [F(rw) / F(out_w), 0, x0, 0, F(rh) / F(out_h), y0], (w, h, out_w, out_h, x0, y0, rw, rh)
    # quarter turns of a square, counter-clockwise: exact entries, and the bytes are np.rot90's
    n = 37
    src = image(n, n, 9)
    for angle, want, turns in ((90, [0, -1, n, 1, 0, 0], 1), (-90, [0, 1, 0, -1, 0, n], -1), (180, [-1, 0, n, 0, -1, n], 2), (270, [0, 1, 0, -1, 0, n], 3),
                               (360, [1, 0, 0, 0, 1, 0], 0)):
        m = affine_matrix((n, n), (n, n), angle=angle)
        assert m.tolist() == want, (angle, m.tolist())
        assert np.array_equal(W.warp(src, m, n, n), np.rot90(src, turns))
    # scale enlarges the content (the inverse map shrinks), translate moves it by canvas pixels
    assert affine_matrix((64, 64), (64, 64), scale=2.0).tolist() == [0.5, 0, 16, 0, 0.5, 16]
    assert affine_matrix((64, 64), (64, 64), translate=(3, -5)).tolist() == [1, 0, -3, 0, 1, 5]
    # against torchvision's formulas (the inverse of RSS), restated: angle 30, shear (10, 5), scale 1.25, about the centre of 64 x 48
    a, sx, sy, sc = math.radians(-30.0), math.radians(10.0), math.radians(5.0), 1.25
    fwd = np.array([[math.cos(a - sy) / math.cos(sy), -math.cos(a - sy) * math.tan(sx) / math.cos(sy) - math.sin(a)],
                    [math.sin(a - sy) / math.cos(sy), -math.sin(a - sy) * math.tan(sx) / math.cos(sy) + math.cos(a)]]) * sc
    inv = np.linalg.inv(fwd)
    t = np.array([32.0, 24.0]) - inv @ np.array([32.0, 24.0])
    want = np.array([inv[0, 0], inv[0, 1], t[0], inv[1, 0], inv[1, 1], t[1]])
    got = affine_matrix((64, 48), (64, 48), angle=30.0, scale=sc, shear=(10.0, 5.0))
    assert np.allclose(got, want, rtol=0, atol=1e-5), (got, want)
    with pytest.raises(ValueError):
        affine_matrix((0, 4), (4, 4))
