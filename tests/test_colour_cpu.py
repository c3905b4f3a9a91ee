"""The colour stage without a device (include/jpeg_amd.h, "colour stage"): the numpy mirror of the contract (_colour_ref)
against the consequences the header names and against the same expression in float64; colour_matrix; and what the six
*_colour_* entry points refuse, through a NULL context -- a call that is right gets as far as the context and is refused there,
so the refusals are told apart from it where a call can end without one: a mixed or file call of no images is OK, and the tap
limit (ENOSUP) and an image of 12 bits (ENOSUP) are judged behind the target and in front of the context.  Two routes have no
such status in between -- jpeg_amd_warp_colour_tensor_batch, and the warped file call with files -- so there a refused colour and
a right one both end in EINVAL and the test shows no more than that a refused colour is not let through; what tells the two
apart for the warp records is the warped mixed call and the calls of no images, which run the same ResampleTarget::check().

A colour on a BYTE target, which no public call can ask for, is forced through the internal routes that take a colour and a
`tensor` flag side by side, by a stand-alone program (tests/cpp/colour_byte_target_test.cpp)."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import _colour_ref as K
import _files as FI
import _tensor_ref as T
import jpeg_amd as J
from _calls import c_layout
from jpeg_amd import _lib

F = np.float32
OK, EINVAL, ENOSUP = 0, -1, -5
PTR = 0x1000                                 # a device pointer that is never followed
RGB = _lib.COLOR_RGB8
N = 2


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(5).integers(0, 256, (37, 70, 3), dtype=np.uint8)


# ---- the mirror -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", T.DTYPES, ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("layout", T.LAYOUTS, ids=["hwc", "chw"])
def test_identity_is_the_tensor_output(image, dtype, layout):
    for spec in (T.Spec(dtype, layout), T.Spec(dtype, layout, *T.SIGNED_ZERO)):
        for flip in (0, 1):
            got = K.normalise(image, K.IDENTITY, K.NO_CLAMP, spec, flip)
            want = T.normalise(image, spec, flip)
            assert got.dtype == want.dtype and np.array_equal(got, want)


def test_permutations_permute_the_channels(image):
    spec = T.Spec(T.F32, T.HWC)
    for order in itertools.permutations(range(3)):
        got = K.normalise(image, K.permutation(order), K.NO_CLAMP, spec, 1)
        assert np.array_equal(got, T.normalise(np.ascontiguousarray(image[..., list(order)]), spec, 1)), order


def test_equal_rows_give_equal_channels(image):
    k = K.matrix([[0.2989, 0.587, 0.114, 3.5]] * 3)
    q = K.mapped(image, k, (0, 255))
    assert np.array_equal(q[..., 0], q[..., 1]) and np.array_equal(q[..., 0], q[..., 2])
    bits = K.convert(q, T.Spec(T.F16, T.CHW, mean=(100.0,) * 3, scale=(0.02,) * 3))
    assert np.array_equal(bits[0], bits[1]) and np.array_equal(bits[0], bits[2])


def test_the_mirror_against_float64():
    """Four roundings -- two sums of products, the third product's sum and the offset's -- of sub-results that are no larger
    than S = |k0| r + |k1| g + |k2| b + |k3|, and three rounded products inside them: the products' errors are at most
    2^-24 of their own size, which S bounds in sum, and each of the three additions adds at most 2^-24 S.  4 * 2^-24 * S."""
    rng = np.random.default_rng(2024)
    points = rng.integers(0, 256, (1, 100000, 3), dtype=np.uint8)          # 10^5 of the 2^24 byte triples
    rgb = points.astype(np.float64)
    worst = 0.0
    for _ in range(200):
        k = np.concatenate([rng.uniform(-4, 4, (3, 3)), rng.uniform(-300, 300, (3, 1))], axis=1).astype(F)
        q = K.mapped(points, k).astype(np.float64)
        kd = k.astype(np.float64)
        exact = rgb @ kd[:, :3].T + kd[:, 3]
        bound = 4.0 * 2.0 ** -24 * (rgb @ np.abs(kd[:, :3]).T + np.abs(kd[:, 3]))
        assert (np.abs(q - exact) <= bound).all()
        worst = max(worst, float((np.abs(q - exact) / bound).max()))
    assert 0.0 < worst <= 1.0


def test_the_clamp(image):
    bright = K.matrix([[3, 0, 0, 40], [0, 3, 0, 40], [0, 0, 3, 40]])
    dark = K.matrix([[-1, -0.5, 0, 20], [0.25, -2, 0, 0], [0, 0, -1, 255]])
    for k in (bright, dark):
        free = K.mapped(image, k)
        assert free.min() < 0 or free.max() > 255
        for lo, hi in ((0, 255), (16, 235), (-50, 1000)):
            q = K.mapped(image, k, (lo, hi))
            assert np.array_equal(q, np.clip(free, F(lo), F(hi))) and q.min() >= lo and q.max() <= hi
        assert np.array_equal(K.mapped(image, k, (-np.inf, np.inf)), free)
        assert np.array_equal(K.mapped(image, k, (-np.inf, 255)), np.minimum(free, F(255)))
        assert np.array_equal(K.mapped(image, k, (0, np.inf)), np.maximum(free, F(0)))
    assert K.mapped(image, bright, (0, 255)).max() == 255 and K.mapped(image, dark, (0, 255)).min() == 0
    # -0 is not below +0: it stays, and shows where the mean is 0
    zero = np.zeros((1, 1, 3), np.uint8)
    q = K.mapped(zero, K.matrix([[-1, -1, -1, -0.0], [1, 0, 0, 0], [0, 0, 0, 0]]), (0, 255))
    assert np.signbit(q[0, 0, 0]) and not np.signbit(q[0, 0, 1])
    bits = K.convert(q, T.Spec(T.F32, T.HWC, mean=(0, 0, 0), scale=(1, 1, 1)))
    assert bits[0, 0].tolist() == [0x80000000, 0, 0]


# ---- colour_matrix --------------------------------------------------------------------------------------------------------------------

def apply64(m, x):
    """float32 [3, 4] on float64 pixels [..., 3]."""
    m = np.asarray(m, np.float64)
    return x @ m[:, :3].T + m[:, 3]


def test_colour_matrix_defaults_and_shapes():
    m = J.colour_matrix()
    assert m.dtype == F and m.shape == (3, 4) and m.flags["C_CONTIGUOUS"]
    assert np.array_equal(m.view(np.uint32), K.IDENTITY.view(np.uint32))              # exactly, +0 everywhere else
    assert np.array_equal(J.colour_matrix(saturation=0.0), J.colour_matrix(grey=True))
    assert np.array_equal(J.colour_matrix(1.3, 0.8, 0.0, 0.2), J.colour_matrix(1.3, 0.8, 0.0, 0.2, grey=False))
    assert np.abs(J.colour_matrix(hue=1.0) - K.IDENTITY).max() <= 1e-6
    assert np.abs(J.colour_matrix(hue=0.25) - K.IDENTITY).max() > 0.1
    assert np.array_equal(J.colour_matrix(order="bgr"), K.permutation((2, 1, 0)))
    full = J.colour_matrix(1.4, 0.7, 1.8, 0.1)
    assert np.array_equal(J.colour_matrix(1.4, 0.7, 1.8, 0.1, order="bgr"), full[::-1])
    grey = J.colour_matrix(1.4, 0.7, 1.8, 0.1, grey=True)
    assert np.array_equal(grey[0], grey[1]) and np.array_equal(grey[0], grey[2])
    with pytest.raises(ValueError):
        J.colour_matrix(order="gbr")


def test_colour_matrix_against_the_operations_in_torch():
    import torch
    x = torch.rand((64, 48, 3), dtype=torch.float64, generator=torch.Generator().manual_seed(3)) * 255.0
    w = torch.tensor([0.2989, 0.587, 0.114], dtype=torch.float64)
    tol = 1e-4 * 255.0
    for b in (0.0, 0.6, 1.0, 1.7):
        assert (torch.from_numpy(apply64(J.colour_matrix(brightness=b), x.numpy())) - x * b).abs().max() <= tol
    for s in (0.0, 0.3, 1.0, 1.8):
        want = s * x + (1.0 - s) * (x * w).sum(-1, keepdim=True)                   # adjust_saturation's blend, before its clamp
        assert (torch.from_numpy(apply64(J.colour_matrix(saturation=s), x.numpy())) - want).abs().max() <= tol
    for c, pivot in ((0.5, 128.0), (1.5, 97.25)):
        want = c * x + (1.0 - c) * pivot
        assert (torch.from_numpy(apply64(J.colour_matrix(contrast=c, pivot=pivot), x.numpy())) - want).abs().max() <= tol
    # B . C . S . H: the hue first, the brightness last
    want = apply64(J.colour_matrix(brightness=1.4), apply64(J.colour_matrix(contrast=0.7), apply64(
        J.colour_matrix(saturation=1.8), apply64(J.colour_matrix(hue=0.1), x.numpy()))))
    assert np.abs(apply64(J.colour_matrix(1.4, 0.7, 1.8, 0.1), x.numpy()) - want).max() <= tol
    # a hue rotation leaves the luma of YIQ alone and is a rotation: four quarter turns are the identity
    y = np.array([0.299, 0.587, 0.114])
    h = J.colour_matrix(hue=0.1).astype(np.float64)
    assert np.abs(y @ h[:, :3] - y).max() <= 1e-6 and np.abs(h[:, 3]).max() == 0
    q = J.colour_matrix(hue=0.25).astype(np.float64)[:, :3]
    assert np.abs(np.linalg.matrix_power(q, 4) - np.eye(3)).max() <= 1e-5


# ---- the entry points -----------------------------------------------------------------------------------------------------------------

SPEC = _lib.TensorSpec(_lib.F32, _lib.TENSOR_CHW, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
GOOD = np.stack([K.IDENTITY, K.permutation((2, 1, 0))])


def c_colour(k=GOOD, clamp=(0.0, 255.0)):
    """-> (keep, struct jpeg_amd_colour); k None: a null matrix array."""
    keep = None if k is None else np.ascontiguousarray(k, F).reshape(-1, 12)
    c = _lib.Colour()
    c.h_matrices, c.lo, c.hi = (None if keep is None else keep.ctypes.data), clamp[0], clamp[1]
    return keep, c


def bad_colours():
    """Every colour the contract refuses for a call of N images."""
    out = []
    for image, k in ((0, 0), (1, 11), (1, 5)):
        for bad in (np.nan, np.inf, -np.inf, 2.0 ** 31, -(2.0 ** 31), F(2.0 ** 30) * F(1.0000002)):
            m = GOOD.copy().reshape(N, 12)
            m[image, k] = bad
            out.append((("entry", image, k, bad), c_colour(m)))
    out.append(("lo > hi", c_colour(clamp=(1.0, 0.5))))
    out.append(("lo NaN", c_colour(clamp=(np.nan, 255.0))))
    out.append(("hi NaN", c_colour(clamp=(0.0, np.nan))))
    out.append(("both NaN", c_colour(clamp=(np.nan, np.nan))))
    out.append(("null matrices", c_colour(None)))
    return out


def good_colours():
    edge = GOOD.copy().reshape(N, 12)
    edge[1, 3], edge[0, 4] = 2.0 ** 30, -(2.0 ** 30)                            # the limit itself is taken
    return [c_colour(), c_colour(clamp=(-np.inf, np.inf)), c_colour(clamp=(7.0, 7.0)), c_colour(edge)]


def resize_call(colour, n=N, size=(20, 10), out=(8, 8), filter=_lib.FILTER_BILINEAR, dst=PTR, spec=True):
    ext = (_lib.Extent * N)(*[_lib.Extent(*size)] * N)
    head = (None, n, PTR, 3 * size[0] * size[1], ext, out[0], out[1], filter, C.byref(SPEC) if spec else None, None, None, None, None)
    if colour is False:
        return _lib.lib().jpeg_amd_resize_placed_tensor_batch(*head, dst, 3 * out[0] * out[1])
    return _lib.lib().jpeg_amd_resize_colour_tensor_batch(*head, None if colour is None else C.byref(colour), dst, 3 * out[0] * out[1])


def images(size, precisions):
    arr = (_lib.Image * N)()
    for i in range(N):
        arr[i].layout = c_layout(size[0], size[1], [(1, 1)] * 3, precision=precisions[i])
        for c in range(3):
            arr[i].d_coef[c] = PTR
        arr[i].d_quanta, arr[i].ntables = PTR, 2
    return arr


def mixed_call(colour, n=N, size=(20, 10), out=(8, 8), filter=_lib.FILTER_BILINEAR, dst=PTR, precisions=(8, 8)):
    views = (_lib.View * N)(*[_lib.View(1, _lib.Region(0, 0, size[0], size[1]))] * N)
    head = (None, n, images(size, precisions), 0, RGB, views, out[0], out[1], filter, C.byref(SPEC), None, None, None, None)
    if colour is False:
        return _lib.lib().jpeg_amd_decode_tensor_placed_mixed(*head, dst, 3 * out[0] * out[1])
    return _lib.lib().jpeg_amd_decode_tensor_colour_mixed(*head, None if colour is None else C.byref(colour), dst, 3 * out[0] * out[1])


IDENT6 = np.array([[1, 0, 0, 0, 1, 0]] * N, F)


def c_warp(edge=0):
    w = _lib.Warp()
    w.edge = edge
    return w


def warp_call(colour, n=N, size=(20, 10), out=(8, 8), edge=0, dst=PTR):
    ext = (_lib.Extent * N)(*[_lib.Extent(*size)] * N)
    wp = c_warp(edge)
    head = (None, n, PTR, 3 * size[0] * size[1], ext, IDENT6.ctypes.data, C.byref(wp), out[0], out[1], C.byref(SPEC), None)
    if colour is False:
        return _lib.lib().jpeg_amd_warp_tensor_batch(*head, dst, 3 * out[0] * out[1])
    return _lib.lib().jpeg_amd_warp_colour_tensor_batch(*head, None if colour is None else C.byref(colour), dst, 3 * out[0] * out[1])


def warped_mixed_call(colour, n=N, size=(20, 10), out=(8, 8), edge=0, dst=PTR, precisions=(8, 8)):
    wp = c_warp(edge)
    head = (None, n, images(size, precisions), 0, RGB, None, IDENT6.ctypes.data, C.byref(wp), out[0], out[1], C.byref(SPEC), None, None,
            None)
    if colour is False:
        return _lib.lib().jpeg_amd_decode_tensor_warped_mixed(*head, dst, 3 * out[0] * out[1])
    return _lib.lib().jpeg_amd_decode_tensor_warped_colour_mixed(*head, None if colour is None else C.byref(colour), dst,
                                                                 3 * out[0] * out[1])


@pytest.fixture(scope="module")
def files():
    datas = [FI.synthetic_file("420", (160, 120), 61)[0], FI.synthetic_file("444", (53, 37), 62)[0]]
    return datas, (C.c_void_p * N)(*[d.ctypes.data for d in datas]), (C.c_size_t * N)(*[d.size for d in datas])


def file_call(files, colour, n=N, out=(8, 8), filter=_lib.FILTER_BILINEAR, dst=PTR, warped=False):
    _, ptrs, nbytes = files
    wp = c_warp()
    tail = (dst, 3 * out[0] * out[1], None, None)
    if warped:
        head = (None, ptrs, nbytes, n, 1, 0, RGB, None, IDENT6.ctypes.data, C.byref(wp), out[0], out[1], C.byref(SPEC), None)
        if colour is False:
            return _lib.lib().jpeg_amd_decompress_tensor_warped_mixed(*head, *tail, None, None)
        return _lib.lib().jpeg_amd_decompress_tensor_warped_colour_mixed(*head, None if colour is None else C.byref(colour), *tail, None, None)
    head = (None, ptrs, nbytes, n, 1, 0, RGB, None, out[0], out[1], filter, C.byref(SPEC), None, None, None, None)
    if colour is False:
        return _lib.lib().jpeg_amd_decompress_tensor_placed_mixed(*head, *tail, None)
    return _lib.lib().jpeg_amd_decompress_tensor_colour_mixed(*head, None if colour is None else C.byref(colour), *tail, None)


AA = _lib.FILTER_ANTIALIAS


def test_the_calls_refuse_a_colour_with_the_target_and_the_context_last(files):
    """Behind the target stand the tap limit (the placed forms: 400 x 400 to 8 x 8 through the antialiasing filter is a scale of
    50) and, in the mixed calls, the second image (12 bits): both ENOSUP, both without a context.  A colour that is right lets
    the call reach them; one that is refused is EINVAL in front of them."""
    big = dict(size=(400, 400), filter=AA)
    for keep, c in good_colours():
        assert resize_call(c, **big) == ENOSUP and mixed_call(c, **big) == ENOSUP
        assert mixed_call(c, precisions=(8, 12)) == ENOSUP and warped_mixed_call(c, precisions=(8, 12)) == ENOSUP
        assert file_call(files, c, out=(1, 1), filter=AA) == ENOSUP                 # 160 x 120 at 1/8 is 20 x 15: a scale of 20
        # ... and a call that is right altogether reaches the context, which is NULL
        for st in (resize_call(c), mixed_call(c), warp_call(c), warped_mixed_call(c), file_call(files, c), file_call(files, c, warped=True)):
            assert st == EINVAL
        # no images: the mixed and the file calls need no context
        assert mixed_call(c, n=0) == OK and warped_mixed_call(c, n=0) == OK
        assert file_call(files, c, n=0) == OK and file_call(files, c, n=0, warped=True) == OK
    for what, (keep, c) in bad_colours():
        assert resize_call(c, **big) == EINVAL and mixed_call(c, **big) == EINVAL, what
        assert mixed_call(c, precisions=(8, 12)) == EINVAL and warped_mixed_call(c, precisions=(8, 12)) == EINVAL, what
        assert file_call(files, c, out=(1, 1), filter=AA) == EINVAL, what
        assert warp_call(c) == EINVAL and file_call(files, c, warped=True) == EINVAL, what
    # the clamp is judged for a call of no images too; its matrices are not looked at
    for clamp in ((1.0, 0.5), (np.nan, 255.0), (0.0, np.nan)):
        keep, c = c_colour(clamp=clamp)
        assert mixed_call(c, n=0) == EINVAL and warped_mixed_call(c, n=0) == EINVAL
        assert file_call(files, c, n=0) == EINVAL and file_call(files, c, n=0, warped=True) == EINVAL
    keep, c = c_colour(None)
    assert mixed_call(c, n=0) == OK and file_call(files, c, n=0) == OK
    # the target in front of the colour: a refused image 0 of a mixed call comes first
    keep, c = c_colour(clamp=(1.0, 0.5))
    assert mixed_call(c, precisions=(12, 8)) == ENOSUP


def test_a_null_colour_is_the_named_call(files):
    calls = [
        (resize_call, [dict(), dict(size=(400, 400), filter=AA), dict(out=(0, 8)), dict(n=-1), dict(n=65536), dict(dst=None), dict(filter=2),
                       dict(spec=False), dict(dst=PTR + 2), dict(size=(200, 200), filter=_lib.FILTER_BICUBIC)]),
        (mixed_call, [dict(), dict(n=0), dict(size=(400, 400), filter=AA), dict(precisions=(8, 12)), dict(precisions=(12, 8), out=(0, 8)),
                      dict(out=(8, 0)), dict(dst=None), dict(n=-1), dict(filter=7)]),
        (warp_call, [dict(), dict(edge=2), dict(out=(0, 8)), dict(dst=None), dict(n=65536), dict(size=(2 ** 24 + 1, 1))]),
        (warped_mixed_call, [dict(), dict(n=0), dict(edge=2), dict(n=0, edge=2), dict(precisions=(8, 12)), dict(precisions=(12, 8), edge=2),
                             dict(dst=None), dict(out=(2 ** 30 + 1, 8))]),
    ]
    seen = set()
    for call, cases in calls:
        for kw in cases:
            st = call(None, **kw)
            assert st == call(False, **kw), (call.__name__, kw)
            seen.add(st)
    for kw in (dict(), dict(n=0), dict(out=(1, 1), filter=AA), dict(out=(0, 8)), dict(dst=None), dict(n=0, out=(0, 8)),
               dict(warped=True), dict(warped=True, n=0), dict(warped=True, out=(0, 8))):
        st = file_call(files, None, **kw)
        assert st == file_call(files, False, **kw), kw
        seen.add(st)
    assert seen == {OK, EINVAL, ENOSUP}


def test_a_colour_forced_through_a_byte_target_is_refused(tmp_path):
    """tests/cpp/colour_byte_target_test.cpp lists the assertions: check_resampled_mixed and decode_views_mixed with a request
    (csrc/resample_request.hpp) of a valid colour and a byte target give EINVAL, for no images and for two, without a map and
    through either map; without the colour, or to a tensor, the same request is judged to the end (OK, and ENOSUP past the
    tap limit)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "colour_byte_target_test")
    libdir = os.path.join(root, "jpeg_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           "-I", os.path.join(root, "jpeg_amd", "csrc"),
                           os.path.join(root, "tests", "cpp", "colour_byte_target_test.cpp"), "-o", exe,
                           "-L", libdir, "-ljpeg_amd", "-Wl,-rpath," + libdir])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), (r.stdout[-800:], r.stderr[-2000:])
