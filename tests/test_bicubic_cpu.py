"""CPU checks of the bicubic filter (include/jpeg_amd.h, "bicubic resample"): the numpy checker the GPU tests compare with
(_bicubic_ref) against torch's antialiased bicubic interpolation, identity sizes, the taps and weights, the tap bound, and
the calls the entry points with a `filter` refuse before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _antialias_ref as A
import _bicubic_ref as B
import _files as F
from _calls import c_layout
from jpeg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ENOSUP = 0, -1, -5
BICUBIC, ANTIALIAS, BILINEAR = _lib.FILTER_BICUBIC, _lib.FILTER_ANTIALIAS, _lib.FILTER_BILINEAR

# (source w, h) -> (target w, h)
PAIRS = [((449, 301), (224, 224)), ((640, 480), (224, 224)), ((500, 375), (224, 224)), ((300, 500), (40, 63)),
         ((57, 131), (224, 224)), ((131, 57), (224, 224)), ((1792, 224), (224, 28)), ((24, 40), (3, 5)), ((200, 8), (25, 1)),
         ((1, 1), (5, 4)), ((3, 2), (1, 1)), ((5, 7), (40, 35)), ((17, 33), (17, 33))]


def _images(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    smooth = np.stack([(255 * xx) // max(w - 1, 1), (255 * yy) // max(h - 1, 1), (255 * (xx + yy)) // max(w + h - 2, 1)], axis=2)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "smooth": smooth.astype(np.uint8), "checker": checker}


def test_reference_is_within_one_level_of_torch_bicubic_antialias():
    """torch.nn.functional.interpolate(bicubic, antialias=True, align_corners=False), rounded half up, is the same filter
    (Keys, a = -0.5, widened by the scale factor, clipped and renormalised) in another operation order.  Both are binary32
    evaluations of one real expression whose error is far below half a level, so the worst difference is one level in every
    case; over the random and the smooth contents together at most 1 sample in 1 000 differs.  The checkerboard is exempt
    from the rate: where it is reduced its true values are ties, which either order may round either way."""
    torch = pytest.importorskip("torch")
    total = differ = 0
    for n, ((w, h), (wt, ht)) in enumerate(PAIRS):
        for name, image in _images(w, h, n).items():
            got = B.resize(image, wt, ht)
            t = torch.from_numpy(image).permute(2, 0, 1)[None].to(torch.float32)
            ref = torch.nn.functional.interpolate(t, size=(ht, wt), mode="bicubic", align_corners=False, antialias=True)
            ref = torch.floor(ref.clamp(0, 255) + 0.5)[0].permute(1, 2, 0).numpy().astype(np.uint8)
            diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
            print((w, h), (wt, ht), name, "worst", int(diff.max()), "differing", int((diff != 0).sum()), "of", diff.size)
            assert diff.max() <= 1, ((w, h), (wt, ht), name)
            if name != "checker":
                total += diff.size
                differ += int((diff != 0).sum())
    print("random and smooth contents: differing", differ, "of", total)
    assert differ * 1000 <= total


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (7, 9), (17, 33), (131, 57)])
def test_identity_size_returns_the_source(size):
    for image in _images(size[0], size[1], 7).values():
        assert (B.resize(image, size[0], size[1]) == image).all()


AXES = [(1, 1), (1, 9), (3, 1), (449, 224), (57, 224), (640, 224), (300, 40), (48, 6), (5, 4000), (80, 10), (1792, 224), (5, 40),
        (7, 35), (375, 224)]


def test_taps_stay_inside_the_source_and_the_weights_sum_to_one():
    for n, n_out in AXES:
        lo, count, W = B.axis_table(n_out, n)
        assert lo.min() >= 0 and (lo + count).max() <= n and count.min() >= 1, (n, n_out)
        assert (np.diff(lo) >= 0).all() and (np.diff(lo + count) >= 0).all()      # what the kernel's footprint relies on
        assert B.axis_total(n_out, n).min() > 0, (n, n_out)
        total = np.zeros(n_out, B.F)
        for i in range(W.shape[1]):
            total = total + W[:, i]
        assert np.abs(total - B.F(1.0)).max() <= 8 * np.finfo(B.F).eps, (n, n_out)
        if n > n_out >= 4:
            assert W.min() < 0, (n, n_out)                  # the lobes: what makes the clamp live
    assert B.axis_total(4000, 5).min() >= 0.5               # the least a clipped edge leaves


def test_the_weights_are_the_keys_cubic():
    u = np.array([0.0, 0.5, -0.5, 1.0, -1.0, 1.5, 2.0, 2.5, -3.0], B.F)
    assert B.weight(u).tolist() == [1.0, 0.5625, 0.5625, 0.0, 0.0, -0.0625, 0.0, 0.0, 0.0]


def test_the_tap_bound_holds_at_a_factor_of_eight():
    assert B.axis_table(10, 80)[1].max() == B.MAX_TAPS - 1 and B.axis_table(20, 160)[1].max() == B.MAX_TAPS - 1
    assert B.axis_table(224, 1792)[1].max() <= B.MAX_TAPS
    with pytest.raises(AssertionError):
        B.axis_table(10, 90)                                # k = 9: 37 taps


def _spec():
    return _lib.TensorSpec(_lib.F16, _lib.TENSOR_CHW, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))


def test_refused_resize_calls_do_not_touch_a_device():
    """Every argument is checked before the context is: without a context a call that is wrong is EINVAL / ENOSUP for its own
    reason, and none of the made-up device pointers is followed.  k = 81 / 10 > 8 is ENOSUP with the bicubic code -- where
    a library without the filter answers EINVAL for an unknown one."""
    lib = _lib.lib()
    src, dst = C.c_void_p(0x1000), C.c_void_p(0x2000)
    ext = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(81, 3))
    spec = _spec()
    orient = (C.c_uint8 * 2)(1, 6)

    def call(n=2, stride=3 * 120 * 16, ext=ext, w=10, h=2, filter=BICUBIC, dst_stride=60):
        return lib.jpeg_amd_resize_filter_batch(None, n, src, stride, ext, w, h, filter, dst, dst_stride)

    def tensor_call(ext=ext, w=10, h=2, filter=BICUBIC):
        return lib.jpeg_amd_resize_filter_tensor_batch(None, 2, src, 3 * 120 * 16, ext, w, h, filter, C.byref(spec), None, dst, 60)

    def oriented_call(ext=ext, w=10, h=2, filter=BICUBIC, orient=orient):
        # image 1 is read transposed: the oriented extent is (h, w), so the extents are handed over transposed
        swapped = (_lib.Extent * 2)(ext[0], _lib.Extent(ext[1].height, ext[1].width))
        return lib.jpeg_amd_resize_oriented_batch(None, 2, src, 3 * 120 * 16, swapped, w, h, filter, orient, dst, 60)

    for f in (call, tensor_call, oriented_call):
        assert f() == ENOSUP                                                 # 81 / 10 > 8, in the second image
        assert f(filter=2) == EINVAL and f(filter=-1) == EINVAL and f(filter=4) == EINVAL       # 2 stays no filter
        assert f(w=0) == EINVAL                                              # ... but the earlier reason comes first
        assert f(filter=BILINEAR) == EINVAL and f(filter=ANTIALIAS) == EINVAL   # inside their limits: the missing context
        fine = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(80, 16))     # k = 8 exactly, on both axes, is inside the limit
        assert f(ext=fine) == EINVAL                                         # a valid bicubic call without a context
        bad = (_lib.Extent * 2)(_lib.Extent(81, 3), _lib.Extent(4, 0))       # image 1 is what the bilinear form refuses
        assert f(ext=bad) == EINVAL
        twelve = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(120, 3))   # k = 12: over this limit, inside the triangle's
        assert f(ext=twelve) == ENOSUP and f(ext=twelve, filter=ANTIALIAS) == EINVAL
    assert call(ext=(_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(3, 17))) == ENOSUP     # ky = 8.5
    assert oriented_call(orient=(C.c_uint8 * 2)(1, 9)) == EINVAL             # a bad orientation in front of the limit
    assert call(stride=3 * 81 * 3 - 1) == EINVAL and call(dst_stride=59) == EINVAL
    assert call(n=0, ext=None) == EINVAL                                     # an empty batch still wants its context


def test_refused_decode_and_mixed_calls_do_not_touch_a_device():
    lib = _lib.lib()
    dst, spec = C.c_void_p(0x2000), _spec()
    # the decode forms validate like the view call, the context last: a 12-bit layout is ENOSUP although there is no context
    L = c_layout(200, 16, [(1, 1)], precision=12)
    view = _lib.View(1, _lib.Region(0, 0, 8, 8))
    args = (_lib.ptr_array([0x3000]), _lib.size_array([0]), C.c_void_p(0x4000), 0, 1, 0, _lib.COLOR_RGB8, C.byref(view))

    def resized(w, h, filter=BICUBIC):
        return lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, w, h, filter, dst, 0)

    def tensor(w, h, filter=BICUBIC):
        return lib.jpeg_amd_decode_tensor_filter_batch(None, C.byref(L), 1, *args, w, h, filter, C.byref(spec), None, dst, 0)

    for f in (resized, tensor):
        L.precision = 12
        view.region = _lib.Region(0, 0, 81, 8)
        assert f(10, 8) == ENOSUP                                            # the layout's verdict, which is the same word
        assert f(0, 8) == ENOSUP                                             # ... and comes in front of the target's
        L.precision = 8
        assert f(0, 8) == EINVAL and f(10, 8, filter=2) == EINVAL
        assert f(10, 8) == ENOSUP                                            # 81 / 10
        assert f(10, 8, filter=ANTIALIAS) == EINVAL and f(10, 8, filter=BILINEAR) == EINVAL    # valid there: no context
        view.region = _lib.Region(0, 0, 80, 8)
        assert f(10, 1) == EINVAL                                            # k = 8 on both axes: valid, no context
        view.region = _lib.Region(0, 0, 120, 8)
        assert f(10, 8) == ENOSUP and f(10, 8, filter=ANTIALIAS) == EINVAL   # k = 12
        view.denom = 3                                                       # what the view call refuses comes first
        assert f(10, 8) == EINVAL
        view.denom = 1

    # the mixed forms: the same verdicts, per image
    image = _lib.Image()
    image.layout, image.d_quanta, image.ntables = L, 0x4000, 1
    image.d_coef[0] = 0x3000
    mixed = (None, 1, C.byref(image), 0, _lib.COLOR_RGB8, C.byref(view))
    view.region = _lib.Region(0, 0, 81, 8)
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 10, 8, BICUBIC, dst, 0) == ENOSUP
    assert lib.jpeg_amd_decode_tensor_filter_mixed(*mixed, 10, 8, BICUBIC, C.byref(spec), None, dst, 0) == ENOSUP
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 10, 8, 2, dst, 0) == EINVAL
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 0, 8, BICUBIC, dst, 0) == EINVAL
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 11, 1, BICUBIC, dst, 0) == EINVAL      # 81 / 11 and 8: valid, no context
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 10, 8, ANTIALIAS, dst, 0) == EINVAL
    orient = (C.c_uint8 * 1)(6)                                              # transposed: 8 x 81, so 81 / 10 is on the other axis
    assert lib.jpeg_amd_decode_tensor_oriented_mixed(*mixed, 8, 10, BICUBIC, C.byref(spec), None, orient, dst, 0) == ENOSUP
    assert lib.jpeg_amd_decode_tensor_oriented_mixed(*mixed, 8, 11, BICUBIC, C.byref(spec), None, orient, dst, 0) == EINVAL


def test_refused_file_calls_do_not_touch_a_device():
    """648 x 16 takes denominator 8 for a 10 x 2 target: the view is 81 x 2 and k = 81 / 10."""
    wide = F.synthetic_file("y8", (648, 16), 1)[0]
    high = F.synthetic_file("y8", (960, 16), 2)[0]                           # 120 x 2 at denominator 8: k = 12
    twelve = F.synthetic_file("y8", (16, 16), 4, precision=12)[0]
    spec = _spec()

    def call(datas, out=(10, 2), filter=BICUBIC, tensor=True):
        n = len(datas)
        ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
        sizes = (C.c_size_t * n)(*[d.size for d in datas])
        buf = np.zeros(4096, np.uint8)
        infos, views = (_lib.FrameInfo * n)(), (_lib.View * n)()
        head = (None, ptrs, sizes, n, 1, 0, _lib.COLOR_RGB8, None, out[0], out[1], filter)
        if tensor:
            st = _lib.lib().jpeg_amd_decompress_tensor_mixed(*head, C.byref(spec), None, buf.ctypes.data, 192, infos, views)
        else:
            st = _lib.lib().jpeg_amd_decompress_resized_mixed(*head, buf.ctypes.data, 192, infos, views)
        return st, [(v.denom, v.region.width, v.region.height) for v in views]

    for tensor in (True, False):
        st, views = call([wide], tensor=tensor)
        assert st == ENOSUP and views == [(8, 81, 2)]
        assert call([wide], filter=2, tensor=tensor)[0] == EINVAL
        assert call([wide], filter=ANTIALIAS, tensor=tensor)[0] == EINVAL    # inside the triangle's limit: the context
        assert call([wide], out=(0, 2), tensor=tensor)[0] == EINVAL          # the earlier reason
        assert call([wide, twelve], tensor=tensor)[0] == ENOSUP
        assert call([wide], out=(11, 2), tensor=tensor)[0] == EINVAL         # 81 / 11: valid, no context
        assert call([high], tensor=tensor)[0] == ENOSUP and call([high], filter=ANTIALIAS, tensor=tensor)[0] == EINVAL


def test_the_binding_names_the_headers_constants():
    text = open(ROOT + "/include/jpeg_amd.h").read()
    m = re.search(r"^enum \{ JPEG_AMD_FILTER_BICUBIC = (\d+) \};$", text, re.M)
    assert m and int(m.group(1)) == _lib.FILTER_BICUBIC == 3
    assert re.search(r"enum \{ JPEG_AMD_FILTER_BILINEAR = 0, JPEG_AMD_FILTER_ANTIALIAS = 1 \};", text)    # as it was
    kernels = open(ROOT + "/jpeg_amd/csrc/kernels.hpp").read()
    assert "kBicubicMaxScale = %.1ff" % float(B.MAX_SCALE) in kernels and "kAntialiasMaxTaps = %d" % B.MAX_TAPS in kernels
    assert "kAntialiasMaxScale = %.1ff" % float(A.MAX_SCALE) in kernels and B.MAX_TAPS == A.MAX_TAPS
