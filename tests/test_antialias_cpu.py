"""CPU checks of the antialiasing filter (include/jpeg_amd.h, "antialiased resample"): the numpy checker the GPU tests compare
with (_antialias_ref) against torch's antialiased bilinear interpolation, identity sizes, the taps and weights, the tap
bound, and the calls the *_filter_* entry points refuse before they touch a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _antialias_ref as A
from _calls import c_layout
from jpeg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (source w, h) -> (target w, h)
PAIRS = [((1, 1), (5, 3)), ((5, 3), (1, 1)), ((37, 23), (8, 8)), ((129, 67), (64, 32)), ((130, 70), (65, 33)),
         ((449, 301), (224, 224)), ((640, 360), (224, 224)), ((300, 200), (19, 13)), ((160, 16), (10, 16)),
         ((131, 57), (224, 224)), ((17, 33), (17, 33))]


def _images(w, h, seed):
    """The contents of test_resize_cpu.py."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "checker": checker,
            "full": np.full((h, w, 3), 255, np.uint8)}


def test_reference_is_within_one_level_of_torch_antialias():
    """torch.nn.functional.interpolate(bilinear, antialias=True, align_corners=False), rounded half up, is the same filter in
    another operation order.  Both are binary32 evaluations of one real expression whose error is far below half a level, so
    the worst difference is one level in every case; over the RANDOM contents together at most 1 sample in 1 000 differs (a
    condition: 5 of 467 k where this was written).  The checkerboard is exempt from the rate: where it is reduced its true
    values are the tie 127.5, which either order may round either way."""
    torch = pytest.importorskip("torch")
    total = differ = 0
    for n, ((w, h), (wt, ht)) in enumerate(PAIRS):
        for name, image in _images(w, h, n).items():
            got = A.resize(image, wt, ht)
            t = torch.from_numpy(image).permute(2, 0, 1)[None].to(torch.float32)
            ref = torch.nn.functional.interpolate(t, size=(ht, wt), mode="bilinear", align_corners=False, antialias=True)
            ref = torch.floor(ref.clamp(0, 255) + 0.5)[0].permute(1, 2, 0).numpy().astype(np.uint8)
            diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
            print((w, h), (wt, ht), name, "worst", int(diff.max()), "differing", int((diff != 0).sum()), "of", diff.size)
            assert diff.max() <= 1, ((w, h), (wt, ht), name)
            if name == "random":
                total += diff.size
                differ += int((diff != 0).sum())
    print("random contents: differing", differ, "of", total)
    assert differ * 1000 <= total


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (7, 9), (131, 57), (449, 301)])
def test_identity_size_returns_the_source(size):
    for image in _images(size[0], size[1], 7).values():
        assert (A.resize(image, size[0], size[1]) == image).all()


def test_taps_stay_inside_the_source_and_the_weights_sum_to_one():
    for n, n_out in [(1, 1), (1, 9), (3, 1), (449, 224), (57, 224), (640, 224), (300, 19), (48, 3), (5, 4000), (160, 10)]:
        lo, count, W = A.axis_table(n_out, n)
        assert lo.min() >= 0 and (lo + count).max() <= n and count.min() >= 1, (n, n_out)
        assert (np.diff(lo) >= 0).all() and (np.diff(lo + count) >= 0).all()      # what the kernel's footprint relies on
        assert W.min() >= 0.0
        total = np.zeros(n_out, A.F)
        for i in range(W.shape[1]):
            total = total + W[:, i]
        assert np.abs(total - A.F(1.0)).max() <= 2 * np.finfo(A.F).eps, (n, n_out)


def test_the_tap_bound_holds_at_a_factor_of_sixteen():
    for n, n_out in [(160, 10), (4000, 250), (16, 1), (161, 11)]:
        _, count, _ = A.axis_table(n_out, n)                # asserts count <= 33 itself
        assert count.max() <= A.MAX_TAPS
    assert A.axis_table(10, 160)[1].max() == A.MAX_TAPS - 1  # an interior output at k = 16 reads 2 s = 32 taps
    with pytest.raises(AssertionError):
        A.axis_table(10, 200)                               # k = 20: 41 taps


def test_refused_calls_do_not_touch_a_device():
    """Every argument is checked before the context is: without a context (no device is needed to load the library) a call
    that is wrong is EINVAL / ENOSUP for its own reason, and none of the made-up device pointers is followed."""
    lib = _lib.lib()
    src, dst = C.c_void_p(0x1000), C.c_void_p(0x2000)
    ext = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(161, 3))
    spec = _lib.TensorSpec(_lib.F16, _lib.TENSOR_CHW, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))

    def call(n=2, stride=3 * 161 * 3, ext=ext, w=10, h=2, filter=_lib.FILTER_ANTIALIAS, dst_stride=60):
        return lib.jpeg_amd_resize_filter_batch(None, n, src, stride, ext, w, h, filter, dst, dst_stride)

    def tensor_call(ext=ext, w=10, h=2, filter=_lib.FILTER_ANTIALIAS):
        return lib.jpeg_amd_resize_filter_tensor_batch(None, 2, src, 3 * 161 * 3, ext, w, h, filter, C.byref(spec), None, dst, 60)

    for f in (call, tensor_call):
        assert f(filter=2) == _lib.EINVAL and f(filter=-1) == _lib.EINVAL      # an unknown filter
        assert f() == _lib.ENOSUP                                            # 161 / 10 > 16, in the second image
        assert f(w=0) == _lib.EINVAL                                         # ... but the earlier reason comes first
        assert f(filter=_lib.FILTER_BILINEAR) == _lib.EINVAL                 # no limit there: refused for the missing context
        fine = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(160, 3))     # k = 16 exactly is inside the limit
        assert f(ext=fine) == _lib.EINVAL                                    # a valid antialiased call without a context
        bad = (_lib.Extent * 2)(_lib.Extent(161, 3), _lib.Extent(4, 0))      # image 1 is what the bilinear form refuses
        assert f(ext=bad) == _lib.EINVAL
    assert call(ext=(_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(3, 33))) == _lib.ENOSUP    # ky = 16.5
    assert call(stride=3 * 161 * 3 - 1) == _lib.EINVAL and call(dst_stride=59) == _lib.EINVAL
    assert call(n=0, ext=None) == _lib.EINVAL                                # an empty batch still wants its context

    # the decode forms validate like the view call, the context last: a 12-bit layout is ENOSUP although there is no context
    L = c_layout(200, 16, [(1, 1)], precision=12)
    view = _lib.View(1, _lib.Region(0, 0, 8, 8))
    args = (_lib.ptr_array([0x3000]), _lib.size_array([0]), C.c_void_p(0x4000), 0, 1, 0, _lib.COLOR_RGB8, C.byref(view))
    aa = _lib.FILTER_ANTIALIAS
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 8, 8, aa, dst, 0) == _lib.ENOSUP
    assert lib.jpeg_amd_decode_tensor_filter_batch(None, C.byref(L), 1, *args, 8, 8, aa, C.byref(spec), None, dst, 0) == _lib.ENOSUP
    L.precision = 8
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 0, 8, aa, dst, 0) == _lib.EINVAL
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 8, 8, 7, dst, 0) == _lib.EINVAL
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 8, 8, aa, dst, 0) == _lib.EINVAL     # valid, no context
    view.region = _lib.Region(0, 0, 170, 8)                                  # 170 / 10 = 17 > 16
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 10, 8, aa, dst, 0) == _lib.ENOSUP
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 10, 8, _lib.FILTER_BILINEAR, dst, 0) == _lib.EINVAL
    view.denom = 3                                                           # what the view call refuses comes first
    assert lib.jpeg_amd_decode_resized_filter_batch(None, C.byref(L), 1, *args, 10, 8, aa, dst, 0) == _lib.EINVAL
    view.denom = 1

    # the mixed forms: the same verdicts, per image
    image = _lib.Image()
    image.layout, image.d_quanta, image.ntables = L, 0x4000, 1
    image.d_coef[0] = 0x3000
    mixed = (None, 1, C.byref(image), 0, _lib.COLOR_RGB8, C.byref(view))
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 10, 8, aa, dst, 0) == _lib.ENOSUP
    assert lib.jpeg_amd_decode_tensor_filter_mixed(*mixed, 10, 8, aa, C.byref(spec), None, dst, 0) == _lib.ENOSUP
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 10, 8, 2, dst, 0) == _lib.EINVAL
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 11, 8, aa, dst, 0) == _lib.EINVAL    # 170 / 11 < 16: valid, no context
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, 10, 8, _lib.FILTER_BILINEAR, dst, 0) == _lib.EINVAL


def test_the_binding_names_the_headers_constants():
    text = open(ROOT + "/include/jpeg_amd.h").read()
    m = re.search(r"enum \{ JPEG_AMD_FILTER_BILINEAR = (\d+), JPEG_AMD_FILTER_ANTIALIAS = (\d+) \};", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (_lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS) == (0, 1)
    kernels = open(ROOT + "/jpeg_amd/csrc/kernels.hpp").read()
    assert "kAntialiasMaxScale = %.1ff" % float(A.MAX_SCALE) in kernels and "kAntialiasMaxTaps = %d" % A.MAX_TAPS in kernels
