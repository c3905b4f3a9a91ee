"""CPU checks of the resample contract (include/jpeg_amd.h, "resized decode"): the numpy checker the GPU tests compare with
(_resize_ref) against torch's bilinear interpolation, identity sizes, and the calls jpeg_amd_resize_batch refuses before it
touches a device."""
import ctypes as C

import numpy as np
import pytest

import _resize_ref as R
from _calls import c_layout
from jpeg_amd import _lib

# (source w, h) -> (target w, h)
PAIRS = [((1, 1), (1, 1)), ((1, 1), (5, 3)), ((2, 3), (7, 7)), ((17, 33), (5, 40)), ((131, 57), (224, 224)),
         ((449, 301), (224, 224)), ((640, 360), (224, 224)), ((17, 33), (17, 33)), ((131, 57), (131, 57))]


def _images(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "checker": checker,
            "full": np.full((h, w, 3), 255, np.uint8)}


def test_checker_is_within_one_level_of_torch_bilinear():
    """torch.nn.functional.interpolate(bilinear, align_corners=False, antialias=False), rounded half up, is the same filter
    in another operation order: the worst difference is one level in every case, and at most 1 sample in 1 000 of all the
    cases together differs at all (a 7 x 7 case has 147 samples; the rate is a statement about the filter, not about one case)."""
    torch = pytest.importorskip("torch")
    total = differ = 0
    for n, ((w, h), (wt, ht)) in enumerate(PAIRS):
        for name, image in _images(w, h, n).items():
            got = R.resize(image, wt, ht)
            t = torch.from_numpy(image).permute(2, 0, 1)[None].to(torch.float32)
            ref = torch.nn.functional.interpolate(t, size=(ht, wt), mode="bilinear", align_corners=False, antialias=False)
            ref = torch.floor(ref.clamp(0, 255) + 0.5)[0].permute(1, 2, 0).numpy().astype(np.uint8)
            diff = np.abs(got.astype(np.int32) - ref.astype(np.int32))
            print((w, h), (wt, ht), name, "worst", int(diff.max()), "differing", int((diff != 0).sum()), "of", diff.size)
            assert diff.max() <= 1, ((w, h), (wt, ht), name)
            total += diff.size
            differ += int((diff != 0).sum())
    print("differing", differ, "of", total)
    assert differ * 1000 <= total


@pytest.mark.parametrize("size", [(1, 1), (2, 3), (7, 9), (131, 57), (449, 301)])
def test_identity_size_returns_the_source(size):
    for image in _images(size[0], size[1], 7).values():
        assert (R.resize(image, size[0], size[1]) == image).all()


def test_taps_stay_inside_the_source():
    for n, n_out in [(1, 1), (1, 9), (3, 1), (449, 224), (57, 224), (4000, 3), (5, 4000)]:
        i0, i1, f = R.axis_taps(n_out, n)
        assert i0.min() >= 0 and i1.max() <= n - 1 and (i1 - i0 <= 1).all() and (i1 >= i0).all()
        assert f.min() >= 0.0


def test_refused_calls_do_not_touch_a_device():
    """Every argument is checked before the context is: without a context (no device is needed to load the library) a call
    that is wrong is EINVAL / ENOSUP for its own reason, and none of the made-up device pointers is followed."""
    lib = _lib.lib()
    src, dst = C.c_void_p(0x1000), C.c_void_p(0x2000)
    ext = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(3, 5))

    def call(n=2, src=src, stride=48, ext=ext, w=8, h=8, dst=dst, dst_stride=192):
        return lib.jpeg_amd_resize_batch(None, n, src, stride, ext, w, h, dst, dst_stride)

    assert call(w=0) == _lib.EINVAL and call(h=0) == _lib.EINVAL and call(w=-3) == _lib.EINVAL
    assert call(ext=(_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(0, 5))) == _lib.EINVAL
    assert call(ext=(_lib.Extent * 2)(_lib.Extent(4, -1), _lib.Extent(3, 5))) == _lib.EINVAL
    assert call(stride=47) == _lib.EINVAL and call(dst_stride=191) == _lib.EINVAL
    assert call(n=65536) == _lib.EINVAL and call(n=-1) == _lib.EINVAL
    assert call(src=None) == _lib.EINVAL and call(dst=None) == _lib.EINVAL and call(ext=None) == _lib.EINVAL
    assert call() == _lib.EINVAL                                 # a valid call without a context: refused, not run

    # the decode form validates like the view call, the context last: a 12-bit layout is ENOSUP although there is no context
    L = c_layout(16, 16, [(1, 1)], precision=12)
    view = _lib.View(1, _lib.Region(0, 0, 8, 8))
    args = (_lib.ptr_array([0x3000]), _lib.size_array([0]), C.c_void_p(0x4000), 0, 1, 0, _lib.COLOR_RGB8, C.byref(view))
    assert lib.jpeg_amd_decode_resized_batch(None, C.byref(L), 1, *args, 8, 8, dst, 0) == _lib.ENOSUP
    L.precision = 8
    assert lib.jpeg_amd_decode_resized_batch(None, C.byref(L), 1, *args, 0, 8, dst, 0) == _lib.EINVAL
    view.denom = 3
    assert lib.jpeg_amd_decode_resized_batch(None, C.byref(L), 1, *args, 8, 8, dst, 0) == _lib.EINVAL
