"""CPU checks of the tensor output (include/jpeg_amd.h, "tensor output"): jpeg_amd_tensor_extent, the numpy checker the GPU tests
compare with (_tensor_ref) against an eager torch pipeline bit for bit, tensor_spec's constants and their distance to the
torchvision operation order, and the calls the tensor entry points refuse before they touch a device."""
import ctypes as C

import numpy as np
import pytest

import _tensor_ref as T
import jpeg_amd as J
from _calls import c_layout
from jpeg_amd import _lib

IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _spec(dtype=_lib.F16, layout=_lib.TENSOR_CHW, mean=T.MEAN, scale=T.SCALE):
    s = _lib.TensorSpec()
    s.dtype, s.layout = dtype, layout
    for c in range(3):
        s.mean[c], s.scale[c] = mean[c], scale[c]
    return s


def _extent(spec, w, h):
    eb, ne = C.c_size_t(0), C.c_size_t(0)
    status = _lib.lib().jpeg_amd_tensor_extent(C.byref(spec) if spec is not None else None, w, h, C.byref(eb), C.byref(ne))
    return status, eb.value, ne.value


def test_binding_names_the_header_constants():
    assert (T.F32, T.F16, T.BF16) == (_lib.F32, _lib.F16, _lib.BF16) == (0, 1, 2)
    assert (T.HWC, T.CHW) == (_lib.TENSOR_HWC, _lib.TENSOR_CHW) == (0, 1)
    assert C.sizeof(_lib.TensorSpec) == 32


def test_tensor_extent():
    for dtype, size in ((_lib.F32, 4), (_lib.F16, 2), (_lib.BF16, 2)):
        for layout in (_lib.TENSOR_HWC, _lib.TENSOR_CHW):
            for w, h in ((1, 1), (13, 5), (224, 224)):
                assert _extent(_spec(dtype, layout), w, h) == (0, size, 3 * w * h)
    assert _lib.lib().jpeg_amd_tensor_extent(C.byref(_spec()), 4, 4, None, None) == 0
    nan, inf = float("nan"), float("inf")
    bad = [_spec(dtype=3), _spec(dtype=-1), _spec(layout=2), _spec(layout=-1), _spec(mean=(0.0, nan, 0.0)),
           _spec(scale=(1.0, 1.0, inf)), _spec(mean=(-inf, 0.0, 0.0)), _spec(scale=(nan, 1.0, 1.0))]
    for spec in bad:
        assert _extent(spec, 4, 4)[0] == _lib.EINVAL
    for w, h in ((0, 4), (4, 0), (-1, 4), (2 ** 30 + 1, 1)):
        assert _extent(_spec(), w, h)[0] == _lib.EINVAL
    assert _extent(None, 4, 4)[0] == _lib.EINVAL


def _images(w, h, seed):
    rng = np.random.default_rng(seed)
    yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
    return {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "checker": (((xx + yy + cc) & 1) * 255).astype(np.uint8),
            "zero": np.zeros((h, w, 3), np.uint8), "full": np.full((h, w, 3), 255, np.uint8)}


@pytest.mark.parametrize("constants", [(T.MEAN, T.SCALE), T.SIGNED_ZERO], ids=["imagenet", "signed-zero"])
def test_reference_is_the_eager_torch_pipeline_bit_for_bit(constants):
    """flip, permute, sub, mul, .to(dtype) on the CPU give the checker's bit patterns -- for every byte value and channel, and
    on images of every content the GPU tests use."""
    torch = pytest.importorskip("torch")
    dtypes = {T.F32: (torch.float32, torch.int32, np.uint32), T.F16: (torch.float16, torch.int16, np.uint16),
              T.BF16: (torch.bfloat16, torch.int16, np.uint16)}
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)          # [1, 256, 3]: all 256 bytes x 3 channels
    images = [ramp] + list(_images(13, 5, 3).values())
    for dtype in T.DTYPES:
        for layout in T.LAYOUTS:
            spec = T.Spec(dtype, layout, *constants)
            mean, scale = torch.from_numpy(spec.mean), torch.from_numpy(spec.scale)
            for image in images:
                for flip in (False, True):
                    t = torch.from_numpy(image)
                    if flip:
                        t = t.flip(1)
                    t = t.to(torch.float32).sub(mean).mul(scale).to(dtypes[dtype][0])
                    if layout == T.CHW:
                        t = t.permute(2, 0, 1)
                    want = t.contiguous().view(dtypes[dtype][1]).numpy().view(dtypes[dtype][2])
                    got = T.normalise(image, spec, flip)
                    assert got.dtype == want.dtype and got.shape == want.shape
                    assert (got == want).all(), (dtype, layout, flip)
    if constants is T.SIGNED_ZERO:                             # the case exists for this: a -0 and a +0 among the results
        bits = T.normalise(np.full((1, 1, 3), 128, np.uint8), T.Spec(T.F32, T.HWC, *constants), False)
        assert bits[0, 0, 1] == 0x80000000 and T.normalise(np.zeros((1, 1, 3), np.uint8), T.Spec(T.F16, T.HWC, *constants), False)[0, 0, 0] == 0


def test_sweep_constants_stay_clear_of_the_subnormal_range():
    """No nonzero result of the sweeps' constants is below 4.9e-3: far above the subnormal range of every dtype."""
    spec = T.Spec(T.F32, T.HWC)
    ramp = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)
    v = np.abs(T.normalise(ramp, spec, False).view(np.float32))
    print("smallest nonzero magnitude", v[v > 0].min())
    assert v[v > 0].min() >= 4.9e-3


def test_tensor_spec_constants_and_their_distance_to_the_torchvision_order():
    """tensor_spec: mean_b = float32(255 mean), scale = float32(1 / (255 std)), computed in float64 and rounded once.  The
    contract (u - mean_b) * scale against the torchvision order ((u / 255) - m) / s, both in float32, over all 256 bytes x 3
    channels of the ImageNet constants: measured on a CPU at most 4.77e-7 absolute on values up to 2.64, which is 2 ulp of
    that largest magnitude (the subtraction cancels near zero, so the distance is absolute: it does not shrink with the
    value).  The two forms differ by three roundings against two; the bound is twice the measured distance, 4 ulp of the
    largest magnitude, 9.54e-7."""
    torch = pytest.importorskip("torch")
    spec = J.tensor_spec(IMAGENET_MEAN, IMAGENET_STD)
    assert (spec.dtype, spec.layout) == (_lib.F16, _lib.TENSOR_CHW)
    f = np.float32
    want_mean = [f(255.0 * m) for m in IMAGENET_MEAN]
    want_scale = [f(1.0 / (255.0 * s)) for s in IMAGENET_STD]
    assert [f(x) for x in spec.mean] == want_mean and [f(x) for x in spec.scale] == want_scale
    assert want_mean == [f(m) for m in T.MEAN] and want_scale == [f(s) for s in T.SCALE]          # the GPU sweeps' constants
    for dtype, code in ((torch.float32, _lib.F32), (torch.bfloat16, _lib.BF16)):
        s = J.tensor_spec(None, None, dtype=dtype, layout="hwc")
        assert (s.dtype, s.layout, list(s.mean), list(s.scale)) == (code, _lib.TENSOR_HWC, [0.0] * 3, [1.0] * 3)
    with pytest.raises(ValueError):
        J.tensor_spec(IMAGENET_MEAN, IMAGENET_STD, dtype=torch.float64)
    with pytest.raises(ValueError):
        J.tensor_spec(IMAGENET_MEAN, IMAGENET_STD, layout="nchw")

    u = np.arange(256, dtype=f)[:, None]
    contract = (u - np.asarray(want_mean, f)) * np.asarray(want_scale, f)
    vision = ((u / f(255.0)) - np.asarray(IMAGENET_MEAN, f)) / np.asarray(IMAGENET_STD, f)
    assert contract.dtype == f and vision.dtype == f
    diff = np.abs(contract.astype(np.float64) - vision.astype(np.float64)).max()
    largest = np.maximum(np.abs(contract), np.abs(vision)).max()
    ulp = float(np.spacing(largest))
    print("largest distance", diff, "largest value", largest, "in ulp of it", diff / ulp)
    assert 2.6 < largest < 2.7
    assert diff <= 4.0 * ulp


def test_refused_calls_do_not_touch_a_device():
    """Every argument is checked before the context is: without a context a call that is wrong is refused for its own
    reason, and none of the made-up device pointers is followed."""
    lib = _lib.lib()
    src, dst = C.c_void_p(0x1000), C.c_void_p(0x2000)
    ext = (_lib.Extent * 2)(_lib.Extent(4, 4), _lib.Extent(3, 5))
    good = _spec(_lib.F32, _lib.TENSOR_HWC)

    def call(n=2, src=src, stride=48, ext=ext, w=8, h=8, spec=good, flip=None, dst=dst, dst_stride=192):
        return lib.jpeg_amd_resize_tensor_batch(None, n, src, stride, ext, w, h, C.byref(spec) if spec is not None else None, flip,
                                                dst, dst_stride)

    assert call(w=0) == _lib.EINVAL and call(h=0) == _lib.EINVAL
    assert call(spec=None) == _lib.EINVAL and call(spec=_spec(dtype=3)) == _lib.EINVAL and call(spec=_spec(layout=2)) == _lib.EINVAL
    assert call(spec=_spec(mean=(float("nan"), 0.0, 0.0))) == _lib.EINVAL
    assert call(dst=C.c_void_p(0x2002)) == _lib.EINVAL                                     # F32 at 2 bytes past a boundary
    assert call(spec=_spec(_lib.F16), dst=C.c_void_p(0x2001)) == _lib.EINVAL
    assert call(stride=47) == _lib.EINVAL and call(dst_stride=191) == _lib.EINVAL
    assert call(n=65536) == _lib.EINVAL and call(n=-1) == _lib.EINVAL
    assert call(src=None) == _lib.EINVAL and call(dst=None) == _lib.EINVAL and call(ext=None) == _lib.EINVAL
    assert call() == _lib.EINVAL                                                           # valid, but no context: refused, not run

    L = c_layout(16, 16, [(1, 1)], precision=12)
    view = _lib.View(1, _lib.Region(0, 0, 8, 8))
    args = (_lib.ptr_array([0x3000]), _lib.size_array([0]), C.c_void_p(0x4000), 0, 1, 0, _lib.COLOR_RGB8, C.byref(view))
    assert lib.jpeg_amd_decode_tensor_batch(None, C.byref(L), 1, *args, 8, 8, C.byref(good), None, dst, 0) == _lib.ENOSUP
    L.precision = 8
    assert lib.jpeg_amd_decode_tensor_batch(None, C.byref(L), 1, *args, 8, 8, None, None, dst, 0) == _lib.EINVAL
    assert lib.jpeg_amd_decode_tensor_batch(None, C.byref(L), 1, *args, 8, 8, C.byref(good), None, C.c_void_p(0x2002), 0) == _lib.EINVAL
    view.denom = 3
    assert lib.jpeg_amd_decode_tensor_batch(None, C.byref(L), 1, *args, 8, 8, C.byref(good), None, dst, 0) == _lib.EINVAL
