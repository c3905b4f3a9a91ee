"""CPU checks of the tensor sources (include/jpeg_amd.h, "tensor sources"): the numpy checker the GPU tests compare with
(_tensor_source_ref) against what the contract states -- it inverts the tensor output on every byte, and the special values
give the bytes the contract names -- then jpeg_amd_tensor_source_extent and the status of every new entry point without a
context.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import _tensor_ref as T
import _tensor_source_ref as S
from _calls import c_layout
from jpeg_amd import _lib

F = np.float32
OK, EINVAL = 0, -1


# ---- the checker ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [S.F32, S.F16, S.BF16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("constants", [S.IMAGENET, S.UNIT], ids=["imagenet", "unit"])
@pytest.mark.parametrize("layout", S.LAYOUTS, ids=["hwc", "chw"])
def test_the_source_inverts_the_tensor_output_on_every_byte(dtype, constants, layout):
    mean, std = constants
    image = np.empty((1, 256, 3), np.uint8)
    image[0, :, :] = np.arange(256, dtype=np.uint8)[:, None]
    elements = T.normalise(image, S.forward_spec(dtype, layout, mean, std), False)
    back = S.pixels(elements, S.inverse(dtype, layout, mean, std))
    assert back.dtype == np.uint8 and back.shape == image.shape
    assert (back == image).all(), np.argwhere(back != image)[:4].tolist()


def _one(value, scale=1.0, offset=0.0):
    bits = np.empty((1, 1, 3), np.uint32)
    bits[:] = np.asarray([value], F).view(np.uint32)[0]
    return S.pixels(bits, S.Source(S.F32, S.HWC, (scale,) * 3, (offset,) * 3))[0, 0].tolist()


@pytest.mark.parametrize("value, byte", S.SPECIALS, ids=[repr(float(v)) for v, _ in S.SPECIALS])
def test_special_values_under_scale_1_offset_0(value, byte):
    assert _one(value) == [byte] * 3


def test_the_table_of_special_values_is_the_contracts():
    assert [(repr(float(v)), b) for v, b in S.SPECIALS] == [
        ("nan", 0), ("inf", 255), ("-inf", 0), ("-0.0", 0), ("0.4999999701976776", 1), ("254.49998474121094", 254),
        ("254.5", 255), ("255.39999389648438", 255)]


def test_subnormal_elements_are_numbers():
    largest = np.asarray([0x007fffff], np.uint32).view(F)[0]
    assert 0.0 < float(largest) < float(np.finfo(F).tiny)
    # flushed they would give 0.  The product is 3.5265 and the contract rounds: (int)(3.5265 + 0.5) = 4; the subnormal 1e-38
    # gives the product 3 and the byte 3
    assert _one(largest, scale=3e38) == [4, 4, 4]
    assert 0.0 < float(F(1e-38)) < float(np.finfo(F).tiny) and _one(F(1e-38), scale=3e38) == [3, 3, 3]
    # ... in the 16-bit types too: the largest binary16 subnormal is 1023 * 2^-24, the largest bfloat16 one 127 * 2^-133
    h = S.pixels(np.full((1, 1, 3), 0x03ff, np.uint16), S.Source(S.F16, S.HWC, (2.0 ** 24 / 8,) * 3))
    assert h[0, 0].tolist() == [128, 128, 128]              # 1023 / 8 = 127.875
    b = S.pixels(np.full((1, 1, 3), 0x007f, np.uint16), S.Source(S.BF16, S.HWC, (2.0 ** 127,) * 3))
    assert S.values(np.asarray([0x007f], np.uint16), S.BF16)[0] == F(127 * 2.0 ** -133)
    assert b[0, 0].tolist() == [2, 2, 2]                    # 127 / 64 = 1.984375


def test_uint8_elements_are_the_bytes_and_the_layouts_agree():
    rng = np.random.default_rng(3)
    image = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    nan = (float("nan"),) * 3
    assert (S.pixels(image, S.Source(S.U8, S.HWC, nan, nan)) == image).all()
    assert (S.pixels(np.ascontiguousarray(image.transpose(2, 0, 1)), S.Source(S.U8, S.CHW, nan, nan)) == image).all()
    for dtype in (S.F32, S.F16, S.BF16):
        bits = S.random_elements(rng, dtype, (5, 7, 3))
        hwc = S.pixels(bits, S.Source(dtype, S.HWC, (0.5, 1.0, 2.0), (3.0, -7.0, 0.25)))
        chw = S.pixels(np.ascontiguousarray(bits.transpose(2, 0, 1)), S.Source(dtype, S.CHW, (0.5, 1.0, 2.0), (3.0, -7.0, 0.25)))
        assert (hwc == chw).all()
        assert hwc.min() == 0 and hwc.max() == 255          # both clamps bind


# ---- jpeg_amd_tensor_source_extent ----------------------------------------------------------------------------------------------------

def _c_source(dtype=S.F32, layout=S.HWC, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
    return _lib.TensorSource(dtype, layout, (C.c_float * 3)(*scale), (C.c_float * 3)(*offset))


def _extent(src, w, h):
    eb, ne = C.c_size_t(77), C.c_size_t(77)
    st = _lib.lib().jpeg_amd_tensor_source_extent(C.byref(src) if src is not None else None, w, h, C.byref(eb), C.byref(ne))
    return st, eb.value, ne.value


def test_the_binding_names_the_headers_constants():
    assert (_lib.F32, _lib.F16, _lib.BF16, _lib.U8) == (S.F32, S.F16, S.BF16, S.U8)
    assert (_lib.TENSOR_HWC, _lib.TENSOR_CHW) == (S.HWC, S.CHW)
    assert C.sizeof(_lib.TensorSource) == 32


def test_extent_sizes():
    for dtype, size in ((S.F32, 4), (S.F16, 2), (S.BF16, 2), (S.U8, 1)):
        for layout in S.LAYOUTS:
            assert _extent(_c_source(dtype, layout), 13, 5) == (OK, size, 3 * 13 * 5)
    assert _extent(_c_source(), 65535, 65535) == (OK, 4, 3 * 65535 * 65535)
    assert _extent(_c_source(), 1, 1) == (OK, 4, 3)
    assert _lib.lib().jpeg_amd_tensor_source_extent(C.byref(_c_source()), 4, 4, None, None) == OK


def test_extent_refusals():
    assert _extent(None, 4, 4)[0] == EINVAL
    for dtype in (-1, 4, 7):
        assert _extent(_c_source(dtype=dtype), 4, 4)[0] == EINVAL
    for layout in (-1, 2):
        assert _extent(_c_source(layout=layout), 4, 4)[0] == EINVAL
    for bad in (float("nan"), float("inf"), float("-inf")):
        for c in range(3):
            v = [1.0, 1.0, 1.0]
            v[c] = bad
            for dtype in (S.F32, S.F16, S.BF16):
                assert _extent(_c_source(dtype, scale=v), 4, 4)[0] == EINVAL
                assert _extent(_c_source(dtype, offset=v), 4, 4)[0] == EINVAL
            # scale and offset are not read under uint8
            assert _extent(_c_source(S.U8, scale=v, offset=v), 4, 4) == (OK, 1, 48)
    for w, h in ((0, 4), (4, 0), (-1, 4), (4, -1), (65536, 4), (4, 65536)):
        assert _extent(_c_source(), w, h)[0] == EINVAL
    # a refused call leaves the outputs alone
    assert _extent(_c_source(dtype=7), 4, 4) == (EINVAL, 77, 77)


def test_jpeg_amd_tensor_extent_keeps_refusing_uint8():
    spec = _lib.TensorSpec(_lib.U8, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
    assert _lib.lib().jpeg_amd_tensor_extent(C.byref(spec), 4, 4, None, None) == EINVAL


# ---- no context ---------------------------------------------------------------------------------------------------------------------

def test_every_new_entry_point_answers_einval_without_a_context():
    lib = _lib.lib()
    L = c_layout(16, 16, [(2, 2), (1, 1), (1, 1)])
    buf = np.zeros(4096, np.uint16)
    p = buf.ctypes.data
    pp, sz = _lib.ptr_array([p] * 4), _lib.size_array([1024] * 4)
    src = _c_source()
    s = C.byref(src)
    assert lib.jpeg_amd_tensor_pixels_batch(None, 1, p, 768, 16, 16, s, p, 768) == EINVAL
    assert lib.jpeg_amd_tensor_pixels_batch(None, 0, p, 768, 16, 16, s, p, 768) == EINVAL
    assert lib.jpeg_amd_encode_tensor_batch(None, C.byref(L), 1, p, 768, s, _lib.COLOR_RGB8, p, 64, 2, pp, sz) == EINVAL
    assert lib.jpeg_amd_encode_tensor(None, C.byref(L), p, s, _lib.COLOR_RGB8, p, 2, pp) == EINVAL
    info = _lib.FrameInfo()
    info.width, info.height, info.precision, info.ncomponents = 16, 16, 8, 3
    for c in range(3):
        info.id[c], info.factor_x[c], info.factor_y[c] = c + 1, 1, 1
    qkey, tk = (C.c_int32 * 3)(0, 1, 1), (C.c_int32 * 2)(0, 1)
    scan = _lib.Scan()
    sizes = (C.c_size_t * 1)()
    assert lib.jpeg_amd_compress_tensor_batch_device(None, C.byref(info), p, 768, s, 1, _lib.COLOR_RGB8, qkey, p, tk, 2,
                                                     C.byref(scan), 1, None, 0, 1, p, 1024, sizes) == EINVAL


def test_tensor_source_of_the_python_layer_inverts_tensor_spec():
    import torch
    import jpeg_amd as J
    mean, std = S.IMAGENET
    src = J.tensor_source(mean, std, torch.bfloat16, "hwc")
    want = S.inverse(S.BF16, S.HWC, mean, std)
    assert (src.dtype, src.layout) == (S.BF16, S.HWC)
    assert [F(v) for v in src.scale] == want.scale.tolist() and [F(v) for v in src.offset] == want.offset.tolist()
    plain = J.tensor_source(dtype=torch.uint8)
    assert (plain.dtype, plain.layout, list(plain.scale), list(plain.offset)) == (S.U8, S.CHW, [1.0] * 3, [0.0] * 3)
    with pytest.raises(ValueError):
        J.tensor_source(dtype=torch.int32)
    with pytest.raises(ValueError):
        J.tensor_source(layout="nchw")
