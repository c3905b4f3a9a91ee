"""Tensor output on the MI355X (jpeg_amd_resize_tensor_batch, jpeg_amd_decode_tensor_batch; k_resize_tensor): every element is
compared AS A BIT PATTERN with _tensor_ref -- the contract of include/jpeg_amd.h restated in numpy -- applied to the source bytes
or to what the existing byte call (decode_resized) returns for the same arguments.  Every output buffer is filled with the byte
0xA5 before the call, and every byte that belongs to no image is checked after it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _resize_ref as R
import _tensor_ref as T
import jpeg_amd as J
from _calls import (RESIZE_CONTENTS as CONTENTS, RESIZE_EXTENTS as EXTENTS, RESIZE_FACTORS as FACTORS, RESIZE_SIZE as SIZE,
                    RESIZE_TILE_H as TILE_H, RESIZE_TILE_W as TILE_W, RESIZE_VIEWS as VIEWS, SENTINEL, Out, c_layout, c_views,
                    pixel_image, plane_ptrs, resize_py_layout, resized_call, strides, synthetic)
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes as _c_flips, c_spec as _c_spec, pack, same as _same
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

FLIPS = [0, 1, 0, 1, 1]
# (out_w, out_h, elements between the output images beyond 3 out_w out_h).  (13, 5): rows of 39 elements -- runs that start at
# every alignment -- and a last run of one pixel, at a stride of 196 elements and, with (13, 5, 2), at an odd one; (224, 224, 0):
# only vector stores; (70, 67, 3): two tiles across and three down, a flip across the partial last tile column
TARGETS = [(1, 1, 0), (13, 5, 1), (13, 5, 2), (224, 224, 0), (TILE_W + 6, 2 * TILE_H + 3, 3)]
DTYPE_NAMES = {T.F32: "f32", T.F16: "f16", T.BF16: "bf16"}
LAYOUT_NAMES = {T.HWC: "hwc", T.CHW: "chw"}
ELEM = {T.F32: 4, T.F16: 2, T.BF16: 2}
COMBOS = [(d, l) for d in T.DTYPES for l in T.LAYOUTS]
COMBO_IDS = ["%s-%s" % (DTYPE_NAMES[d], LAYOUT_NAMES[l]) for d, l in COMBOS]


@functools.lru_cache(maxsize=None)
def _sources(content):
    return tuple(pixel_image(content, w, h, 100 * w + h) for w, h in EXTENTS)


@functools.lru_cache(maxsize=None)
def _resized(content, out_w, out_h):
    """The byte images of the contract for the sources of `content`: computed once, shared by every dtype and layout, and
    never written to."""
    out = tuple(R.resize(image, out_w, out_h) for image in _sources(content))
    for o in out:
        o.setflags(write=False)
    return out


class TensorOut(Out):
    """The output of one call: n images of 3 out_w out_h elements of spec's dtype, `gap` elements between them, the first one
    `lead` elements behind an allocation boundary, and a few elements of room behind the last."""

    def __init__(self, ctx, torch, n, out_w, out_h, spec, gap=0, lead=0):
        super().__init__(ctx, torch, [3 * out_w * out_h] * n, elem=ELEM[spec.dtype], gap=gap, lead=lead, tail=7)
        self.shape = (3, out_h, out_w) if spec.layout == T.CHW else (out_h, out_w, 3)
        self.bits = T.BITS[spec.dtype]

    def images(self):
        """The n images as bit patterns; asserts the sentinel in every byte that belongs to none of them."""
        return [b.copy().view(self.bits).reshape(self.shape) for b in super().images()]


def _resize_tensor_call(ctx, torch, images, out_w, out_h, spec, flips, gap=0, lead=0, src_gap=3):
    n = len(images)
    d_src, src_stride, ext = pack(ctx, torch, images, src_gap)
    out = TensorOut(ctx, torch, n, out_w, out_h, spec, gap=gap, lead=lead)
    assert _lib.lib().jpeg_amd_resize_tensor_batch(ctx.handle, n, d_src.data_ptr(), src_stride, ext, out_w, out_h,
                                                   C.byref(_c_spec(spec)), _c_flips(flips), out.ptr, out.stride) == 0
    return out.images()


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", TARGETS, ids=["%dx%d+%d" % t for t in TARGETS])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_kernel_matches_the_contract(ctx, torch, combo, target):
    out_w, out_h, gap = target
    assert (out_w, out_h) != (13, 5) or (out_w % 4 == 1 and (3 * out_w) % 4 == 3)
    assert (out_w, out_h, gap) != (13, 5, 2) or (3 * out_w * out_h + gap) % 2 == 1
    assert out_w != TILE_W + 6 or (out_w > TILE_W and out_h > 2 * TILE_H and out_w % TILE_W % 4 != 0)
    assert (out_w, out_h, gap) != (224, 224, 0) or out_w % 4 == 0
    spec = T.Spec(*combo)
    for content in CONTENTS:
        got = _resize_tensor_call(ctx, torch, list(_sources(content)), out_w, out_h, spec, FLIPS, gap=gap)
        for i, (g, u) in enumerate(zip(got, _resized(content, out_w, out_h))):
            _same(g, T.normalise(u, spec, FLIPS[i]), (content, EXTENTS[i], target))


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_exact_zeros_keep_their_sign(ctx, torch, combo):
    """mean (0, 128, 255), scale (1, -1, 0.5): bytes 0, 128 and 255 give +0, -0 and +0, in every dtype."""
    spec = T.Spec(*combo, *T.SIGNED_ZERO)
    flat = np.empty((9, 7, 3), np.uint8)
    flat[:] = (0, 128, 255)
    images = [flat, pixel_image("random", 7, 9, 5), pixel_image("checker", 131, 57, 0)]
    got = _resize_tensor_call(ctx, torch, images, 13, 5, spec, [1, 0, 1], gap=1)
    want = [T.tensor(im, 13, 5, spec, f) for im, f in zip(images, [1, 0, 1])]
    sign = {T.F32: 0x80000000}.get(spec.dtype, 0x8000)
    first = want[0] if spec.layout == T.HWC else want[0].transpose(1, 2, 0)
    assert (first[..., 0] == 0).all() and (first[..., 1] == sign).all() and (first[..., 2] == 0).all()
    for i, (g, w) in enumerate(zip(got, want)):
        _same(g, w, i)


# ---- 2. a base that is aligned to the element only ----------------------------------------------------------------------------------

@pytest.mark.parametrize("target", [(13, 5, 1), (224, 224, 0)], ids=["13x5+1", "224x224+0"])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_a_base_one_element_past_an_allocation_boundary(ctx, torch, combo, target):
    out_w, out_h, gap = target
    spec = T.Spec(*combo)
    images = list(_sources("random"))
    aligned = _resize_tensor_call(ctx, torch, images, out_w, out_h, spec, FLIPS, gap=gap)
    shifted = _resize_tensor_call(ctx, torch, images, out_w, out_h, spec, FLIPS, gap=gap, lead=1)   # checks the element in front
    for i, (a, s, u) in enumerate(zip(aligned, shifted, _resized("random", out_w, out_h))):
        _same(s, a, i)
        _same(s, T.normalise(u, spec, FLIPS[i]), i)


# ---- 3. decode + resample + output stage ------------------------------------------------------------------------------------------

def _tensor_call(ctx, L, planes, dq, ntables, cosited, color, views, out_w, out_h, spec, flips, ptr, stride, layout=None):
    return _lib.lib().jpeg_amd_decode_tensor_batch(
        ctx.handle, C.byref(layout or L), len(views), plane_ptrs(planes), _lib.size_array(strides(L)),
        dq.data_ptr(), ntables * 64, ntables, cosited, color, c_views(views), out_w, out_h,
        C.byref(spec) if spec is not None else None, _c_flips(flips), ptr, stride)


@pytest.mark.parametrize("name", sorted(FACTORS))
def test_decode_tensor_is_the_byte_call_normalised(ctx, torch, name):
    """The existing byte call is the yardstick: this test does not depend on the decoder."""
    L = c_layout(SIZE[0], SIZE[1], FACTORS[name])
    cosited = 1 if name.endswith("cosited") else 0
    views, flips = VIEWS, [1, 0, 1, 0, 0]
    n = len(views)
    assert sorted({v[0] for v in views}) == [1, 2, 4, 8]
    planes, dq, ntables = synthetic(ctx, torch, L, n, 17)
    for color in (J.RGB, J.YCbCr):
        for out_w, out_h, gap in [(32, 32, 0), (7, 5, 3)]:
            u = J.decode_resized(ctx, SIZE, resize_py_layout(name), planes, dq, views, (out_w, out_h), color=color,
                                 cosite=bool(cosited)).cpu().numpy()
            for combo in COMBOS:
                spec = T.Spec(*combo)
                out = TensorOut(ctx, torch, n, out_w, out_h, spec, gap=gap)
                assert _tensor_call(ctx, L, planes, dq, ntables, cosited, color.code, views, out_w, out_h, _c_spec(spec), flips,
                                    out.ptr, out.stride) == 0
                for i, g in enumerate(out.images()):
                    _same(g, T.normalise(u[i], spec, flips[i]), (name, color.__name__, out_w, out_h, combo, i))


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------

def test_mean_0_scale_1_gives_the_bytes_as_floats(ctx, torch):
    L = c_layout(SIZE[0], SIZE[1], FACTORS["420"])
    n = len(VIEWS)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 29)
    out_w, out_h = 32, 20
    u = J.decode_resized(ctx, SIZE, resize_py_layout("420"), planes, dq, VIEWS, (out_w, out_h)).cpu().numpy()
    spec = T.Spec(T.F32, T.HWC, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    for flips, want in ((None, u), ([0] * n, u), ([1] * n, u[:, :, ::-1])):
        out = TensorOut(ctx, torch, n, out_w, out_h, spec)
        assert _tensor_call(ctx, L, planes, dq, ntables, 0, _lib.COLOR_RGB8, VIEWS, out_w, out_h, _c_spec(spec), flips, out.ptr,
                            out.stride) == 0
        for i, g in enumerate(out.images()):
            assert (g.view(np.float32) == want[i].astype(np.float32)).all(), (flips, i)


# ---- 5. queued calls ----------------------------------------------------------------------------------------------------------------

def test_three_calls_queued_back_to_back_on_a_fresh_context(torch):
    """No synchronise between the calls: a tensor call of 2 small views, a tensor call of 256 larger ones -- the context's
    intermediate and its record buffer both grow while the first call's kernels may still be running from them -- then a
    byte call of the same 256 views, whose records overwrite the second call's.  All three must be the contract's."""
    name = "420"
    ctx = J.Context(0)
    L = c_layout(SIZE[0], SIZE[1], FACTORS[name])
    small = [(4, 1, 1, 9, 7), (8, 0, 0, 5, 5)]
    large = [(1, 0, 0, 131, 257), (2, 1, 1, 64, 120), (1, 3, 3, 120, 250)] + [(2, 0, 0, 66, 129)] * 253
    n = len(large)
    flips = [[1, 0], [(i * 7 + 1) % 3 != 0 for i in range(n)]]
    flips[1] = [int(f) for f in flips[1]]
    planes, dq, ntables = synthetic(ctx, torch, L, n, 5)
    out_w, out_h = 24, 40
    specs = [T.Spec(T.F32, T.HWC), T.Spec(T.F16, T.CHW)]
    outs = [TensorOut(ctx, torch, len(v), out_w, out_h, s) for v, s in zip((small, large), specs)]
    stride = 3 * out_w * out_h
    bytes_out = Out(ctx, torch, [stride] * n, tail=5)
    decoded = [[d.cpu().numpy() for d in J.decode_views(ctx, SIZE, resize_py_layout(name), [p[:len(v)] for p in planes], dq[:len(v)], v)]
               for v in (small[:2], large[:4])]
    ctx.close()
    ctx = J.Context(0)                                      # nothing allocated yet: the calls grow the buffers
    for views, out, spec, f in zip((small, large), outs, specs, flips):
        assert _tensor_call(ctx, L, planes, dq, ntables, 0, _lib.COLOR_RGB8, views, out_w, out_h, _c_spec(spec), f, out.ptr,
                            out.stride) == 0
    assert resized_call(ctx, L, planes, dq, ntables, 0, _lib.COLOR_RGB8, large, out_w, out_h, bytes_out.ptr, stride) == 0
    got = [o.images() for o in outs]
    host = bytes_out.images()                               # asserts the sentinel behind the last image
    for i in range(2):
        _same(got[0][i], T.tensor(decoded[0][i], out_w, out_h, specs[0], flips[0][i]), ("first", i))
    for i in range(4):
        _same(got[1][i], T.tensor(decoded[1][i], out_w, out_h, specs[1], flips[1][i]), ("second", i))
    # images 3 .. n - 1 of the second call have the same view of different images: the last ones against the view decode alone
    rest = J.decode_views(ctx, SIZE, resize_py_layout(name), [p[250:] for p in planes], dq[250:], large[250:])
    assert {flips[1][i] for i in range(250, n)} == {0, 1}
    for j, d in enumerate(rest):
        i = 250 + j
        u = R.resize(d.cpu().numpy(), out_w, out_h)
        _same(got[1][i], T.normalise(u, specs[1], flips[1][i]), ("second", i))
        assert (host[i].reshape(out_h, out_w, 3) == u).all(), ("bytes", i)
    for i in range(4):
        assert (host[i].reshape(out_h, out_w, 3) == R.resize(decoded[1][i], out_w, out_h)).all(), ("bytes", i)
    ctx.close()


# ---- 6. the Python API ------------------------------------------------------------------------------------------------------------

def test_python_api(ctx, torch):
    L = c_layout(SIZE[0], SIZE[1], FACTORS["420"])
    layout = resize_py_layout("420")
    source = [(0, 0, 131, 257), (10, 7, 100, 200), (90, 30, 41, 35), (3, 100, 70, 150), (64, 128, 9, 6)]
    flips = [0, 1, 1, 0, 1]
    planes, dq, _ = synthetic(ctx, torch, L, len(source), 23)
    out_size = (16, 20)
    u, want_views = J.decode_crops_resized(ctx, SIZE, layout, planes, dq, source, out_size, color=J.YCbCr)
    u = u.cpu().numpy()
    for dtype, code in ((torch.float32, T.F32), (torch.float16, T.F16), (torch.bfloat16, T.BF16)):
        for name, lay in (("chw", T.CHW), ("hwc", T.HWC)):
            spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=dtype, layout=name)
            got, views = J.decode_crops_tensor(ctx, SIZE, layout, planes, dq, source, out_size, spec, flips=flips, color=J.YCbCr)
            assert views.dtype == np.int32 and views.tolist() == want_views.tolist()
            assert got.dtype == dtype and tuple(got.shape) == ((len(source), 3, 20, 16) if lay == T.CHW else (len(source), 20, 16, 3))
            ref = T.Spec(code, lay)
            bits = got.contiguous().view(torch.int32 if code == T.F32 else torch.int16).cpu().numpy().view(T.BITS[code])
            for i in range(len(source)):
                _same(bits[i], T.normalise(u[i], ref, flips[i]), (name, code, i))
    same = J.decode_tensors(ctx, SIZE, layout, planes, dq, want_views, out_size, J.tensor_spec(None, None, torch.float32, "hwc"),
                            color=J.YCbCr)
    assert (same.cpu().numpy() == u.astype(np.float32)).all()

    images = [torch.from_numpy(pixel_image("random", w, h, w)).to(ctx.torch_device) for w, h in EXTENTS[:2] + EXTENTS[3:4]]
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
    got = J.resize_tensor(ctx, images, (31, 9), spec, flips=[1, 0, 1])
    assert got.dtype == torch.float16 and tuple(got.shape) == (3, 3, 9, 31)
    bits = got.view(torch.int16).cpu().numpy().view(np.uint16)
    for i, im in enumerate(images):
        _same(bits[i], T.tensor(im.cpu().numpy(), 31, 9, T.Spec(T.F16, T.CHW), [1, 0, 1][i]), i)
    with pytest.raises(J.JpegAmdError):
        J.resize_tensor(ctx, images, (0, 9), spec)
    with pytest.raises(ValueError):
        J.resize_tensor(ctx, images, (31, 9), spec, flips=[1, 0])


# ---- 7. refusals; the empty batch ---------------------------------------------------------------------------------------------------

def test_invalid_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    L = c_layout(131, 65, FACTORS["420"])
    good = [(2, 3, 5, 20, 9), (4, 1, 1, 20, 9)]
    n = len(good)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 3)
    out_w, out_h = 10, 6
    f32, f16 = T.Spec(T.F32, T.CHW), T.Spec(T.F16, T.HWC)
    out = TensorOut(ctx, torch, n, out_w, out_h, f32)
    out16 = TensorOut(ctx, torch, n, out_w, out_h, f16)

    def call(views=good, spec=_c_spec(f32), ptr=out.ptr, s=out.stride, w=out_w, h=out_h, layout=None):
        return _tensor_call(ctx, L, planes, dq, ntables, 0, _lib.COLOR_RGB8, views, w, h, spec, [1, 0], ptr, s, layout=layout)

    bad_dtype, bad_layout, bad_mean, bad_scale = _c_spec(f32), _c_spec(f32), _c_spec(f32), _c_spec(f32)
    bad_dtype.dtype, bad_layout.layout, bad_mean.mean[1], bad_scale.scale[2] = 3, 2, float("nan"), float("inf")
    for spec in (bad_dtype, bad_layout, bad_mean, bad_scale, None):
        assert call(spec=spec) == _lib.EINVAL
    assert call(ptr=out.ptr + 2) == _lib.EINVAL                                          # F32 two bytes past an element boundary
    assert call(spec=_c_spec(f16), ptr=out16.ptr + 1, s=out16.stride) == _lib.EINVAL      # F16 one byte past
    assert call(s=out.stride - 1) == _lib.EINVAL
    assert call(ptr=None) == _lib.EINVAL
    assert call(views=good[:1] + [(4, 33 - 20 + 1, 1, 20, 9)]) == _lib.EINVAL            # one pixel past W' = 33
    assert call(views=good[:1] + [(3, 0, 0, 17, 9)]) == _lib.EINVAL
    assert call(w=0) == _lib.EINVAL and call(h=0) == _lib.EINVAL
    assert call(layout=c_layout(131, 65, FACTORS["420"], precision=12)) == _lib.ENOSUP

    lib = _lib.lib()
    d = torch.full((512,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    e = (_lib.Extent * 2)(_lib.Extent(2, 2), _lib.Extent(3, 1))
    ok = _c_spec(f32)
    for args in ((2, d.data_ptr(), 12, e, 2, 2, C.byref(bad_dtype), None, d.data_ptr() + 256, 12),
                 (2, d.data_ptr(), 12, e, 2, 2, C.byref(bad_mean), None, d.data_ptr() + 256, 12),
                 (2, d.data_ptr(), 12, e, 2, 2, None, None, d.data_ptr() + 256, 12),
                 (2, d.data_ptr(), 12, e, 2, 2, C.byref(ok), None, d.data_ptr() + 258, 12),
                 (2, d.data_ptr(), 12, e, 2, 2, C.byref(_c_spec(f16)), None, d.data_ptr() + 257, 12),
                 (2, d.data_ptr(), 12, e, 2, 2, C.byref(ok), None, d.data_ptr() + 256, 11),
                 (2, d.data_ptr(), 11, e, 2, 2, C.byref(ok), None, d.data_ptr() + 256, 12),
                 (2, None, 12, e, 2, 2, C.byref(ok), None, d.data_ptr() + 256, 12),
                 (2, d.data_ptr(), 12, e, 2, 2, C.byref(ok), None, None, 12)):
        assert lib.jpeg_amd_resize_tensor_batch(ctx.handle, *args) == _lib.EINVAL
    ctx.synchronize()
    assert out.untouched() and out16.untouched() and (d == SENTINEL).all()

    assert call() == 0                                                                    # the context is usable
    u = J.decode_resized(ctx, (131, 65), resize_py_layout("420"), planes, dq, good, (out_w, out_h)).cpu().numpy()
    for i, g in enumerate(out.images()):
        _same(g, T.normalise(u[i], f32, [1, 0][i]), i)


def test_an_empty_batch_is_ok(ctx, torch):
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    spec = _c_spec(T.Spec(T.BF16, T.CHW))
    assert _lib.lib().jpeg_amd_resize_tensor_batch(ctx.handle, 0, None, 0, None, 4, 4, C.byref(spec), None, out.data_ptr(), 0) == 0
    L = c_layout(33, 17, FACTORS["420"])
    assert _lib.lib().jpeg_amd_decode_tensor_batch(ctx.handle, C.byref(L), 0, None, None, None, 0, 2, 0, _lib.COLOR_RGB8, None, 4, 4,
                                                   C.byref(spec), None, out.data_ptr(), 0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all()
