"""The antialiased resample on the MI355X (the six *_filter_* calls; k_tables_bytes, k_tables_tensor): every output is
compared byte for byte, or element for element as a bit pattern, with _antialias_ref -- the contract of include/jpeg_amd.h
("antialiased resample") restated in numpy -- applied to the source bytes or to what the existing view decode returns for the
same views; tensors go through _tensor_ref's output stage.  With JPEG_AMD_FILTER_BILINEAR the six calls must be the calls they
are named after.  Every output buffer is filled with a sentinel before the call, and the bytes between and behind the images
are checked after it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _antialias_ref as A
import _tensor_ref as T
import jpeg_amd as J
from _calls import (FUSED, RESIZE_EXTENTS, RESIZE_SIZE, RESIZE_TILE_H as TILE_H, RESIZE_TILE_W as TILE_W, RESIZE_VIEWS, SENTINEL,
                    Out, c_layout, c_views, pixel_image, plane_ptrs, resize_py_layout, strides, synthetic)
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _mixed import c_images
from _resample import c_bytes as _c_flips, c_spec as _c_spec, host_bits, pack as _pack, same as _same
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

AA, BILINEAR = _lib.FILTER_ANTIALIAS, _lib.FILTER_BILINEAR
CHUNK = 32                                                  # source rows per chunk of the kernel's walk (antialias.hpp)
# (out_w, out_h, bytes between the output images beyond 3 out_w out_h).  (13, 5, 2): 39-byte rows at an odd stride, so no run
# is aligned; (64, 32): one exact tile; (70, 67): partial tiles on both axes and three tile rows
TARGETS = [(1, 1, 0), (5, 3, 4), (13, 5, 2), (TILE_W, TILE_H, 0), (TILE_W + 6, 2 * TILE_H + 3, 1)]
ELEM = {T.F32: 4, T.F16: 2, T.BF16: 2}
COMBOS = [(d, l) for d in T.DTYPES for l in T.LAYOUTS]
COMBO_IDS = ["%s-%s" % ({T.F32: "f32", T.F16: "f16", T.BF16: "bf16"}[d], {T.HWC: "hwc", T.CHW: "chw"}[l]) for d, l in COMBOS]


def _extents(out_w, out_h):
    """The six sources of one call for a target: upscaled (k < 1 where the target is larger than a pixel), the identity, a
    factor inside (1, 2), 2 exactly, 16 -- the tap limit -- and a single pixel."""
    return [(max(out_w * 3 // 5, 1), max(out_h * 2 // 3, 1)), (out_w, out_h), (out_w * 3 // 2 + 1, out_h * 5 // 3 + 1),
            (2 * out_w, 2 * out_h), (16 * out_w, 16 * out_h), (1, 1)]


@functools.lru_cache(maxsize=None)
def _sources(content, out_w, out_h):
    return tuple(pixel_image(content, w, h, 100 * w + h) for w, h in _extents(out_w, out_h))


@functools.lru_cache(maxsize=None)
def _resampled(content, out_w, out_h):
    """The byte images of the contract for the sources of a target: computed once, shared, never written to."""
    out = tuple(A.resize(image, out_w, out_h) for image in _sources(content, out_w, out_h))
    for o in out:
        o.setflags(write=False)
    return out


def _filter_call(ctx, torch, images, out_w, out_h, filter=AA, gap=0, src_gap=3, expect=0):
    """jpeg_amd_resize_filter_batch on host images [h, w, 3] -> the outputs as host arrays; the sentinel in every byte of the
    output buffer that belongs to no image is asserted here."""
    d_src, src_stride, ext = _pack(ctx, torch, images, src_gap)
    out = Out(ctx, torch, [3 * out_w * out_h] * len(images), gap=gap, tail=7)
    assert _lib.lib().jpeg_amd_resize_filter_batch(ctx.handle, len(images), d_src.data_ptr(), src_stride, ext, out_w, out_h, filter,
                                                   out.ptr, out.stride) == expect
    if expect != 0:
        ctx.synchronize()
        assert out.untouched()
        return None
    return [g.reshape(out_h, out_w, 3) for g in out.images()]


def _bits(out, spec, out_w, out_h):
    """The images of a tensor call's Out as bit patterns in the spec's layout (the sentinel is asserted by Out.images)."""
    shape = (3, out_h, out_w) if spec.layout == T.CHW else (out_h, out_w, 3)
    return [host_bits(b, spec).reshape(shape) for b in out.images()]


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------

def test_the_sources_of_a_call_hold_every_kind_of_factor():
    for out_w, out_h, _ in TARGETS[1:]:
        ext = _extents(out_w, out_h)
        kx = [w / out_w for w, _ in ext]
        assert kx[0] < 1 and kx[1] == 1 and 1 < kx[2] < 2 and kx[3] == 2 and kx[4] == 16 and ext[5] == (1, 1)
        assert len(set(ext)) == len(ext)
    assert 2 * (2 * TILE_H + 3) < 140 <= 16 * (2 * TILE_H + 3)       # (70, 67): at 16 a tile's footprint crosses chunk boundaries
    assert (3 * 13) % 4 != 0 and (3 * 13 * 5 + 2) % 2 == 1            # (13, 5, 2): runs at every alignment


@pytest.mark.parametrize("target", TARGETS, ids=["%dx%d+%d" % t for t in TARGETS])
@pytest.mark.parametrize("content", ["random", "checker"])
def test_kernel_matches_the_contract(ctx, torch, content, target):
    out_w, out_h, gap = target
    got = _filter_call(ctx, torch, list(_sources(content, out_w, out_h)), out_w, out_h, gap=gap)
    for ext, g, want in zip(_extents(out_w, out_h), got, _resampled(content, out_w, out_h)):
        _same(g, want, (content, ext, target))


@pytest.mark.parametrize("height", [16 * TILE_H, 16 * TILE_H - 5])
def test_a_footprint_of_many_chunks_for_a_single_tile(ctx, torch, height):
    """One tile whose vertical footprint is the whole source, sixteen chunks of it: ky = 16 exactly, and 15.84, where neither
    the taps nor the image end on a chunk boundary.  (A source of 16 x 32 + 5 rows is ky = 16.16: over the limit, refused
    below.)"""
    assert height > CHUNK * 15 and np.float32(height) / np.float32(TILE_H) <= 16
    images = [pixel_image("random", 37, height, height), pixel_image("checker", 70, height, 0)]
    got = _filter_call(ctx, torch, images, 9, TILE_H, gap=1)
    for image, g in zip(images, got):
        _same(g, A.resize(image, 9, TILE_H), (image.shape, height))
    assert _filter_call(ctx, torch, [pixel_image("random", 9, 16 * TILE_H + 5, 1)], 9, TILE_H, expect=_lib.ENOSUP) is None


def test_identity_size_returns_the_source_bytes(ctx, torch):
    for w, h in [(1, 1), (7, 9), (TILE_W + 1, TILE_H + 1)]:
        image = pixel_image("random", w, h, w + h)
        got = _filter_call(ctx, torch, [image, image[::-1].copy()], w, h, gap=1)
        assert (got[0] == image).all() and (got[1] == image[::-1]).all(), (w, h)


# ---- 2. the tensor form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_tensor_form_matches_the_contract(ctx, torch, combo):
    out_w, out_h, gap = TILE_W + 6, TILE_H + 3, 3             # a flip across the partial last tile column
    spec = T.Spec(*combo)
    images = list(_sources("random", out_w, out_h))
    flips = [i & 1 for i in range(len(images))]
    d_src, src_stride, ext = _pack(ctx, torch, images, 3)
    out = Out(ctx, torch, [3 * out_w * out_h] * len(images), elem=ELEM[spec.dtype], gap=gap, tail=7)
    assert _lib.lib().jpeg_amd_resize_filter_tensor_batch(ctx.handle, len(images), d_src.data_ptr(), src_stride, ext, out_w, out_h, AA,
                                                          C.byref(_c_spec(spec)), _c_flips(flips), out.ptr, out.stride) == 0
    for i, (g, u) in enumerate(zip(_bits(out, spec, out_w, out_h), _resampled("random", out_w, out_h))):
        _same(g, T.normalise(u, spec, flips[i]), (combo, i))


# ---- 3. the bilinear filter through the new calls is the old call ------------------------------------------------------------------

def test_the_bilinear_filter_is_the_call_it_is_named_after(ctx, torch):
    lib = _lib.lib()
    images = [pixel_image("random", w, h, 100 * w + h) for w, h in RESIZE_EXTENTS]
    n = len(images)
    d_src, src_stride, ext = _pack(ctx, torch, images, 3)
    out_w, out_h = 13, 5
    spec, flips = _c_spec(T.Spec(T.F16, T.CHW)), _c_flips([0, 1, 0, 1, 1])

    def pair(elem=1):
        return [Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=2, tail=7) for _ in range(2)]

    def same(old, new):
        assert all((a == b).all() for a, b in zip(old.images(), new.images()))

    old, new = pair()
    assert lib.jpeg_amd_resize_batch(ctx.handle, n, d_src.data_ptr(), src_stride, ext, out_w, out_h, old.ptr, old.stride) == 0
    assert lib.jpeg_amd_resize_filter_batch(ctx.handle, n, d_src.data_ptr(), src_stride, ext, out_w, out_h, BILINEAR, new.ptr,
                                            new.stride) == 0
    same(old, new)
    old, new = pair(2)
    assert lib.jpeg_amd_resize_tensor_batch(ctx.handle, n, d_src.data_ptr(), src_stride, ext, out_w, out_h, C.byref(spec), flips,
                                            old.ptr, old.stride) == 0
    assert lib.jpeg_amd_resize_filter_tensor_batch(ctx.handle, n, d_src.data_ptr(), src_stride, ext, out_w, out_h, BILINEAR,
                                                   C.byref(spec), flips, new.ptr, new.stride) == 0
    same(old, new)

    L = c_layout(RESIZE_SIZE[0], RESIZE_SIZE[1], FUSED["420"])
    planes, dq, ntables = synthetic(ctx, torch, L, n, 17)
    head = (ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0,
            _lib.COLOR_RGB8, c_views(RESIZE_VIEWS), out_w, out_h)
    old, new = pair()
    assert lib.jpeg_amd_decode_resized_batch(*head, old.ptr, old.stride) == 0
    assert lib.jpeg_amd_decode_resized_filter_batch(*head, BILINEAR, new.ptr, new.stride) == 0
    same(old, new)
    old, new = pair(2)
    assert lib.jpeg_amd_decode_tensor_batch(*head, C.byref(spec), flips, old.ptr, old.stride) == 0
    assert lib.jpeg_amd_decode_tensor_filter_batch(*head, BILINEAR, C.byref(spec), flips, new.ptr, new.stride) == 0
    same(old, new)

    mixed = (ctx.handle, n, c_images([(L, [p[i].data_ptr() for p in planes], dq[i].data_ptr(), ntables) for i in range(n)]), 0,
             _lib.COLOR_RGB8, c_views(RESIZE_VIEWS), out_w, out_h)
    old, new = pair()
    assert lib.jpeg_amd_decode_resized_mixed(*mixed, old.ptr, old.stride) == 0
    assert lib.jpeg_amd_decode_resized_filter_mixed(*mixed, BILINEAR, new.ptr, new.stride) == 0
    same(old, new)
    old, new = pair(2)
    assert lib.jpeg_amd_decode_tensor_mixed(*mixed, C.byref(spec), flips, old.ptr, old.stride) == 0
    assert lib.jpeg_amd_decode_tensor_filter_mixed(*mixed, BILINEAR, C.byref(spec), flips, new.ptr, new.stride) == 0
    same(old, new)


# ---- 4. decode + resample ---------------------------------------------------------------------------------------------------------

VIEWS = [(1, 10, 20, 100, 200), (2, 3, 5, 60, 100), (8, 0, 0, 17, 33)]      # denominators 1, 2 and 8 of a 131 x 257 image


@pytest.mark.parametrize("name", ["420", "y8"])
def test_decode_resized_is_the_view_decode_resampled(ctx, torch, name):
    L = c_layout(RESIZE_SIZE[0], RESIZE_SIZE[1], FUSED[name])
    n = len(VIEWS)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 17)
    decoded = [v.cpu().numpy() for v in J.decode_views(ctx, RESIZE_SIZE, resize_py_layout(name), planes, dq, VIEWS)]
    for out_w, out_h, gap in [(24, 20, 0), (7, 13, 3)]:
        out = Out(ctx, torch, [3 * out_w * out_h] * n, gap=gap, tail=5)
        assert _lib.lib().jpeg_amd_decode_resized_filter_batch(
            ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0,
            _lib.COLOR_RGB8, c_views(VIEWS), out_w, out_h, AA, out.ptr, out.stride) == 0
        for i, (g, d) in enumerate(zip(out.images(), decoded)):
            _same(g.reshape(out_h, out_w, 3), A.resize(d, out_w, out_h), (name, out_w, out_h, i))


def test_the_mixed_tensor_call_is_the_uniform_call_image_by_image(ctx, torch):
    cases = [("420", (300, 140), (2, 5, 3, 140, 60)), ("y8", (131, 257), (1, 0, 0, 131, 257)), ("444", (64, 48), (8, 1, 1, 6, 4))]
    out_w, out_h = 24, 20
    spec, flips = _c_spec(T.Spec(T.BF16, T.HWC)), [1, 0, 1]
    images, want = [], []
    for i, (name, size, view) in enumerate(cases):
        L = c_layout(size[0], size[1], FUSED[name])
        planes, dq, ntables = synthetic(ctx, torch, L, 1, 900 + i)
        images.append((L, [p.data_ptr() for p in planes], dq.data_ptr(), ntables, planes, dq))
        one = Out(ctx, torch, [3 * out_w * out_h], elem=2, tail=8)
        assert _lib.lib().jpeg_amd_decode_tensor_filter_batch(
            ctx.handle, C.byref(L), 1, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0,
            _lib.COLOR_RGB8, c_views([view]), out_w, out_h, AA, C.byref(spec), _c_flips(flips[i:i + 1]), one.ptr, 0) == 0
        want.append(one.images()[0])
    views = [c[2] for c in cases]
    out = Out(ctx, torch, [3 * out_w * out_h] * 3, elem=2, gap=5, tail=8)
    assert _lib.lib().jpeg_amd_decode_tensor_filter_mixed(ctx.handle, 3, c_images([im[:4] for im in images]), 0, _lib.COLOR_RGB8,
                                                          c_views(views), out_w, out_h, AA, C.byref(spec), _c_flips(flips), out.ptr,
                                                          out.stride) == 0
    for i, (g, w) in enumerate(zip(out.images(), want)):
        assert (g == w).all(), i
    # ... and the bytes of the mixed byte call are the view decode's through the reference
    bytes_out = Out(ctx, torch, [3 * out_w * out_h] * 3, gap=1, tail=8)
    assert _lib.lib().jpeg_amd_decode_resized_filter_mixed(ctx.handle, 3, c_images([im[:4] for im in images]), 0, _lib.COLOR_RGB8,
                                                           c_views(views), out_w, out_h, AA, bytes_out.ptr, bytes_out.stride) == 0
    T_spec = T.Spec(T.BF16, T.HWC)
    for i, ((name, size, view), g) in enumerate(zip(cases, bytes_out.images())):
        L, _, _, ntables, planes, dq = images[i]
        decoded = Out(ctx, torch, [3 * view[3] * view[4]], tail=8)
        assert _lib.lib().jpeg_amd_decode_view_batch(ctx.handle, C.byref(L), 1, plane_ptrs(planes), _lib.size_array(strides(L)),
                                                     dq.data_ptr(), ntables * 64, ntables, 0, _lib.COLOR_RGB8, c_views([view]),
                                                     decoded.ptr, 0) == 0
        u = A.resize(decoded.images()[0].reshape(view[4], view[3], 3), out_w, out_h)
        _same(g.reshape(out_h, out_w, 3), u, (name, "bytes"))
        _same(want[i].copy().view(np.uint16).reshape(out_h, out_w, 3), T.normalise(u, T_spec, flips[i]), (name, "tensor"))


# ---- 5. empty batch; refused calls ------------------------------------------------------------------------------------------------

def test_an_empty_batch_is_ok(ctx, torch):
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    spec = _c_spec(T.Spec(T.F32, T.CHW))
    lib = _lib.lib()
    assert lib.jpeg_amd_resize_filter_batch(ctx.handle, 0, None, 0, None, 4, 4, AA, out.data_ptr(), 0) == 0
    assert lib.jpeg_amd_resize_filter_tensor_batch(ctx.handle, 0, None, 0, None, 4, 4, AA, C.byref(spec), None, out.data_ptr(), 0) == 0
    L = c_layout(33, 17, FUSED["420"])
    assert lib.jpeg_amd_decode_resized_filter_batch(ctx.handle, C.byref(L), 0, None, None, None, 0, 2, 0, _lib.COLOR_RGB8, None,
                                                    4, 4, AA, out.data_ptr(), 0) == 0
    assert lib.jpeg_amd_decode_tensor_filter_mixed(ctx.handle, 0, None, 0, _lib.COLOR_RGB8, None, 4, 4, AA, C.byref(spec), None,
                                                   out.data_ptr(), 0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all()


def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    images = [pixel_image("random", 9, 7, 1), pixel_image("random", 161, 11, 2)]
    assert _filter_call(ctx, torch, images, 10, 4, expect=_lib.ENOSUP) is None          # kx = 16.1 in the second image
    assert _filter_call(ctx, torch, images[::-1], 20, 1, expect=0) is not None          # ky = 11: inside the limit
    assert _filter_call(ctx, torch, images, 20, 4, filter=2, expect=_lib.EINVAL) is None
    assert _filter_call(ctx, torch, images, 20, 4, filter=-1, expect=_lib.EINVAL) is None
    assert _filter_call(ctx, torch, images, 0, 4, expect=_lib.EINVAL) is None
    got = _filter_call(ctx, torch, images, 11, 4, gap=1)
    for image, g in zip(images, got):
        _same(g, A.resize(image, 11, 4), image.shape)

    # the decode form: the limit in the LAST view of the batch, judged by the view's own size
    L = c_layout(RESIZE_SIZE[0], RESIZE_SIZE[1], FUSED["420"])
    views = VIEWS[:2] + [(1, 0, 0, 131, 257)]
    planes, dq, ntables = synthetic(ctx, torch, L, 3, 3)
    out = Out(ctx, torch, [3 * 9 * 17] * 3)

    def call(w, h, filter=AA):
        return _lib.lib().jpeg_amd_decode_resized_filter_batch(
            ctx.handle, C.byref(L), 3, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0,
            _lib.COLOR_RGB8, c_views(views), w, h, filter, out.ptr, out.stride)

    assert call(8, 16) == _lib.ENOSUP and call(8, 16, filter=9) == _lib.EINVAL           # 131 / 8 = 16.4 in the third view
    assert call(9, 18) == _lib.EINVAL                                                    # (a stride that is too small)
    ctx.synchronize()
    assert out.untouched()
    assert call(9, 17) == 0                                                              # 14.6 and 15.1
    decoded = J.decode_views(ctx, RESIZE_SIZE, resize_py_layout("420"), planes, dq, views)
    for i, (g, d) in enumerate(zip(out.images(), decoded)):
        _same(g.reshape(17, 9, 3), A.resize(d.cpu().numpy(), 9, 17), i)


# ---- 6. the Python keyword ------------------------------------------------------------------------------------------------------------

def test_python_keyword(ctx, torch):
    L = c_layout(RESIZE_SIZE[0], RESIZE_SIZE[1], FUSED["420"])
    layout = resize_py_layout("420")
    planes, dq, _ = synthetic(ctx, torch, L, 2, 11)
    qh = dq.cpu().numpy().astype(np.uint16)
    sp = [J.Spectral(ctx, RESIZE_SIZE, layout, [p[i] for p in planes], [qh[i, 0], qh[i, 1]], [0, 1, 1]) for i in range(2)]
    view = (2, 3, 5, 60, 100)
    plain = sp[1].view(view[1:], view[0], J.RGB).cpu().numpy()
    one = sp[1].view(view[1:], view[0], J.RGB, size=(32, 20), filter="antialias")
    assert tuple(one.shape) == (20, 32, 3) and (one.cpu().numpy() == A.resize(plain, 32, 20)).all()
    old = sp[1].view(view[1:], view[0], J.RGB, size=(32, 20))
    assert (old.cpu().numpy() == sp[1].view(view[1:], view[0], J.RGB, size=(32, 20), filter="bilinear").cpu().numpy()).all()
    assert (old.cpu().numpy() != one.cpu().numpy()).any()                     # the default is today's filter, not this one
    batch = J.decode_resized(ctx, RESIZE_SIZE, layout, planes, dq, [view, view], (32, 20), filter="antialias").cpu().numpy()
    assert (batch[1] == one.cpu().numpy()).all()

    source = [(10, 7, 100, 200), (3, 100, 70, 150)]
    out_size = (24, 20)
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    flips = [1, 0]
    for name in ("antialias", "bilinear"):
        tensor, chosen = J.decode_crops_tensor_mixed(ctx, sp, source, out_size, spec, flips=flips, filter=name)
        default, chosen_default = J.decode_crops_tensor_mixed(ctx, sp, source, out_size, spec, flips=flips)
        assert chosen.tolist() == chosen_default.tolist()                    # the denominators do not depend on the filter
        assert (name == "bilinear") == bool((tensor.view(torch.int16) == default.view(torch.int16)).all())
    tensor, chosen = J.decode_crops_tensor_mixed(ctx, sp, source, out_size, spec, flips=flips, filter="antialias")
    want_spec = T.Spec(T.F16, T.CHW, mean=[spec.mean[c] for c in range(3)], scale=[spec.scale[c] for c in range(3)])
    for i in range(2):
        decoded = sp[i].view(tuple(int(v) for v in chosen[i, 1:]), int(chosen[i, 0]), J.RGB).cpu().numpy()
        want = T.normalise(A.resize(decoded, *out_size), want_spec, flips[i])
        _same(tensor[i].view(torch.int16).cpu().numpy().view(np.uint16), want, i)

    images = [torch.from_numpy(pixel_image("random", w, h, w)).to(ctx.torch_device) for w, h in RESIZE_EXTENTS[:4]]
    got = J.resize(ctx, images, (31, 9), filter="antialias")
    for g, im in zip(got.cpu().numpy(), images):
        assert (g == A.resize(im.cpu().numpy(), 31, 9)).all()
    both = J.resize_tensor(ctx, images, (31, 9), spec, flips=[0, 1, 0, 1], filter="antialias")
    for i, im in enumerate(images):
        want = T.normalise(A.resize(im.cpu().numpy(), 31, 9), want_spec, i & 1)
        _same(both[i].view(torch.int16).cpu().numpy().view(np.uint16), want, i)
    with pytest.raises(ValueError):
        J.resize(ctx, images, (31, 9), filter="lanczos")
    with pytest.raises(J.JpegAmdError):
        J.resize(ctx, images, (8, 9), filter="antialias")                    # 131 / 8 > 16
