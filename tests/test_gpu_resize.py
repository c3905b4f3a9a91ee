"""Resized decode on the MI355X (jpeg_amd_resize_batch, jpeg_amd_decode_resized_batch; k_resize_bilinear): every output is
compared byte for byte with _resize_ref -- the contract of include/jpeg_amd.h restated in numpy -- applied to the source
bytes or to what the existing view decode returns for the same views.  Every output buffer is filled with a sentinel before
the call and the bytes between and behind the images are checked after it."""
import ctypes as C

import numpy as np
import pytest

import _resize_ref as R
import jpeg_amd as J
from _calls import (RESIZE_CONTENTS as CONTENTS, RESIZE_EXTENTS as EXTENTS, RESIZE_FACTORS as FACTORS, RESIZE_SIZE as SIZE,
                    RESIZE_TILE_H as TILE_H, RESIZE_TILE_W as TILE_W, RESIZE_VIEWS as VIEWS, SENTINEL, Out, c_layout, pixel_image,
                    resize_py_layout, resized_call, synthetic)
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import pack
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

RUN = 4                                                     # output pixels per work-item: 12 bytes, three dwords
# (out_w, out_h, bytes between the output images beyond 3 out_w out_h).  (13, 5): 39-byte rows at an odd stride -- runs that
# start at every alignment, and a last run of one pixel; (TILE_W + 6, 2 * TILE_H + 3): two tiles across, three down
TARGETS = [(1, 1, 0), (5, 3, 4), (224, 224, 0), (13, 5, 2), (TILE_W + 6, 2 * TILE_H + 3, 1)]
def _resize_call(ctx, torch, images, out_w, out_h, gap=0, src_gap=0, expect=0):
    """jpeg_amd_resize_batch on host images [h, w, 3] -> the outputs as host arrays; the sentinel in every byte of the output
    buffer that belongs to no image is asserted here."""
    n = len(images)
    d_src, src_stride, ext = pack(ctx, torch, images, src_gap)
    out = Out(ctx, torch, [3 * max(out_w, 0) * max(out_h, 0)] * n, gap=gap, tail=7)
    assert _lib.lib().jpeg_amd_resize_batch(ctx.handle, n, d_src.data_ptr(), src_stride, ext, out_w, out_h, out.ptr,
                                            out.stride) == expect
    if expect != 0:
        assert out.untouched()
        return None
    return [g.reshape(out_h, out_w, 3) for g in out.images()]


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("target", TARGETS, ids=["%dx%d+%d" % t for t in TARGETS])
@pytest.mark.parametrize("content", CONTENTS)
def test_kernel_matches_the_contract(ctx, torch, content, target):
    out_w, out_h, gap = target
    assert (out_w, out_h) != (TILE_W + 6, 2 * TILE_H + 3) or (out_w > TILE_W and out_h > 2 * TILE_H)
    assert (out_w, out_h) != (13, 5) or ((3 * out_w) % 4 != 0 and (3 * out_w * out_h + gap) % 2 == 1 and out_w % RUN == 1)
    images = [pixel_image(content, w, h, 100 * w + h) for w, h in EXTENTS]
    got = _resize_call(ctx, torch, images, out_w, out_h, gap=gap, src_gap=3)
    for (w, h), image, g in zip(EXTENTS, images, got):
        assert (g == R.resize(image, out_w, out_h)).all(), (content, (w, h), target)


def test_identity_size_returns_the_source_bytes(ctx, torch):
    for w, h in EXTENTS + [(TILE_W + 1, TILE_H + 1)]:
        image = pixel_image("random", w, h, w + h)
        got = _resize_call(ctx, torch, [image, image[::-1].copy()], w, h, gap=1)
        assert (got[0] == image).all() and (got[1] == image[::-1]).all(), (w, h)


def test_upscaling_and_a_source_far_larger_than_the_target(ctx, torch):
    images = [pixel_image("random", 3, 2, 1), pixel_image("random", 1000, 40, 2)]
    for out_w, out_h in [(97, 33), (4, 3)]:
        got = _resize_call(ctx, torch, images, out_w, out_h)
        for image, g in zip(images, got):
            assert (g == R.resize(image, out_w, out_h)).all(), (image.shape, out_w, out_h)


# ---- 2. decode + resample -------------------------------------------------------------------------------------------------------

def _check_images(out, out_w, out_h, want, what):
    """The first len(want) images of `out` are `want`; the sentinel in every byte that belongs to no image of `out`."""
    for got, w, i in zip(out.images(), want, range(len(want))):
        assert (got.reshape(out_h, out_w, 3) == w).all(), (what, i)


@pytest.mark.parametrize("name", sorted(FACTORS))
def test_decode_resized_is_the_view_decode_resampled(ctx, torch, name):
    L = c_layout(SIZE[0], SIZE[1], FACTORS[name])
    cosited = 1 if name.endswith("cosited") else 0
    n = len(VIEWS)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 17)
    assert sorted({v[0] for v in VIEWS}) == [1, 2, 4, 8]
    for color in (J.RGB, J.YCbCr):
        decoded = [v.cpu().numpy() for v in J.decode_views(ctx, SIZE, resize_py_layout(name), planes, dq, VIEWS, color=color,
                                                          cosite=bool(cosited))]
        for out_w, out_h, gap in [(32, 32, 0), (7, 5, 3)]:
            want = [R.resize(d, out_w, out_h) for d in decoded]
            out = Out(ctx, torch, [3 * out_w * out_h] * n, gap=gap, tail=5)
            assert resized_call(ctx, L, planes, dq, ntables, cosited, color.code, VIEWS, out_w, out_h, out.ptr, out.stride) == 0
            _check_images(out, out_w, out_h, want, (name, color.__name__, out_w, out_h))


def test_decode_crops_resized_picks_the_views_and_decodes_them(ctx, torch):
    L = c_layout(SIZE[0], SIZE[1], FACTORS["420"])
    layout = resize_py_layout("420")
    source = [(0, 0, 131, 257), (10, 7, 100, 200), (90, 30, 41, 35), (3, 100, 70, 150), (64, 128, 9, 6)]
    planes, dq, _ = synthetic(ctx, torch, L, len(source), 23)
    out_size = (16, 20)
    got, views = J.decode_crops_resized(ctx, SIZE, layout, planes, dq, source, out_size, color=J.YCbCr)
    want_views = [(J.view_denom(s[2:], out_size),) for s in source]
    want_views = [d + J.view_of_source(SIZE, d[0], s) for d, s in zip(want_views, source)]
    assert views.dtype == np.int32 and views.tolist() == [list(v) for v in want_views]
    assert [v[0] for v in want_views] == [8, 4, 1, 4, 1]
    assert tuple(got.shape) == (len(source), 20, 16, 3) and got.dtype == torch.uint8
    decoded = J.decode_views(ctx, SIZE, layout, planes, dq, want_views, color=J.YCbCr)
    got = got.cpu().numpy()
    for i, d in enumerate(decoded):
        assert (got[i] == R.resize(d.cpu().numpy(), 16, 20)).all(), i
    same = J.decode_resized(ctx, SIZE, layout, planes, dq, want_views, out_size, color=J.YCbCr)
    assert (same.cpu().numpy() == got).all()


@pytest.mark.parametrize("name", ["420", "420-cosited"])
def test_two_calls_queued_back_to_back_on_a_fresh_context(torch, name):
    """No synchronise between the calls, the second with larger views and more images than the first: the context's
    intermediate and its record buffer both grow (a synchronise, a free and an allocation inside the second call) while the
    first call's kernels may still be running from them; the view call in between regrows the scratch and restages its
    rectangles.  Both results must be the contract's."""
    ctx = J.Context(0)
    L = c_layout(SIZE[0], SIZE[1], FACTORS[name])
    cosited = 1 if name.endswith("cosited") else 0
    small = [(4, 1, 1, 9, 7), (8, 0, 0, 5, 5)]
    large = [(1, 0, 0, 131, 257), (2, 1, 1, 64, 120), (1, 3, 3, 120, 250)] + [(2, 0, 0, 66, 129)] * 253
    n = len(large)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 5)
    out_w, out_h = 24, 40
    outs = [Out(ctx, torch, [3 * out_w * out_h] * len(v), tail=5) for v in (small, large)]
    decoded = [[d.cpu().numpy() for d in J.decode_views(ctx, SIZE, resize_py_layout(name), [p[:len(v)] for p in planes], dq[:len(v)], v,
                                                        cosite=bool(cosited))] for v in (small[:2], large[:4])]
    ctx.close()
    ctx = J.Context(0)                                      # nothing allocated yet: both calls grow the buffers
    for views, out in zip((small, large), outs):
        assert resized_call(ctx, L, planes, dq, ntables, cosited, _lib.COLOR_RGB8, views, out_w, out_h, out.ptr, out.stride) == 0
    _check_images(outs[0], out_w, out_h, [R.resize(d, out_w, out_h) for d in decoded[0]], (name, "first"))
    want = [R.resize(d, out_w, out_h) for d in decoded[1]]
    _check_images(outs[1], out_w, out_h, want, (name, "second"))      # the first 4 of n, and the sentinel behind the last
    # images 3 .. n - 1 of the second call have the same view of different images: checked against the view decode alone
    rest = J.decode_views(ctx, SIZE, resize_py_layout(name), [p[250:] for p in planes], dq[250:], large[250:], cosite=bool(cosited))
    tail = outs[1].images()[250:]
    for i, d in enumerate(rest):
        assert (tail[i].reshape(out_h, out_w, 3) == R.resize(d.cpu().numpy(), out_w, out_h)).all(), (name, 250 + i)
    ctx.close()


# ---- 3. empty batch; invalid calls ------------------------------------------------------------------------------------------------

def test_an_empty_batch_is_ok(ctx, torch):
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    assert _lib.lib().jpeg_amd_resize_batch(ctx.handle, 0, None, 0, None, 4, 4, out.data_ptr(), 0) == 0
    L = c_layout(33, 17, FACTORS["420"])
    assert _lib.lib().jpeg_amd_decode_resized_batch(ctx.handle, C.byref(L), 0, None, None, None, 0, 2, 0, _lib.COLOR_RGB8, None,
                                                    4, 4, out.data_ptr(), 0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all()


def test_invalid_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    lib = _lib.lib()
    images = [pixel_image("random", 9, 7, 1), pixel_image("random", 5, 11, 2)]
    for kw in ({"out_w": 0}, {"out_h": 0}, {"out_w": -1}, {"gap": -1}, {"src_gap": -1}):
        args = {"out_w": 6, "out_h": 4, **kw}
        assert _resize_call(ctx, torch, images, expect=_lib.EINVAL, **args) is None
    d = torch.full((512,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    for ext in ((0, 7), (9, 0), (-9, 7)):
        e = (_lib.Extent * 2)(_lib.Extent(*ext), _lib.Extent(5, 11))
        assert lib.jpeg_amd_resize_batch(ctx.handle, 2, d.data_ptr(), 0, e, 2, 2, d.data_ptr() + 256, 12) == _lib.EINVAL
    e = (_lib.Extent * 1)(_lib.Extent(2, 2))
    assert lib.jpeg_amd_resize_batch(ctx.handle, 65536, d.data_ptr(), 12, e, 2, 2, d.data_ptr() + 256, 12) == _lib.EINVAL
    assert lib.jpeg_amd_resize_batch(ctx.handle, 1, None, 12, e, 2, 2, d.data_ptr() + 256, 12) == _lib.EINVAL
    ctx.synchronize()
    assert (d == SENTINEL).all()

    L = c_layout(131, 65, FACTORS["420"])
    good = [(2, 3, 5, 20, 9), (4, 1, 1, 20, 9), (8, 0, 0, 17, 9), (1, 100, 40, 20, 9)]
    n = len(good)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 3)
    out_w, out_h = 10, 6
    out = Out(ctx, torch, [3 * out_w * out_h] * n)
    stride = out.stride

    def call(views=good, layout=None, w=out_w, h=out_h, ptr=out.ptr, s=stride):
        return resized_call(ctx, L, planes, dq, ntables, 0, _lib.COLOR_RGB8, views, w, h, ptr, s, layout=layout)

    for denom in (0, 3, 16):                                # what the view call refuses, in the LAST image of the batch
        assert call(views=good[:3] + [(denom, 0, 0, 17, 9)]) == _lib.EINVAL
    assert call(views=good[:3] + [(4, 33 - 20 + 1, 1, 20, 9)]) == _lib.EINVAL       # one pixel past W' = 33
    assert call(layout=c_layout(131, 65, FACTORS["420"], precision=12)) == _lib.ENOSUP
    assert call(w=0) == _lib.EINVAL and call(h=0) == _lib.EINVAL
    assert call(s=stride - 1) == _lib.EINVAL
    assert call(ptr=None) == _lib.EINVAL
    ctx.synchronize()
    assert out.untouched()
    assert call() == 0
    decoded = J.decode_views(ctx, (131, 65), resize_py_layout("420"), planes, dq, good)
    _check_images(out, out_w, out_h, [R.resize(v.cpu().numpy(), out_w, out_h) for v in decoded], "valid")
    got = _resize_call(ctx, torch, images, 6, 4)
    assert all((g == R.resize(im, 6, 4)).all() for g, im in zip(got, images))


# ---- 4. the Python API ------------------------------------------------------------------------------------------------------------

def test_python_api(ctx, torch):
    L = c_layout(SIZE[0], SIZE[1], FACTORS["420"])
    layout = resize_py_layout("420")
    planes, dq, _ = synthetic(ctx, torch, L, 2, 11)
    qh = dq.cpu().numpy().astype(np.uint16)
    sp = J.Spectral(ctx, SIZE, layout, [p[1] for p in planes], [qh[1, 0], qh[1, 1]], [0, 1, 1])
    view = (2, 3, 5, 60, 100)
    batch = J.decode_resized(ctx, SIZE, layout, planes, dq, [view, view], (32, 20)).cpu().numpy()
    for cosite in (False, True):
        plain = sp.view(view[1:], view[0], J.RGB, cosite=cosite)
        assert tuple(plain.shape) == (100, 60, 3)          # size=None: the view itself, as before
        one = sp.view(view[1:], view[0], J.RGB, cosite=cosite, size=(32, 20))
        assert tuple(one.shape) == (20, 32, 3)
        assert (one.cpu().numpy() == R.resize(plain.cpu().numpy(), 32, 20)).all()
        assert cosite or (one.cpu().numpy() == batch[1]).all()
    images = [torch.from_numpy(pixel_image("random", w, h, w)).to(ctx.torch_device) for w, h in EXTENTS]
    got = J.resize(ctx, images, (31, 9))
    assert tuple(got.shape) == (len(EXTENTS), 9, 31, 3) and got.dtype == torch.uint8
    for g, im in zip(got.cpu().numpy(), images):
        assert (g == R.resize(im.cpu().numpy(), 31, 9)).all()
    with pytest.raises(J.JpegAmdError):
        sp.view(view[1:], view[0], size=(0, 4))
