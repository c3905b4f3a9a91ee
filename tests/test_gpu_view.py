"""View decode on the MI355X (jpeg_amd_decode_view_batch; k_view_decode and the crop fallback): image i is the image the
scaled contract defines for its denominator, cropped to its rectangle, byte for byte.  The checker is independent of the code
under test: _scaled_ref.decode_scaled cropped in numpy and, at denominator 1, the oracle's full decode cropped.  Every output
buffer is filled with a sentinel before the call and the bytes between and behind the images are checked after it."""
import ctypes as C

import numpy as np
import pytest

import _scaled_ref as S
import jpeg_amd as J
from _calls import COLORS, FUSED, SENTINEL, Out, c_layout, c_regions, c_views, plane_ptrs, strides, synthetic
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _tile import TILE_H, TILE_W, crop as _crop, random_region, reference as _reference
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

DENOMS = (1, 2, 4, 8)

# name -> (factors, cosited)
LAYOUTS = {**{k: (v, 0) for k, v in FUSED.items()}, "411": ([(4, 1), (1, 1), (1, 1)], 0),
           "420-cosited": ([(2, 2), (1, 1), (1, 1)], 1)}
# (1100, 300): the smallest at which the 1/8 image (138 x 38) still spans two tiles on each axis
SIZES = [(1, 1), (7, 9), (17, 33), (131, 257), (1100, 300)]


def _call(ctx, L, n, planes, coef_stride, dq, q_stride, ntables, cosited, color, h_views, out_ptr, stride):
    return _lib.lib().jpeg_amd_decode_view_batch(
        ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(coef_stride),
        dq.data_ptr(), q_stride, ntables, cosited, color, h_views, out_ptr, stride)


def _view_batch(ctx, torch, L, planes, dq, ntables, cosited, color, views, gap=0, distinct=True):
    """One call for `views`, image i from image i of planes / dq (distinct) or every image from image 0.  -> the images as
    host arrays [h_i, w_i, 3]; the sentinel in every byte of the buffer that belongs to no image is asserted here."""
    out = Out(ctx, torch, [3 * r[2] * r[3] for _, r in views], gap=gap, tail=gap)
    assert _call(ctx, L, len(views), planes, strides(L, distinct), dq, ntables * 64 if distinct else 0, ntables, cosited, color,
                 c_views(views), out.ptr, out.stride) == 0
    return [image.reshape(r[3], r[2], 3) for image, (_, r) in zip(out.images(), views)]


def _random_region(rng, W, H, max_w=200, max_h=100):
    return random_region(rng, W, H, max_w, max_h)


def _regions(rng, W, H, N):
    """The rectangles of a (W, H) scaled image, whole image apart: 1 x 1 at each corner; an origin that is no multiple of
    N; one that ends on the last column and row; one that straddles x = 128 and y = 32 and 64 of its own tile grid (as far
    as the image goes); 30 random ones."""
    out = [(0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1)]
    x0, y0 = min(W - 1, N + 1), min(H - 1, 2 * N + 1)
    out.append((x0, y0, min(W - x0, 40), min(H - y0, 20)))
    out.append((max(0, W - 9), max(0, H - 5), min(W, 9), min(H, 5)))
    x0, y0 = min(W - 1, 3 * N + 1), min(H - 1, N + 1)
    out.append((x0, y0, min(W - x0, TILE_W + 12), min(H - y0, 2 * TILE_H + 6)))
    return out + [_random_region(rng, W, H) for _ in range(30)]


# ---- 1. shapes where it can go wrong ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_views_match_the_reference(ctx, torch, name, size):
    factors, cosited = LAYOUTS[name]
    L = c_layout(size[0], size[1], factors)
    planes, dq, ntables = synthetic(ctx, torch, L, 1, size[0] * 31 + size[1])
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    rng = np.random.default_rng(size[0] + 1000 * size[1])
    want = {denom: _reference(L, ph, qh, 0, denom, cosited) for denom in DENOMS}
    whole = [(denom, (0, 0) + S.scaled_size(size, denom)) for denom in DENOMS]
    views = [(denom, r) for denom, (_, _, W1, H1) in whole for r in _regions(rng, W1, H1, 8 // denom)]
    if size == (1100, 300):   # the tile grid is straddled where the image allows: on both axes down to the 1/8 image
        for denom, (_, _, W1, H1) in whole:
            r = _regions(rng, W1, H1, 8 // denom)[6]
            assert r[0] % (8 // denom) + r[2] > TILE_W and r[1] % (8 // denom) + r[3] > (TILE_H if denom == 8 else 2 * TILE_H)
    for color in COLORS:
        # the whole images in a call of their own (four denominators: k_view_decode or the crop, not the scaled call), so
        # that their size does not set the stride of the small ones
        for batch in (whole, views):
            got = _view_batch(ctx, torch, L, planes, dq, ntables, cosited, color, batch, gap=3, distinct=False)
            for (denom, r), image in zip(batch, got):
                assert (image == _crop(want[denom][color], r)).all(), (name, size, color, denom, r)


# ---- 2. mixed denominators --------------------------------------------------------------------------------------------------

def test_a_batch_of_64_with_mixed_denominators(ctx, torch):
    L = c_layout(403, 150, FUSED["420"])
    n, gap = 64, 5
    planes, dq, ntables = synthetic(ctx, torch, L, n, 64)
    ph = [p.cpu().numpy() for p in planes]
    qh = np.ascontiguousarray(dq.cpu().numpy().astype(np.uint16))
    rng = np.random.default_rng(64)
    denoms = [DENOMS[i % 4] for i in range(n)]
    rng.shuffle(denoms)
    assert sorted(denoms) == sorted(DENOMS * 16) and denoms != [DENOMS[i % 4] for i in range(n)]
    views = [(d, _random_region(rng, *S.scaled_size((403, 150), d), max_w=403, max_h=150)) for d in denoms]
    got = _view_batch(ctx, torch, L, planes, dq, ntables, 0, _lib.COLOR_RGB8, views, gap=gap)
    for i, ((denom, r), image) in enumerate(zip(views, got)):
        want = _crop(_reference(L, ph, qh, i, denom, 0)[_lib.COLOR_RGB8], r)
        assert (image == want).all(), (i, denom, r)
        one = torch.full((image.size + 8,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
        view = _lib.View(denom, _lib.Region(*r))
        assert _lib.lib().jpeg_amd_decode_view(ctx.handle, C.byref(L), plane_ptrs([p[i] for p in planes]),
                                               qh[i].ctypes.data, ntables, 0, _lib.COLOR_RGB8, C.byref(view), one.data_ptr()) == 0
        one = one.cpu().numpy()
        assert (one[:image.size] == image.reshape(-1)).all() and (one[image.size:] == SENTINEL).all(), (i, denom, r)


# ---- 3. equality with the existing calls --------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["y8", "420", "422", "411", "420-cosited"])
def test_views_equal_the_existing_calls(ctx, torch, name):
    factors, cosited = LAYOUTS[name]
    size = (131, 65)
    L = c_layout(size[0], size[1], factors)
    n = 5
    planes, dq, ntables = synthetic(ctx, torch, L, n, 33)
    ptrs, coef_strides = plane_ptrs(planes), _lib.size_array(strides(L))
    rng = np.random.default_rng(33)
    lib = _lib.lib()
    for color in COLORS:
        # whole-image views at one denominator: jpeg_amd_decode_scaled_batch's bytes
        for denom in DENOMS:
            w, h = S.scaled_size(size, denom)
            got = _view_batch(ctx, torch, L, planes, dq, ntables, cosited, color, [(denom, (0, 0, w, h))] * n)
            scaled = torch.empty((n, h, w, 3), dtype=torch.uint8, device=ctx.torch_device)
            assert lib.jpeg_amd_decode_scaled_batch(ctx.handle, C.byref(L), n, ptrs, coef_strides, dq.data_ptr(), ntables * 64, ntables,
                                                    cosited, color, denom, scaled.data_ptr(), 3 * w * h) == 0
            scaled = scaled.cpu().numpy()
            assert all((got[i] == scaled[i]).all() for i in range(n)), (name, color, denom)
        # denominator-1 views: jpeg_amd_decode_region_batch's bytes -- in a call of their own, and as the first n images of a
        # call that holds another denominator too, where they run through the view kernel's own N = 8 form
        regions = [_random_region(rng, size[0], size[1]) for _ in range(n)]
        stride = max(3 * r[2] * r[3] for r in regions)
        out = torch.empty((n * stride,), dtype=torch.uint8, device=ctx.torch_device)
        assert lib.jpeg_amd_decode_region_batch(ctx.handle, C.byref(L), n, ptrs, coef_strides, dq.data_ptr(), ntables * 64, ntables,
                                                cosited, color, c_regions(regions), out.data_ptr(), stride) == 0
        out = out.cpu().numpy()
        want = [out[i * stride:i * stride + 3 * r[2] * r[3]].reshape(r[3], r[2], 3) for i, r in enumerate(regions)]
        alone = _view_batch(ctx, torch, L, planes, dq, ntables, cosited, color, [(1, r) for r in regions])
        mixed_views = [(1, r) for r in regions[:n - 1]] + [(2, (1, 1, 9, 5))]
        mixed = _view_batch(ctx, torch, L, planes, dq, ntables, cosited, color, mixed_views)
        for i in range(n):
            assert (alone[i] == want[i]).all(), (name, color, i)
            assert i == n - 1 or (mixed[i] == want[i]).all(), (name, color, i)


@pytest.mark.parametrize("name", ["y8", "444", "420", "422"])
def test_the_two_full_size_kernels_agree_across_their_tile_seams(ctx, torch, name):
    """k_region_decode (128 x 64 tiles) and k_view_decode<8> (128 x 32) run one tile body.  The rectangle's tile grid is
    anchored at (8, 8): it crosses x = 136 and 264, and y = 40, 72 and 104 of the view kernel, y = 72 of the region kernel."""
    size, r = (300, 150), (13, 11, 270, 120)
    L = c_layout(size[0], size[1], FUSED[name])
    planes, dq, ntables = synthetic(ctx, torch, L, 2, 77)
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    want = _reference(L, ph, qh, 0, 1, 0)
    area = 3 * r[2] * r[3]
    for color in COLORS:
        out = torch.full((area + 16,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
        assert _lib.lib().jpeg_amd_decode_region_batch(
            ctx.handle, C.byref(L), 1, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(),
            ntables * 64, ntables, 0, color, (_lib.Region * 1)(_lib.Region(*r)), out.data_ptr(), area) == 0
        out = out.cpu().numpy()
        assert (out[area:] == SENTINEL).all()
        region = out[:area].reshape(r[3], r[2], 3)
        alone = _view_batch(ctx, torch, L, planes, dq, ntables, 0, color, [(1, r)], gap=16)[0]
        mixed = _view_batch(ctx, torch, L, planes, dq, ntables, 0, color, [(1, r), (2, (1, 1, 9, 5))], gap=16)[0]
        for how, got in (("region call", region), ("view alone", alone), ("mixed call", mixed)):
            assert (got == _crop(want[color], r)).all(), (name, color, how)


# ---- 4. unread coefficients do not matter -------------------------------------------------------------------------------------

@pytest.mark.parametrize("denom", [4, 2])
@pytest.mark.parametrize("name", ["y8", "420"])
def test_unread_coefficients_do_not_matter(ctx, torch, name, denom):
    """Every coefficient with k >= N or h >= N (at denominator 4 that holds every k >= 4 or h >= 4), and every block outside
    jpeg_amd_view_window, randomised: the same bytes."""
    N = 8 // denom
    L = c_layout(403, 150, FUSED[name])
    n = 3
    planes, dq, ntables = synthetic(ctx, torch, L, n, 99)
    rng = np.random.default_rng(denom)
    W1, H1 = S.scaled_size((403, 150), denom)
    views = [(denom, r) for r in ((37, 11, 60, 20), (W1 - 31, H1 - 9, 31, 9), _random_region(rng, W1, H1, 150, 60))]
    head = torch.zeros(64, dtype=torch.bool, device=ctx.torch_device)
    head[torch.as_tensor(sorted(int(S.Z[h][k]) for h in range(N) for k in range(N)), device=ctx.torch_device)] = True
    gen = torch.Generator(device=ctx.torch_device).manual_seed(denom)
    noisy = []
    windows = (_lib.Region * _lib.MAX_PLANES)()
    for p, plane in enumerate(planes):
        read = torch.zeros(plane.shape, dtype=torch.bool, device=ctx.torch_device)
        for i, (_, r) in enumerate(views):
            assert _lib.lib().jpeg_amd_view_window(C.byref(L), 0, denom, C.byref(_lib.Region(*r)), windows) == 0
            w = windows[p]
            assert w.width > 0 and w.height > 0 and w.x + w.width <= L.units_x[p] and w.y + w.height <= L.units_y[p]
            read[i, w.y:w.y + w.height, w.x:w.x + w.width] = head
        noise = torch.randint(-32768, 32768, plane.shape, dtype=torch.int32, device=ctx.torch_device, generator=gen).to(torch.int16)
        assert 0 < int(read.sum()) < read.numel() // 4
        noisy.append(torch.where(read, plane, noise).contiguous())
    for color in COLORS:
        a = _view_batch(ctx, torch, L, planes, dq, ntables, 0, color, views)
        b = _view_batch(ctx, torch, L, noisy, dq, ntables, 0, color, views)
        assert all((x == y).all() for x, y in zip(a, b)), (name, denom, color)


# ---- 5. empty batch; invalid calls --------------------------------------------------------------------------------------------

def test_an_empty_batch_is_ok(ctx, torch):
    L = c_layout(33, 17, FUSED["420"])
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    assert _lib.lib().jpeg_amd_decode_view_batch(ctx.handle, C.byref(L), 0, None, None, None, 0, 2, 0, _lib.COLOR_RGB8, None,
                                                 out.data_ptr(), 0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all()


def test_invalid_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    L = c_layout(131, 65, FUSED["420"])
    n = 4
    planes, dq, ntables = synthetic(ctx, torch, L, n, 3)
    good = [(2, (3, 5, 20, 9)), (4, (1, 1, 20, 9)), (8, (0, 0, 17, 9)), (1, (100, 40, 20, 9))]
    stride = 3 * 20 * 9
    out = torch.full((n * stride,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)

    def call(views=good, layout=L, ptr=out.data_ptr(), s=stride):
        return _call(ctx, layout, n, planes, strides(L), dq, ntables * 64, ntables, 0, _lib.COLOR_RGB8, c_views(views), ptr, s)

    for denom in (0, 3, 16, -1):                           # a bad denominator in the middle of the batch
        assert call(views=good[:2] + [(denom, (0, 0, 17, 9))] + good[3:]) == _lib.EINVAL
    assert call(views=good[:1] + [(4, (33 - 20 + 1, 1, 20, 9))] + good[2:]) == _lib.EINVAL   # one pixel past W' = 33
    assert call(views=good[:2] + [(8, (0, 0, 17, 10))] + good[3:]) == _lib.EINVAL            # one pixel past H' = 9
    assert call(layout=c_layout(131, 65, FUSED["420"], precision=12)) == _lib.ENOSUP
    assert call(s=stride - 1) == _lib.EINVAL
    assert call(ptr=None) == _lib.EINVAL
    ctx.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0
    host = out.cpu().numpy()
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    for i, (denom, r) in enumerate(good):
        want = _crop(_reference(L, ph, qh, i, denom, 0)[_lib.COLOR_RGB8], r)
        assert (host[i * stride:i * stride + 3 * r[2] * r[3]].reshape(r[3], r[2], 3) == want).all(), i


# ---- 6. the Python API ----------------------------------------------------------------------------------------------------------

def test_python_api(ctx, torch):
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    size = (131, 65)
    L = c_layout(size[0], size[1], FUSED["420"])
    planes, dq, ntables = synthetic(ctx, torch, L, 3, 11)
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    source = [(10, 7, 100, 50), (90, 30, 41, 35), (0, 0, 131, 65)]
    denoms = [J.view_denom(s[2:], (24, 12)) for s in source]
    assert denoms == [4, 1, 4]
    views = [(d,) + J.view_of_source(size, d, s) for d, s in zip(denoms, source)]
    assert views[0] == (4, 2, 1, 26, 14) and views[2] == (4, 0, 0) + S.scaled_size(size, 4)
    got = J.decode_views(ctx, size, layout, planes, dq, views, q=[0, 1, 1], color=J.YCbCr)
    assert len(got) == 3
    for i, v in enumerate(views):
        assert tuple(got[i].shape) == (v[4], v[3], 3)
        assert (got[i].cpu().numpy() == _crop(_reference(L, ph, qh, i, v[0], 0)[_lib.COLOR_YCC8], v[1:])).all()
    sp = J.Spectral(ctx, size, layout, [p[1] for p in planes], [qh[1, 0], qh[1, 1]], [0, 1, 1])
    for denom in DENOMS:
        w, h = S.scaled_size(size, denom)
        r = (w // 3, h // 4, w - w // 3, h // 2)
        for cosite in (False, True):
            one = sp.view(r, denom, J.RGB, cosite=cosite)
            assert tuple(one.shape) == (r[3], r[2], 3)
            assert (one.cpu().numpy() == _crop(_reference(L, ph, qh, 1, denom, cosite)[_lib.COLOR_RGB8], r)).all()
    assert J.view_window(size, layout, 2, (5, 5, 20, 10)) == [(1, 1, 6, 3), (0, 0, 4, 2), (0, 0, 4, 2)]
    with pytest.raises(ValueError):
        sp.decode(J.RGB, region=(0, 0, 8, 8), scale=2)
    with pytest.raises(J.JpegAmdError):
        sp.view((0, 0, 67, 1), 2)                          # W' = 66
