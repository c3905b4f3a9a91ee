"""Every kernel of the tile decode family once, on the MI355X: launch_tile_decode picks k_region_decode<planes, rgb> (4),
k_scaled_decode<N, planes, rgb> (12), k_view_decode<N, planes, rgb> (16) or k_view_decode_mixed<N, planes, rgb> (16) from the
kernel, N = 8 / denominator, the number of planes and the colour target, and each cell of that table is reached below through
the C call that ends in it, with the layouts y8 and 4:2:0; the two fallback kernels of the layouts without a tile kernel follow.
Expected bytes come from the checkers of the family's own tests, which share nothing with the code under test: _scaled_ref's
scaled decode and, at denominator 1, the oracle's full decode, cropped in numpy; compared exactly.  The bytes around the images
are checked through _calls.Out.  Inputs and references are made once per module and never written to."""
import ctypes as C

import numpy as np
import pytest

import _scaled_ref as S
from _calls import COLORS, FUSED, Out, c_layout, c_regions, c_views, plane_ptrs, strides, synthetic
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _mixed import view_mixed
from _tile import TILE_H, TILE_W, crop, reference
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

LAYOUTS = {"y8": FUSED["y8"], "420": FUSED["420"], "411": [(4, 1), (1, 1), (1, 1)]}   # 4:1:1: no tile kernel takes it
COLOR_IDS = {_lib.COLOR_RGB8: "rgb", _lib.COLOR_YCC8: "ycc"}
# sources that scale to 138 x 38 at their denominator: two tile columns and two tile rows, both partial
SCALED_SOURCE = {2: (275, 75), 4: (549, 149), 8: (1100, 300)}

_inputs, _wanted = {}, {}


def _images(ctx, torch, name, size, n):
    """n synthetic images of one layout and size, made once: -> (L, planes, dq, ntables, host planes, host tables)."""
    key = (name, size, n)
    if key not in _inputs:
        L = c_layout(size[0], size[1], LAYOUTS[name])
        planes, dq, ntables = synthetic(ctx, torch, L, n, 1000 * size[0] + size[1] + len(name))
        _inputs[key] = (L, planes, dq, ntables, [p.cpu().numpy() for p in planes], dq.cpu().numpy().astype(np.uint16))
    return _inputs[key]


def _want(ctx, torch, name, size, n, i, denom):
    """Image i of _images(...) at `denom`, whole, through the checker, made once -> {color: [H', W', 3]}, read-only."""
    key = (name, size, n, i, denom)
    if key not in _wanted:
        L, _, _, _, ph, qh = _images(ctx, torch, name, size, n)
        _wanted[key] = reference(L, ph, qh, i, denom, 0)
        for image in _wanted[key].values():
            image.setflags(write=False)
    return _wanted[key]


def _straddles(denom, r, tile_h=TILE_H):
    """r crosses a tile seam of its own tile grid on both axes."""
    n = 8 // denom
    return r[0] % n + r[2] > TILE_W and r[1] % n + r[3] > tile_h


# ---- k_region_decode<planes, rgb> ---------------------------------------------------------------------------------------------

REGION_SIZE = (138, 70)
# off the block grid and across x = 128 and y = 64 of its tile grid; 1 x 1 at the last pixel; up to the last column and row
REGIONS = [(3, 2, 133, 66), (137, 69, 1, 1), (100, 50, 38, 20)]


def _region_call(ctx, torch, name, color):
    L, planes, dq, ntables, _, _ = _images(ctx, torch, name, REGION_SIZE, len(REGIONS))
    out = Out(ctx, torch, [3 * r[2] * r[3] for r in REGIONS], gap=5, tail=7)
    assert _lib.lib().jpeg_amd_decode_region_batch(
        ctx.handle, C.byref(L), len(REGIONS), plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables,
        0, color, c_regions(REGIONS), out.ptr, out.stride) == 0
    for i, (r, g) in enumerate(zip(REGIONS, out.images())):
        want = crop(_want(ctx, torch, name, REGION_SIZE, len(REGIONS), i, 1)[color], r)
        assert (g.reshape(r[3], r[2], 3) == want).all(), (name, COLOR_IDS[color], r)


@pytest.mark.parametrize("color", COLORS, ids=list(COLOR_IDS.values()))
@pytest.mark.parametrize("name", ["y8", "420"])
def test_region_kernels(ctx, torch, name, color):
    assert _straddles(1, REGIONS[0], 64) and REGIONS[0][0] % 8 and REGIONS[0][1] % 8
    assert REGIONS[1][:2] == (REGION_SIZE[0] - 1, REGION_SIZE[1] - 1)
    assert (REGIONS[2][0] + REGIONS[2][2], REGIONS[2][1] + REGIONS[2][3]) == REGION_SIZE
    _region_call(ctx, torch, name, color)


# ---- k_scaled_decode<N, planes, rgb> ------------------------------------------------------------------------------------------

def _scaled_call(ctx, torch, name, denom, color):
    size, n = SCALED_SOURCE[denom], 2
    assert S.scaled_size(size, denom) == (138, 38)
    L, planes, dq, ntables, ph, qh = _images(ctx, torch, name, size, n)
    out = Out(ctx, torch, [3 * 138 * 38] * n, gap=11, tail=11)
    assert _lib.lib().jpeg_amd_decode_scaled_batch(
        ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0, color,
        denom, out.ptr, out.stride) == 0
    for i, g in enumerate(out.images()):
        want = S.decode_scaled([pl[i] for pl in ph], [qh[i, L.qi[p]] for p in range(L.nplanes)], LAYOUTS[name], size, denom, False,
                               color == _lib.COLOR_RGB8, (L.scale_x, L.scale_y))
        assert (g.reshape(38, 138, 3) == want).all(), (name, denom, COLOR_IDS[color], i)


@pytest.mark.parametrize("color", COLORS, ids=list(COLOR_IDS.values()))
@pytest.mark.parametrize("denom", [2, 4, 8])
@pytest.mark.parametrize("name", ["y8", "420"])
def test_scaled_kernels(ctx, torch, name, denom, color):
    _scaled_call(ctx, torch, name, denom, color)


# ---- k_view_decode<N, planes, rgb> --------------------------------------------------------------------------------------------

VIEW_SIZE = (1100, 300)
# one view per denominator in one call; none whole, each across a seam of its tile grid on both axes
VIEWS = [(8, (1, 1, 133, 35)), (1, (13, 11, 140, 40)), (4, (3, 5, 140, 40)), (2, (5, 3, 150, 50))]


@pytest.mark.parametrize("color", COLORS, ids=list(COLOR_IDS.values()))
@pytest.mark.parametrize("name", ["y8", "420"])
def test_view_kernels(ctx, torch, name, color):
    n = len(VIEWS)
    for denom, r in VIEWS:
        W1, H1 = S.scaled_size(VIEW_SIZE, denom)
        assert _straddles(denom, r) and r[0] + r[2] <= W1 and r[1] + r[3] <= H1 and r[2:] != (W1, H1)
    assert sorted(d for d, _ in VIEWS) == [1, 2, 4, 8]
    L, planes, dq, ntables, _, _ = _images(ctx, torch, name, VIEW_SIZE, n)
    out = Out(ctx, torch, [3 * r[2] * r[3] for _, r in VIEWS], gap=5, tail=7)
    assert _lib.lib().jpeg_amd_decode_view_batch(
        ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0, color,
        c_views(VIEWS), out.ptr, out.stride) == 0
    for i, ((denom, r), g) in enumerate(zip(VIEWS, out.images())):
        want = crop(_want(ctx, torch, name, VIEW_SIZE, n, i, denom)[color], r)
        assert (g.reshape(r[3], r[2], 3) == want).all(), (name, COLOR_IDS[color], denom, r)


# ---- k_view_decode_mixed<N, planes, rgb> --------------------------------------------------------------------------------------

# eight images of different sizes in one call: y8 and 4:2:0 at each denominator, in no order; the views cross a seam of their
# tile grid on both axes where the scaled image is large enough
MIXED = [("420", (300, 140), 2, (3, 1, 140, 60)), ("y8", (138, 70), 1, (5, 3, 130, 40)), ("420", (1100, 300), 8, (1, 1, 133, 35)),
         ("y8", (549, 149), 4, (1, 2, 131, 34)), ("420", (150, 90), 1, (9, 7, 135, 50)), ("y8", (275, 75), 2, (0, 0, 138, 38)),
         ("420", (403, 150), 4, (2, 1, 99, 37)), ("y8", (1000, 280), 8, (0, 0, 125, 35))]


@pytest.mark.parametrize("color", COLORS, ids=list(COLOR_IDS.values()))
def test_mixed_kernels(ctx, torch, color):
    assert sorted((name, denom) for name, _, denom, _ in MIXED) == sorted((nm, d) for nm in ("y8", "420") for d in (1, 2, 4, 8))
    assert len({size for _, size, _, _ in MIXED}) == len(MIXED)
    assert sum(_straddles(denom, r) for _, _, denom, r in MIXED) >= 5
    images = [_images(ctx, torch, name, size, 1) for name, size, _, _ in MIXED]
    args = [(L, [p.data_ptr() for p in planes], dq.data_ptr(), ntables) for L, planes, dq, ntables, _, _ in images]
    views = [(denom, r) for _, _, denom, r in MIXED]
    out = Out(ctx, torch, [3 * r[2] * r[3] for _, r in views], gap=5, tail=7)
    assert view_mixed(ctx.handle, args, 0, color, views, out.ptr, out.stride) == 0
    for (name, size, denom, r), g in zip(MIXED, out.images()):
        want = crop(_want(ctx, torch, name, size, 1, 0, denom)[color], r)
        assert (g.reshape(r[3], r[2], 3) == want).all(), (name, size, denom, COLOR_IDS[color])


# ---- the fallbacks: k_region_crop, k_idct_scaled<N, uint8_t>, k_idct_scaled<N, uint16_t> ----------------------------------------

def test_a_411_region_call_reaches_the_crop_kernel(ctx, torch):
    _region_call(ctx, torch, "411", _lib.COLOR_RGB8)


@pytest.mark.parametrize("denom", [2, 4, 8])
def test_a_411_scaled_call_reaches_the_byte_plane_kernel(ctx, torch, denom):
    _scaled_call(ctx, torch, "411", denom, _lib.COLOR_YCC8)


@pytest.mark.parametrize("denom", [2, 4, 8])
def test_the_scaled_planes_reach_the_uint16_plane_kernel(ctx, torch, denom):
    size = SCALED_SOURCE[denom]
    L, planes, dq, ntables, ph, qh = _images(ctx, torch, "420", size, 2)
    sl = _lib.Layout()
    assert _lib.lib().jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(sl)) == 0
    outs = [Out(ctx, torch, [64 * sl.units_x[p] * sl.units_y[p]], elem=2, tail=8) for p in range(L.nplanes)]
    tables = np.ascontiguousarray(qh[1])
    assert _lib.lib().jpeg_amd_spectral_idct_scaled(ctx.handle, C.byref(L), plane_ptrs([p[1] for p in planes]), tables.ctypes.data,
                                                    ntables, denom, _lib.ptr_array([o.ptr for o in outs])) == 0
    for p, o in enumerate(outs):
        want = S.pad_planes([S.idct_plane_scaled(ph[p][1], tables[L.qi[p]], 8 // denom)])[0]
        got = o.images()[0].view(np.uint16).reshape(8 * sl.units_y[p], 8 * sl.units_x[p])
        assert (got == want).all(), (denom, p)
