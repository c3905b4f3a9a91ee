"""Scaled decode on the MI355X (jpeg_amd_decode_scaled_batch; k_scaled_decode and the k_idct_scaled fallback): byte for byte
the contract of include/jpeg_amd.h as restated in _scaled_ref -- fixtures and synthetic coefficients at sizes that straddle
the block, MCU and tile edges -- the fused launch against the staged route, unread coefficients, an anchor to the existing
decode that needs no test-side reference, batches with stride gaps, and the argument checks."""
import ctypes as C
import os

import numpy as np
import pytest

import _scaled_ref as S
import jpeg_amd as J
from _calls import (COLORS, FUSED, SENTINEL, Out, c_layout, full_batch, plane_factors, plane_ptrs, plane_units, strides,
                    synthetic)
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _tile import FIXTURES, fixture
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

def _call(ctx, L, n, planes, coef_stride, dq, q_stride, ntables, cosited, color, denom, out_ptr, stride):
    return _lib.lib().jpeg_amd_decode_scaled_batch(
        ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(coef_stride),
        dq.data_ptr(), q_stride, ntables, cosited, color, denom, out_ptr, stride)


def _scaled_batch(ctx, torch, L, n, planes, dq, ntables, cosited, color, denom, gap=0, distinct=True):
    """-> (the output buffer, filled with SENTINEL before the call, (W', H'))."""
    w, h = S.scaled_size((L.width, L.height), denom)
    out = Out(ctx, torch, [3 * w * h] * n, gap=gap, tail=gap)
    assert _call(ctx, L, n, planes, strides(L, distinct), dq, ntables * 64 if distinct else 0, ntables, cosited, color, denom,
                 out.ptr, out.stride) == 0
    return out, (w, h)


def _images(out, n, size):
    """The n images, still on the device."""
    w, h = size
    return [out.device(i).view(h, w, 3) for i in range(n)]


def _reference(L, planes_host, quanta_host, i, denom, cosited, color):
    """Image i of a batch through _scaled_ref: planes_host[p] [n, uy, ux, 64], quanta_host [n, ntables, 64]."""
    return S.decode_scaled([pl[i] for pl in planes_host], [quanta_host[i, L.qi[p]] for p in range(L.nplanes)], plane_factors(L),
                           (L.width, L.height), denom, bool(cosited), color == _lib.COLOR_RGB8, (L.scale_x, L.scale_y))


# ---- the fixtures --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_fixtures_match_the_reference(ctx, torch, path):
    info, L, planes, quanta = fixture(path)
    nc = info.ncomponents
    dev = [ctx.upload(p) for p in planes]
    factors = [(info.factor_x[c], info.factor_y[c]) for c in range(nc)]
    for denom in (2, 4, 8):
        w, h = S.scaled_size((info.width, info.height), denom)
        for cosited in (0, 1):
            _, rect = S.interleaved_scaled(planes, list(quanta[:nc]), factors, (info.width, info.height), denom, bool(cosited),
                                           (info.scale_x, info.scale_y))
            for color in COLORS:
                want = (S.O.unpack_rgb8 if color == _lib.COLOR_RGB8 else S.O.unpack_ycc8)(rect, nc).reshape(h, w, 3)
                out = torch.full((3 * w * h + 8,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
                assert _lib.lib().jpeg_amd_decode_scaled(ctx.handle, C.byref(L), plane_ptrs(dev), quanta.ctypes.data, nc, cosited,
                                                         color, denom, out.data_ptr()) == 0
                got = out.cpu().numpy()
                assert (got[:3 * w * h].reshape(h, w, 3) == want).all(), (os.path.basename(path), denom, cosited, color)
                assert (got[3 * w * h:] == SENTINEL).all()


# ---- synthetic coefficients ------------------------------------------------------------------------------------------------

# name -> (factors, cosited): the layouts the fused kernel does not take
FALLBACK = {"411": ([(4, 1), (1, 1), (1, 1)], 0), "420-cosited": ([(2, 2), (1, 1), (1, 1)], 1),
            "422-cosited": ([(2, 1), (1, 1), (1, 1)], 1)}
LAYOUTS = {**{k: (v, 0) for k, v in FUSED.items()}, **FALLBACK}
# W, H from {1, 7, 8, 9, 15, 16, 17, 33, 131, 257}: the block (8), the MCU (16, 32 for 4:1:1) and, scaled, the 128 x 32 tile
SIZES = [(1, 1), (257, 1), (7, 9), (8, 16), (9, 15), (15, 8), (16, 33), (17, 7), (33, 17), (131, 257), (257, 131)]


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_synthetic_batches_match_the_reference(ctx, torch, name, size):
    factors, cosited = LAYOUTS[name]
    L = c_layout(size[0], size[1], factors)
    n = 2
    for k, kind in enumerate(("natural", "saturating")):
        planes, dq, ntables = synthetic(ctx, torch, L, n, size[0] * 31 + size[1] + k, kind)
        ph = [p.cpu().numpy() for p in planes]
        qh = dq.cpu().numpy().astype(np.uint16)
        for denom in (1, 2, 4, 8):
            color = COLORS[(denom // 2 + k) % 2]        # every denom sees both colour targets, one per kind of data
            out, ssize = _scaled_batch(ctx, torch, L, n, planes, dq, ntables, cosited, color, denom)
            got = _images(out, n, ssize)
            if denom == 1:                               # jpeg_amd_decode_batch itself
                full = full_batch(ctx, torch, L, n, planes, strides(L), dq, ntables * 64, ntables, cosited, color)
                assert all(torch.equal(got[i], full[i]) for i in range(n))
                continue
            for i in range(n):
                want = _reference(L, ph, qh, i, denom, cosited, color)
                assert (got[i].cpu().numpy() == want).all(), (name, size, kind, denom, i)


@pytest.mark.parametrize("size", [(9, 15), (131, 257), (257, 131)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(FUSED))
def test_fused_launch_equals_the_staged_route(ctx, torch, name, size):
    """k_idct_scaled planes -> the EXISTING jpeg_amd_planar_interleaved + jpeg_amd_rectangular_unpack under
    jpeg_amd_scaled_layout's layout give the bytes of the fused launch."""
    lib = _lib.lib()
    L = c_layout(size[0], size[1], FUSED[name])
    planes, dq, ntables = synthetic(ctx, torch, L, 1, size[0] + 7 * size[1])
    one = [p[0] for p in planes]
    qh = np.ascontiguousarray(dq[0].cpu().numpy().astype(np.uint16))
    for denom in (2, 4, 8):
        sl = _lib.Layout()
        assert lib.jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(sl)) == 0
        w, h = sl.width, sl.height
        staged = [torch.full((64 * sl.units_x[p] * sl.units_y[p],), -1, dtype=torch.int16, device=ctx.torch_device)
                  for p in range(L.nplanes)]
        assert lib.jpeg_amd_spectral_idct_scaled(ctx.handle, C.byref(L), plane_ptrs(one), qh.ctypes.data, ntables, denom,
                                                 plane_ptrs(staged)) == 0
        rect = torch.empty((w * h * L.nplanes,), dtype=torch.int16, device=ctx.torch_device)
        assert lib.jpeg_amd_planar_interleaved(ctx.handle, C.byref(sl), plane_ptrs(staged), 0, rect.data_ptr()) == 0
        for color in COLORS:
            px = torch.empty((3 * w * h,), dtype=torch.uint8, device=ctx.torch_device)
            assert lib.jpeg_amd_rectangular_unpack(ctx.handle, rect.data_ptr(), w * h, L.nplanes, color, px.data_ptr()) == 0
            fused = torch.empty((3 * w * h,), dtype=torch.uint8, device=ctx.torch_device)
            assert lib.jpeg_amd_decode_scaled(ctx.handle, C.byref(L), plane_ptrs(one), qh.ctypes.data, ntables, 0, color, denom,
                                              fused.data_ptr()) == 0
            assert torch.equal(px, fused), (name, size, denom, color)
        # the staged planes themselves: the reference's, edge-replicated to whole blocks
        for p in range(L.nplanes):
            want = S.pad_planes([S.idct_plane_scaled(one[p].cpu().numpy(), qh[L.qi[p]], 8 // denom)])[0]
            got = staged[p].cpu().numpy().view(np.uint16).reshape(8 * sl.units_y[p], 8 * sl.units_x[p])
            assert (got == want).all(), (name, size, denom, p)


@pytest.mark.parametrize("name", ["y8", "420", "411"])
def test_unread_coefficients_do_not_matter(ctx, torch, name):
    factors, cosited = LAYOUTS[name]
    L = c_layout(131, 65, factors)
    planes, dq, ntables = synthetic(ctx, torch, L, 2, 99)
    for denom in (2, 4, 8):
        N = 8 // denom
        unread = torch.ones(64, dtype=torch.bool, device=ctx.torch_device)
        unread[torch.as_tensor(sorted(int(S.Z[h][k]) for h in range(N) for k in range(N)), device=ctx.torch_device)] = False
        gen = torch.Generator(device=ctx.torch_device).manual_seed(denom)
        zeroed, noisy = [], []
        for p in planes:
            z = p.clone()
            z[..., unread] = 0
            r = torch.randint(-32768, 32768, p.shape, dtype=torch.int32, device=ctx.torch_device, generator=gen).to(torch.int16)
            r[0, 0, 0, :] = 32767                         # the extremes are in for certain
            r[0, 0, -1, :] = -32767
            zeroed.append(z)
            noisy.append(torch.where(unread, r, p).contiguous())
        before = [p.clone() for p in noisy]
        a, _ = _scaled_batch(ctx, torch, L, 2, zeroed, dq, ntables, cosited, _lib.COLOR_RGB8, denom)
        b, _ = _scaled_batch(ctx, torch, L, 2, noisy, dq, ntables, cosited, _lib.COLOR_RGB8, denom)
        assert torch.equal(a.buf, b.buf), (name, denom)
        assert all(torch.equal(x, y) for x, y in zip(noisy, before))


@pytest.mark.parametrize("name", ["y8", "444"])
def test_dc_only_images_are_the_existing_decode_subsampled(ctx, torch, name):
    """No test-side reference in between: with only the DC coefficient every butterfly returns shift + h0, so scaled pixel
    (X, Y) at denom d is pixel (d X, d Y) of jpeg_amd_decode_batch of the same image, exactly."""
    L = c_layout(131, 77, FUSED[name])
    n = 3
    gen = torch.Generator(device=ctx.torch_device).manual_seed(5)
    planes = []
    for ux, uy in plane_units(L):
        p = torch.zeros((n, uy, ux, 64), dtype=torch.int16, device=ctx.torch_device)
        p[..., 0] = torch.randint(-90, 91, (n, uy, ux), dtype=torch.int32, device=ctx.torch_device, generator=gen).to(torch.int16)
        planes.append(p)
    ntables = 2 if L.nplanes == 3 else 1
    dq = torch.randint(1, 24, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen)
    for color in COLORS:
        full = full_batch(ctx, torch, L, n, planes, strides(L), dq, ntables * 64, ntables, 0, color)
        assert full.unique().numel() > 16
        for denom in (2, 4, 8):
            out, ssize = _scaled_batch(ctx, torch, L, n, planes, dq, ntables, 0, color, denom)
            for i, img in enumerate(_images(out, n, ssize)):
                assert torch.equal(img, full[i, ::denom, ::denom]), (name, color, denom, i)


@pytest.mark.parametrize("name", ["420", "422-cosited"])
def test_batch_of_64_with_stride_gaps_and_against_single_calls(ctx, torch, name):
    factors, cosited = LAYOUTS[name]
    L = c_layout(33, 17, factors)
    n, gap = 64, 37
    planes, dq, ntables = synthetic(ctx, torch, L, n, 64)
    qh = np.ascontiguousarray(dq.cpu().numpy().astype(np.uint16))
    for denom in (2, 8):
        out, (w, h) = _scaled_batch(ctx, torch, L, n, planes, dq, ntables, cosited, _lib.COLOR_RGB8, denom, gap=gap)
        out.images()                                     # the sentinel in the n gaps and in the tail, of `gap` bytes each
        assert out.buf.numel() == n * (3 * w * h + gap) + gap
        for i in range(n):
            one = torch.empty((3 * w * h,), dtype=torch.uint8, device=ctx.torch_device)
            assert _lib.lib().jpeg_amd_decode_scaled(ctx.handle, C.byref(L), plane_ptrs([p[i] for p in planes]),
                                                     qh[i].ctypes.data, ntables, cosited, _lib.COLOR_RGB8, denom,
                                                     one.data_ptr()) == 0
            assert torch.equal(one, out.device(i)), (name, denom, i)


def test_an_empty_batch_is_ok(ctx, torch):
    L = c_layout(33, 17, FUSED["420"])
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    assert _lib.lib().jpeg_amd_decode_scaled_batch(ctx.handle, C.byref(L), 0, None, None, None, 0, 2, 0, _lib.COLOR_RGB8, 2,
                                                   out.data_ptr(), 0) == 0
    assert (out == SENTINEL).all()


def test_invalid_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    L = c_layout(33, 17, FUSED["420"])
    n = 2
    planes, dq, ntables = synthetic(ctx, torch, L, n, 3)
    w, h = S.scaled_size((33, 17), 2)
    stride = 3 * w * h
    out = torch.full((n * stride,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)

    def call(layout=L, denom=2, ptr=out.data_ptr(), s=stride):
        return _call(ctx, layout, n, planes, strides(L), dq, ntables * 64, ntables, 0, _lib.COLOR_RGB8, denom, ptr, s)

    for denom in (0, 3, 16, -1):
        assert call(denom=denom) == _lib.EINVAL
    L12 = c_layout(33, 17, FUSED["420"], precision=12)
    assert call(layout=L12) == _lib.ENOSUP
    assert call(s=stride - 1) == _lib.EINVAL
    assert call(ptr=None) == _lib.EINVAL
    ctx.synchronize()
    assert (out == SENTINEL).all()
    assert call() == 0
    want = _reference(L, [p.cpu().numpy() for p in planes], dq.cpu().numpy().astype(np.uint16), 1, 2, 0, _lib.COLOR_RGB8)
    assert (out[stride:].view(h, w, 3).cpu().numpy() == want).all()


def test_python_api(ctx, torch):
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    size = (131, 65)
    L = c_layout(size[0], size[1], FUSED["420"])
    planes, dq, ntables = synthetic(ctx, torch, L, 3, 11)
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    for denom in (2, 4, 8):
        assert J.scaled_size(size, denom) == S.scaled_size(size, denom)
        got = J.decode_scaled(ctx, size, layout, planes, dq, denom, q=[0, 1, 1], color=J.YCbCr)
        w, h = S.scaled_size(size, denom)
        assert tuple(got.shape) == (3, h, w, 3)
        for i in range(3):
            assert (got[i].cpu().numpy() == _reference(L, ph, qh, i, denom, 0, _lib.COLOR_YCC8)).all()
        sp = J.Spectral(ctx, size, layout, [p[1] for p in planes], [qh[1, 0], qh[1, 1]], [0, 1, 1])
        one = sp.decode(J.RGB, scale=denom)
        assert tuple(one.shape) == (h * w, 3)
        assert (one.cpu().numpy().reshape(h, w, 3) == _reference(L, ph, qh, 1, denom, 0, _lib.COLOR_RGB8)).all()
        cos = sp.decode(J.RGB, cosite=True, scale=denom)
        assert (cos.cpu().numpy().reshape(h, w, 3) == _reference(L, ph, qh, 1, denom, 1, _lib.COLOR_RGB8)).all()
    assert torch.equal(sp.decode(J.RGB, scale=1), sp.decode(J.RGB))
    with pytest.raises(ValueError):
        sp.decode(J.RGB, region=(0, 0, 8, 8), scale=2)
    with pytest.raises(ValueError):
        J.decode_scaled(ctx, size, layout, planes, dq, 3)
