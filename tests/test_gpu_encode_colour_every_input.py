"""The colour stage of the fused ENCODE kernel on the device, every input -- the counterpart of
tests/test_gpu_colour_every_input.py.  k_encode_fused's rgb_to_ycc fuses exactly two steps of the reference's matrix, its
raw-chroma path truncates four values at a time under round-toward-zero, the pooled mean is one FMA whose round-to-nearest
is the truncation, and long 4:2:0 launches pool in the integer domain; tests/test_colour_rounding.py proves models of these
on the CPU.  Here all 2^24 RGB go through the 4:4:4 RGB instantiation itself, and cells of different colours through the
pooling ones, against the reference's formula (jpeg.swift:463-478: x = ((m0 + m_r r) + m_g g) + m_b b, clamp, truncate)
evaluated in binary32 with numpy.

A flat block of value v under an all-ones table transforms exactly: every AC coefficient is 0 and the DC is
(64 v - 8192) / 8 = 8 (v - 128).  So the colour value of a flat block is read off its DC."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu
f32 = np.float32


def _ycc(rgb):
    """uint8 [..., 3] -> uint8 [..., 3] and the float32 values before clamp and truncation."""
    r, g, b = (rgb[..., i].astype(f32) for i in range(3))
    y = ((f32(0.0) + f32(0.2990) * r) + f32(0.5870) * g) + f32(0.1140) * b
    cb = ((f32(128.0) + f32(-0.1687) * r) + f32(-0.3313) * g) + f32(0.5000) * b
    cr = ((f32(128.0) + f32(0.5000) * r) + f32(-0.4187) * g) + f32(-0.0813) * b
    raw = np.stack([y, cb, cr], axis=-1)
    assert raw.dtype == f32
    return np.clip(raw, f32(0), f32(255)).astype(np.uint8), raw


@pytest.fixture(scope="module")
def env():
    import torch
    import jpeg_amd as J
    from jpeg_amd import _lib
    ctx = J.Context(0)
    d_ones = torch.ones(128, dtype=torch.int16, device=ctx.torch_device)
    return dict(torch=torch, J=J, _lib=_lib, lib=_lib.lib(), ctx=ctx, d_ones=d_ones)


def _encode(e, factors, size, d_px, n):
    """jpeg_amd_encode_batch, RGB input, all-ones tables -> per plane int16 [n, uy ux, 64] on the device (sentinel-filled)."""
    J, _lib, torch = e["J"], e["_lib"], e["torch"]
    layout = J.Layout("ycc8", {i + 1: J.Component(f, min(i, 1)) for i, f in enumerate(factors)})
    units = layout.units(size)
    L = layout.c_layout(size, units, [0, 1, 1])
    outs = [torch.full((n, ux * uy, 64), 0x5A5A, dtype=torch.int16, device=e["ctx"].torch_device) for ux, uy in units]
    st = e["lib"].jpeg_amd_encode_batch(e["ctx"].handle, C.byref(L), n, d_px.data_ptr(), size[0] * size[1] * 3, _lib.COLOR_RGB8,
                                        e["d_ones"].data_ptr(), 0, 2, _lib.ptr_array([o.data_ptr() for o in outs]),
                                        _lib.size_array([64 * ux * uy for ux, uy in units]))
    assert st == 0, st
    return outs, units


def _every_rgb(e, size, greens):
    """Block (j, i) of the image is the flat colour (R = i, G, B = j); only the DC planes come back to the host."""
    torch = e["torch"]
    w, h = size
    dev = e["ctx"].torch_device
    px = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    px[..., 0] = (torch.arange(w, device=dev) // 8).to(torch.uint8)[None, :]
    px[..., 2] = (torch.arange(h, device=dev) // 8).to(torch.uint8)[:, None]
    bb, rr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")     # [j][i]
    for g in greens:
        px[..., 1] = g
        outs, units = _encode(e, [(1, 1)] * 3, size, px, 1)
        assert units == [(256, 256)] * 3
        want, _ = _ycc(np.stack([rr, np.full_like(rr, g), bb], axis=-1))
        for p, o in enumerate(outs):
            assert not bool((o[0, :, 1:] != 0).any()), (g, p)
            dc = o[0, :, 0].cpu().numpy().reshape(256, 256).astype(np.int32)
            expect = 8 * (want[..., p].astype(np.int32) - 128)
            assert (dc == expect).all(), f"G = {g}, plane {p}: {int((dc != expect).sum())} colours differ, first (B, R) = {np.argwhere(dc != expect)[0].tolist()}"


def test_the_numpy_formula_is_the_oracles():
    g = 151
    bb, rr = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    rgb = np.stack([rr, np.full_like(rr, g), bb], axis=-1).reshape(-1, 3)
    assert (_ycc(rgb)[0] == O.pack_rgb8(rgb, 3)).all()
    edge = np.array([[255, 255, 0], [0, 0, 255], [0, 255, 255], [255, 0, 0], [0, 0, 0], [255, 255, 255]], np.uint8)
    assert (_ycc(edge)[0] == O.pack_rgb8(edge, 3)).all()


def test_every_rgb_through_the_444_kernel(env):
    _every_rgb(env, (2048, 2048), range(256))


def test_a_sample_of_rgb_through_an_odd_width(env):
    """2045 x 2043: no row is 8-byte aligned, so every block takes the byte-wise fetch, and the last block column and row are
    edge-replicated -- flat all the same."""
    _every_rgb(env, (2045, 2043), [0, 37, 61, 74, 128, 200, 255])


# ---- pooled chroma ---------------------------------------------------------------------------------------------------------------

EXTREMES = np.array([[255, 255, 0], [0, 0, 255], [0, 255, 255], [255, 0, 0], [0, 0, 0], [255, 255, 255]], np.uint8)
#                     Cb = 0.5       Cb = 255.5    Cr = 0.5       Cr = 255.5   (before the truncation)
SIZE = (512, 256)
BASE = 8                       # distinct images; a long batch repeats them


def _cells(sx, sy):
    """uint8 [BASE, gy, gx, sy, sx, 3]: per MCU a cell of sx sy colours.  Image 0: each extreme alone, then cells drawn from
    the extremes without repetition; the other images: random colours, a quarter of the cells within 2 of one colour (sums of
    every residue next to each other)."""
    rng = np.random.default_rng(100 * sx + sy)
    gx, gy = SIZE[0] // (8 * sx), SIZE[1] // (8 * sy)
    cells = rng.integers(0, 256, (BASE, gy, gx, sy, sx, 3)).astype(np.uint8)
    near = rng.random((BASE, gy, gx)) < 0.25
    jitter = np.clip(cells[:, :, :, :1, :1].astype(int) + rng.integers(-2, 3, cells.shape), 0, 255).astype(np.uint8)
    cells[near] = jitter[near]
    first = cells[0].reshape(gy * gx, sy * sx, 3)
    for i, c in enumerate(EXTREMES):
        first[i] = c
    for i in range(len(EXTREMES), gy * gx):
        first[i] = EXTREMES[rng.permutation(len(EXTREMES))[:sx * sy]]
    cells[0] = first.reshape(gy, gx, sy, sx, 3)
    return cells


def _pixels(cells, sx, sy):
    """Every cell replicated over its MCU: uint8 [BASE, H, W, 3]."""
    w, h = SIZE
    yy, xx = np.mgrid[0:h, 0:w]
    return np.ascontiguousarray(cells[:, yy // (8 * sy), xx // (8 * sx), yy % sy, xx % sx])


def _pooled(cells):
    """The chroma sample of every MCU: trunc(Float(sum) / Float(n)) of the cell's truncated values (encode.swift:419-421)
    -> (uint8 [BASE, gy, gx, 2], the integer sums, the float32 values before truncation)."""
    ycc, raw = _ycc(cells)
    n = cells.shape[3] * cells.shape[4]
    sums = ycc[..., 1:].astype(np.int64).sum(axis=(3, 4))
    mean = (sums.astype(f32) / f32(n)).astype(np.uint8)
    return mean, sums, raw[..., 1:]


@pytest.mark.parametrize("sx,sy", [(2, 2), (2, 1), (1, 2)], ids=["420", "422", "440"])
def test_pooled_chroma_of_cells_of_different_colours(env, sx, sy):
    """The chroma block of an MCU whose cell is replicated over it is flat, so its DC shows trunc(sum / n): every residue of
    the sum and the raw extremes 0.5 and 255.5 are among the cells.  Image by image (4:2:0: the float box filter) and, for
    4:2:0, as a batch of 2 400 tiles, long enough for the integer-pooling variant; the luma planes of one image against the
    oracle."""
    e, torch = env, env["torch"]
    cells = _cells(sx, sy)
    mean, sums, raw = _pooled(cells)
    n = sx * sy
    for c in range(2):
        assert set(np.unique(sums[..., c] % n).tolist()) == set(range(n))
        assert raw[..., c].min() < f32(0.5001) and raw[..., c].max() == f32(255.5)       # (Cb's lower end is 0.5000076 in binary32)
        assert mean[..., c].min() == 0 and mean[..., c].max() == 255
    px = _pixels(cells, sx, sy)
    factors = [(sx, sy), (1, 1), (1, 1)]
    ones = np.ones(64, np.uint16)
    oracle0 = O.encode(px[0].reshape(-1, 3), SIZE, factors, [ones] * 3)
    for p in (1, 2):                                         # the reasoning above, on the oracle: flat chroma blocks, DC = 8 (v - 128)
        assert (oracle0[p][..., 1:] == 0).all() and (oracle0[p][..., 0] == 8 * (mean[0, ..., p - 1].astype(int) - 128)).all()
    d_px = torch.from_numpy(px).to(e["ctx"].torch_device)
    expect = torch.from_numpy((8 * (mean.astype(np.int16) - 128)).reshape(BASE, -1, 2)).to(e["ctx"].torch_device)

    def check(outs, images, tag):
        for p in (1, 2):
            assert not bool((outs[p][:, :, 1:] != 0).any()), (tag, p)
            same = outs[p][:, :, 0] == expect[images][:, :, p - 1]
            assert bool(same.all()), f"{tag}, plane {p}: {int((~same).sum())} MCUs differ, first (image, MCU) = {torch.nonzero(~same)[0].tolist()}"
        for j in torch.nonzero(images == 0).reshape(-1).tolist()[:2]:
            assert (outs[0][j].cpu().numpy().reshape(oracle0[0].shape) == oracle0[0]).all(), (tag, j)

    for i in range(BASE):
        outs, _ = _encode(e, factors, SIZE, d_px[i], 1)
        check(outs, torch.tensor([i], device=e["ctx"].torch_device), f"image {i} alone")
    count = 300 if (sx, sy) == (2, 2) else BASE             # 300 images x 8 tiles: more than the 1 024 resident workgroups
    images = torch.arange(count, device=e["ctx"].torch_device) % BASE
    images = torch.flip(images, [0]) if count > BASE else images
    outs, _ = _encode(e, factors, SIZE, d_px[images].contiguous(), count)
    check(outs, images, f"batch of {count}")
