"""The encoders' quantisers on the device, aimed at exact ties (tests/_quantiser_ref.py builds the data,
tests/test_quantiser_cases_cpu.py judges it on the reference alone): k_encode_fused and k_generic_fused divide by a
reciprocal with one Markstein correction step and round as trunc(y1 + copysign(pred(1/2), y1)) into a two-conversion pack
(quantise.hpp); k_fdct_plane and k_spectral_reduce divide and round with round_half_away (dct.hpp).  Whole coefficient
planes, bit for bit against oracle.decompose + oracle.fdct_plane, outputs filled with a sentinel beforehand.

One table value Q per image -- the table is the image's own: Q at the four exact positions, zigzag 0, 10, 14, 39 -- and the
image's blocks are that value's ties, H = 4 Q m for every odd m the samples reach (a value with more ties than an image
holds takes several images).  Table 0 (luma) runs through Q = 1 .. 255 while table 1 (chroma) takes 256 - Q."""
import ctypes as C
from functools import lru_cache

import numpy as np
import pytest

import _quantiser_ref as QR
import _reduce_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu
FILL = 0x5A5A
CROP = (3, 5)                 # a width that is no multiple of 8: the byte-wise fetch, an edge-replicated block column and row


@pytest.fixture(scope="module")
def env():
    import torch
    import jpeg_amd as J
    from jpeg_amd import _lib
    return dict(torch=torch, J=J, _lib=_lib, lib=_lib.lib(), ctx=J.Context(0))


@lru_cache(maxsize=None)
def _batch8(name, crop):
    return QR.batch(name, 8, QR.pairs8(), crop=crop)


@lru_cache(maxsize=None)
def _batch_wide(name, precision, over_limit=False):
    """12 and 16 bits: the 8-bit table values and the 16-bit ones that admit a tie, sampled multipliers (+-1, +-3, the largest,
    seeded others).  over_limit (12 bits): every luma sample at the limit 2^P - 1 is raised above it, where load(limit:)
    brings it back (encode.swift:85) -- the blocks stay the ties they were."""
    b = QR.batch(name, precision, QR.pairs8() + QR.pairs16(precision), grid=(18, 10), every_m=False)
    if over_limit:
        top = (1 << precision) - 1
        luma = b.samples[..., 0]
        at = luma == top
        assert at.sum() > 1000
        luma[at] = np.random.default_rng(12).integers(top + 1, 65536, int(at.sum())).astype(np.uint16)
    return b


@lru_cache(maxsize=None)
def _reference(b):
    return [b.reference(i) for i in range(b.n)]


def _layout(e, b):
    J = e["J"]
    comps = {i + 1: J.Component(f, min(i, 1)) for i, f in enumerate(b.factors)}
    fmt = ("custom", b.precision, len(b.factors)) if b.precision != 8 else ("y8" if len(b.factors) == 1 else "ycc8")
    layout = J.Layout(fmt, comps)
    units = layout.units(b.size)
    return layout.c_layout(b.size, units, [min(i, 1) for i in range(len(b.factors))]), units


def _outputs(e, units, n):
    return [e["torch"].full((n, 64 * ux * uy), FILL, dtype=e["torch"].int16, device=e["ctx"].torch_device) for ux, uy in units]


def _device(e, a):
    a = np.ascontiguousarray(a)
    return e["torch"].from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(e["ctx"].torch_device)


def _compare(outs, units, want, images, tag):
    """outs[p] [len(images), 64 ux uy] on the device against want[image][p]."""
    for p, (ux, uy) in enumerate(units):
        got = outs[p].cpu().numpy().reshape(len(images), uy, ux, 64)
        for j, i in enumerate(images):
            bad = got[j] != want[i][p]
            assert not bad.any(), f"{tag}: image {i}, plane {p}: {int(bad.sum())} of {bad.size} coefficients differ, first at {np.argwhere(bad)[0].tolist()}"


def _fused(e, b, pixels, color, images, want, tag):
    """jpeg_amd_encode_batch on the images `images` (indices into the batch, repeats allowed) in ONE call."""
    _lib = e["_lib"]
    L, units = _layout(e, b)
    w, h = b.size
    idx = np.asarray(images)
    d_px = _device(e, pixels[idx])
    d_q = _device(e, b.tables[idx])
    outs = _outputs(e, units, len(idx))
    st = e["lib"].jpeg_amd_encode_batch(e["ctx"].handle, C.byref(L), len(idx), d_px.data_ptr(), w * h * 3, color, d_q.data_ptr(), 128, 2,
                                        _lib.ptr_array([o.data_ptr() for o in outs]), _lib.size_array([64 * a * c for a, c in units]))
    assert st == 0, st
    _compare(outs, units, want, list(idx), tag)


def _ycc_pixels(b):
    """The samples ARE the pixels of a YCbCr input (a one-plane layout ignores the chroma bytes it is given)."""
    if b.samples.shape[-1] == 3:
        return b.samples.astype(np.uint8)
    px = np.random.default_rng(5).integers(0, 256, b.samples.shape[:3] + (3,)).astype(np.uint8)
    px[..., 0] = b.samples[..., 0]
    return px


def _tiles(b):
    return -(-b.size[0] // 256) * -(-b.size[1] // 64)          # k_encode_fused: tiles of 32 x 8 luma blocks


# ---- k_encode_fused ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("crop", [(0, 0), CROP], ids=["w320", "w317"])
@pytest.mark.parametrize("name", ["grey", "444", "420", "422", "440"])
def test_fused_encode_ycc_input_every_tie(env, name, crop):
    """YCbCr input: luma ties under table 0, chroma ties under table 1 (every chroma sample replicated over its cell, so the
    box mean is exact), every image of the layout in one batch.  4:2:0 in calls of at most 512 tiles, which keep the float
    box filter; the next test takes the integer one."""
    b = _batch8(name, crop)
    want = _reference(b)
    px = _ycc_pixels(b)
    step = b.n if name != "420" else 512 // _tiles(b)
    for at in range(0, b.n, step):
        _fused(env, b, px, env["_lib"].COLOR_YCC8, range(at, min(at + step, b.n)), want, f"{name} {b.size}")


@pytest.mark.parametrize("crop", [(0, 0), CROP], ids=["w320", "w317"])
def test_fused_encode_420_integer_pooling_variant_every_tie(env, crop):
    """The same 4:2:0 batch, repeated until the launch is more than 2 048 tiles long: more workgroups than are resident at once
    (at most 1 024 tiles of 32 x 8 luma blocks), which is where the launcher takes k_encode_fused<..., POOLI = true> -- as
    test_420_encode_of_several_rounds_integer_box_filter reaches it."""
    b = _batch8("420", crop)
    images = list(range(b.n)) * -(-2049 // (b.n * _tiles(b)))
    assert len(images) * _tiles(b) > 2048
    _fused(env, b, _ycc_pixels(b), env["_lib"].COLOR_YCC8, images, _reference(b), f"420 integer pooling {b.size}")


@lru_cache(maxsize=None)
def _rgb_case(name, crop):
    """Luma ties through the RGB instantiations: every Y of the batch replaced by a near-grey RGB with that Y
    (QR.grey_rgb_map; the CPU module shows that every luma tie survives).  The chroma is whatever the conversion gives."""
    b = _batch8(name, crop)
    rgb = QR.grey_rgb_map()[b.samples[..., 0]]
    want = [O.encode(rgb[i].reshape(-1, 3), b.size, b.factors, b.plane_tables(i)) for i in range(b.n)]
    for i in (0, b.n - 1):
        assert (want[i][0] == _reference(b)[i][0]).all()          # the luma planes are those of the YCbCr batch: the ties are there
    return b, rgb, want


@pytest.mark.parametrize("name,crop", [("444", (0, 0)), ("420", (0, 0)), ("420", CROP)], ids=["444", "420", "420-w317"])
def test_fused_encode_rgb_input_luma_ties(env, name, crop):
    b, rgb, want = _rgb_case(name, crop)
    step = b.n if name != "420" else 512 // _tiles(b)
    for at in range(0, b.n, step):
        _fused(env, b, rgb, env["_lib"].COLOR_RGB8, range(at, min(at + step, b.n)), want, f"rgb {name} {b.size}")
    if name == "420":                                             # ... and the integer-pooling instantiation
        images = list(range(b.n)) * -(-2049 // (b.n * _tiles(b)))
        _fused(env, b, rgb, env["_lib"].COLOR_RGB8, images, want, f"rgb 420 integer pooling {b.size}")


# ---- k_generic_fused and k_fdct_plane ------------------------------------------------------------------------------------------

WIDE = [("grey", 8, False), ("420", 8, False), ("grey", 12, False), ("420", 12, False), ("420", 12, True), ("grey", 16, False),
        ("420", 16, False)]
WIDE_IDS = [f"{n}-{p}" + ("-over-limit" if o else "") for n, p, o in WIDE]


def _wide(name, precision, over):
    return _batch8(name, CROP if name == "420" else (0, 0)) if precision == 8 else _batch_wide(name, precision, over)


@pytest.mark.parametrize("name,precision,over", WIDE, ids=WIDE_IDS)
def test_generic_fused_encode_every_tie(env, name, precision, over):
    """jpeg_amd_rectangular_spectral_batch (k_generic_fused, the reciprocal form proven for 16-bit tables): the 8-bit batch as
    it is, and at 12 and 16 bits the 8-bit table values plus {1, 2, 255, 256, 257, 32767, 32768, 65521, 65535} and a seeded
    1 024 more, one image each, in one call."""
    e, _lib = env, env["_lib"]
    b = _wide(name, precision, over)
    want = _reference(b)
    L, units = _layout(e, b)
    npl = len(b.factors)
    stride = b.size[0] * b.size[1] * npl
    d_rect = _device(e, b.samples)
    d_q = _device(e, b.tables)
    outs = _outputs(e, units, b.n)
    st = e["lib"].jpeg_amd_rectangular_spectral_batch(e["ctx"].handle, C.byref(L), b.n, d_rect.data_ptr(), stride, d_q.data_ptr(), 128, 2,
                                                      _lib.ptr_array([o.data_ptr() for o in outs]),
                                                      _lib.size_array([64 * a * c for a, c in units]))
    assert st == 0, st
    _compare(outs, units, want, list(range(b.n)), f"generic {name} P = {precision}")


@pytest.mark.parametrize("name,precision,over", WIDE, ids=WIDE_IDS)
def test_staged_fdct_every_tie(env, name, precision, over):
    """jpeg_amd_planar_fdct (k_fdct_plane: the literal division and round_half_away) on the oracle's decomposed planes of the
    same batches, one call per image (the tables are host tables)."""
    e, _lib = env, env["_lib"]
    b = _wide(name, precision, over)
    want = _reference(b)
    L, units = _layout(e, b)
    planar = [b.planar(i) for i in range(b.n)]
    d_planes = [_device(e, np.stack([pl[p] for pl in planar])) for p in range(len(units))]
    outs = _outputs(e, units, b.n)
    tables = np.ascontiguousarray(b.tables)
    for i in range(b.n):
        st = e["lib"].jpeg_amd_planar_fdct(e["ctx"].handle, C.byref(L), _lib.ptr_array([d[i].data_ptr() for d in d_planes]),
                                           tables[i].ctypes.data, 2, _lib.ptr_array([o[i].data_ptr() for o in outs]))
        assert st == 0, (st, i)
    _compare(outs, units, want, list(range(b.n)), f"staged {name} P = {precision}")


# ---- k_spectral_reduce ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("denom", [8, 4])
def test_spectral_reduce_output_ties(env, denom):
    """DC-only inputs under an all-ones table give freely chosen samples at 1/8 (and 2 x 2 cells of them at 1/4), so the output
    planes are tie blocks under the OUTPUT table, which takes every Q = 1 .. 255: m = +-1, +-3 and the largest +-m per Q.  The
    reference is _reduce_ref."""
    e, _lib, torch = env, env["_lib"], env["torch"]
    coef, size, samples, tables = QR.reduce_batch(denom)
    n, uy, ux, _ = coef.shape
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes, L.scale_x, L.scale_y = size[0], size[1], 8, 1, 1, 1
    L.factor_x[0], L.factor_y[0], L.qi[0] = 1, 1, 0
    assert e["lib"].jpeg_amd_layout_units(C.byref(L)) == 0 and (L.units_x[0], L.units_y[0]) == (ux, uy)
    out_layout = _lib.Layout()
    assert e["lib"].jpeg_amd_reduce_layout(C.byref(L), denom, C.byref(out_layout)) == 0
    units = (out_layout.units_x[0], out_layout.units_y[0])
    assert units == (samples.shape[2] // 8, samples.shape[1] // 8)
    ones = np.ones(64, np.uint16)
    d_in = _device(e, coef.reshape(n, -1))
    d_q = _device(e, np.ones((n, 1, 64), np.uint16))
    d_qo = _device(e, tables)
    out = torch.full((n, 64 * units[0] * units[1]), FILL, dtype=torch.int16, device=e["ctx"].torch_device)
    st = e["lib"].jpeg_amd_spectral_reduce_batch(e["ctx"].handle, C.byref(L), n, denom, _lib.ptr_array([d_in.data_ptr()]),
                                                 _lib.size_array([64 * ux * uy]), d_q.data_ptr(), 64, 1, d_qo.data_ptr(),
                                                 _lib.ptr_array([out.data_ptr()]), _lib.size_array([64 * units[0] * units[1]]))
    assert st == 0, st
    got = out.cpu().numpy().reshape(n, units[1], units[0], 64)
    for i in range(n):
        want = R.reduce_plane(coef[i], ones, denom, units, tables[i, 0])
        bad = got[i] != want
        assert not bad.any(), f"Q = {i + 1}: {int(bad.sum())} coefficients differ, first at {np.argwhere(bad)[0].tolist()}"


# ---- full swing --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("crop", [0, 3], ids=["w80", "w77"])
@pytest.mark.parametrize("name", ["grey", "444", "420", "422", "440"])
def test_full_swing_through_the_fused_generic_and_staged_encoders(env, name, crop):
    """0 / 255 checkerboards and 8-pixel stripes in both axes under tables of all ones and of all 255: the largest magnitudes
    of either sign, next to each other in the packed pairs.  The pattern in every plane (one chroma plane inverted, one shifted) as
    YCbCr input and as a grey RGB input of the fused encoder, and as samples of the generic and the staged one."""
    e, _lib, J = env, env["_lib"], env["J"]
    pats = QR.swing_images()[:, :, :80 - crop]
    n0, h, w = pats.shape
    factors = QR.FACTORS[name]
    scale = (max(f[0] for f in factors), max(f[1] for f in factors))
    ycc = np.stack([pats, 255 - pats, np.roll(pats, 1, axis=0)], axis=-1)         # uint8 [n0, h, w, 3]
    grey = np.stack([pats, pats, pats], axis=-1)                                  # R = G = B: the luma keeps the whole swing
    tables = np.concatenate([np.full((n0, 2, 64), 1, np.uint16), np.full((n0, 2, 64), 255, np.uint16)])
    n = 2 * n0
    comps = {i + 1: J.Component(f, min(i, 1)) for i, f in enumerate(factors)}
    layout = J.Layout("y8" if len(factors) == 1 else "ycc8", comps)
    units = layout.units((w, h))
    L = layout.c_layout((w, h), units, [min(i, 1) for i in range(len(factors))])
    d_q = _device(e, tables)
    sizes = _lib.size_array([64 * a * c for a, c in units])

    def reference(rect):                                                       # rect uint16 [h, w, planes]
        return O.decompose(rect, (w, h), factors, scale)

    for color, pack, half in ((_lib.COLOR_YCC8, O.pack_ycc8, ycc), (_lib.COLOR_RGB8, O.pack_rgb8, grey)):
        px = np.concatenate([half, half])
        rects = [pack(px[i].reshape(-1, 3), len(factors)).reshape(h, w, len(factors)) for i in range(n)]
        planar = [reference(r) for r in rects]
        want = [[O.fdct_plane(p, tables[i][min(k, 1)]) for k, p in enumerate(planar[i])] for i in range(n)]
        luma = np.stack([want[i][0] for i in range(n0)])                       # under the all-ones table: flat 0 and flat 255 (254 from RGB)
        assert int(luma.min()) == -1024 and int(luma.max()) >= 1008
        outs = _outputs(e, units, n)
        d_px = _device(e, px)
        st = e["lib"].jpeg_amd_encode_batch(e["ctx"].handle, C.byref(L), n, d_px.data_ptr(), w * h * 3, color, d_q.data_ptr(), 128, 2,
                                            _lib.ptr_array([o.data_ptr() for o in outs]), sizes)
        assert st == 0, st
        _compare(outs, units, want, list(range(n)), f"fused {name} colour {color}")
        # the generic encoder on the packed samples
        outs = _outputs(e, units, n)
        d_rect = _device(e, np.stack(rects))
        st = e["lib"].jpeg_amd_rectangular_spectral_batch(e["ctx"].handle, C.byref(L), n, d_rect.data_ptr(), w * h * len(factors),
                                                          d_q.data_ptr(), 128, 2, _lib.ptr_array([o.data_ptr() for o in outs]), sizes)
        assert st == 0, st
        _compare(outs, units, want, list(range(n)), f"generic {name} colour {color}")
        # the staged transform on the decomposed planes
        outs = _outputs(e, units, n)
        d_planes = [_device(e, np.stack([pl[p] for pl in planar])) for p in range(len(units))]
        for i in range(n):
            st = e["lib"].jpeg_amd_planar_fdct(e["ctx"].handle, C.byref(L), _lib.ptr_array([d[i].data_ptr() for d in d_planes]),
                                               np.ascontiguousarray(tables[i]).ctypes.data, 2, _lib.ptr_array([o[i].data_ptr() for o in outs]))
            assert st == 0, (st, i)
        _compare(outs, units, want, list(range(n)), f"staged {name} colour {color}")
