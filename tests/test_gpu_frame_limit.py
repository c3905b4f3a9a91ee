"""Every kernel family at the 65535-pixel frame limit, on the MI355X: images whose long side is the most a frame header can say
(65535, and 65529 with a single pixel column in the last block) and whose short side is one MCU plus one pixel, "widest" and
"tallest".  What goes wrong here and nowhere else: a coordinate or product that no longer fits its type, a magic-number quotient
outside its proven range (div_trunc_small: a + b t reaches 131066 on a centred axis of thirds or quarters), a tile count or
prefix that outgrows its field, float32 source coordinates whose ulp is 2^-8.

Every comparison is exact, sample for sample, against the family's own reference (the oracle, _scaled_ref, _transform_ref,
_reduce_ref, the float32 mirrors of the resample contracts), none of which shares code with the kernels.  The cases, shapes and
inputs are in tests/_frame_limit.py; tests/test_frame_limit_cpu.py holds the inputs to their conditions without a GPU, so that
no test here passes on clamped or self-similar data.  Outputs go through _calls.Out: a sentinel in every byte between and behind
the images.  A failing assertion names the case, the first four mismatching coordinates and their tile."""
import ctypes as C

import numpy as np
import pytest

import _frame_limit as FL
import _generic_cases as GC
import _reduce_ref as RR
import _scaled_ref as S
import _tensor_ref as T
import _transform_ref as X
import _warp_ref as W
from _calls import Out, c_layout, c_regions, c_views, pixel_image, plane_ptrs, plane_units, strides
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _mixed import view_mixed
from _resample import c_spec, pack
from _tile import crop
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

RGB, YCC = _lib.COLOR_RGB8, _lib.COLOR_YCC8
_ids = lambda cases: ["-".join(str(v) for v in c) for c in cases]


# ---- the reports ------------------------------------------------------------------------------------------------------------------------------

def _samples(got, want, what, tile):
    """'' when got [H, W, C] is want; else the count and the first four positions with the kernel's tile (tile: (w, h) in pixels)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return f"{what}: {got.dtype} {got.shape} against {want.dtype} {want.shape}"
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    first = "; ".join(f"(x {x}, y {y}, channel {c}) [tile column {x // tile[0]}, row {y // tile[1]}]: {int(got[y, x, c])} != {int(want[y, x, c])}"
                      for y, x, c in bad[:4])
    return f"{what}: {len(bad)} of {want.size} samples differ (tiles of {tile[0]} x {tile[1]}); first {first}"


def _coefficients(got, want, what, tile):
    """The same for the coefficient planes [uy, ux, 64] of an image (tile: (w, h) in blocks of that plane)."""
    for p, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return f"{what}: plane {p}: {a.shape} against {b.shape}"
        bad = np.argwhere(a != b)
        if len(bad):
            first = "; ".join(f"(block x {x}, block y {y}, zigzag {z}) [tile column {x // tile[0]}, row {y // tile[1]}]: {int(a[y, x, z])} != {int(b[y, x, z])}"
                              for y, x, z in bad[:4])
            return f"{what}: plane {p}: {len(bad)} of {b.size} coefficients differ (tiles of {tile[0]} x {tile[1]} blocks); first {first}"
    return ""


def _check(report):
    assert not report, report


def _upload(ctx, torch, a, dtype=None):
    a = np.array(a)                                             # the shared inputs are read-only
    return torch.from_numpy(a if dtype is None else a.view(dtype)).to(ctx.torch_device)


def _guarded(ctx, torch, images, gap):
    """Host arrays of one size in one device buffer, `gap` elements of a filler between and behind them -> (tensor, stride)."""
    flat = np.stack([np.asarray(im).reshape(-1) for im in images])
    room = np.full((len(images), flat.shape[1] + gap), 0x5A, flat.dtype)
    room[:, :flat.shape[1]] = flat
    return torch.from_numpy(room).to(ctx.torch_device), flat.shape[1] + gap


def _coef_outs(ctx, torch, units, n, gap=64, lead=64):
    """One guarded buffer per plane: whole blocks of gap and lead (the transform kernel's test asks for multiples of 8 elements)."""
    return [Out(ctx, torch, [64 * ux * uy] * n, elem=2, gap=gap * (p + 1), lead=lead, tail=8) for p, (ux, uy) in enumerate(units)]


def _coef_images(outs, units, i):
    return [o.images()[i].view(np.int16).reshape(uy, ux, 64) for o, (ux, uy) in zip(outs, units)]


# ---- 1. k_luma_fused, k_encode_fused: the 8-bit layouts other than 4:2:0 ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,cosited,long,orient", FL.FUSED8_CASES, ids=_ids(FL.FUSED8_CASES))
def test_fused_8_bit_decode_and_encode(ctx, torch, name, cosited, long, orient):
    """jpeg_amd_decode_batch == the oracle's decode + unpack, and jpeg_amd_encode_batch on those pixels == the oracle's encode, RGB
    and YCbCr; the 65529 cases as batches of two images with a gap.  (Tiles in the reports: the MCU for the decode, whose strips
    are rows of MCUs; 256 x 64 pixels for the encoder, stated in blocks of the plane at the image's scale.)"""
    factors = FL.LAYOUTS[name]
    scale = FL.scale_of(factors)
    w, h = size = FL.extent(scale, long, orient)
    n = FL.fused8_images(long)
    L = c_layout(w, h, factors)
    ph, qh = FL.image8(name, size, n)
    planes, dq, ntables = [_upload(ctx, torch, p) for p in ph], _upload(ctx, torch, qh, np.int16), qh.shape[1]
    for color in (RGB, YCC):
        what = (name, "cosited" if cosited else "centred", size, FL.COLORS[color])
        out = Out(ctx, torch, [3 * w * h] * n, gap=5, tail=7)
        assert _lib.lib().jpeg_amd_decode_batch(ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(),
                                               ntables * 64, ntables, cosited, color, out.ptr, out.stride) == 0
        wants = [FL.decoded8(name, size, 1, cosited, i, n)[color] for i in range(n)]
        for i, g in enumerate(out.images()):
            _check(_samples(g.reshape(h, w, 3), wants[i], (what, "decode", "image", i), (8 * scale[0], 8 * scale[1])))
        px, px_stride = _guarded(ctx, torch, wants, 5)
        outs = _coef_outs(ctx, torch, plane_units(L), n)
        assert _lib.lib().jpeg_amd_encode_batch(ctx.handle, C.byref(L), n, px.data_ptr(), px_stride, color, dq.data_ptr(), ntables * 64, ntables,
                                               _lib.ptr_array([o.ptr for o in outs]), _lib.size_array([o.stride for o in outs])) == 0
        for i in range(n):
            _check(_coefficients(_coef_images(outs, plane_units(L), i), FL.encoded8(wants[i], size, factors, color),
                                 (what, "encode", "image", i), (32, 8)))


# ---- 2. k_generic_fused, k_generic_encode ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def J():
    import jpeg_amd
    return jpeg_amd


def _generic_layout(J, c):
    comps = {i + 1: J.Component(f, i & 1) for i, f in enumerate(c.factors)}
    layout = J.Layout(("custom", c.precision, c.count), comps)
    assert layout.scale == c.scale and [p.factor for p in layout.planes] == list(c.factors)
    return layout


GENERIC_TILE = (GC.TILE_W, 32)                             # 128 x 64 or 128 x 32: the reports name the 32-row band


@pytest.mark.parametrize("number,cosite,long,orient", FL.GENERIC_CASES, ids=_ids(FL.GENERIC_CASES))
def test_generic_decode_and_encode(J, ctx, number, cosite, long, orient):
    """Spectral.rectangular(cosite:) == the oracle's idct + interleaved == the staged kernels, and Rectangular.spectral on the
    oracle's samples == the oracle's decomposed + fdct (cases 5 and 6 take the staged encoder inside the same call: a box of 3).
    A centred axis of thirds or quarters reaches a + b t = 131066 here, 127 times what the seam tests reach.  None of these
    cases takes the ticket walk (each has a plane on the literal filter): a workgroup per tile, about 2048 tiles when tallest;
    the walk has its own test below."""
    c = GC.case(number)
    size = FL.extent(c.scale, long, orient)
    what = (f"case {number}", "cosited" if cosite else "centred", size)
    planes, tables, q = FL.generic_input(number, size)
    want = FL.generic_rect(number, size, cosite)
    layout = _generic_layout(J, c)
    spectral = J.Spectral.from_host(ctx, size, layout, [np.array(p) for p in planes], tables, q=q)
    got = spectral.rectangular(cosite=cosite).host_values()
    _check(_samples(got, want, (what, "one call against the oracle"), GENERIC_TILE))
    _check(_samples(spectral.idct().interleaved(cosite=cosite).host_values(), want, (what, "the staged kernels against the oracle"), GENERIC_TILE))
    etables = GC.encode_tables(c)
    _, want_f = GC.oracle_encode(c, size, want, etables)
    assert max(int(np.abs(f.astype(np.int32)).max()) for f in want_f) < 32000      # where the reference would trap
    rect = J.Rectangular.from_host(ctx, size, layout, np.array(want))
    _check(_coefficients(rect.spectral(etables).host_planes(), want_f, (what, "encode against the oracle"), (32, 8)))


def test_generic_ticket_walk_batch_of_three_tallest_420_twelve_bit(J, ctx, torch):
    """THE case that takes the ticket walk (`walk` in launch_generic_fused: 64-row tiles, every subsampled plane on the exact
    filter, more tiles than resident workgroups): 4:2:0 at 12 bits, 17 x 65535, three images in one
    jpeg_amd_spectral_rectangular_batch call -- 3072 tiles, drawn from the counter, image = tile / 1024 -- with their own tables and
    a gap between the images; then jpeg_amd_rectangular_spectral_batch on the oracle's samples."""
    c, n, gap = FL.WALK, FL.WALK_IMAGES, 24
    w, h = size = FL.extent(c.scale, FL.LONGS[0], "tallest")
    layout = _generic_layout(J, c)
    units = layout.units(size)
    L = layout.c_layout(size, units, c.q)
    inputs = [FL.generic_input(0, size, i) for i in range(n)]
    tables = np.stack([np.stack(t) for _, t, _ in inputs])                     # [n, 2, 64]
    assert not (tables[0] == tables[1]).all()
    d_planes = [_upload(ctx, torch, np.stack([inputs[i][0][p] for i in range(n)])) for p in range(c.count)]
    d_q = _upload(ctx, torch, tables, np.int16)
    out = Out(ctx, torch, [w * h * c.count] * n, elem=2, gap=gap, tail=8)
    assert _lib.lib().jpeg_amd_spectral_rectangular_batch(ctx.handle, C.byref(L), n, plane_ptrs(d_planes), _lib.size_array([64 * a * b for a, b in units]),
                                                         d_q.data_ptr(), 128, 2, 0, out.ptr, out.stride) == 0
    wants = [FL.generic_rect(0, size, False, i) for i in range(n)]
    for i, g in enumerate(out.images()):
        _check(_samples(g.view(np.uint16).reshape(h, w, c.count), wants[i], ("the walk", size, "image", i), (128, 64)))
    rng = np.random.default_rng(7800)
    etables = rng.integers(16, 60, (n, 2, 64)).astype(np.uint16)
    d_rect, rect_stride = _guarded(ctx, torch, [np.array(x).view(np.int16) for x in wants], gap)
    outs = _coef_outs(ctx, torch, units, n)
    assert _lib.lib().jpeg_amd_rectangular_spectral_batch(ctx.handle, C.byref(L), n, d_rect.data_ptr(), rect_stride, _upload(ctx, torch, etables, np.int16).data_ptr(),
                                                         128, 2, _lib.ptr_array([o.ptr for o in outs]), _lib.size_array([o.stride for o in outs])) == 0
    for i in range(n):
        _, want_f = GC.oracle_encode(c, size, wants[i], list(etables[i]))
        _check(_coefficients(_coef_images(outs, units, i), want_f, ("encode", size, "image", i), (32, 8)))


# ---- 3. the tile family: k_region_decode, k_scaled_decode, k_view_decode, k_view_decode_mixed, k_region_crop, k_idct_scaled ------------------------------

def _device_image(ctx, torch, name, size):
    """-> (L, device planes, device tables, ntables) of FL.image8(name, size)."""
    ph, qh = FL.image8(name, size)
    return c_layout(size[0], size[1], FL.LAYOUTS[name]), [_upload(ctx, torch, p) for p in ph], _upload(ctx, torch, qh, np.int16), qh.shape[1]


@pytest.mark.parametrize("name,long,orient", FL.TILE_CASES, ids=_ids(FL.TILE_CASES))
def test_tile_family_at_the_far_end(ctx, torch, name, long, orient):
    """Regions at the far end (the last 200 columns whole, the last pixel alone, a window across the last MCU boundary) and one
    across pixel 32768, the whole image at 1/2, 1/4 and 1/8, and one view per denominator at the far end of its scaled image
    plus one across pixel 32768 at full size, RGB and YCbCr, each as one call
    of several images (every image reads image 0; the outputs lie apart, with gaps).  4:1:1 has no tile kernel: its region and
    scaled calls reach k_region_crop and k_idct_scaled, and it has no view call."""
    lib = _lib.lib()
    scale = FL.scale_of(FL.LAYOUTS[name])
    size = FL.extent(scale, long, orient)
    L, planes, dq, ntables = _device_image(ctx, torch, name, size)
    head = (ctx.handle, C.byref(L))
    source = (plane_ptrs(planes), _lib.size_array(strides(L, distinct=False)), dq.data_ptr(), 0, ntables, 0)
    regions = FL.far_regions(size, scale, orient)
    views = [FL.far_view(size, d, orient) for d in (8, 1, 4, 2)] + [FL.wrap_view(size, orient)]
    for color in (RGB, YCC):
        what = (name, size, FL.COLORS[color])
        want = {d: FL.decoded8(name, size, d)[color] for d in (1, 2, 4, 8)}
        out = Out(ctx, torch, [3 * r[2] * r[3] for r in regions], gap=5, tail=7)
        assert lib.jpeg_amd_decode_region_batch(*head, len(regions), *source, color, c_regions(regions), out.ptr, out.stride) == 0
        for r, g in zip(regions, out.images()):
            _check(_samples(g.reshape(r[3], r[2], 3), crop(want[1], r), (what, "region", r), (128, 64)))
        for denom in FL.DENOMS:
            W1, H1 = S.scaled_size(size, denom)
            out = Out(ctx, torch, [3 * W1 * H1] * 2, gap=11, tail=11)
            assert lib.jpeg_amd_decode_scaled_batch(*head, 2, *source, color, denom, out.ptr, out.stride) == 0
            for g in out.images():
                _check(_samples(g.reshape(H1, W1, 3), want[denom], (what, "scaled", denom), (128, 32)))
        if name == "411":
            continue
        out = Out(ctx, torch, [3 * r[2] * r[3] for _, r in views], gap=5, tail=7)
        assert lib.jpeg_amd_decode_view_batch(*head, len(views), *source, color, c_views(views), out.ptr, out.stride) == 0
        for (denom, r), g in zip(views, out.images()):
            _check(_samples(g.reshape(r[3], r[2], 3), crop(want[denom], r), (what, "view", denom, r), (128, 32)))


@pytest.mark.parametrize("color", [RGB, YCC], ids=["rgb", "ycc"])
@pytest.mark.parametrize("order", ["as listed", "reversed"])
def test_mixed_call_of_a_widest_a_tallest_and_a_small_image(ctx, torch, order, color):
    """jpeg_amd_decode_view_mixed on a 65535 x 17 4:2:0 image at 1/2, a 9 x 65535 grey image at 1/4 and a 17 x 33 4:2:0 image, far-end
    views, in both orders: the per-image tile prefix and the per-image geometry side by side."""
    cases = FL.MIXED if order == "as listed" else FL.MIXED[::-1]
    images = [_device_image(ctx, torch, name, size) for name, size, _ in cases]
    args = [(L, [p.data_ptr() for p in planes], dq.data_ptr(), ntables) for L, planes, dq, ntables in images]
    views = [v for _, _, v in cases]
    out = Out(ctx, torch, [3 * r[2] * r[3] for _, r in views], gap=5, tail=7)
    assert view_mixed(ctx.handle, args, 0, color, views, out.ptr, out.stride) == 0
    for (name, size, (denom, r)), g in zip(cases, out.images()):
        _check(_samples(g.reshape(r[3], r[2], 3), crop(FL.decoded8(name, size, denom)[color], r), (order, name, size, denom, r, FL.COLORS[color]), (128, 32)))


# ---- 4. the coefficient domain: k_spectral_transform, k_spectral_reduce -----------------------------------------------------------------------------

@pytest.mark.parametrize("name,long,orient", FL.SPECTRAL_CASES, ids=_ids(FL.SPECTRAL_CASES))
def test_transform_every_op_at_the_far_end(ctx, torch, name, long, orient):
    """All eight ops, with and without requantisation, on the whole image and on a crop region that begins ten MCUs in front of the
    last MCU boundary; two images with gaps.  The transposing ops turn the widest image into the tallest and back: planes 8192
    blocks long on either axis of the 256 x 1 and the 32 x 8 workgroups."""
    factors = FL.LAYOUTS[name]
    scale = FL.scale_of(factors)
    size = FL.extent(scale, long, orient)
    n = 2
    ph, q_in, q_out = FL.transform_input(name, size, n)
    qi, ntables = X.layout_tables(name)
    L = c_layout(size[0], size[1], factors, qi=qi)
    d_in, d_q, d_qo = [_upload(ctx, torch, p) for p in ph], _upload(ctx, torch, q_in, np.int16), _upload(ctx, torch, q_out, np.int16)
    flag = torch.zeros(1, dtype=torch.int32, device=ctx.torch_device)
    for op in range(8):
        m, _ = X.mapping_arrays(op)
        for region in (None, FL.far_crop(size, scale, orient)):
            _, _, _, units, cropped, origin = X.layout_ref(size[0], size[1], factors, op, region)
            moved = [[X.transform_plane(ph[p][i], op, cropped[p], origin[p]) for i in range(n)] for p in range(len(factors))]
            for requantise in (False, True):
                outs = _coef_outs(ctx, torch, units, n, gap=8, lead=24)
                reg = None if region is None else _lib.Region(*region)
                assert _lib.lib().jpeg_amd_spectral_transform_batch(
                    ctx.handle, C.byref(L), n, op, None if reg is None else C.byref(reg), plane_ptrs(d_in), _lib.size_array(strides(L)),
                    d_q.data_ptr() if requantise else None, 64 * ntables, ntables, d_qo.data_ptr() if requantise else None,
                    _lib.ptr_array([o.ptr for o in outs]), _lib.size_array([o.stride for o in outs]), flag.data_ptr()) == 0
                assert int(flag.item()) == 0
                for i in range(n):
                    want = [moved[p][i] for p in range(len(factors))]
                    if requantise:
                        want = [X.requantize_ref(t, q_in[i, qi[p]][m], q_out[i, qi[p]]) for p, t in enumerate(want)]
                        assert not any(trap for _, trap in want)
                        want = [t for t, _ in want]
                    tile = (32, 8) if op & 1 else (256, 1)
                    _check(_coefficients(_coef_images(outs, units, i), want, (name, size, "op", op, "region", region, "requantise", requantise, "image", i), tile))


@pytest.mark.parametrize("name,long,orient", FL.SPECTRAL_CASES, ids=_ids(FL.SPECTRAL_CASES))
def test_reduce_at_every_denominator(ctx, torch, name, long, orient):
    """jpeg_amd_spectral_reduce_batch at 1/2, 1/4 and 1/8, with the input tables and with others, two images with gaps, against
    _reduce_ref (tiles: 16 x 16 output blocks at 1/2 and 1/4, 8 x 8 at 1/8)."""
    factors = FL.LAYOUTS[name]
    scale = FL.scale_of(factors)
    size = FL.extent(scale, long, orient)
    n = 2
    ph, qh = FL.image8(name, size, n)
    L = c_layout(size[0], size[1], factors)
    qi = [L.qi[p] for p in range(L.nplanes)]
    planes, dq, ntables = [_upload(ctx, torch, p) for p in ph], _upload(ctx, torch, qh, np.int16), qh.shape[1]
    qoh = np.random.default_rng(long).integers(1, 40, qh.shape).astype(np.uint16)
    dqo = _upload(ctx, torch, qoh, np.int16)
    for denom in FL.DENOMS:
        reduced = _lib.Layout()
        assert _lib.lib().jpeg_amd_reduce_layout(C.byref(L), denom, C.byref(reduced)) == 0
        units = plane_units(reduced)
        for others in (False, True):
            outs = _coef_outs(ctx, torch, units, n)
            assert _lib.lib().jpeg_amd_spectral_reduce_batch(
                ctx.handle, C.byref(L), n, denom, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables,
                dqo.data_ptr() if others else None, _lib.ptr_array([o.ptr for o in outs]), _lib.size_array([o.stride for o in outs])) == 0
            for i in range(n):
                _, want = RR.reduce_image([p[i] for p in ph], [qh[i, t] for t in qi], factors, scale, size, denom,
                                          [qoh[i, t] for t in qi] if others else None)
                tile = (8, 8) if denom == 8 else (16, 16)
                _check(_coefficients(_coef_images(outs, units, i), want, (name, size, "denominator", denom, "other tables", others, "image", i), tile))


# ---- 5. the resample and mapped walks from pixel sources ----------------------------------------------------------------------------------------------

RESAMPLE_TILE = (64, 32)
SMALL = (40, 30)                                            # the second source of every call: another extent, a nonzero record offset


def _small():
    return pixel_image("random", SMALL[0], SMALL[1], 4030)


@pytest.mark.parametrize("name,orient,k", FL.RESIZE_CASES, ids=_ids(FL.RESIZE_CASES))
def test_resize_from_a_source_65535_long(ctx, torch, name, orient, k):
    """jpeg_amd_resize_batch (bilinear) / jpeg_amd_resize_filter_batch to bytes and jpeg_amd_resize_filter_tensor_batch to a mirrored
    float32 CHW tensor: k = 0, the same long side over a larger short side (a factor of 1 along 65535 pixels); k = 1, the
    strongest reduction the filter takes.  The source coordinates are float32: one ulp at 65535 is 2^-8."""
    lib = _lib.lib()
    code, mirror, _ = FL.FILTERS[name]
    out_w, out_h = FL.resize_targets(name, orient)[k]
    images = [np.array(FL.source(orient)), _small()]
    wants = [FL.resized(name, orient, k), mirror(images[1], out_w, out_h)]
    d_src, src_stride, ext = pack(ctx, torch, images)
    head = (ctx.handle, len(images), d_src.data_ptr(), src_stride, ext, out_w, out_h)
    out = Out(ctx, torch, [3 * out_w * out_h] * 2, gap=5, lead=4, tail=7)
    if name == "bilinear":
        assert lib.jpeg_amd_resize_batch(*head, out.ptr, out.stride) == 0
    else:
        assert lib.jpeg_amd_resize_filter_batch(*head, code, out.ptr, out.stride) == 0
    for i, g in enumerate(out.images()):
        _check(_samples(g.reshape(out_h, out_w, 3), wants[i], (name, orient, (out_w, out_h), "bytes", "image", i), RESAMPLE_TILE))
    spec, flips = T.Spec(T.F32, T.CHW), [1, 0]
    out = Out(ctx, torch, [3 * out_w * out_h] * 2, elem=4, gap=3, tail=7)
    assert lib.jpeg_amd_resize_filter_tensor_batch(*head, code, C.byref(c_spec(spec)), (C.c_uint8 * 2)(*flips), out.ptr, out.stride) == 0
    for i, g in enumerate(out.images()):
        got = g.copy().view(np.uint32).reshape(3, out_h, out_w).transpose(1, 2, 0)
        _check(_samples(got, T.normalise(wants[i], spec, flips[i]).transpose(1, 2, 0), (name, orient, (out_w, out_h), "f32 chw, bit patterns", "image", i),
                        RESAMPLE_TILE))


@pytest.mark.parametrize("name,orient,filt,edge", FL.MAP_CASES, ids=_ids(FL.MAP_CASES))
def test_warp_and_projective_maps_at_the_far_end(ctx, torch, name, orient, filt, edge):
    """A translation that lays a 320-pixel window over the last 300 source pixels (FILL and REPLICATE both bind), the same under a
    mild perspective, and a quarter turn of the long side into the other axis: jpeg_amd_project_batch (bilinear) or
    jpeg_amd_project_filter_batch (bicubic), and for the two affine maps jpeg_amd_warp_batch as well."""
    lib = _lib.lib()
    m, (out_w, out_h) = FL.mapped(name, orient)
    images = [np.array(FL.source(orient)), _small()]
    second = np.array([1, 0, -2, 0, 1, 3, 0, 0, 1], np.float32)                # a shift: taps off both of its edges
    matrices = np.ascontiguousarray(np.stack([m, second]), np.float32)
    project = FL.P.project if filt == "bilinear" else FL.Q.project
    wants = [FL.projected(name, orient, filt, edge), project(images[1], second, out_w, out_h, FL.EDGES[edge], FL.FILL)]
    d_src, src_stride, ext = pack(ctx, torch, images)
    wp = _lib.Warp()
    wp.edge = FL.EDGES[edge]
    wp.fill[0], wp.fill[1], wp.fill[2] = FL.FILL
    head = (ctx.handle, 2, d_src.data_ptr(), src_stride, ext)
    out = Out(ctx, torch, [3 * out_w * out_h] * 2, gap=5, lead=3, tail=7)
    if filt == "bilinear":
        assert lib.jpeg_amd_project_batch(*head, matrices.ctypes.data, C.byref(wp), out_w, out_h, out.ptr, out.stride) == 0
    else:
        assert lib.jpeg_amd_project_filter_batch(*head, matrices.ctypes.data, C.byref(wp), _lib.FILTER_BICUBIC, out_w, out_h, out.ptr, out.stride) == 0
    ctx.synchronize()
    for i, g in enumerate(out.images()):
        _check(_samples(g.reshape(out_h, out_w, 3), wants[i], (name, orient, filt, edge, "image", i), RESAMPLE_TILE))
    if filt == "bilinear" and name != "perspective":
        six = np.ascontiguousarray(np.stack([FL.affine(m), FL.affine(second)]), np.float32)
        out = Out(ctx, torch, [3 * out_w * out_h] * 2, gap=5, lead=3, tail=7)
        assert lib.jpeg_amd_warp_batch(*head, six.ctypes.data, C.byref(wp), out_w, out_h, out.ptr, out.stride) == 0
        ctx.synchronize()
        for i, g in enumerate(out.images()):
            want = W.warp(images[i], six[i], out_w, out_h, FL.EDGES[edge], FL.FILL)
            _check(_samples(g.reshape(out_h, out_w, 3), want, (name, orient, "jpeg_amd_warp_batch", edge, "image", i), RESAMPLE_TILE))


@pytest.mark.parametrize("color", [RGB, YCC], ids=["rgb", "ycc"])
def test_decode_resized_and_decode_tensor_of_a_far_end_view(ctx, torch, color):
    """The composed route: the last 300 columns of the 65535 x 17 4:2:0 image at 1/2, decoded and resampled to 64 x 5 in one call,
    against _tile.reference, cropped, through _resize_ref; two images (both read image 0), bytes and a float32 CHW tensor."""
    name, size, view, (out_w, out_h) = FL.COMPOSED
    L, planes, dq, ntables = _device_image(ctx, torch, name, size)
    want = FL.composed()[color]
    views = [view, view]
    head = (ctx.handle, C.byref(L), 2, plane_ptrs(planes), _lib.size_array(strides(L, distinct=False)), dq.data_ptr(), 0, ntables, 0, color,
            c_views(views), out_w, out_h)
    out = Out(ctx, torch, [3 * out_w * out_h] * 2, gap=5, tail=7)
    assert _lib.lib().jpeg_amd_decode_resized_batch(*head, out.ptr, out.stride) == 0
    for g in out.images():
        _check(_samples(g.reshape(out_h, out_w, 3), want, ("decode_resized", view, FL.COLORS[color]), RESAMPLE_TILE))
    spec, flips = T.Spec(T.F32, T.CHW), [0, 1]
    out = Out(ctx, torch, [3 * out_w * out_h] * 2, elem=4, gap=3, tail=7)
    assert _lib.lib().jpeg_amd_decode_tensor_batch(*head, C.byref(c_spec(spec)), (C.c_uint8 * 2)(*flips), out.ptr, out.stride) == 0
    for i, g in enumerate(out.images()):
        got = g.copy().view(np.uint32).reshape(3, out_h, out_w).transpose(1, 2, 0)
        _check(_samples(got, T.normalise(want, spec, flips[i]).transpose(1, 2, 0), ("decode_tensor", view, FL.COLORS[color], "image", i), RESAMPLE_TILE))
