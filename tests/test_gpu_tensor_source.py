"""Tensor sources on the MI355X (jpeg_amd_tensor_pixels_batch, jpeg_amd_encode_tensor_batch, jpeg_amd_compress_tensor_batch_device;
k_tensor_pixels): every byte is compared with _tensor_source_ref -- the contract of include/jpeg_amd.h restated in numpy -- and
every coefficient and file with what the existing calls (jpeg_amd_encode_batch, jpeg_amd_compress_batch_device) give on that
reference's bytes.  Every output buffer is filled with the byte 0xA5 before the call, and every byte that belongs to no image is
checked after it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _tensor_source_ref as S
import jpeg_amd as J
from _calls import (FUSED, RESIZE_SIZE as SIZE, RESIZE_TILE_H as TILE_H, RESIZE_TILE_W as TILE_W, RESIZE_VIEWS as VIEWS, c_layout,
                    resize_py_layout, synthetic)
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import same as _same
from jpeg_amd import _lib
from jpeg_amd.api import _metadata_array, _scan_array

pytestmark = pytest.mark.gpu

F = np.float32
OK, EINVAL = 0, -1
COMBOS = [(d, l) for d in S.DTYPES for l in S.LAYOUTS]
COMBO_IDS = ["%s-%s" % (S.DTYPE_NAMES[d], S.LAYOUT_NAMES[l]) for d, l in COMBOS]
# (13, 5): rows of 13 and 39 elements -- runs begin at every alignment -- and a last run of one pixel; (224, 224): vector
# loads only; (70, 67): two tiles across, three down, and a partial last run
EXTENTS = [(1, 1), (13, 5), (224, 224), (TILE_W + 6, 2 * TILE_H + 3)]
N = 3
ENCODE_FACTORS = dict(FUSED, **{"411": [(4, 1), (1, 1), (1, 1)]})   # 4:1:1 takes the staged kernels
ENCODE_SIZES = [(16, 16), (17, 9), (264, 72)]                      # 264 x 72: one 256 x 64 encoder tile plus a block each way


def _c_source(src):
    s = _lib.TensorSource()
    s.dtype, s.layout = src.dtype, src.layout
    for c in range(3):
        s.scale[c], s.offset[c] = float(src.scale[c]), float(src.offset[c])
    return s


def _shape(layout, w, h):
    return (h, w, 3) if layout == S.HWC else (3, h, w)


def _elements(seed, src, w, h, n=N):
    """n images of element bit patterns in src's dtype and layout whose bytes span [-64, 320] before the clamp, with the
    special values at the first and last element of rows."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        if src.dtype == S.U8:
            bits = rng.integers(0, 256, _shape(src.layout, w, h), dtype=np.uint8)
        else:
            want = rng.uniform(-64.0, 320.0, (h, w, 3))
            e = ((want - src.offset.astype(np.float64)) / src.scale.astype(np.float64)).astype(F)
            bits = S.to_bits(e, src.dtype)
            if src.layout == S.CHW:
                bits = np.ascontiguousarray(bits.transpose(2, 0, 1))
            bits = S.with_specials(bits, src.dtype, src.layout)
        out.append(bits)
    return out


def _front(ctx, torch, images, w, h, src, gap=0, lead=0, dst_gap=3):
    """jpeg_amd_tensor_pixels_batch on `images` -> the n byte images [h, w, 3]."""
    d_in = S.SourceIn(ctx, torch, images, src.dtype, gap=gap, lead=lead)
    out = S.PixelsOut(ctx, torch, len(images), w, h, gap=dst_gap)
    st = _lib.lib().jpeg_amd_tensor_pixels_batch(ctx.handle, len(images), d_in.ptr, d_in.stride, w, h, C.byref(_c_source(src)),
                                                 out.ptr, out.stride)
    assert st == OK, st
    return out.images()


# ---- 1. the front alone -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extent", EXTENTS, ids=["%dx%d" % e for e in EXTENTS])
@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_front_matches_the_contract(ctx, torch, combo, extent):
    w, h = extent
    assert extent != (13, 5) or (w % 4 == 1 and (3 * w) % 4 == 3 and (3 * w * h + 2) % 2 == 1)
    assert w != TILE_W + 6 or (w > TILE_W and h > 2 * TILE_H and w % 4 != 0)
    mean, std = S.IMAGENET
    unit, inverse = S.Source(*combo), S.inverse(*combo, mean, std)
    # (source, elements between the images beyond 3 w h, elements from an allocation boundary to the first image)
    for src, gap, lead in ((unit, 1, 0), (unit, 2, 0), (unit, 1, 1), (inverse, 1, 0)):
        images = _elements(1000 * w + h + gap, src, w, h)
        want = [S.pixels(im, src) for im in images]
        if src.dtype != S.U8 and w * h >= 64:                # both clamps bind
            assert min(u.min() for u in want) == 0 and max(u.max() for u in want) == 255
        for i, (g, u) in enumerate(zip(_front(ctx, torch, images, w, h, src, gap=gap, lead=lead), want)):
            _same(g, u, (combo, extent, gap, lead, i))


@pytest.mark.parametrize("combo", [c for c in COMBOS if c[0] != S.U8], ids=[i for i in COMBO_IDS if not i.startswith("u8")])
def test_front_special_values_and_subnormals(ctx, torch, combo):
    """The table of the contract under scale 1 and offset 0, and subnormal elements under a scale that makes bytes of them."""
    dtype, layout = combo
    w, h = 8, 3
    values = np.zeros((h, w, 3), F)
    for k, (v, _) in enumerate(S.SPECIALS):
        values[0, k, :] = v
    bits = S.to_bits(values, dtype)
    if layout == S.CHW:
        bits = np.ascontiguousarray(bits.transpose(2, 0, 1))
    src = S.Source(dtype, layout)
    got = _front(ctx, torch, [bits], w, h, src)[0]
    _same(got, S.pixels(bits, src), combo)
    if dtype == S.F32:
        assert got[0, :, 0].tolist() == [b for _, b in S.SPECIALS]
    # the largest subnormals of the dtype and the 15 below each; the scale brings them to about 200, or as far as a finite
    # binary32 scale can (3e38: bytes 3 and 4) -- flushed, every byte would be 0
    top = {S.F32: 0x007fffff, S.F16: 0x03ff, S.BF16: 0x007f}[dtype]
    sub = np.empty((h, w, 3), S.BITS[dtype])
    sub.reshape(-1)[:] = [top - k % 16 for k in range(3 * w * h)]
    sub[1] |= {S.F32: 0x80000000}.get(dtype, 0x8000)         # a row of negative ones
    if layout == S.CHW:
        sub = np.ascontiguousarray(sub.transpose(2, 0, 1))
    largest = float(S.values(np.asarray([top], S.BITS[dtype]), dtype)[0])
    src = S.Source(dtype, layout, (min(200.0 / largest, 3e38),) * 3)
    want = S.pixels(sub, src)
    assert want[0].min() >= 3 and want[2].min() >= 3 and want[1].max() == 0
    _same(_front(ctx, torch, [sub], w, h, src)[0], want, (combo, "subnormal"))


# ---- 2. extreme extents ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extent", [(65535, 3), (3, 65535)], ids=["65535x3", "3x65535"])
def test_front_extreme_extents(ctx, torch, extent):
    w, h = extent
    gen = torch.Generator(device=ctx.torch_device).manual_seed(w)
    t = torch.randint(0, 256, (2, 3, h, w), dtype=torch.uint8, device=ctx.torch_device, generator=gen)
    out = S.PixelsOut(ctx, torch, 2, w, h, gap=1)
    src = _lib.TensorSource(S.U8, S.CHW, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
    assert _lib.lib().jpeg_amd_tensor_pixels_batch(ctx.handle, 2, t.data_ptr(), 3 * w * h, w, h, C.byref(src), out.ptr, out.stride) == OK
    want = t.permute(0, 2, 3, 1).contiguous()
    for i in range(2):
        assert torch.equal(out.device(i).view(h, w, 3), want[i])
    out.images()                                              # the sentinel check


# ---- 3. encode ----------------------------------------------------------------------------------------------------------------------

def _tables(ctx, torch, L, n, seed):
    ntables = 2 if L.nplanes == 3 else 1
    gen = torch.Generator(device=ctx.torch_device).manual_seed(seed)
    return torch.randint(1, 24, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen), ntables


def _encode_bytes(ctx, torch, L, n, d_px, px_stride, color, dq, ntables):
    """jpeg_amd_encode_batch -> [plane][image] int16 [uy, ux, 64]."""
    out = S.CoefOut(ctx, torch, L, n)
    st = _lib.lib().jpeg_amd_encode_batch(ctx.handle, C.byref(L), n, d_px, px_stride, color, dq.data_ptr(), ntables * 64, ntables,
                                          _lib.ptr_array(out.ptrs()), _lib.size_array(out.strides()))
    assert st == OK, st
    return out.planes()


def _encode_tensor(ctx, torch, L, n, d_src, src_stride, src, color, dq, ntables):
    """jpeg_amd_encode_tensor_batch -> [plane][image] int16 [uy, ux, 64]."""
    out = S.CoefOut(ctx, torch, L, n)
    st = _lib.lib().jpeg_amd_encode_tensor_batch(ctx.handle, C.byref(L), n, d_src, src_stride, C.byref(_c_source(src)), color,
                                                 dq.data_ptr(), ntables * 64, ntables, _lib.ptr_array(out.ptrs()),
                                                 _lib.size_array(out.strides()))
    assert st == OK, st
    return out.planes()


def _same_planes(got, want, what):
    assert len(got) == len(want)
    for p, (gp, wp) in enumerate(zip(got, want)):
        for i, (g, w) in enumerate(zip(gp, wp)):
            _same(g, w, (what, "plane", p, "image", i))


@functools.lru_cache(maxsize=None)
def _encode_inputs(w, h, dtype, layout):
    mean, std = S.IMAGENET
    src = S.inverse(dtype, layout, mean, std)
    images = _elements(7 * w + h, src, w, h)
    return src, images, np.stack([S.pixels(im, src) for im in images])


@pytest.mark.parametrize("size", ENCODE_SIZES, ids=["%dx%d" % s for s in ENCODE_SIZES])
@pytest.mark.parametrize("name", sorted(ENCODE_FACTORS))
def test_encode_is_the_byte_call_on_the_contracts_bytes(ctx, torch, name, size):
    w, h = size
    L = c_layout(w, h, ENCODE_FACTORS[name])
    dq, ntables = _tables(ctx, torch, L, N, 11)
    for dtype, layout in ((S.F16, S.CHW), (S.F32, S.HWC)):
        src, images, u = _encode_inputs(w, h, dtype, layout)
        d_in = S.SourceIn(ctx, torch, images, dtype, gap=1)
        d_u = torch.from_numpy(u).to(ctx.torch_device)
        for color in (_lib.COLOR_RGB8, _lib.COLOR_YCC8):
            want = _encode_bytes(ctx, torch, L, N, d_u.data_ptr(), 3 * w * h, color, dq, ntables)
            got = _encode_tensor(ctx, torch, L, N, d_in.ptr, d_in.stride, src, color, dq, ntables)
            _same_planes(got, want, (name, size, S.DTYPE_NAMES[dtype], color))


def test_encode_matches_the_oracle(ctx, torch):
    """pack -> decomposed -> fdct of the CPU restatement of the reference on the contract's bytes."""
    from oracle import oracle as O
    w, h = 17, 9
    factors = ENCODE_FACTORS["420"]
    L = c_layout(w, h, factors)
    src, images, u = _encode_inputs(w, h, S.F16, S.CHW)
    quanta = [np.asarray(J.compression_quanta("luminance", 1.0), np.uint16), np.asarray(J.compression_quanta("chrominance", 1.0), np.uint16)]
    dq = torch.from_numpy(np.tile(np.stack(quanta).astype(np.int16)[None], (N, 1, 1))).to(ctx.torch_device)
    d_in = S.SourceIn(ctx, torch, images, S.F16, gap=1)
    got = _encode_tensor(ctx, torch, L, N, d_in.ptr, d_in.stride, src, _lib.COLOR_RGB8, dq, 2)
    for i in range(N):
        ref = O.encode(u[i].reshape(-1, 3), (w, h), factors, [quanta[0], quanta[1], quanta[1]])
        for p, r in enumerate(ref):
            _same(got[p][i], np.asarray(r, np.int16).reshape(got[p][i].shape), ("oracle", i, p))


def test_encode_tensor_single_image_with_host_tables(ctx, torch):
    w, h = 17, 9
    L = c_layout(w, h, ENCODE_FACTORS["422"])
    src, images, u = _encode_inputs(w, h, S.F32, S.HWC)
    tables = np.stack([J.compression_quanta("luminance", 0.5), J.compression_quanta("chrominance", 0.5)]).astype(np.uint16)
    dq = torch.from_numpy(tables.astype(np.int16)[None]).to(ctx.torch_device)
    d_u = torch.from_numpy(u[:1]).to(ctx.torch_device)
    want = _encode_bytes(ctx, torch, L, 1, d_u.data_ptr(), 0, _lib.COLOR_RGB8, dq, 2)
    d_in = S.SourceIn(ctx, torch, images[:1], S.F32)
    out = S.CoefOut(ctx, torch, L, 1)
    assert _lib.lib().jpeg_amd_encode_tensor(ctx.handle, C.byref(L), d_in.ptr, C.byref(_c_source(src)), _lib.COLOR_RGB8, tables.ctypes.data,
                                            2, _lib.ptr_array(out.ptrs())) == OK
    _same_planes(out.planes(), want, "single")


# ---- 4. bytes in the encoder's own order ------------------------------------------------------------------------------------------------

def test_u8_hwc_is_the_byte_call_on_the_same_pointer(ctx, torch):
    """(Whether the context's byte buffer grew cannot be seen from here: the Python context does not expose it.)"""
    w, h = 264, 72
    L = c_layout(w, h, ENCODE_FACTORS["420"])
    dq, ntables = _tables(ctx, torch, L, N, 5)
    src = S.Source(S.U8, S.HWC, (float("nan"),) * 3, (float("nan"),) * 3)    # not read
    images = _elements(9, src, w, h)
    d_in = S.SourceIn(ctx, torch, images, S.U8, gap=4)
    want = _encode_bytes(ctx, torch, L, N, d_in.ptr, d_in.stride, _lib.COLOR_RGB8, dq, ntables)
    got = _encode_tensor(ctx, torch, L, N, d_in.ptr, d_in.stride, src, _lib.COLOR_RGB8, dq, ntables)
    _same_planes(got, want, "u8 hwc")


# ---- 5. two chunks ----------------------------------------------------------------------------------------------------------------------

def test_encode_over_two_chunks(ctx, torch):
    """6 images of 8192 x 8192: 5 fill the 1 GiB of a chunk, the sixth is a chunk of its own.  Compared on the device."""
    w = h = 8192
    n = 6
    assert (1 << 30) // (3 * w * h) == 5
    L = c_layout(w, h, ENCODE_FACTORS["y8"])
    dq, ntables = _tables(ctx, torch, L, n, 3)
    gen = torch.Generator(device=ctx.torch_device).manual_seed(8192)
    t = torch.randint(0, 256, (n, 3, h, w), dtype=torch.uint8, device=ctx.torch_device, generator=gen)
    units = 64 * L.units_x[0] * L.units_y[0]
    src = _lib.TensorSource(S.U8, S.CHW, (C.c_float * 3)(1, 1, 1), (C.c_float * 3)(0, 0, 0))
    got = torch.full((n, units), 0x5A5A, dtype=torch.int16, device=ctx.torch_device)
    assert _lib.lib().jpeg_amd_encode_tensor_batch(ctx.handle, C.byref(L), n, t.data_ptr(), 3 * w * h, C.byref(src), _lib.COLOR_RGB8,
                                                   dq.data_ptr(), ntables * 64, ntables, _lib.ptr_array([got.data_ptr()]),
                                                   _lib.size_array([units])) == OK
    u = t.permute(0, 2, 3, 1).contiguous()
    del t
    want = torch.full((n, units), 0x2B2B, dtype=torch.int16, device=ctx.torch_device)
    assert _lib.lib().jpeg_amd_encode_batch(ctx.handle, C.byref(L), n, u.data_ptr(), 3 * w * h, _lib.COLOR_RGB8, dq.data_ptr(), ntables * 64,
                                            ntables, _lib.ptr_array([want.data_ptr()]), _lib.size_array([units])) == OK
    for i in range(n):
        assert torch.equal(got[i], want[i]), i
    assert not torch.equal(got[4], got[5])


# ---- 6. files ---------------------------------------------------------------------------------------------------------------------------

def _progressive_scans():
    Y, Cb, Cr = 0, 1, 2
    Scan = J.Scan
    return [Scan.progressive_dc((Y, 0), (Cb, 1), (Cr, 1), bits=1), Scan.progressive_dc_refine(Y, Cb, Cr, bit=0),
            Scan.progressive_ac((Y, 0), (1, 64), bits=1), Scan.progressive_ac((Cb, 0), (1, 64), bits=1),
            Scan.progressive_ac((Cr, 0), (1, 64), bits=1), Scan.progressive_ac_refine((Y, 0), (1, 64), bit=0),
            Scan.progressive_ac_refine((Cb, 0), (1, 64), bit=0), Scan.progressive_ac_refine((Cr, 0), (1, 64), bit=0)]


@pytest.mark.parametrize("process", ["baseline", "progressive"])
@pytest.mark.parametrize("size", [(17, 9), (264, 72)], ids=["17x9", "264x72"])
def test_files_are_those_of_the_byte_call(ctx, torch, size, process):
    w, h = size
    n = 5
    mean, std = S.IMAGENET
    src = S.inverse(S.F16, S.CHW, mean, std)
    images = _elements(31 * w + h, src, w, h, n=n)
    u = np.stack([S.pixels(im, src) for im in images])
    scans = _progressive_scans() if process == "progressive" else [[(0, 0, 0)], [(1, 1, 1), (2, 1, 1)]]
    metadata = [("jfif", (2, 2, 1, 1))]
    quanta = {0: J.compression_quanta("luminance", 1.0), 1: J.compression_quanta("chrominance", 1.0)}
    # the byte call
    info = _lib.FrameInfo()
    info.width, info.height, info.precision, info.ncomponents = w, h, 8, 3
    info.process = 2 if process == "progressive" else 0
    for c, (fx, fy) in enumerate(FUSED["420"]):
        info.id[c], info.factor_x[c], info.factor_y[c] = c + 1, fx, fy
    tables = np.stack([quanta[0], quanta[1]]).astype(np.uint16)
    qkey, tk = (C.c_int32 * 3)(0, 1, 1), (C.c_int32 * 2)(0, 1)
    sarr = _scan_array(scans)
    marr, nmeta, _keep = _metadata_array(metadata)
    cap = 1 << 18
    out = np.zeros((n, cap), np.uint8)
    sizes = (C.c_size_t * n)()
    d_u = torch.from_numpy(u).to(ctx.torch_device)
    st = _lib.lib().jpeg_amd_compress_batch_device(ctx.handle, C.byref(info), d_u.data_ptr(), 0, n, J.RGB.code, qkey, tables.ctypes.data, tk, 2,
                                                   sarr, len(scans), marr, nmeta, 3, out.ctypes.data, cap, sizes)
    assert st == OK, st
    want = [out[i, :sizes[i]].tobytes() for i in range(n)]
    # the tensor call, through the Python layer, on a batch with a gap between the images
    dtype = torch.float16
    room = torch.zeros((n, 3 * h * w + 2), dtype=dtype, device=ctx.torch_device)
    for i, im in enumerate(images):
        room[i, :3 * h * w] = torch.from_numpy(im.view(np.float16).reshape(-1)).to(ctx.torch_device)
    tensors = room[:, :3 * h * w].unflatten(1, (3, h, w))
    assert tensors.stride(0) == 3 * h * w + 2 and tensors[0].is_contiguous()
    layout = J.Layout("ycc8", {1: ((2, 2), 0), 2: ((1, 1), 1), 3: ((1, 1), 1)})
    got = J.compress_tensors(ctx, tensors, layout, quanta, J.tensor_source(mean, std, dtype, "chw"), scans, process=process,
                             metadata=metadata, threads=3)
    assert got == want
    assert len(set(want)) == n and J.inspect(want[0]).process == info.process


# ---- 7. round trip on the device ----------------------------------------------------------------------------------------------------------

def test_decode_tensors_then_encode_tensors_is_the_byte_route(ctx, torch):
    mean, std = S.IMAGENET
    L = c_layout(SIZE[0], SIZE[1], FUSED["420"])
    n = len(VIEWS)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 23)
    out_size = (40, 24)
    py = resize_py_layout("420")
    u = J.decode_resized(ctx, SIZE, py, planes, dq, VIEWS, out_size)
    t = J.decode_tensors(ctx, SIZE, py, planes, dq, VIEWS, out_size, J.tensor_spec(mean, std, torch.float16, "chw"))
    assert t.shape == (n, 3, 24, 40) and u.shape == (n, 24, 40, 3)
    quanta = {0: J.compression_quanta("luminance", 1.0), 1: J.compression_quanta("chrominance", 1.0)}
    got = J.encode_tensors(ctx, t, py, quanta, J.tensor_source(mean, std, torch.float16, "chw"))
    assert len(got) == n
    assert (J.tensor_pixels(ctx, t, J.tensor_source(mean, std, torch.float16, "chw")) == u).all().item()
    for i in range(n):
        want = J.Rectangular.encode(ctx, out_size, py, u[i].reshape(-1, 3), quanta).host_planes()
        for p, (a, b) in enumerate(zip(got[i].host_planes(), want)):
            _same(a, b, (i, p))


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing_and_leave_the_context_usable(ctx, torch):
    w, h = 13, 5
    lib = _lib.lib()
    L = c_layout(w, h, ENCODE_FACTORS["420"])
    dq, ntables = _tables(ctx, torch, L, N, 2)
    good = S.Source(S.F16, S.CHW)
    images = _elements(77, good, w, h)
    want = [S.pixels(im, good) for im in images]
    d_in = S.SourceIn(ctx, torch, images, S.F16, gap=1)
    d_u = torch.from_numpy(np.stack(want)).to(ctx.torch_device)
    want_coef = _encode_bytes(ctx, torch, L, N, d_u.data_ptr(), 3 * w * h, _lib.COLOR_RGB8, dq, ntables)
    nan = S.Source(S.F16, S.CHW, (1.0, float("nan"), 1.0))
    seven = S.Source(S.F16, S.CHW)
    seven.dtype = 7
    # (what, source pointer, source stride, source)
    bad = [("misaligned", d_in.ptr + 1, d_in.stride, good), ("short stride", d_in.ptr, 3 * w * h - 1, good),
           ("nan scale", d_in.ptr, d_in.stride, nan), ("dtype 7", d_in.ptr, d_in.stride, seven)]
    for what, ptr, stride, src in bad:
        out = S.PixelsOut(ctx, torch, N, w, h, gap=3)
        assert lib.jpeg_amd_tensor_pixels_batch(ctx.handle, N, ptr, stride, w, h, C.byref(_c_source(src)), out.ptr, out.stride) == EINVAL, what
        ctx.synchronize()
        assert out.untouched(), what
        coef = S.CoefOut(ctx, torch, L, N)
        assert lib.jpeg_amd_encode_tensor_batch(ctx.handle, C.byref(L), N, ptr, stride, C.byref(_c_source(src)), _lib.COLOR_RGB8, dq.data_ptr(),
                                                ntables * 64, ntables, _lib.ptr_array(coef.ptrs()), _lib.size_array(coef.strides())) == EINVAL, what
        ctx.synchronize()
        assert coef.untouched(), what
        # the next valid calls on the same context
        for g, u in zip(_front(ctx, torch, images, w, h, good, gap=1), want):
            _same(g, u, ("after", what))
        _same_planes(_encode_tensor(ctx, torch, L, N, d_in.ptr, d_in.stride, good, _lib.COLOR_RGB8, dq, ntables), want_coef, ("after", what))
    # a short destination stride, and what jpeg_amd_encode_batch refuses comes first, with its status
    out = S.PixelsOut(ctx, torch, N, w, h)
    assert lib.jpeg_amd_tensor_pixels_batch(ctx.handle, N, d_in.ptr, d_in.stride, w, h, C.byref(_c_source(good)), out.ptr, 3 * w * h - 1) == EINVAL
    assert out.untouched()
    L12 = c_layout(w, h, ENCODE_FACTORS["420"], precision=12)
    coef = S.CoefOut(ctx, torch, L, N)
    assert lib.jpeg_amd_encode_tensor_batch(ctx.handle, C.byref(L12), N, d_in.ptr, d_in.stride, C.byref(_c_source(seven)), _lib.COLOR_RGB8,
                                            dq.data_ptr(), ntables * 64, ntables, _lib.ptr_array(coef.ptrs()),
                                            _lib.size_array(coef.strides())) == _lib.ENOSUP
    assert coef.untouched()
    # empty calls
    assert lib.jpeg_amd_tensor_pixels_batch(ctx.handle, 0, None, 0, w, h, C.byref(_c_source(good)), None, 0) == OK
    assert lib.jpeg_amd_encode_tensor_batch(ctx.handle, C.byref(L), 0, None, 0, C.byref(_c_source(good)), _lib.COLOR_RGB8, None, 0, ntables,
                                            None, None) == OK


def test_python_layer_refuses_a_wrong_dtype_or_shape_before_the_call(ctx, torch):
    src = J.tensor_source(dtype=torch.float16, layout="chw")
    dev = ctx.torch_device
    with pytest.raises(ValueError):
        J.tensor_pixels(ctx, torch.zeros((2, 3, 4, 5), dtype=torch.float32, device=dev), src)
    with pytest.raises(ValueError):
        J.tensor_pixels(ctx, torch.zeros((2, 4, 5, 3), dtype=torch.float16, device=dev), src)
    with pytest.raises(ValueError):
        J.tensor_pixels(ctx, torch.zeros((3, 4, 5), dtype=torch.float16, device=dev), src)
    with pytest.raises(ValueError):
        J.tensor_pixels(ctx, torch.zeros((2, 3, 4, 10), dtype=torch.float16, device=dev)[..., ::2], src)
    with pytest.raises(ValueError):
        J.tensor_pixels(ctx, torch.zeros((2, 3, 4, 5), dtype=torch.float16), src)
    t = torch.full((2, 3, 4, 5), 7.25, dtype=torch.float16, device=dev)
    assert (J.tensor_pixels(ctx, t, src) == 7).all().item() and J.tensor_pixels(ctx, t[:0], src).shape == (0, 4, 5, 3)
