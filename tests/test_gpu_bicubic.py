"""The bicubic resample on the MI355X (JPEG_AMD_FILTER_BICUBIC through every call that takes `filter`; k_tables_bytes and
k_tables_tensor with the BicubicFilter): every output is compared byte for byte, or element for element as a bit pattern,
with _bicubic_ref -- the contract of include/jpeg_amd.h ("bicubic resample") restated in numpy -- applied to the source
bytes or to what the existing view decode returns for the same views; tensors go through _tensor_ref's output stage,
orientations through _orient.  The bilinear and the antialiasing filter must give what they gave.  Every raw call writes
into a buffer filled with a sentinel, whose bytes between and behind the images are checked after it."""
import ctypes as C
import functools

import numpy as np
import pytest

import _antialias_ref as A
import _bicubic_ref as B
import _files as F
import _orient as E
import _tensor_ref as T
import jpeg_amd as J
from _calls import (FUSED, RESIZE_SIZE, RESIZE_TILE_H as TILE_H, RESIZE_TILE_W as TILE_W, Out, c_layout, c_views, pixel_image,
                    plane_ptrs, resize_py_layout, strides, synthetic)
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_spec as _c_spec, pack as _pack, same as _same, tensor_bits as _bits, torch_orient
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

BICUBIC, AA, BILINEAR = _lib.FILTER_BICUBIC, _lib.FILTER_ANTIALIAS, _lib.FILTER_BILINEAR
CHUNK = 32                                                  # source rows per chunk of the kernel's walk (antialias.hpp)
# (out_w, out_h, bytes between the output images beyond 3 out_w out_h).  (40, 35): the target of the 5 x 7 source; (64, 32):
# one exact tile, 512 x 256 at k = 8; (70, 37): partial tiles on both axes, and two tile rows
TARGETS = [(1, 1, 0), (40, 35, 3), (TILE_W, TILE_H, 0), (TILE_W + 6, TILE_H + 5, 1)]
ELEM = {T.F32: 4, T.F16: 2, T.BF16: 2}
COMBOS = [(d, l) for d in T.DTYPES for l in T.LAYOUTS]
COMBO_IDS = ["%s-%s" % ({T.F32: "f32", T.F16: "f16", T.BF16: "bf16"}[d], {T.HWC: "hwc", T.CHW: "chw"}[l]) for d, l in COMBOS]


def _extents(out_w, out_h):
    """The six sources of one call for a target: upscaled (k < 1 where the target is larger than a pixel), the identity, a
    factor inside (1, 2), 2 exactly, 8 -- the tap limit -- and a single pixel."""
    return [(max(out_w // 8, 1), max(out_h // 5, 1)), (out_w, out_h), (out_w * 3 // 2 + 1, out_h * 5 // 3 + 1),
            (2 * out_w, 2 * out_h), (8 * out_w, 8 * out_h), (1, 1)]


def _edges(w, h, seed):
    """Hard edges: every sample 0 or 255, in runs, so that the lobes overshoot at both ends."""
    rng = np.random.default_rng(seed)
    coarse = rng.integers(0, 2, ((h + 2) // 3, (w + 1) // 2, 3), dtype=np.uint8) * 255
    return np.ascontiguousarray(np.repeat(np.repeat(coarse, 3, axis=0), 2, axis=1)[:h, :w])


@functools.lru_cache(maxsize=None)
def _sources(out_w, out_h):
    ext = _extents(out_w, out_h)
    return tuple(_edges(w, h, 100 * w + h) if i in (0, 3) else pixel_image("random", w, h, 100 * w + h) for i, (w, h) in enumerate(ext))


@functools.lru_cache(maxsize=None)
def _resampled(out_w, out_h):
    """The byte images of the contract for the sources of a target: computed once, shared, never written to."""
    out = tuple(B.resize(image, out_w, out_h) for image in _sources(out_w, out_h))
    for o in out:
        o.setflags(write=False)
    return out


def _filter_call(ctx, torch, images, out_w, out_h, filter=BICUBIC, gap=0, expect=0):
    """jpeg_amd_resize_filter_batch on host images [h, w, 3] -> the outputs as host arrays; the sentinel in every byte of the
    output buffer that belongs to no image is asserted here."""
    d_src, src_stride, ext = _pack(ctx, torch, images)
    out = Out(ctx, torch, [3 * out_w * out_h] * len(images), gap=gap, lead=4, tail=7)
    assert _lib.lib().jpeg_amd_resize_filter_batch(ctx.handle, len(images), d_src.data_ptr(), src_stride, ext, out_w, out_h, filter,
                                                   out.ptr, out.stride) == expect
    ctx.synchronize()
    if expect != 0:
        assert out.untouched()
        return None
    return [g.reshape(out_h, out_w, 3) for g in out.images()]


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------

def test_the_sources_of_a_call_hold_every_kind_of_factor():
    for out_w, out_h, _ in TARGETS[1:]:
        ext = _extents(out_w, out_h)
        for axis, n_out in ((0, out_w), (1, out_h)):
            k = [np.float32(e[axis]) / np.float32(n_out) for e in ext]
            assert k[0] < 1 and k[1] == 1 and 1 < k[2] < 2 and k[3] == 2 and k[4] == 8 and ext[5] == (1, 1)
    assert _extents(40, 35)[0] == (5, 7) and _extents(TILE_W, TILE_H)[4] == (512, 256)
    assert B.axis_table(TILE_W, 512)[1].max() == 32                      # 32 taps across
    lo, count, _ = B.axis_table(TILE_H + 5, 8 * (TILE_H + 5))            # the first tile's rows at k = 8: more than eight chunks
    assert lo[TILE_H - 1] + count[TILE_H - 1] - lo[0] > 8 * CHUNK
    # both clamps bind: the 5 x 7 source of hard edges overshoots below 0 and above 255 before the conversion
    image = _sources(40, 35)[0]
    v = B._pass(B._pass(image.astype(B.F), *B.axis_table(40, 5), 1), *B.axis_table(35, 7), 0)
    assert v.min() < -1 and v.max() > 256 and set(np.unique(image)) == {0, 255}


@pytest.mark.parametrize("target", TARGETS, ids=["%dx%d+%d" % t for t in TARGETS])
def test_kernel_matches_the_contract(ctx, torch, target):
    out_w, out_h, gap = target
    got = _filter_call(ctx, torch, list(_sources(out_w, out_h)), out_w, out_h, gap=gap)
    for ext, g, want in zip(_extents(out_w, out_h), got, _resampled(out_w, out_h)):
        _same(g, want, (ext, target))
    _same(got[1], _sources(out_w, out_h)[1], "the identity size returns the source bytes")


# ---- 2. the tensor form ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_tensor_form_matches_the_contract(ctx, torch, combo):
    out_w, out_h, gap = TILE_W + 6, TILE_H + 5, 3             # a flip across the partial last tile column
    spec = T.Spec(*combo)
    images = list(_sources(out_w, out_h))
    flips = [i & 1 for i in range(len(images))]
    d_src, src_stride, ext = _pack(ctx, torch, images)
    out = Out(ctx, torch, [3 * out_w * out_h] * len(images), elem=ELEM[spec.dtype], gap=gap, tail=7)
    assert _lib.lib().jpeg_amd_resize_filter_tensor_batch(ctx.handle, len(images), d_src.data_ptr(), src_stride, ext, out_w, out_h, BICUBIC,
                                                          C.byref(_c_spec(spec)), (C.c_uint8 * len(flips))(*flips), out.ptr,
                                                          out.stride) == 0
    shape = (3, out_h, out_w) if spec.layout == T.CHW else (out_h, out_w, 3)
    for i, (b, u) in enumerate(zip(out.images(), _resampled(out_w, out_h))):
        _same(b.copy().view(T.BITS[spec.dtype]).reshape(shape), T.normalise(u, spec, flips[i]), (combo, i))


# ---- 3. orientations --------------------------------------------------------------------------------------------------------------

def test_all_eight_orientations(ctx, torch):
    out_w, out_h = 24, 40
    cases = [(size, o) for size in ((130, 70), (70, 130)) for o in range(1, 9)] + [((40, 192), 6), ((192, 40), 1)]   # k = 8 along x
    images = [pixel_image("random", w, h, 3 * w + h + o) for (w, h), o in cases]
    orient = [o for _, o in cases]
    dev = [torch.from_numpy(im).to(ctx.torch_device) for im in images]
    got = J.resize(ctx, dev, (out_w, out_h), filter="bicubic", orientations=orient).cpu().numpy()
    witness = J.resize(ctx, [torch_orient(torch, t, o) for t, o in zip(dev, orient)], (out_w, out_h), filter="bicubic").cpu().numpy()
    for i, (im, (size, o)) in enumerate(zip(images, cases)):
        _same(got[i], B.resize(E.orient(im, o), out_w, out_h), (size, o))
        _same(got[i], witness[i], (size, o, "the unoriented call on an oriented copy"))
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.bfloat16, layout="hwc")
    want_spec = T.Spec(T.BF16, T.HWC, mean=[spec.mean[c] for c in range(3)], scale=[spec.scale[c] for c in range(3)])
    flips = [i % 3 == 1 for i in range(len(cases))]
    tensor = J.resize_tensor(ctx, dev, (out_w, out_h), spec, flips=flips, filter="bicubic", orientations=orient)
    for i, (im, (size, o)) in enumerate(zip(images, cases)):
        _same(_bits(tensor[i], torch), T.normalise(B.resize(E.orient(im, o), out_w, out_h), want_spec, flips[i]), (size, o, "tensor"))


# ---- 4. decode + resample ---------------------------------------------------------------------------------------------------------

VIEWS = [(1, 10, 20, 100, 200), (2, 3, 5, 60, 100), (8, 0, 0, 17, 33)]      # denominators 1, 2 and 8 of a 131 x 257 image


def test_decode_resized_and_decode_tensors_are_the_view_decode_resampled(ctx, torch):
    L = c_layout(RESIZE_SIZE[0], RESIZE_SIZE[1], FUSED["420"])
    layout = resize_py_layout("420")
    n = len(VIEWS)
    planes, dq, ntables = synthetic(ctx, torch, L, n, 17)
    decoded = [v.cpu().numpy() for v in J.decode_views(ctx, RESIZE_SIZE, layout, planes, dq, VIEWS)]
    out_w, out_h = 13, 25                                     # k = 100 / 13 = 7.7 and 8 exactly in the first view
    out = Out(ctx, torch, [3 * out_w * out_h] * n, gap=3, tail=5)
    assert _lib.lib().jpeg_amd_decode_resized_filter_batch(
        ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0,
        _lib.COLOR_RGB8, c_views(VIEWS), out_w, out_h, BICUBIC, out.ptr, out.stride) == 0
    want = [B.resize(d, out_w, out_h) for d in decoded]
    for i, g in enumerate(out.images()):
        _same(g.reshape(out_h, out_w, 3), want[i], ("decode_resized", i))
    api = J.decode_resized(ctx, RESIZE_SIZE, layout, planes, dq, VIEWS, (out_w, out_h), filter="bicubic").cpu().numpy()
    for i in range(n):
        _same(api[i], want[i], ("the keyword", i))
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    want_spec = T.Spec(T.F16, T.CHW, mean=[spec.mean[c] for c in range(3)], scale=[spec.scale[c] for c in range(3)])
    flips = [1, 0, 1]
    tensor = J.decode_tensors(ctx, RESIZE_SIZE, layout, planes, dq, VIEWS, (out_w, out_h), spec, flips=flips, filter="bicubic")
    for i in range(n):
        _same(_bits(tensor[i], torch), T.normalise(want[i], want_spec, flips[i]), ("decode_tensors", i))


@pytest.fixture(scope="module")
def spectrals(ctx):
    """4:2:0 at 53 x 37, 4:4:4 at 40 x 24, grey at 17 x 33."""
    made = [F.synthetic_file("420", (53, 37), 41), F.synthetic_file("444", (40, 24), 42), F.synthetic_file("y8", (17, 33), 43)]
    return [J.Spectral.decompress(ctx, d) for d, _ in made]


def test_the_mixed_forms_and_the_view_of_one_image(ctx, torch, spectrals):
    views = [(1, 0, 0, 53, 37), (2, 1, 1, 17, 9), (1, 0, 0, 17, 33)]      # a 4:2:0, a 4:4:4 and a grey image in one call
    out_w, out_h = 7, 5                                       # k = 7.57 and 7.4 in the first image
    decoded = [v.cpu().numpy() for v in J.decode_views_mixed(ctx, spectrals, views)]
    want = [B.resize(d, out_w, out_h) for d in decoded]
    got = J.decode_resized_mixed(ctx, spectrals, views, (out_w, out_h), filter="bicubic").cpu().numpy()
    for i in range(3):
        _same(got[i], want[i], ("decode_resized_mixed", i))
    spec = J.tensor_spec((0.5, 0.5, 0.5), (0.25, 0.25, 0.25), dtype=torch.float32, layout="hwc")
    want_spec = T.Spec(T.F32, T.HWC, mean=[spec.mean[c] for c in range(3)], scale=[spec.scale[c] for c in range(3)])
    flips = [0, 1, 1]
    tensor = J.decode_tensors_mixed(ctx, spectrals, views, (out_w, out_h), spec, flips=flips, filter="bicubic")
    for i in range(3):
        _same(_bits(tensor[i], torch), T.normalise(want[i], want_spec, flips[i]), ("decode_tensors_mixed", i))
    for sp, v, d in zip(spectrals, views, decoded):
        one = sp.view(v[1:], v[0], J.RGB, size=(11, 6), filter="bicubic").cpu().numpy()
        _same(one, B.resize(d, 11, 6), ("Spectral.view", v))


# ---- 5. files -----------------------------------------------------------------------------------------------------------------------

def test_the_file_calls_are_the_mixed_call_on_the_decoded_files(ctx, torch):
    datas = [F.synthetic_file("420", (160, 120), 61)[0], F.synthetic_file("y8", (163, 117), 62, kind="progressive")[0],
             E.insert(F.synthetic_file("444", (150, 123), 63)[0], E.exif_segment(6, big=True))]
    named = [1, 1, 6]
    assert [J.exif_orientation(d) for d in datas] == named
    rects = [(3, 5, 150, 110), (0, 0, 163, 117), (2, 1, 120, 140)]   # of the ORIENTED images: the third file is 123 x 150 there
    out_size = (24, 16)
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    want_spec = T.Spec(T.F16, T.CHW, mean=[spec.mean[c] for c in range(3)], scale=[spec.scale[c] for c in range(3)])
    flips = [1, 0, 1]
    got, views, _, applied = J.decompress_tensors(ctx, datas, out_size, spec, source_regions=rects, flips=flips, filter="bicubic",
                                                  threads=2, orientation="exif")
    assert applied.tolist() == named
    sps = [J.Spectral.decompress(ctx, d) for d in datas]
    mixed, mixed_views = J.decode_crops_tensor_mixed(ctx, sps, rects, out_size, spec, flips=flips, filter="bicubic", orientations=named)
    assert views.tolist() == mixed_views.tolist() and {int(v[0]) for v in views} == {4}
    _same(_bits(got, torch), _bits(mixed, torch), "decompress_tensors against the mixed call")
    stored = [v.cpu().numpy() for v in J.decode_views_mixed(ctx, sps, [tuple(int(x) for x in v) for v in views])]
    want = [B.resize(E.orient(s, o), *out_size) for s, o in zip(stored, named)]
    for i in range(3):
        _same(_bits(got[i], torch), T.normalise(want[i], want_spec, flips[i]), ("decompress_tensors", i))
    resized = J.decompress_resized(ctx, datas, out_size, source_regions=rects, filter="bicubic", orientation="exif").cpu().numpy()
    for i in range(3):
        _same(resized[i], want[i], ("decompress_resized", i))
    # ... and without an orientation the third file is resampled as it is stored
    plain = J.decompress_resized(ctx, datas[2:], out_size, filter="bicubic").cpu().numpy()
    full = sps[2].view((0, 0, 38, 31), 4, J.RGB).cpu().numpy()            # 150 x 123 at denominator 4
    _same(plain[0], B.resize(full, *out_size), "as stored")


# ---- 6. the other filters are what they were; refusals ----------------------------------------------------------------------------

def test_bilinear_and_antialias_give_what_they_gave(ctx, torch):
    images = [pixel_image("random", w, h, 100 * w + h) for w, h in [(7, 9), (131, 57), (449, 301), (64, 33)]]
    dev = [torch.from_numpy(im).to(ctx.torch_device) for im in images]
    out_w, out_h = 64, 40                                     # 449 / 64 and 301 / 40: inside every filter's limit
    plain = J.resize(ctx, dev, (out_w, out_h)).cpu().numpy()
    _same(J.resize(ctx, dev, (out_w, out_h), filter="bilinear").cpu().numpy(), plain, "bilinear")
    lib = _lib.lib()
    d_src, src_stride, ext = _pack(ctx, torch, images)
    old = Out(ctx, torch, [3 * out_w * out_h] * 4, gap=2, tail=7)
    assert lib.jpeg_amd_resize_batch(ctx.handle, 4, d_src.data_ptr(), src_stride, ext, out_w, out_h, old.ptr, old.stride) == 0
    for g, w in zip(old.images(), plain):
        _same(g.reshape(out_h, out_w, 3), w, "the call without a filter")
    aa = J.resize(ctx, dev, (out_w, out_h), filter="antialias").cpu().numpy()
    bic = J.resize(ctx, dev, (out_w, out_h), filter="bicubic").cpu().numpy()
    for i, im in enumerate(images):
        _same(aa[i], A.resize(im, out_w, out_h), ("antialias", i))
        _same(bic[i], B.resize(im, out_w, out_h), ("bicubic", i))
    assert (aa != bic).any() and (plain != bic).any()
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    flips = [0, 1, 0, 1]
    _same(_bits(J.resize_tensor(ctx, dev, (out_w, out_h), spec, flips=flips, filter="bilinear"), torch),
          _bits(J.resize_tensor(ctx, dev, (out_w, out_h), spec, flips=flips), torch), "bilinear tensor")
    want_spec = T.Spec(T.F16, T.CHW, mean=[spec.mean[c] for c in range(3)], scale=[spec.scale[c] for c in range(3)])
    tensor = J.resize_tensor(ctx, dev, (out_w, out_h), spec, flips=flips, filter="antialias")
    for i, im in enumerate(images):
        _same(_bits(tensor[i], torch), T.normalise(A.resize(im, out_w, out_h), want_spec, flips[i]), ("antialias tensor", i))
    # the triangle's limit is where it was: 160 -> 10 passes it, and is over this filter's
    wide = [pixel_image("random", 160, 3, 5)]
    _same(_filter_call(ctx, torch, wide, 10, 3, filter=AA)[0], A.resize(wide[0], 10, 3), "k = 16")
    assert _filter_call(ctx, torch, wide, 10, 3, expect=_lib.ENOSUP) is None


def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    images = [pixel_image("random", 9, 7, 1), pixel_image("random", 80, 11, 2), pixel_image("random", 81, 11, 3)]
    assert _filter_call(ctx, torch, images, 10, 4, expect=_lib.ENOSUP) is None          # kx = 8.1 in the third image
    assert _filter_call(ctx, torch, images, 10, 4, filter=2, expect=_lib.EINVAL) is None
    assert _filter_call(ctx, torch, images, 0, 4, expect=_lib.EINVAL) is None
    got = _filter_call(ctx, torch, images[:2], 10, 4, gap=1)                             # kx = 8 exactly: inside the limit
    for image, g in zip(images, got):
        _same(g, B.resize(image, 10, 4), image.shape)
    got = _filter_call(ctx, torch, images, 11, 4, gap=1)
    for image, g in zip(images, got):
        _same(g, B.resize(image, 11, 4), image.shape)
    dev = [torch.from_numpy(im).to(ctx.torch_device) for im in images]
    with pytest.raises(ValueError):
        J.resize(ctx, dev, (11, 4), filter="lanczos")
    with pytest.raises(J.JpegAmdError):
        J.resize(ctx, dev, (10, 4), filter="bicubic")
