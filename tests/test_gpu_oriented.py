"""The oriented resample on the MI355X (the six *_oriented_* calls; the kernels over the Oriented* records): the contract
of include/jpeg_amd.h ("oriented resample") is by reference -- the filter's contract applied to the oriented image -- so every
output is compared byte for byte, or element for element as a bit pattern, with the existing numpy mirrors (_resize_ref,
_antialias_ref, _tensor_ref) applied to orient(source, o), and, as a second witness, with what the existing GPU call writes for
a contiguous oriented copy made with torch.  Sizes are non-square or degenerate throughout, so a swapped axis or a wrong sign
shows.  Every raw call writes into a sentinel-filled buffer whose bytes in front of, between and behind the images are checked."""
import ctypes as C

import numpy as np
import pytest

import _antialias_ref as A
import _files as F
import _orient as E
import _resize_ref as R
import _tensor_ref as T
import jpeg_amd as J
from _calls import Out, pixel_image
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, c_spec, host_bits as bits, pack, same, torch_orient
from jpeg_amd import _lib
from jpeg_amd.api import _mixed_args

pytestmark = pytest.mark.gpu

AA, BILINEAR = _lib.FILTER_ANTIALIAS, _lib.FILTER_BILINEAR
MIRROR = {BILINEAR: R.resize, AA: A.resize}
NAME = {BILINEAR: "bilinear", AA: "antialias"}
SIZES = [(37, 23), (23, 37), (64, 33), (130, 70), (70, 130), (1, 9), (9, 1), (1, 1)]      # (w, h) as stored


def resize_call(ctx, torch, images, orient, out_w, out_h, filter, spec=None, flips=None, expect=0, old=False):
    """jpeg_amd_resize_oriented_batch (spec: _tensor_batch), or with old=True the *_filter_* call, into a guarded buffer
    -> (status, the images' bytes)."""
    d_src, stride, ext = pack(ctx, torch, images)
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_w * out_h] * len(images), elem=elem, gap=5, lead=4, tail=7)
    head = (ctx.handle, len(images), d_src.data_ptr(), stride, ext, out_w, out_h, filter)
    L = _lib.lib()
    if spec is None:
        st = (L.jpeg_amd_resize_filter_batch(*head, out.ptr, out.stride) if old else
              L.jpeg_amd_resize_oriented_batch(*head, c_bytes(orient), out.ptr, out.stride))
    else:
        cs = c_spec(spec)
        st = (L.jpeg_amd_resize_filter_tensor_batch(*head, C.byref(cs), c_bytes(flips), out.ptr, out.stride) if old else
              L.jpeg_amd_resize_oriented_tensor_batch(*head, C.byref(cs), c_bytes(flips), c_bytes(orient), out.ptr, out.stride))
    assert st == expect
    ctx.synchronize()
    if st != 0:
        assert out.untouched()
        return st, None
    return st, out.images()


# ---- 1. bilinear bytes: eight orientations in one launch --------------------------------------------------------------------------

@pytest.mark.parametrize("target", [(70, 37), (5, 3)], ids=["70x37", "5x3"])
def test_bilinear_bytes_eight_orientations_in_one_launch(ctx, torch, target):
    out_w, out_h = target                                      # 70 x 37: two tile columns and two tile rows, both partial
    images = [pixel_image("random", w, h, 31 * w + h) for w, h in SIZES]
    for shift in (0, 1):                                       # ... and again with the orientations moved on by one image
        orient = [(i + shift) % 8 + 1 for i in range(8)]
        _, got = resize_call(ctx, torch, images, orient, out_w, out_h, BILINEAR)
        copies = [torch_orient(torch, torch.from_numpy(im).to(ctx.torch_device), o) for im, o in zip(images, orient)]
        witness = J.resize(ctx, copies, target).cpu().numpy()
        for i, (im, o) in enumerate(zip(images, orient)):
            assert E.orient(im, o).shape[:2] == E.oriented_size(o, *SIZES[i])[::-1]
            same(got[i], R.resize(E.orient(im, o), out_w, out_h), (SIZES[i], o, target))
            same(got[i], witness[i], (SIZES[i], o, target, "the existing call on an oriented copy"))


# ---- 2. the tensor forms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", [(T.F16, T.CHW), (T.F32, T.HWC), (T.BF16, T.CHW)], ids=["f16-chw", "f32-hwc", "bf16-chw"])
@pytest.mark.parametrize("filter", [BILINEAR, AA], ids=["bilinear", "antialias"])
def test_tensor_forms_flip_after_the_orientation(ctx, torch, combo, filter):
    out_w, out_h = 70, 37
    spec = T.Spec(*combo)
    cases = [(size, o, flip) for size in ((37, 23), (64, 33)) for o in (1, 3, 6, 7) for flip in (0, 1)]
    images = [pixel_image("random", w, h, 7 * w + h + o) for (w, h), o, _ in cases]
    orient, flips = [o for _, o, _ in cases], [f for _, _, f in cases]
    _, got = resize_call(ctx, torch, images, orient, out_w, out_h, filter, spec, flips)
    copies = [torch_orient(torch, torch.from_numpy(im).to(ctx.torch_device), o) for im, o in zip(images, orient)]
    witness = J.resize_tensor(ctx, copies, (out_w, out_h), c_spec(spec), flips=flips, filter=NAME[filter])
    witness = witness.contiguous().view(len(cases), -1).view(torch.uint8).cpu().numpy()
    for i, (im, (size, o, flip)) in enumerate(zip(images, cases)):
        want = T.normalise(MIRROR[filter](E.orient(im, o), out_w, out_h), spec, flip)
        same(bits(got[i], spec), want, (size, o, flip, combo))
        same(got[i], witness[i], (size, o, flip, combo, "the existing call on an oriented copy"))


# ---- 3. antialias ----------------------------------------------------------------------------------------------------------------

def test_antialias_bytes_all_orientations(ctx, torch):
    out_w, out_h = 24, 40
    cases = [(size, o) for size in ((130, 70), (70, 130), (90, 200)) for o in range(1, 9)]
    k = [(E.oriented_size(o, w, h)[0] / out_w, E.oriented_size(o, w, h)[1] / out_h) for (w, h), o in cases]
    assert any(1 < kx < 2 and ky > 2 for kx, ky in k) or any(1 < ky < 2 and kx > 2 for kx, ky in k)
    images = [pixel_image("random", w, h, 3 * w + h + o) for (w, h), o in cases]
    _, got = resize_call(ctx, torch, images, [o for _, o in cases], out_w, out_h, AA)
    copies = [torch_orient(torch, torch.from_numpy(im).to(ctx.torch_device), o) for im, (_, o) in zip(images, cases)]
    witness = J.resize(ctx, copies, (out_w, out_h), filter="antialias").cpu().numpy()
    for i, (im, (size, o)) in enumerate(zip(images, cases)):
        same(got[i], A.resize(E.orient(im, o), out_w, out_h), (size, o))
        same(got[i], witness[i], (size, o, "the existing call on an oriented copy"))


def test_antialias_at_the_limit_along_the_transposed_axis(ctx, torch):
    """Stored 40 x 512 in orientation 6 is 512 x 40: kx = 16 exactly, the limit, and the horizontal pass walks stored rows."""
    image = pixel_image("random", 40, 512, 9)
    other = pixel_image("checker", 40, 512, 0)
    _, got = resize_call(ctx, torch, [image, other], [6, 8], 32, 32, AA)
    same(got[0], A.resize(E.orient(image, 6), 32, 32), "6")
    same(got[1], A.resize(E.orient(other, 8), 32, 32), "8")


def test_the_tap_limit_is_judged_on_the_oriented_factors(ctx, torch):
    image = pixel_image("random", 600, 40, 4)                          # to 32 x 40: kx = 18.75 as stored; 1.25 and ky = 15 transposed
    assert resize_call(ctx, torch, [image], [1], 32, 40, AA, expect=_lib.ENOSUP)[0] == _lib.ENOSUP
    assert resize_call(ctx, torch, [image], None, 32, 40, AA, expect=_lib.ENOSUP)[0] == _lib.ENOSUP
    assert resize_call(ctx, torch, [image], None, 32, 40, AA, expect=_lib.ENOSUP, old=True)[0] == _lib.ENOSUP
    assert resize_call(ctx, torch, [image, image], [6, 3], 32, 40, AA, expect=_lib.ENOSUP)[0] == _lib.ENOSUP
    _, got = resize_call(ctx, torch, [image, image], [6, 5], 32, 40, AA)
    same(got[0], A.resize(E.orient(image, 6), 32, 40), "6")
    same(got[1], A.resize(E.orient(image, 5), 32, 40), "5")


# ---- 4. no orientations, and all ones: the old calls ---------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def spectrals(ctx):
    """4:2:0 at 53 x 37, 4:4:4 at 40 x 24, grey at 17 x 33."""
    made = [F.synthetic_file("420", (53, 37), 41), F.synthetic_file("444", (40, 24), 42), F.synthetic_file("y8", (17, 33), 43)]
    return [J.Spectral.decompress(ctx, d) for d, _ in made]


# (image, denom, x, y, w, h): denominators 1 and 2, a one-pixel view, the bottom right corner of every image
MIXED_VIEWS = [(0, 1, 0, 0, 53, 37), (0, 2, 3, 2, 20, 15), (0, 1, 40, 30, 13, 7), (1, 1, 5, 4, 30, 17), (1, 2, 10, 5, 10, 7),
               (2, 1, 0, 0, 17, 33), (2, 2, 4, 7, 1, 1), (2, 2, 5, 10, 4, 7)]


def mixed_call(ctx, torch, spectrals, views, orient, out_w, out_h, filter, spec=None, flips=None, old=False):
    """jpeg_amd_decode_resized_oriented_mixed (spec: _tensor_), or the *_filter_mixed call -> (status, the images' bytes)."""
    vs, h_images, h_views, keep = _mixed_args(ctx, spectrals, views)
    n = len(spectrals)
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=5, lead=4, tail=7)
    head = (ctx.handle, n, h_images, 0, _lib.COLOR_RGB8, h_views, out_w, out_h, filter)
    L = _lib.lib()
    if spec is None:
        st = (L.jpeg_amd_decode_resized_filter_mixed(*head, out.ptr, out.stride) if old else
              L.jpeg_amd_decode_resized_oriented_mixed(*head, c_bytes(orient), out.ptr, out.stride))
    else:
        cs = c_spec(spec)
        st = (L.jpeg_amd_decode_tensor_filter_mixed(*head, C.byref(cs), c_bytes(flips), out.ptr, out.stride) if old else
              L.jpeg_amd_decode_tensor_oriented_mixed(*head, C.byref(cs), c_bytes(flips), c_bytes(orient), out.ptr, out.stride))
    ctx.synchronize()
    return st, out.images() if st == 0 else None


def file_call(ctx, torch, datas, regions, orient, out_size, filter, spec=None, flips=None, old=False):
    """The two file calls -> (status, the images' bytes, views, the orientations applied)."""
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    sizes = (C.c_size_t * n)(*[d.size for d in datas])
    regs = None if regions is None else (_lib.Region * n)(*[_lib.Region(*r) for r in regions])
    infos, views, applied = (_lib.FrameInfo * n)(), (_lib.View * n)(), (C.c_int32 * n)()
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_size[0] * out_size[1]] * n, elem=elem, gap=5, lead=4, tail=7)
    head = (ctx.handle, ptrs, sizes, n, 2, 0, _lib.COLOR_RGB8, regs, out_size[0], out_size[1], filter)
    L = _lib.lib()
    if spec is None:
        st = (L.jpeg_amd_decompress_resized_mixed(*head, out.ptr, out.stride, infos, views) if old else
              L.jpeg_amd_decompress_resized_oriented_mixed(*head, c_bytes(orient), out.ptr, out.stride, infos, views, applied))
    else:
        cs = c_spec(spec)
        st = (L.jpeg_amd_decompress_tensor_mixed(*head, C.byref(cs), c_bytes(flips), out.ptr, out.stride, infos, views) if old else
              L.jpeg_amd_decompress_tensor_oriented_mixed(*head, C.byref(cs), c_bytes(flips), c_bytes(orient), out.ptr, out.stride, infos,
                                                          views, applied))
    ctx.synchronize()
    return (st, out.images() if st == 0 else None, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views],
            list(applied))


@pytest.mark.parametrize("filter", [BILINEAR, AA], ids=["bilinear", "antialias"])
def test_null_and_all_ones_are_the_old_calls(ctx, torch, spectrals, filter):
    spec = T.Spec(T.F16, T.CHW)
    # pixel sources
    images = [pixel_image("random", w, h, w + h) for w, h in SIZES[:5]]
    flips = [1, 0, 1, 0, 1]
    for sp, fl in ((None, None), (spec, flips)):
        old = resize_call(ctx, torch, images, None, 24, 40, filter, sp, fl, old=True)[1]
        for orient in (None, [1] * 5):
            for g, w in zip(resize_call(ctx, torch, images, orient, 24, 40, filter, sp, fl)[1], old):
                same(g, w, ("resize", orient))
    # coefficient sources
    sps = [spectrals[v[0]] for v in MIXED_VIEWS]
    views = [v[1:] for v in MIXED_VIEWS]
    flips = [i % 2 for i in range(len(views))]
    for sp, fl in ((None, None), (spec, flips)):
        st, old = mixed_call(ctx, torch, sps, views, None, 24, 16, filter, sp, fl, old=True)
        assert st == 0
        for orient in (None, [1] * len(views)):
            st, got = mixed_call(ctx, torch, sps, views, orient, 24, 16, filter, sp, fl)
            assert st == 0
            for g, w in zip(got, old):
                same(g, w, ("mixed", orient))
    # files
    datas = [d for d, _ in base_files(700)]
    regions = [(3, 5, 100, 80)] * len(datas)
    for sp, fl in ((None, None), (spec, [1] * len(datas))):
        st, old, old_views, _ = file_call(ctx, torch, datas, regions, None, (24, 16), filter, sp, fl, old=True)
        assert st == 0
        for orient in (None, [1] * len(datas)):
            st, got, views_, applied = file_call(ctx, torch, datas, regions, orient, (24, 16), filter, sp, fl)
            assert st == 0 and views_ == old_views and applied == [1] * len(datas)
            for g, w in zip(got, old):
                same(g, w, ("files", orient))
    # ... and a refusal: the same status, nothing written
    wide = [F.synthetic_file("444", (600, 40), 21)[0]]
    assert file_call(ctx, torch, wide, None, None, (2, 2), AA, old=True)[0] == file_call(ctx, torch, wide, None, None, (2, 2), AA)[0] \
        == file_call(ctx, torch, wide, None, [1], (2, 2), AA)[0] == _lib.ENOSUP


# ---- 5. mixed decode ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter", [BILINEAR, AA], ids=["bilinear", "antialias"])
def test_mixed_decode_orients_each_views_pixels(ctx, torch, spectrals, filter):
    sps = [spectrals[v[0]] for v in MIXED_VIEWS]
    views = [v[1:] for v in MIXED_VIEWS]
    orient = [(2, 5, 6, 8)[i % 4] for i in range(len(views))]
    orient[6], orient[7] = orient[7], orient[6]                        # the one-pixel view transposed too
    stored = [v.cpu().numpy() for v in J.decode_views_mixed(ctx, sps, views)]
    assert [s.shape[:2] for s in stored] == [(v[4], v[3]) for v in views]
    out_w, out_h = 24, 16
    st, got = mixed_call(ctx, torch, sps, views, orient, out_w, out_h, filter)
    assert st == 0
    for i, (s, o) in enumerate(zip(stored, orient)):
        same(got[i], MIRROR[filter](E.orient(s, o), out_w, out_h), (MIXED_VIEWS[i], o))
    spec = T.Spec(T.F16, T.CHW)
    flips = [i % 3 == 1 for i in range(len(views))]
    st, got = mixed_call(ctx, torch, sps, views, orient, out_w, out_h, filter, spec, flips)
    assert st == 0
    for i, (s, o) in enumerate(zip(stored, orient)):
        same(bits(got[i], spec), T.normalise(MIRROR[filter](E.orient(s, o), out_w, out_h), spec, flips[i]), (MIXED_VIEWS[i], o, "tensor"))
    # the Python keyword is the same call
    api = J.decode_resized_mixed(ctx, sps, views, (out_w, out_h), filter=NAME[filter], orientations=orient).cpu().numpy()
    for i, (s, o) in enumerate(zip(stored, orient)):
        same(api[i], MIRROR[filter](E.orient(s, o), out_w, out_h), (MIXED_VIEWS[i], o, "api"))


# ---- 6. files --------------------------------------------------------------------------------------------------------------------

BASE = [("420", (160, 120), "sequential", 0), ("422", (158, 121), "sequential", 0), ("440", (161, 119), "sequential", 0),
        ("444", (150, 123), "sequential", 0), ("y8", (163, 117), "progressive", 0), ("420", (157, 122), "sequential", 3)]


def base_files(seed):
    return [F.synthetic_file(name, size, seed + i, kind, restart) for i, (name, size, kind, restart) in enumerate(BASE)]


def tagged_files(seed):
    """Every base file with an inserted segment for each of the orientations 1 .. 8, and one file without any
    -> (files, the orientation each names)."""
    datas, named = [], []
    for i, (d, _) in enumerate(base_files(seed)):
        for o in range(1, 9):
            datas.append(E.insert(d, (E.XMP if o % 3 == 0 else b"") + E.exif_segment(o, big=(i + o) % 2 == 1, type=E.SHORT if o % 2 else E.LONG)))
            named.append(o)
    datas.append(base_files(seed)[0][0])
    named.append(1)
    return datas, named


def oriented_crops(datas, orient, seed):
    rng = np.random.default_rng(seed)
    rects = []
    for d, o in zip(datas, orient):
        info = F.inspect(d)
        ow, oh = E.oriented_size(o, info.width, info.height)
        w, h = int(rng.integers(1, ow + 1)), int(rng.integers(1, oh + 1))
        rects.append((int(rng.integers(0, ow - w + 1)), int(rng.integers(0, oh - h + 1)), w, h))
    rects[0] = (0, 0) + E.oriented_size(orient[0], F.inspect(datas[0]).width, F.inspect(datas[0]).height)     # a whole image
    rects[5] = tuple(np.subtract(E.oriented_size(orient[5], F.inspect(datas[5]).width, F.inspect(datas[5]).height), 1)) + (1, 1)
    return rects


def contract(ctx, torch, datas, rects, orient, out_size, spec, flips, filter):
    """The reference of the file calls' contract, from existing calls: the oriented rectangle mapped in numpy, the view of the
    stored rectangle decoded from whole planes, oriented, and resampled by the existing tensor call.
    -> (bit patterns per image, the stored views)"""
    sps = [J.Spectral.decompress(ctx, d) for d in datas]
    views = []
    for s, r, o in zip(sps, rects, orient):
        denom = J.view_denom(r[2:], out_size)
        views.append((denom,) + J.view_of_source(s.size, denom, E.stored_rect(o, s.size[0], s.size[1], r)))
    stored = J.decode_views_mixed(ctx, sps, views)
    copies = [torch_orient(torch, v, o) for v, o in zip(stored, orient)]
    want = J.resize_tensor(ctx, copies, out_size, spec, flips=flips, filter=filter)
    return want.contiguous().view(len(datas), -1).view(torch.uint8).cpu().numpy(), views


@pytest.mark.parametrize("filter", ["bilinear", "antialias"])
def test_files_in_their_exif_orientation_with_oriented_crops(ctx, torch, filter):
    """Two sets of files of the same sizes through ONE context: the second must not see the first one's planes."""
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    for seed in (500, 900):
        datas, named = tagged_files(seed)
        assert [J.exif_orientation(d) for d in datas] == named
        rects = oriented_crops(datas, named, seed + 1)
        flips = [i % 3 == 1 for i in range(len(datas))]
        got, views, infos, applied = J.decompress_tensors(ctx, datas, (24, 16), spec, source_regions=rects, flips=flips, filter=filter,
                                                          threads=2, orientation="exif")
        want, want_views = contract(ctx, torch, datas, rects, named, (24, 16), spec, flips, filter)
        assert applied.tolist() == named and views.tolist() == [list(v) for v in want_views]
        assert {v[0] for v in want_views} >= {1, 2, 4}
        got = got.contiguous().view(len(datas), -1).view(torch.uint8).cpu().numpy()
        for i in range(len(datas)):
            same(got[i], want[i], (seed, i, named[i], rects[i], want_views[i]))
        # the mixed call's keyword on whole planes is the same contract (decode_crops_tensor_mixed maps the rectangles)
        sps = [J.Spectral.decompress(ctx, d) for d in datas[:9]]
        crops, crop_views = J.decode_crops_tensor_mixed(ctx, sps, rects[:9], (24, 16), spec, flips=flips[:9], filter=filter, orientations=named[:9])
        assert crop_views.tolist() == [list(v) for v in want_views[:9]]
        same(crops.contiguous().view(9, -1).view(torch.uint8).cpu().numpy(), want[:9], (seed, "decode_crops_tensor_mixed"))


def test_a_forced_value_overrides_the_tag(ctx, torch):
    spec = J.tensor_spec(dtype=torch.float32, layout="hwc")
    datas, named = tagged_files(300)
    datas, named = datas[::5], named[::5]
    forced = [(3 * i) % 8 + 1 for i in range(len(datas))]
    mixed = [f if i % 2 else "exif" for i, f in enumerate(forced)]
    expect = [f if i % 2 else t for i, (f, t) in enumerate(zip(forced, named))]
    assert any(e != t for e, t in zip(expect, named))
    rects = oriented_crops(datas, expect, 8)
    got, views, _, applied = J.decompress_tensors(ctx, datas, (24, 16), spec, source_regions=rects, orientation=mixed, threads=1)
    want, want_views = contract(ctx, torch, datas, rects, expect, (24, 16), spec, None, "bilinear")
    assert applied.tolist() == expect and views.tolist() == [list(v) for v in want_views]
    same(got.contiguous().view(len(datas), -1).view(torch.uint8).cpu().numpy(), want, "forced")


@pytest.mark.parametrize("o", [6, 8])
def test_whole_file_at_its_own_oriented_size_is_the_oriented_decode(ctx, torch, o):
    """No mirror in this one: at k = 1 the bilinear filter is the identity, so the byte call gives orient(full decode)."""
    data = E.insert(F.synthetic_file("420", (53, 37), 77)[0], E.exif_segment(o, big=True))
    full = J.Spectral.decompress(ctx, data).decode(J.RGB).cpu().numpy().reshape(37, 53, 3)
    got = J.decompress_resized(ctx, [data], (37, 53), orientation="exif").cpu().numpy()
    assert got.shape == (1, 53, 37, 3)
    same(got[0], E.orient(full, o), o)
    assert not (E.orient(full, o) == E.orient(full, 14 - o)).all()      # 6 and 8 differ on this image
    st, images, views, applied = file_call(ctx, torch, [data], None, [0], (37, 53), BILINEAR)
    assert st == 0 and views == [(1, 0, 0, 53, 37)] and applied == [o]
    same(images[0], E.orient(full, o), (o, "guarded"))


@pytest.mark.parametrize("filter", ["bilinear", "antialias"])
@pytest.mark.parametrize("out_size", [(12, 36), (36, 12)], ids=["12x36", "36x12"])
def test_whole_files_without_rectangles_at_a_target_that_is_not_square(ctx, torch, filter, out_size):
    """source_regions=None is the whole ORIENTED image: the denominator is chosen for w' x h'.  At 12 x 36 a transposed
    160 x 120 file takes denominator 4 where its stored extent would take 2, and at 36 x 12 the other way round."""
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    datas, named = tagged_files(640)
    rects = [(0, 0) + E.oriented_size(o, F.inspect(d).width, F.inspect(d).height) for d, o in zip(datas, named)]
    flips = [i % 2 for i in range(len(datas))]
    got, views, _, applied = J.decompress_tensors(ctx, datas, out_size, spec, flips=flips, filter=filter, threads=2, orientation="exif")
    want, want_views = contract(ctx, torch, datas, rects, named, out_size, spec, flips, filter)
    assert applied.tolist() == named and views.tolist() == [list(v) for v in want_views]
    stored = [J.view_denom((F.inspect(d).width, F.inspect(d).height), out_size) for d in datas]
    assert all((v[0] != s) == (o >= 5) for v, s, o in zip(want_views, stored, named))     # the case is the one it is meant to be
    assert {v[0] for v in want_views} == {2, 4}
    got = got.contiguous().view(len(datas), -1).view(torch.uint8).cpu().numpy()
    for i in range(len(datas)):
        same(got[i], want[i], (i, named[i], want_views[i]))
    # ... and the byte call, against naming the whole oriented rectangles
    a = J.decompress_resized(ctx, datas, out_size, filter=filter, orientation="exif")
    b = J.decompress_resized(ctx, datas, out_size, source_regions=rects, filter=filter, orientation="exif")
    assert torch.equal(a, b)
