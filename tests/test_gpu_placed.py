"""The placed resample on the MI355X (the six *_placed_* calls; the kernels over the Placed* records): the contract of
include/jpeg_amd.h ("placed resample") is by reference -- inside the window the filter's contract at the window's size, the
fill outside -- so every output is compared byte for byte, or element for element as a bit pattern, with _placed_ref.place of
the existing numpy mirrors (_resize_ref, _antialias_ref, _bicubic_ref), and, as a second witness, with what the existing GPU
call writes at ww x wh, pasted into a canvas of the fill.  The canvas is 70 x 37 -- two tile columns and two tile rows, both
partial -- and the windows leave tiles without a window pixel, straddle all four tiles with runs that straddle their edges,
cover the canvas, and are one pixel in the last partial tile.  Every raw call writes into a sentinel-filled buffer whose bytes
in front of, between and behind the images are checked."""
import ctypes as C

import numpy as np
import pytest

import _antialias_ref as A
import _bicubic_ref as B
import _files as F
import _orient as E
import _placed_ref as P
import _resize_ref as R
import _tensor_ref as T
import jpeg_amd as J
from _calls import Out, pixel_image
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, c_spec, host_bits as bits, pack, same
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

BILINEAR, AA, BICUBIC = _lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS, _lib.FILTER_BICUBIC
FILTERS = [BILINEAR, AA, BICUBIC]
MIRROR = {BILINEAR: R.resize, AA: A.resize, BICUBIC: B.resize}
NAME = {BILINEAR: "bilinear", AA: "antialias", BICUBIC: "bicubic"}
LIMIT = {BILINEAR: float("inf"), AA: 16.0, BICUBIC: 8.0}
CANVAS = (70, 37)
INSIDE, STRADDLE, WHOLE, PIXEL = (5, 3, 33, 21), (62, 30, 7, 6), (0, 0, 70, 37), (69, 36, 1, 1)
WINDOWS = [INSIDE, STRADDLE, WHOLE, PIXEL]
SIZES = [(37, 23), (23, 37), (130, 70), (1, 9), (300, 200), (5, 7)]          # (w, h) as stored
FILL = (124, 116, 104)


def c_placement(windows=None, mode=P.WINDOWS, anchor=P.CENTRE, fill=FILL):
    p = _lib.Placement()
    p.mode, p.anchor = mode, anchor
    keep = None
    if windows is not None:
        keep = (_lib.Region * len(windows))(*[_lib.Region(*w) for w in windows])
        p.h_windows = C.cast(keep, C.c_void_p)
    p.fill[0], p.fill[1], p.fill[2] = fill
    return keep, p


def placed_call(ctx, torch, images, place, canvas, filter, orient=None, spec=None, flips=None, oriented_call=False):
    """jpeg_amd_resize_placed_batch (spec: _tensor_batch) with `place` (a struct, or None for NULL), or the *_oriented_* call,
    into a guarded buffer -> (the images' bytes, the windows written)."""
    out_w, out_h = canvas
    n = len(images)
    d_src, stride, ext = pack(ctx, torch, images)
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=5, lead=4, tail=7)
    wout = (_lib.Region * n)(*[_lib.Region(-7, -7, -7, -7)] * n)
    pl = () if oriented_call else (None if place is None else C.byref(place), wout)
    head = (ctx.handle, n, d_src.data_ptr(), stride, ext, out_w, out_h, filter)
    L = _lib.lib()
    if spec is None:
        st = (L.jpeg_amd_resize_oriented_batch if oriented_call else L.jpeg_amd_resize_placed_batch)(*head, c_bytes(orient), *pl, out.ptr, out.stride)
    else:
        cs = c_spec(spec)
        st = (L.jpeg_amd_resize_oriented_tensor_batch if oriented_call else L.jpeg_amd_resize_placed_tensor_batch)(
            *head, C.byref(cs), c_bytes(flips), c_bytes(orient), *pl, out.ptr, out.stride)
    assert st == 0
    ctx.synchronize()
    return out.images(), [(r.x, r.y, r.width, r.height) for r in wout]


def inside_limit(size, window, filter, o=1):
    w, h = E.oriented_size(o, *size)
    return max(w / window[2], h / window[3]) <= LIMIT[filter]


@pytest.fixture(scope="module")
def sources():
    return {size: pixel_image("random", size[0], size[1], 31 * size[0] + size[1]) for size in SIZES + [(450, 520), (230, 270)]}


# ---- 1. bytes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter", FILTERS, ids=[NAME[f] for f in FILTERS])
def test_bytes_every_window_in_one_launch(ctx, torch, sources, filter):
    cases = [(size, win) for win in WINDOWS for size in SIZES if inside_limit(size, win, filter)]
    assert {win for _, win in cases} == set(WINDOWS) and len(cases) >= 14
    images = [sources[size] for size, _ in cases]
    keep, place = c_placement([win for _, win in cases])
    got, windows = placed_call(ctx, torch, images, place, CANVAS, filter)
    assert windows == [win for _, win in cases]
    # the second witness: the existing call at ww x wh, one call per window size, pasted into a canvas of the fill
    witness = {}
    for win in WINDOWS:
        sizes = [size for size, w in cases if w == win]
        dev = [torch.from_numpy(sources[size]).to(ctx.torch_device) for size in sizes]
        res = J.resize(ctx, dev, win[2:], filter=NAME[filter]).cpu().numpy()
        for size, r in zip(sizes, res):
            canvas = torch.full((CANVAS[1], CANVAS[0], 3), 0, dtype=torch.uint8)
            canvas[:, :] = torch.tensor(FILL, dtype=torch.uint8)
            canvas[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = torch.from_numpy(r)
            witness[(size, win)] = canvas.numpy()
    for i, (size, win) in enumerate(cases):
        same(got[i], P.place(MIRROR[filter](sources[size], win[2], win[3]), win, CANVAS, FILL), (size, win))
        same(got[i], witness[(size, win)], (size, win, "the existing call at the window's size, pasted"))


# ---- 2. the tensor forms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", [(T.F16, T.CHW), (T.F32, T.HWC), (T.BF16, T.CHW)], ids=["f16-chw", "f32-hwc", "bf16-chw"])
@pytest.mark.parametrize("filter", FILTERS, ids=[NAME[f] for f in FILTERS])
def test_tensor_forms_pad_with_the_fill_and_flip_the_canvas(ctx, torch, sources, combo, filter):
    spec = T.Spec(*combo)                                            # ImageNet's mean and std, in bytes
    cases = [(size, win, flip) for win in (INSIDE, STRADDLE, PIXEL) for size in ((37, 23), (23, 37), (5, 7)) for flip in (0, 1)
             if inside_limit(size, win, filter)]
    assert {win for _, win, _ in cases} == {INSIDE, STRADDLE, PIXEL}
    images = [sources[size] for size, _, _ in cases]
    flips = [flip for _, _, flip in cases]
    keep, place = c_placement([win for _, win, _ in cases])
    got, _ = placed_call(ctx, torch, images, place, CANVAS, filter, spec=spec, flips=flips)
    pad = T.normalise(np.asarray(FILL, np.uint8).reshape(1, 1, 3), spec, 0).reshape(3)     # the epilogue of the fill byte, per channel
    for i, (size, win, flip) in enumerate(cases):
        canvas = P.place(MIRROR[filter](sources[size], win[2], win[3]), win, CANVAS, FILL)
        g = bits(got[i], spec)
        same(g, T.normalise(canvas, spec, flip), (size, win, flip, combo))
        # ... and, said directly: outside the mirrored window every element is the fill's, inside the window's pixels are mirrored
        g = g.reshape(3, CANVAS[1], CANVAS[0]).transpose(1, 2, 0) if spec.layout == T.CHW else g.reshape(CANVAS[1], CANVAS[0], 3)
        x0 = CANVAS[0] - win[0] - win[2] if flip else win[0]
        outside = np.ones((CANVAS[1], CANVAS[0]), bool)
        outside[win[1]:win[1] + win[3], x0:x0 + win[2]] = False
        assert (g[outside] == pad).all(), (size, win, flip)
        inner = T.normalise(canvas[win[1]:win[1] + win[3], win[0]:win[0] + win[2]], T.Spec(combo[0], T.HWC), flip)
        same(g[win[1]:win[1] + win[3], x0:x0 + win[2]], inner, (size, win, flip, "the window"))


# ---- 3. orientations --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter", FILTERS, ids=[NAME[f] for f in FILTERS])
def test_orientations_with_windows(ctx, torch, sources, filter):
    cases = [(size, o, win) for size in ((37, 23), (23, 37)) for o in (1, 3, 6, 7) for win in (INSIDE, STRADDLE)]
    assert all(inside_limit(size, win, filter, o) for size, o, win in cases)
    images = [sources[size] for size, _, _ in cases]
    keep, place = c_placement([win for _, _, win in cases])
    got, _ = placed_call(ctx, torch, images, place, CANVAS, filter, orient=[o for _, o, _ in cases])
    for i, (size, o, win) in enumerate(cases):
        same(got[i], P.place(MIRROR[filter](E.orient(sources[size], o), win[2], win[3]), win, CANVAS, FILL), (size, o, win))
    # FIT fits the ORIENTED image
    keep, fit = c_placement(mode=P.FIT)
    got, windows = placed_call(ctx, torch, images, fit, CANVAS, filter, orient=[o for _, o, _ in cases])
    for i, (size, o, _) in enumerate(cases):
        ow, oh = E.oriented_size(o, *size)
        win = P.place_window(P.FIT, P.CENTRE, ow, oh, *CANVAS)
        assert windows[i] == win and (win[2] == CANVAS[0] or win[3] == CANVAS[1])
        same(got[i], P.place(MIRROR[filter](E.orient(sources[size], o), win[2], win[3]), win, CANVAS, FILL), (size, o, "fit"))


# ---- 4. whole-canvas windows and no placement: the oriented call ------------------------------------------------------------------------

@pytest.mark.parametrize("filter", FILTERS, ids=[NAME[f] for f in FILTERS])
def test_whole_canvas_windows_and_null_are_the_oriented_call(ctx, torch, sources, filter):
    sizes = [(37, 23), (23, 37), (130, 70), (5, 7)]
    images = [sources[size] for size in sizes]
    flips = [1, 0, 1, 0]
    keep, whole = c_placement([WHOLE] * len(sizes))
    for orient in (None, [1] * 4, [6, 3, 1, 7]):
        for spec, fl in ((None, None), (T.Spec(T.F16, T.CHW), flips)):
            old, _ = placed_call(ctx, torch, images, None, CANVAS, filter, orient=orient, spec=spec, flips=fl, oriented_call=True)
            null, windows = placed_call(ctx, torch, images, None, CANVAS, filter, orient=orient, spec=spec, flips=fl)
            assert windows == [(-7, -7, -7, -7)] * 4
            got, windows = placed_call(ctx, torch, images, whole, CANVAS, filter, orient=orient, spec=spec, flips=fl)
            assert windows == [WHOLE] * 4
            for i in range(4):
                same(null[i], old[i], (sizes[i], orient, "NULL"))
                same(got[i], old[i], (sizes[i], orient, "whole-canvas windows"))


# ---- 5. the footprint of the table kernels ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("filter,size", [(AA, (450, 520)), (BICUBIC, (230, 270))], ids=["antialias", "bicubic"])
def test_the_vertical_footprint_comes_from_the_window_rows(ctx, torch, sources, filter, size):
    """40 x 70 with the window (3, 33, 30, 35): the first tile row is padding alone, the second tile's first row is padded, and
    the third tile's rows behind row 3 are; k is about 15 (bicubic: 7.7), so a footprint taken from a padded row would show."""
    canvas, win = (40, 70), (3, 33, 30, 35)
    assert LIMIT[filter] * 0.9 < max(size[0] / win[2], size[1] / win[3]) <= LIMIT[filter]
    keep, place = c_placement([win, win])
    got, _ = placed_call(ctx, torch, [sources[size], sources[(37, 23)]], place, canvas, filter)
    same(got[0], P.place(MIRROR[filter](sources[size], win[2], win[3]), win, canvas, FILL), (size, win))
    same(got[1], P.place(MIRROR[filter](sources[(37, 23)], win[2], win[3]), win, canvas, FILL), ((37, 23), win))


# ---- 6. the mixed and the file calls ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def files():
    """Four files of different sizes and layouts, one of them with an EXIF orientation; a crop rectangle for one of them (of the
    ORIENTED image where there is an orientation).  -> (datas, rectangles of the oriented images, the orientations)"""
    made = [F.synthetic_file("420", (160, 120), 61)[0], F.synthetic_file("444", (53, 37), 62)[0], F.synthetic_file("y8", (37, 83), 63)[0],
            F.synthetic_file("420", (150, 123), 64, "progressive")[0]]
    made[1] = E.insert(made[1], E.exif_segment(6, big=True))
    orient = [1, 6, 1, 1]
    rects = [(0, 0) + E.oriented_size(o, F.inspect(d).width, F.inspect(d).height) for d, o in zip(made, orient)]
    rects[3] = (7, 11, 120, 40)
    return made, rects, orient


@pytest.mark.parametrize("filter", FILTERS, ids=[NAME[f] for f in FILTERS])
@pytest.mark.parametrize("anchor", ["centre", "top-left"])
def test_files_and_mixed_decodes_fitted_into_a_canvas(ctx, torch, files, filter, anchor):
    datas, rects, orient = files
    canvas = (48, 32)
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    flips = [0, 1, 0, 1]
    got, views, infos, applied, windows = J.decompress_tensors(ctx, datas, canvas, spec, source_regions=rects, flips=flips, filter=NAME[filter],
                                                               threads=2, orientation="exif", place="fit", anchor=anchor, fill=FILL)
    assert applied.tolist() == orient
    want_windows = [P.place_window(P.FIT, P.CENTRE if anchor == "centre" else P.TOP_LEFT, r[2], r[3], *canvas) for r in rects]
    assert windows.tolist() == [list(w) for w in want_windows]
    assert windows.tolist() == [list(J.place_window("fit", r[2:], canvas, anchor)) for r in rects]
    assert views[:, 0].tolist() == [J.view_denom(r[2:], w[2:]) for r, w in zip(rects, want_windows)]
    assert len({tuple(w[2:]) for w in want_windows}) > 2 and len(set(views[:, 0].tolist())) > 1
    pad = torch.tensor(FILL, dtype=torch.uint8, device=ctx.torch_device).reshape(1, 1, 1, 3)
    pad = J.resize_tensor(ctx, [pad[0]], (1, 1), spec).reshape(3)          # the epilogue of the fill byte
    want = torch.empty_like(got)
    for i, (d, r, w) in enumerate(zip(datas, rects, want_windows)):
        one, one_views, _, _ = J.decompress_tensors(ctx, [d], w[2:], spec, source_regions=[r], flips=[0], filter=NAME[filter], threads=1,
                                                     orientation="exif")
        assert one_views.tolist() == [views[i].tolist()]
        want[i] = pad.reshape(3, 1, 1)
        want[i, :, w[1]:w[1] + w[3], w[0]:w[0] + w[2]] = one[0]
        if flips[i]:
            want[i] = want[i].flip(2)                                      # the flip mirrors the whole canvas
    same(got.view(torch.int16).cpu().numpy(), want.view(torch.int16).cpu().numpy(), (NAME[filter], anchor, "files"))
    # the byte call, and the mixed call on whole planes: the same windows, the same pixels
    raw, raw_windows = J.decompress_resized(ctx, datas, canvas, source_regions=rects, filter=NAME[filter], orientation="exif", place="fit",
                                            anchor=anchor, fill=FILL)
    assert raw_windows.tolist() == windows.tolist()
    for i, w in enumerate(want_windows):
        one = J.decompress_resized(ctx, [datas[i]], w[2:], source_regions=[rects[i]], filter=NAME[filter], orientation="exif").cpu().numpy()[0]
        same(raw[i].cpu().numpy(), P.place(one, w, canvas, FILL), (i, "bytes"))
    sps = [J.Spectral.decompress(ctx, d) for d in datas]
    crops, crop_views, crop_windows = J.decode_crops_tensor_mixed(ctx, sps, rects, canvas, spec, flips=flips, filter=NAME[filter],
                                                                  orientations=orient, place="fit", anchor=anchor, fill=FILL)
    assert crop_views.tolist() == views.tolist() and crop_windows.tolist() == windows.tolist()
    same(crops.view(torch.int16).cpu().numpy(), want.view(torch.int16).cpu().numpy(), (NAME[filter], anchor, "decode_crops_tensor_mixed"))
