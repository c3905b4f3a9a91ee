"""The placed resample (include/jpeg_amd.h, "placed resample") without a GPU: jpeg_amd_place_window against the Python integers
of _placed_ref, and what the six *_placed_* calls refuse, and in which order, with a NULL context.

A call that passes every check reaches the context, which is NULL: EINVAL.  So, as in test_orient_cpu, the verdict that shows
how far a call came is the tap limit's ENOSUP, which is given last and before the context is looked at: an antialias call
over the limit that is refused for anything else says EINVAL, one that is refused for nothing else says ENOSUP.  The windows
a call writes to h_windows_out are written before the context is looked at, so they show what was judged."""
import ctypes as C
import itertools

import numpy as np
import pytest

import _files as F
import _placed_ref as P
from _calls import c_layout
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, -1, -5
RGB = _lib.COLOR_RGB8
BILINEAR, ANTIALIAS, BICUBIC = _lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS, _lib.FILTER_BICUBIC
UNSET = (-7, -7, -7, -7)


# ---- jpeg_amd_place_window ----------------------------------------------------------------------------------------------------------

def c_window(mode, anchor, src, out):
    r = _lib.Region(*UNSET)
    st = _lib.lib().jpeg_amd_place_window(mode, anchor, src[0], src[1], out[0], out[1], C.byref(r))
    return st, (r.x, r.y, r.width, r.height)


def check_properties(mode, src, out, win):
    x0, y0, ww, wh = win
    assert ww >= 1 and wh >= 1 and 0 <= x0 and 0 <= y0 and x0 + ww <= out[0] and y0 + wh <= out[1], (mode, src, out, win)
    fits = src[0] <= out[0] and src[1] <= out[1]
    if mode == P.FIT or not fits:               # in FIT one side is the canvas's
        assert ww == out[0] or wh == out[1], (mode, src, out, win)
    if mode == P.FIT_DOWN:                      # FIT_DOWN never enlarges, and keeps a source that fits as it is
        assert ww <= src[0] and wh <= src[1], (mode, src, out, win)
        assert not fits or (ww, wh) == tuple(src), (mode, src, out, win)


def test_place_window_is_the_python_integers():
    cases = [((w, h), out) for w in range(1, 41) for h in range(1, 41) for out in ((1, 1), (7, 5), (5, 7), (64, 33))]
    big = 2 ** 30
    cases += [(src, out) for src in ((65535, 1), (1, 65535), (65535, 65535), (3, 2))
              for out in ((big, big), (big, 1), (1, big), (big, 7), (64, 33))]
    for (src, out), mode, anchor in itertools.product(cases, (P.FIT, P.FIT_DOWN), (P.CENTRE, P.TOP_LEFT)):
        st, win = c_window(mode, anchor, src, out)
        assert st == OK and win == P.place_window(mode, anchor, src[0], src[1], out[0], out[1]), (mode, anchor, src, out, win)
        check_properties(mode, src, out, win)
        if anchor == P.TOP_LEFT:
            assert win[:2] == (0, 0)
        else:
            assert win[:2] == ((out[0] - win[2]) // 2, (out[1] - win[3]) // 2)


def test_place_window_refuses():
    assert c_window(P.FIT, P.CENTRE, (3, 2), (8, 8)) == (OK, (0, 1, 8, 5))
    for mode, anchor, src, out in ((P.WINDOWS, 0, (3, 2), (8, 8)), (3, 0, (3, 2), (8, 8)), (-1, 0, (3, 2), (8, 8)), (P.FIT, 2, (3, 2), (8, 8)),
                                   (P.FIT, -1, (3, 2), (8, 8)), (P.FIT, 0, (0, 2), (8, 8)), (P.FIT, 0, (3, 0), (8, 8)), (P.FIT, 0, (3, 2), (0, 8)),
                                   (P.FIT, 0, (3, 2), (8, 0)), (P.FIT, 0, (3, 2), (2 ** 30 + 1, 8)), (P.FIT, 0, (3, 2), (8, 2 ** 30 + 1))):
        assert c_window(mode, anchor, src, out) == (EINVAL, UNSET), (mode, anchor, src, out)
    assert _lib.lib().jpeg_amd_place_window(P.FIT, 0, 3, 2, 8, 8, None) == EINVAL


# ---- the four calls above the file level --------------------------------------------------------------------------------------------

def placement(mode=P.WINDOWS, anchor=P.CENTRE, windows=None, fill=(1, 2, 3)):
    """-> (keep, struct jpeg_amd_placement)"""
    p = _lib.Placement()
    p.mode, p.anchor = mode, anchor
    keep = None
    if windows is not None:
        keep = (_lib.Region * len(windows))(*[_lib.Region(*w) for w in windows])
        p.h_windows = C.cast(keep, C.c_void_p)
    p.fill[0], p.fill[1], p.fill[2] = fill
    return keep, p


SPEC = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
BUF = np.zeros(16, np.uint16)
PTR = BUF.ctypes.data
N = 2


def resize_call(form, place, w=200, h=40, out=(100, 40), filter=ANTIALIAS, n=N, orient=None, windows_out=True, old=False):
    """jpeg_amd_resize_placed_batch / _tensor_batch on two w x h sources, or the oriented call -> (status, windows written)."""
    ext = (_lib.Extent * N)(*[_lib.Extent(w, h)] * N)
    o = None if orient is None else (C.c_uint8 * N)(*orient)
    wout = (_lib.Region * N)(*[_lib.Region(*UNSET)] * N)
    pl = () if old else (None if place is None else C.byref(place), wout if windows_out else None)
    L = _lib.lib()
    head = (None, n, PTR, 3 * w * h, ext, out[0], out[1], filter)
    if form == "bytes":
        st = (L.jpeg_amd_resize_oriented_batch if old else L.jpeg_amd_resize_placed_batch)(*head, o, *pl, PTR, 3 * out[0] * out[1])
    else:
        st = (L.jpeg_amd_resize_oriented_tensor_batch if old else L.jpeg_amd_resize_placed_tensor_batch)(
            *head, C.byref(SPEC), None, o, *pl, PTR, 3 * out[0] * out[1])
    return st, [(r.x, r.y, r.width, r.height) for r in wout]


def mixed_call(form, place, w=200, h=40, out=(100, 40), filter=ANTIALIAS, n=N, orient=None, windows_out=True, old=False, precisions=(8, 8)):
    """The mixed calls on two whole 4:4:4 images of w x h at denominator 1."""
    images = (_lib.Image * N)()
    for i in range(N):
        images[i].layout = c_layout(w, h, [(1, 1)] * 3, precision=precisions[i])
        for c in range(3):
            images[i].d_coef[c] = PTR
        images[i].d_quanta, images[i].ntables = PTR, 2
    views = (_lib.View * N)(*[_lib.View(1, _lib.Region(0, 0, w, h))] * N)
    o = None if orient is None else (C.c_uint8 * N)(*orient)
    wout = (_lib.Region * N)(*[_lib.Region(*UNSET)] * N)
    pl = () if old else (None if place is None else C.byref(place), wout if windows_out else None)
    L = _lib.lib()
    head = (None, n, images, 0, RGB, views, out[0], out[1], filter)
    if form == "bytes":
        st = (L.jpeg_amd_decode_resized_oriented_mixed if old else L.jpeg_amd_decode_resized_placed_mixed)(*head, o, *pl, PTR, 3 * out[0] * out[1])
    else:
        st = (L.jpeg_amd_decode_tensor_oriented_mixed if old else L.jpeg_amd_decode_tensor_placed_mixed)(
            *head, C.byref(SPEC), None, o, *pl, PTR, 3 * out[0] * out[1])
    return st, [(r.x, r.y, r.width, r.height) for r in wout]


CALLS = [(resize_call, "bytes"), (resize_call, "tensor"), (mixed_call, "bytes"), (mixed_call, "tensor")]
IDS = ["resize", "resize-tensor", "mixed", "mixed-tensor"]
WHOLE = [(0, 0, 100, 40)] * N
NARROW = [(0, 0, 100, 40), (45, 0, 10, 40)]                # image 1: 200 wide into 10: k = 20, over the antialias limit


@pytest.mark.parametrize("call,form", CALLS, ids=IDS)
def test_null_placement_is_the_oriented_call(call, form):
    seen = set()
    for n, out, filter, orient, size in itertools.product((2, 0, -1), ((100, 40), (0, 40), (10, 40), (100, 2 ** 30 + 1)),
                                                          (BILINEAR, ANTIALIAS, BICUBIC, 7), (None, [1, 1], [6, 3], [1, 9]),
                                                          ((200, 40), (40, 200))):
        old = call(form, None, *size, out=out, filter=filter, n=n, orient=orient, old=True)[0]
        got, windows = call(form, None, *size, out=out, filter=filter, n=n, orient=orient)
        assert got == old and windows == [UNSET] * N, (n, out, filter, orient, size)
        seen.add(old)
    assert seen == {OK, EINVAL, ENOSUP} if call is mixed_call else seen == {EINVAL, ENOSUP}


@pytest.mark.parametrize("call,form", CALLS, ids=IDS)
def test_the_tap_limit_is_judged_on_the_window_and_last(call, form):
    keep, whole = placement(windows=WHOLE)
    keep2, narrow = placement(windows=NARROW)
    # a 200-wide source into a 10-wide window of a 100-wide canvas: ENOSUP; into the whole canvas: as far as the (NULL) context
    assert call(form, narrow) == (ENOSUP, NARROW)
    assert call(form, whole) == (EINVAL, WHOLE)
    assert call(form, narrow, filter=BILINEAR) == (EINVAL, NARROW)           # no limit for the bilinear filter
    assert call(form, whole, filter=BICUBIC)[0] == EINVAL                     # k = 2
    keep3, w12 = placement(windows=[(0, 0, 100, 40), (0, 0, 12, 40)])        # k = 16.67: over both limits
    keep4, w13 = placement(windows=[(0, 0, 100, 40), (0, 0, 13, 40)])        # k = 15.4: inside the antialias limit, over the bicubic
    assert call(form, w12)[0] == ENOSUP and call(form, w13)[0] == EINVAL and call(form, w13, filter=BICUBIC)[0] == ENOSUP
    # the canvas does not count: 10 x 40 as a canvas is over the limit, the same sources in FIT windows of a large canvas are not
    assert call(form, None, out=(10, 40))[0] == ENOSUP
    keep5, fit = placement(P.FIT)
    assert call(form, fit, out=(10, 40)) == (ENOSUP, [(0, 19, 10, 2)] * N)      # 200 x 40 fitted into 10 x 40 is 10 x 2: kx = ky = 20
    assert call(form, fit, out=(1000, 40)) == (EINVAL, [(400, 0, 200, 40)] * N)
    # ... on the ORIENTED factors: transposed, 40 x 200 fits into 100 x 40 as 8 x 40
    assert call(form, fit, orient=[6, 8]) == (EINVAL, [(46, 0, 8, 40)] * N)
    keep6, tl = placement(P.FIT, P.TOP_LEFT)
    assert call(form, tl, orient=[6, 1]) == (EINVAL, [(0, 0, 8, 40), (0, 0, 100, 20)])
    keep7, down = placement(P.FIT_DOWN)
    assert call(form, down, out=(300, 100)) == (EINVAL, [(50, 30, 200, 40)] * N)
    assert call(form, down, out=(300, 100), windows_out=False)[0] == EINVAL   # h_windows_out is optional


@pytest.mark.parametrize("call,form", CALLS, ids=IDS)
def test_each_refusal_of_a_placement_in_front_of_the_tap_limit(call, form):
    """Every call here is over the tap limit in image 1 (ENOSUP if nothing else is wrong) and wrong in one more way."""
    def status(mode=P.WINDOWS, anchor=P.CENTRE, windows=NARROW, **kw):
        keep, p = placement(mode, anchor, windows)
        return call(form, p, **kw)[0]

    assert status() == ENOSUP
    for mode in (3, -1, 255):
        assert status(mode=mode) == EINVAL
    for anchor in (2, -1):
        assert status(anchor=anchor) == EINVAL and status(P.FIT, anchor, None, out=(10, 40)) == EINVAL
    assert status(windows=None) == EINVAL                                  # WINDOWS without windows
    for bad in ((0, 0, 0, 40), (0, 0, 10, 0), (0, 0, -1, 40), (-1, 0, 10, 40), (0, -1, 10, 40), (91, 0, 10, 40), (0, 1, 10, 40), (0, 0, 101, 40),
                (2 ** 31 - 5, 0, 10, 40), (0, 2 ** 31 - 5, 10, 40)):
        assert status(windows=[NARROW[1], bad]) == EINVAL, bad             # in image 1, behind image 0's limit
        assert status(windows=[bad, NARROW[1]]) == EINVAL, bad
    # the order: the target and image i's orientation in front of image i's window, the window in front of image i + 1
    assert status(windows=[(0, 0, 0, 40), NARROW[1]], out=(0, 40)) == EINVAL
    assert status(orient=[1, 9]) == EINVAL and status(orient=[1, 6]) == EINVAL      # 6: 40 x 200 into 10 x 40 is inside the limit
    keep, p = placement(windows=[(0, 0, 100, 40), (0, 0, 0, 0)])
    assert call(form, p, orient=[9, 1]) == (EINVAL, [UNSET] * N)           # image 0's orientation: no window was judged
    assert call(form, p) == (EINVAL, [(0, 0, 100, 40), UNSET])             # image 1's window: image 0's was written
    keep, p = placement(windows=None)
    assert call(form, p, n=0)[0] == (EINVAL if call is resize_call else OK)   # an empty call: no windows needed (the resize calls: the context)
    keep, p = placement(mode=3)
    assert call(form, p, n=0)[0] == EINVAL                                  # ... but its placement is judged with the target


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_mixed_calls_judge_a_window_with_its_image(form):
    keep, p = placement(windows=[(0, 0, 0, 0), NARROW[1]])
    assert mixed_call(form, p, precisions=(12, 8))[0] == ENOSUP            # image 0's layout in front of image 0's window
    assert mixed_call(form, p, precisions=(8, 12))[0] == EINVAL            # image 0's window in front of image 1's layout
    keep, p = placement(windows=[NARROW[0], (0, 0, 0, 0)])
    assert mixed_call(form, p, precisions=(8, 12))[0] == ENOSUP            # image 1's layout in front of image 1's window


# ---- the file calls ---------------------------------------------------------------------------------------------------------------

def file_call(datas, place, regions=None, out=(100, 40), filter=ANTIALIAS, tensor=False, orient=None, old=False):
    """-> (status, the views written, the windows written)"""
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    sizes = (C.c_size_t * n)(*[d.size for d in datas])
    regs = None if regions is None else (_lib.Region * n)(*[_lib.Region(*r) for r in regions])
    o = None if orient is None else (C.c_uint8 * n)(*orient)
    infos, views = (_lib.FrameInfo * n)(), (_lib.View * n)()
    for v in views:
        v.denom = -7
    wout = (_lib.Region * n)(*[_lib.Region(*UNSET)] * n)
    pl = () if old else (None if place is None else C.byref(place), wout)
    head = (None, ptrs, sizes, n, 1, 0, RGB, regs, out[0], out[1], filter)
    L = _lib.lib()
    if tensor:
        st = (L.jpeg_amd_decompress_tensor_oriented_mixed if old else L.jpeg_amd_decompress_tensor_placed_mixed)(
            *head, C.byref(SPEC), None, o, *pl, PTR, 3 * out[0] * out[1], infos, views, None)
    else:
        st = (L.jpeg_amd_decompress_resized_oriented_mixed if old else L.jpeg_amd_decompress_resized_placed_mixed)(
            *head, o, *pl, PTR, 3 * out[0] * out[1], infos, views, None)
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views], [(r.x, r.y, r.width, r.height) for r in wout]


@pytest.fixture(scope="module")
def wide():
    return F.synthetic_file("444", (200, 40), 21)[0]


@pytest.mark.parametrize("tensor", [False, True], ids=["bytes", "tensor"])
def test_the_file_calls_judge_windows_in_pass_0(wide, tensor):
    two = [wide, wide]
    # NULL is the oriented call, on good and bad arguments
    seen = set()
    for out, filter, orient, datas in itertools.product(((100, 40), (0, 40), (10, 40), (2, 2)), (BILINEAR, ANTIALIAS, 7), (None, [1, 6], [1, 9]),
                                                        (two, [wide, wide[:30]], [])):
        if not datas:
            orient = None
        old = file_call(datas, None, out=out, filter=filter, tensor=tensor, orient=orient, old=True)
        got = file_call(datas, None, out=out, filter=filter, tensor=tensor, orient=orient)
        assert got[:2] == old[:2] and got[2] == [UNSET] * len(datas), (out, filter, orient, len(datas))
        seen.add(old[0])
    assert {OK, EINVAL, ENOSUP} <= seen
    # the limit on the window, 200 x 40 into a 10 x 40 window is denominator 1 (the height) and kx = 20
    keep, narrow = placement(windows=NARROW)
    assert file_call(two, narrow, tensor=tensor) == (ENOSUP, [(1, 0, 0, 200, 40)] * 2, NARROW)
    keep, whole = placement(windows=WHOLE)
    assert file_call(two, whole, tensor=tensor) == (EINVAL, [(1, 0, 0, 200, 40)] * 2, WHOLE)                  # the (NULL) context
    keep, small = placement(windows=[(3, 3, 25, 5), (0, 0, 50, 10)])
    assert file_call(two, small, filter=BILINEAR, tensor=tensor)[1] == [(8, 0, 0, 25, 5), (4, 0, 0, 50, 10)]  # ... never the canvas (denominator 1)
    # FIT on the ORIENTED crop rectangle's size
    keep, fit = placement(P.FIT)
    st, views, windows = file_call(two, fit, regions=[(0, 0, 200, 40), (10, 0, 20, 40)], tensor=tensor)
    assert st == EINVAL and windows == [(0, 10, 100, 20), (40, 0, 20, 40)] and [v[0] for v in views] == [2, 1]
    st, views, windows = file_call(two, fit, regions=[(0, 0, 40, 200), (0, 10, 40, 20)], orient=[6, 8], tensor=tensor)
    assert st == EINVAL and windows == [(46, 0, 8, 40), (10, 0, 80, 40)]
    # refusals: written as far as the files were judged
    for mode, anchor, wins in ((3, 0, NARROW), (0, 2, NARROW), (0, 0, None)):
        keep, bad = placement(mode, anchor, wins)
        assert file_call(two, bad, tensor=tensor) == (EINVAL, [(-7, 0, 0, 0, 0)] * 2, [UNSET] * 2)
    keep, bad = placement(windows=[NARROW[1], (95, 0, 10, 40)])
    assert file_call(two, bad, tensor=tensor) == (EINVAL, [(1, 0, 0, 200, 40), (-7, 0, 0, 0, 0)], [NARROW[1], UNSET])
    keep, bad = placement(windows=[(0, 0, 0, 1), NARROW[1]])
    assert file_call(two, bad, tensor=tensor)[0] == EINVAL
    st, views, windows = file_call([wide, wide[:30], wide], narrow_three(), tensor=tensor)
    assert st not in (OK, ENOSUP) and windows == [NARROW[1], UNSET, UNSET] and views[1][0] == -7
    assert file_call([F.lossless_marker(wide)], bad, tensor=tensor)[0] == ENOSUP                              # the file's verdict first
    keep, none = placement(windows=None)
    assert file_call([], none, tensor=tensor)[0] == OK


def narrow_three():
    keep, p = placement(windows=[NARROW[1]] * 3)
    narrow_three.keep = keep
    return p
