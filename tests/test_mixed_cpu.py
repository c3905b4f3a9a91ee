"""The refusals of the mixed calls (jpeg_amd_decode_view_mixed, _resized_mixed, _tensor_mixed) -- no GPU.  Every call has a
NULL context: the calls judge every other argument first and the context last, so a call that is right in everything else
answers the context's EINVAL, and one that is wrong answers for its first offending image, each image judged against its own
layout.  A host buffer stands in for the device's: a refused call reads none of it."""
import ctypes as C

import numpy as np
import pytest

from _calls import FUSED, c_layout
from _mixed import resized_mixed, tensor_mixed, view_mixed
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, -1, -5
RGB = _lib.COLOR_RGB8
BUF = np.zeros(1024, np.uint16)
P = BUF.ctypes.data                                           # any pointer: planes, tables, pixels
SPEC = _lib.TensorSpec(_lib.F16, _lib.TENSOR_CHW, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))


def image(w, h, name, ptrs=None, ntables=None, quanta=P, **kw):
    L = c_layout(w, h, FUSED[name], **kw)
    return L, [P] * L.nplanes if ptrs is None else ptrs, quanta, (2 if L.nplanes == 3 else 1) if ntables is None else ntables


# two images of different geometry: at denominator 2 they are 32 x 32 and 8 x 8
GOOD = [image(64, 64, "420"), image(16, 16, "444")]
VIEWS = [(2, (0, 0, 20, 20)), (2, (1, 1, 7, 7))]
STRIDE = 3 * 20 * 20


def calls(images=GOOD, views=VIEWS, n=None, stride=STRIDE, out=P, color=RGB):
    """The status of each of the three calls."""
    return (view_mixed(None, images, 0, color, views, out, stride, n),
            resized_mixed(None, images, 0, color, views, 8, 8, out, 3 * 8 * 8, n),
            tensor_mixed(None, images, 0, color, views, 8, 8, SPEC, None, out, 3 * 8 * 8, n))


def test_a_valid_call_reaches_the_context_check():
    assert calls() == (EINVAL,) * 3                           # the NULL context's


def test_an_empty_call_is_ok():
    assert calls(n=0) == (OK,) * 3
    assert _lib.lib().jpeg_amd_decode_view_mixed(None, 0, None, 0, RGB, None, None, 0) == OK
    assert resized_mixed(None, GOOD, 0, RGB, VIEWS, 0, 8, P, 192, n=0) == EINVAL     # ... but its target is still judged


def test_a_twelve_bit_image_shows_that_the_context_comes_last():
    """ENOSUP can only come from the image: the calls judged it before they looked at the NULL context."""
    for at in (0, 1):
        images = list(GOOD)
        images[at] = image(64, 64, "420", precision=12) if at == 0 else image(16, 16, "444", precision=12)
        assert calls(images) == (ENOSUP,) * 3, at


# a 12-bit image behind the others: a call that is right up to it answers ENOSUP, not the context's EINVAL
LAST = image(32, 32, "y8", precision=12)
LAST_VIEW = (1, (0, 0, 4, 4))


def test_each_view_is_judged_against_its_own_image():
    def status(second):
        return calls(GOOD + [LAST], [VIEWS[0], second, LAST_VIEW])

    assert status(VIEWS[1]) == (ENOSUP,) * 3
    assert status(VIEWS[0]) == (EINVAL,) * 3                  # inside image 0's 32 x 32, outside image 1's 8 x 8
    assert status((2, (0, 0, 8, 8))) == (ENOSUP,) * 3         # the whole of image 1 at denominator 2
    assert status((2, (0, 0, 9, 8))) == (EINVAL,) * 3         # one pixel past W' = 8
    assert status((1, (0, 0, 16, 16))) == (ENOSUP,) * 3       # ... which denominator 1 has


@pytest.mark.parametrize("what", ["null plane pointer", "bad denominator", "ntables below qi", "empty rectangle", "null tables",
                                  "two planes"])
def test_the_first_offending_image_decides(what):
    images, views = list(GOOD), list(VIEWS)
    if what == "null plane pointer":
        images[1] = image(16, 16, "444", ptrs=[P, None, P])
    elif what == "bad denominator":
        views[1] = (3, (1, 1, 7, 7))
    elif what == "ntables below qi":
        images[1] = image(16, 16, "444", ntables=1)              # planes 1 and 2 name table 1
    elif what == "empty rectangle":
        views[1] = (2, (1, 1, 0, 7))
    elif what == "null tables":
        images[1] = image(16, 16, "444", quanta=None)
    else:
        L = c_layout(16, 16, FUSED["444"][:2])
        images[1] = (L, [P, P], P, 2)
    assert calls(images + [LAST], views + [LAST_VIEW]) == (EINVAL,) * 3    # image 1 before image 2
    assert calls([LAST] + images, [LAST_VIEW] + views) == (ENOSUP,) * 3    # image 0 before image 2


def test_the_arguments_of_the_call():
    from _calls import c_views
    from _mixed import c_images
    images, views = GOOD + [LAST], VIEWS + [LAST_VIEW]           # valid up to the last image: ENOSUP
    assert calls(images, views) == (ENOSUP,) * 3
    assert calls(images, views, n=-1) == (EINVAL,) * 3
    assert calls(images, views, n=65536) == (EINVAL,) * 3
    lib = _lib.lib()
    assert lib.jpeg_amd_decode_view_mixed(None, 3, None, 0, RGB, c_views(views), P, STRIDE) == EINVAL
    assert lib.jpeg_amd_decode_view_mixed(None, 3, c_images(images), 0, RGB, None, P, STRIDE) == EINVAL
    assert lib.jpeg_amd_decode_resized_mixed(None, 3, None, 0, RGB, c_views(views), 8, 8, P, 192) == EINVAL
    assert lib.jpeg_amd_decode_tensor_mixed(None, 3, c_images(images), 0, RGB, None, 8, 8, C.byref(SPEC), None, P, 192) == EINVAL
    # the output: a null pointer, a stride below the largest view (the view call) or below the target (the others), a target
    # of no pixels, a tensor that is not aligned to its element, a colour that is none
    assert calls(images, views, out=None) == (EINVAL,) * 3
    assert view_mixed(None, images, 0, RGB, views, P, STRIDE - 1) == EINVAL
    assert resized_mixed(None, images, 0, RGB, views, 8, 8, P, 191) == EINVAL
    assert tensor_mixed(None, images, 0, RGB, views, 8, 8, SPEC, None, P, 191) == EINVAL
    assert resized_mixed(None, images, 0, RGB, views, 0, 8, P, 192) == EINVAL
    assert tensor_mixed(None, images, 0, RGB, views, 8, 8, SPEC, None, P + 1, 192) == EINVAL
    assert calls(images, views, color=7) == (EINVAL,) * 3
    # one image: any stride, as in the uniform calls
    assert view_mixed(None, [LAST], 0, RGB, [LAST_VIEW], P, 0) == ENOSUP
