"""The status of a refused call, entry point by entry point -- no GPU.  Every entry point that takes a context and device
pointers is called with a NULL context (bind then returns EINVAL before any HIP call) under a small table of argument sets,
one of them valid and the others wrong in one more way.  Most entry points look at the context first and so answer EINVAL
whatever else is wrong; the view, resized and resize calls judge everything else first, and there the layout's verdict
(ENOSUP for 12 bits) comes through.  The expected statuses are not reasoned out: they are what the library returned before
the argument handling of the C layer (jpeg_amd/csrc/capi*.hip) was gathered into one record, so a change of the order of
checks shows here.  The six resample calls are there twice, without a filter argument and as their *_filter_* forms with the
bilinear filter: the first forward to the second.  A second table holds calls that are wrong twice, in the view (ENOSUP) and
in the target (EINVAL), and calls with an unknown filter: there the order between the checks shows, and what an empty call
answers without a context.  The oriented, placed, warped, colour and projected forms and the file calls
(jpeg_amd_decompress_*_mixed, on one small in-memory file) stand in both tables as well; the second table holds them with a
per-image argument that is wrong (an orientation of 9, an unknown placement mode, a non-finite matrix, a homography whose
denominator changes sign on the canvas, a colour with lo > hi) next to a bad target, and again on a 12-bit image: the order
between the image, the per-image argument and the target shows there."""
import ctypes as C
import functools

import numpy as np
import pytest

from _calls import c_layout
from _files import synthetic_file
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, -1, -5                                     # JPEG_AMD_OK, _EINVAL, _ENOSUP, as literals
CASES = ("valid", "null layout", "12-bit layout", "two planes", "n_images = -1", "bad denominator or empty region")


class Args:
    """One argument set: a 16 x 16 4:2:0 layout and made-up non-null pointers (a host buffer stands in for the device's:
    a refused call reads none of them), then the case's one change."""

    def __init__(self, case):
        f420 = [(2, 2), (1, 1), (1, 1)]
        self.layout = c_layout(16, 16, f420[:2] if case == "two planes" else f420, precision=12 if case == "12-bit layout" else 8)
        self.L = None if case == "null layout" else C.byref(self.layout)
        self.precision = self.layout.precision
        self.nplanes = self.layout.nplanes
        self.n = -1 if case == "n_images = -1" else 1
        bad = case == "bad denominator or empty region"
        self.denom = 3 if bad else 2
        self.buf = np.zeros(1024, np.uint16)
        self.p = self.buf.ctypes.data                              # any pointer: tables, pixels, planes
        self.pp = _lib.ptr_array([self.p] * 4)
        self.sz = _lib.size_array([1024] * 4)
        self.region = _lib.Region(0, 0, 0 if bad else 4, 4)
        self.view = _lib.View(self.denom, _lib.Region(0, 0, 4, 4))
        self.extent = _lib.Extent(4, 4)
        self.out = (8, 8)                                          # the canvas of the later forms
        self.r, self.v, self.e = C.byref(self.region), C.byref(self.view), C.byref(self.extent)
        self.spec = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
        self.s = C.byref(self.spec)
        # the mixed calls: the layout lies inside the image, so "null layout" is a null image array there
        self.image = image(self.layout, self.p)
        self.im = None if case == "null layout" else C.byref(self.image)
        # the per-image arguments of the later forms, all valid: an orientation, a placement, a warp with an affine and a
        # projective matrix, a colour
        self.orient = np.array([6], np.uint8)
        self.o = self.orient.ctypes.data
        self.placement = _lib.Placement(_lib.PLACE_FIT, _lib.ANCHOR_CENTRE, None, (C.c_uint8 * 3)(1, 2, 3), 0)
        self.pl = C.byref(self.placement)
        self.warp = _lib.Warp(_lib.EDGE_FILL, (C.c_uint8 * 3)(1, 2, 3))
        self.w = C.byref(self.warp)
        self.matrix6 = np.array([0.5, 0, 0, 0, 0.5, 0], np.float32)
        self.matrix9 = np.array([0.5, 0, 0, 0, 0.5, 0, 0, 0, 1], np.float32)
        self.m6, self.m9 = self.matrix6.ctypes.data, self.matrix9.ctypes.data
        self.colour_matrix = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
        self.colour = _lib.Colour(self.colour_matrix.ctypes.data, 0.0, 255.0)
        self.c = C.byref(self.colour)
        # the file calls: one file of 16 x 16, 4:2:0 ("null layout": no file array)
        self.file = small_file()
        self.jpeg = (C.c_void_p * 1)(self.file.ctypes.data)
        self.nbytes = (C.c_size_t * 1)(self.file.size)
        self.jp = None if case == "null layout" else self.jpeg


@functools.lru_cache(maxsize=None)
def small_file():
    return synthetic_file("420", (16, 16), 1)[0]


def image(layout, p):
    """struct jpeg_amd_image of `layout` with the pointer p for every plane and for its two tables."""
    im = _lib.Image()
    im.layout = layout
    for c in range(layout.nplanes):
        im.d_coef[c] = p
    im.d_quanta, im.ntables = p, 2
    return im


def files(a):
    """The leading arguments of a file call behind the context."""
    return a.jp, a.nbytes, a.n, 1, 0, RGB


RGB = _lib.COLOR_RGB8
BILINEAR = _lib.FILTER_BILINEAR
UNKNOWN_FILTER = 7
# name -> the arguments behind the context, from an Args
CALLS = {
    "jpeg_amd_decode_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.p, 768),
    "jpeg_amd_decode": lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.p),
    "jpeg_amd_decode_region_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.r, a.p, 768),
    "jpeg_amd_decode_region": lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.r, a.p),
    "jpeg_amd_decode_scaled_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.denom, a.p, 768),
    "jpeg_amd_decode_scaled": lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.denom, a.p),
    "jpeg_amd_decode_view_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, a.p, 768),
    "jpeg_amd_decode_view": lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.v, a.p),
    "jpeg_amd_decode_resized_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, a.p, 768),
    "jpeg_amd_decode_resized": lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.v, 8, 8, a.p),
    "jpeg_amd_resize_batch": lambda a: (a.n, a.p, 48, a.e, 8, 8, a.p, 192),
    "jpeg_amd_resize_tensor_batch": lambda a: (a.n, a.p, 48, a.e, 8, 8, a.s, None, a.p, 192),
    "jpeg_amd_decode_tensor_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, a.s, None, a.p, 192),
    "jpeg_amd_decode_tensor": lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.v, 8, 8, a.s, 0, a.p),
    "jpeg_amd_decode_view_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, a.p, 768),
    "jpeg_amd_decode_resized_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, 8, 8, a.p, 768),
    "jpeg_amd_decode_tensor_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, 8, 8, a.s, None, a.p, 192),
    # ... and with the filter named: the argument sets of the six calls without one, the bilinear filter
    "jpeg_amd_resize_filter_batch": lambda a: (a.n, a.p, 48, a.e, 8, 8, BILINEAR, a.p, 192),
    "jpeg_amd_resize_filter_tensor_batch": lambda a: (a.n, a.p, 48, a.e, 8, 8, BILINEAR, a.s, None, a.p, 192),
    "jpeg_amd_decode_resized_filter_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, BILINEAR, a.p, 768),
    "jpeg_amd_decode_tensor_filter_batch":
        lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, BILINEAR, a.s, None, a.p, 192),
    "jpeg_amd_decode_resized_filter_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, 8, 8, BILINEAR, a.p, 768),
    "jpeg_amd_decode_tensor_filter_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, 8, 8, BILINEAR, a.s, None, a.p, 192),
    # ... with an orientation per image, a placement, an affine map, a colour and a homography
    "jpeg_amd_resize_oriented_batch": lambda a: (a.n, a.p, 48, a.e, *a.out, BILINEAR, a.o, a.p, 192),
    "jpeg_amd_resize_oriented_tensor_batch": lambda a: (a.n, a.p, 48, a.e, *a.out, BILINEAR, a.s, None, a.o, a.p, 192),
    "jpeg_amd_decode_resized_oriented_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, *a.out, BILINEAR, a.o, a.p, 768),
    "jpeg_amd_decode_tensor_oriented_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, *a.out, BILINEAR, a.s, None, a.o, a.p, 192),
    "jpeg_amd_resize_placed_batch": lambda a: (a.n, a.p, 48, a.e, *a.out, BILINEAR, a.o, a.pl, None, a.p, 192),
    "jpeg_amd_resize_placed_tensor_batch": lambda a: (a.n, a.p, 48, a.e, *a.out, BILINEAR, a.s, None, a.o, a.pl, None, a.p, 192),
    "jpeg_amd_decode_resized_placed_mixed": lambda a: (a.n, a.im, 0, RGB, a.v, *a.out, BILINEAR, a.o, a.pl, None, a.p, 768),
    "jpeg_amd_decode_tensor_placed_mixed":
        lambda a: (a.n, a.im, 0, RGB, a.v, *a.out, BILINEAR, a.s, None, a.o, a.pl, None, a.p, 192),
    "jpeg_amd_warp_batch": lambda a: (a.n, a.p, 48, a.e, a.m6, a.w, *a.out, a.p, 192),
    "jpeg_amd_warp_tensor_batch": lambda a: (a.n, a.p, 48, a.e, a.m6, a.w, *a.out, a.s, None, a.p, 192),
    "jpeg_amd_decode_warped_mixed": lambda a: (a.n, a.im, 0, RGB, a.o, a.m6, a.w, *a.out, None, None, a.p, 768),
    "jpeg_amd_decode_tensor_warped_mixed": lambda a: (a.n, a.im, 0, RGB, a.o, a.m6, a.w, *a.out, a.s, None, None, None, a.p, 192),
    "jpeg_amd_resize_colour_tensor_batch":
        lambda a: (a.n, a.p, 48, a.e, *a.out, BILINEAR, a.s, None, a.o, a.pl, None, a.c, a.p, 192),
    "jpeg_amd_decode_tensor_colour_mixed":
        lambda a: (a.n, a.im, 0, RGB, a.v, *a.out, BILINEAR, a.s, None, a.o, a.pl, None, a.c, a.p, 192),
    "jpeg_amd_warp_colour_tensor_batch": lambda a: (a.n, a.p, 48, a.e, a.m6, a.w, *a.out, a.s, None, a.c, a.p, 192),
    "jpeg_amd_decode_tensor_warped_colour_mixed":
        lambda a: (a.n, a.im, 0, RGB, a.o, a.m6, a.w, *a.out, a.s, None, None, None, a.c, a.p, 192),
    "jpeg_amd_project_batch": lambda a: (a.n, a.p, 48, a.e, a.m9, a.w, *a.out, a.p, 192),
    "jpeg_amd_project_tensor_batch": lambda a: (a.n, a.p, 48, a.e, a.m9, a.w, *a.out, a.s, None, a.c, a.p, 192),
    "jpeg_amd_decode_projected_mixed": lambda a: (a.n, a.im, 0, RGB, a.o, a.m9, a.w, *a.out, None, None, a.p, 768),
    "jpeg_amd_decode_tensor_projected_mixed":
        lambda a: (a.n, a.im, 0, RGB, a.o, a.m9, a.w, *a.out, a.s, None, None, None, a.c, a.p, 192),
    # the file calls: (files, sizes, n, one thread, centred, RGB), then the call's own; "empty region": the source rectangle's
    "jpeg_amd_decompress_tensor_mixed": lambda a: (*files(a), a.r, *a.out, BILINEAR, a.s, None, a.p, 192, None, None),
    "jpeg_amd_decompress_resized_mixed": lambda a: (*files(a), a.r, *a.out, BILINEAR, a.p, 192, None, None),
    "jpeg_amd_decompress_tensor_oriented_mixed":
        lambda a: (*files(a), a.r, *a.out, BILINEAR, a.s, None, a.o, a.p, 192, None, None, None),
    "jpeg_amd_decompress_resized_oriented_mixed": lambda a: (*files(a), a.r, *a.out, BILINEAR, a.o, a.p, 192, None, None, None),
    "jpeg_amd_decompress_tensor_placed_mixed":
        lambda a: (*files(a), a.r, *a.out, BILINEAR, a.s, None, a.o, a.pl, None, a.p, 192, None, None, None),
    "jpeg_amd_decompress_resized_placed_mixed":
        lambda a: (*files(a), a.r, *a.out, BILINEAR, a.o, a.pl, None, a.p, 192, None, None, None),
    "jpeg_amd_decompress_resized_warped_mixed": lambda a: (*files(a), a.o, a.m6, a.w, *a.out, a.p, 192, None, None, None, None),
    "jpeg_amd_decompress_tensor_warped_mixed":
        lambda a: (*files(a), a.o, a.m6, a.w, *a.out, a.s, None, a.p, 192, None, None, None, None),
    "jpeg_amd_decompress_tensor_colour_mixed":
        lambda a: (*files(a), a.r, *a.out, BILINEAR, a.s, None, a.o, a.pl, None, a.c, a.p, 192, None, None, None),
    "jpeg_amd_decompress_tensor_warped_colour_mixed":
        lambda a: (*files(a), a.o, a.m6, a.w, *a.out, a.s, None, a.c, a.p, 192, None, None, None, None),
    "jpeg_amd_decompress_resized_projected_mixed": lambda a: (*files(a), a.o, a.m9, a.w, *a.out, a.p, 192, None, None, None, None),
    "jpeg_amd_decompress_tensor_projected_mixed":
        lambda a: (*files(a), a.o, a.m9, a.w, *a.out, a.s, None, a.c, a.p, 192, None, None, None, None),
    "jpeg_amd_encode_batch": lambda a: (a.L, a.n, a.p, 768, RGB, a.p, 64, 2, a.pp, a.sz),
    "jpeg_amd_encode": lambda a: (a.L, a.p, RGB, a.p, 2, a.pp),
    "jpeg_amd_spectral_rectangular_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, 2, 0, a.p, 768),
    "jpeg_amd_spectral_rectangular": lambda a: (a.L, a.pp, a.p, 2, 0, a.p),
    "jpeg_amd_rectangular_spectral_batch": lambda a: (a.L, a.n, a.p, 768, a.p, 64, 2, a.pp, a.sz),
    "jpeg_amd_rectangular_spectral": lambda a: (a.L, a.p, a.p, 2, a.pp),
    "jpeg_amd_spectral_transform_batch": lambda a: (a.L, a.n, 0, a.r, a.pp, a.sz, a.p, 64, 2, None, a.pp, a.sz, None),
    "jpeg_amd_spectral_transform": lambda a: (a.L, 0, a.r, a.pp, a.p, 2, None, a.pp),
    "jpeg_amd_spectral_reduce_batch": lambda a: (a.L, a.n, a.denom, a.pp, a.sz, a.p, 64, 2, None, a.pp, a.sz),
    "jpeg_amd_spectral_reduce": lambda a: (a.L, a.denom, a.pp, a.p, 2, None, a.pp),
    "jpeg_amd_spectral_expand_batch": lambda a: (a.L, a.n, a.p, 64, a.p, 64, None, a.pp, a.sz),
    "jpeg_amd_spectral_sparsify_batch": lambda a: (a.L, a.n, a.pp, a.sz, a.p, 64, a.p, 64, 64, a.p),
    # the stages
    "jpeg_amd_idct_plane": lambda a: (a.p, 2, 2, a.p, a.precision, a.p),
    "jpeg_amd_spectral_idct": lambda a: (a.L, a.pp, a.p, 2, a.pp),
    "jpeg_amd_spectral_idct_scaled": lambda a: (a.L, a.pp, a.p, 2, a.denom, a.pp),
    "jpeg_amd_planar_interleaved": lambda a: (a.L, a.pp, 0, a.p),
    "jpeg_amd_rectangular_unpack": lambda a: (a.p, 256, a.nplanes, RGB, a.p),
    "jpeg_amd_rectangular_pack": lambda a: (a.p, 256, a.nplanes, RGB, a.p),
    "jpeg_amd_rectangular_decomposed": lambda a: (a.L, a.p, a.pp),
    "jpeg_amd_fdct_plane": lambda a: (a.p, 2, 2, a.p, a.precision, a.p),
    "jpeg_amd_planar_fdct": lambda a: (a.L, a.pp, a.p, 2, a.pp),
}

# The statuses of the library before the change, in the order of CASES; a case that changes no argument of the call is left out
# of it (None).
_ = None
BIND_FIRST = (EINVAL,) * 6
EXPECTED = {
    "jpeg_amd_decode_batch": (EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, _),
    "jpeg_amd_decode": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_decode_region_batch": BIND_FIRST,
    "jpeg_amd_decode_region": (EINVAL, EINVAL, EINVAL, EINVAL, _, EINVAL),
    "jpeg_amd_decode_scaled_batch": BIND_FIRST,
    "jpeg_amd_decode_scaled": (EINVAL, EINVAL, EINVAL, EINVAL, _, EINVAL),
    "jpeg_amd_decode_view_batch": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_view": (EINVAL, EINVAL, ENOSUP, EINVAL, _, EINVAL),
    "jpeg_amd_decode_resized_batch": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_resized": (EINVAL, EINVAL, ENOSUP, EINVAL, _, EINVAL),
    "jpeg_amd_resize_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_resize_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_tensor_batch": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_tensor": (EINVAL, EINVAL, ENOSUP, EINVAL, _, EINVAL),
    "jpeg_amd_decode_view_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_resized_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_tensor_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_resize_filter_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_resize_filter_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_resized_filter_batch": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_tensor_filter_batch": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_resized_filter_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_tensor_filter_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_resize_oriented_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_resize_oriented_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_resized_oriented_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_tensor_oriented_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_resize_placed_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_resize_placed_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_resized_placed_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_decode_tensor_placed_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_warp_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_warp_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_warped_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, _),
    "jpeg_amd_decode_tensor_warped_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, _),
    "jpeg_amd_resize_colour_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_tensor_colour_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, EINVAL),
    "jpeg_amd_warp_colour_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_tensor_warped_colour_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, _),
    "jpeg_amd_project_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_project_tensor_batch": (EINVAL, _, _, _, EINVAL, _),
    "jpeg_amd_decode_projected_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, _),
    "jpeg_amd_decode_tensor_projected_mixed": (EINVAL, EINVAL, ENOSUP, EINVAL, EINVAL, _),
    "jpeg_amd_decompress_tensor_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_resized_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_tensor_oriented_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_resized_oriented_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_tensor_placed_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_resized_placed_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_resized_warped_mixed": (EINVAL, EINVAL, _, _, EINVAL, _),
    "jpeg_amd_decompress_tensor_warped_mixed": (EINVAL, EINVAL, _, _, EINVAL, _),
    "jpeg_amd_decompress_tensor_colour_mixed": (EINVAL, EINVAL, _, _, EINVAL, EINVAL),
    "jpeg_amd_decompress_tensor_warped_colour_mixed": (EINVAL, EINVAL, _, _, EINVAL, _),
    "jpeg_amd_decompress_resized_projected_mixed": (EINVAL, EINVAL, _, _, EINVAL, _),
    "jpeg_amd_decompress_tensor_projected_mixed": (EINVAL, EINVAL, _, _, EINVAL, _),
    "jpeg_amd_encode_batch": (EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, _),
    "jpeg_amd_encode": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_spectral_rectangular_batch": (EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, _),
    "jpeg_amd_spectral_rectangular": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_rectangular_spectral_batch": (EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, _),
    "jpeg_amd_rectangular_spectral": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_spectral_transform_batch": BIND_FIRST,
    "jpeg_amd_spectral_transform": (EINVAL, EINVAL, EINVAL, EINVAL, _, EINVAL),
    "jpeg_amd_spectral_reduce_batch": BIND_FIRST,
    "jpeg_amd_spectral_reduce": (EINVAL, EINVAL, EINVAL, EINVAL, _, EINVAL),
    "jpeg_amd_spectral_expand_batch": (EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, _),
    "jpeg_amd_spectral_sparsify_batch": (EINVAL, EINVAL, EINVAL, EINVAL, EINVAL, _),
    "jpeg_amd_idct_plane": (EINVAL, _, EINVAL, _, _, _),
    "jpeg_amd_spectral_idct": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_spectral_idct_scaled": (EINVAL, EINVAL, EINVAL, EINVAL, _, EINVAL),
    "jpeg_amd_planar_interleaved": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_rectangular_unpack": (EINVAL, _, _, EINVAL, _, _),
    "jpeg_amd_rectangular_pack": (EINVAL, _, _, EINVAL, _, _),
    "jpeg_amd_rectangular_decomposed": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
    "jpeg_amd_fdct_plane": (EINVAL, _, EINVAL, _, _, _),
    "jpeg_amd_planar_fdct": (EINVAL, EINVAL, EINVAL, EINVAL, _, _),
}


assert set(CALLS) == set(EXPECTED)


def statuses(name):
    """The status of `name` with a NULL context under every case that applies to it."""
    fn = getattr(_lib.lib(), name)
    out = []
    for case, want in zip(CASES, EXPECTED[name]):
        a = Args(case)
        out.append(None if want is None else fn(None, *CALLS[name](a)))
    return tuple(out)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_status_of_a_refused_call(name):
    assert statuses(name) == EXPECTED[name]



def two_images(first_12_bit):
    """(keep, image array, view array) of two images, one of them of 12 bits: the first, or the second behind a valid one."""
    a = [Args("12-bit layout" if (i == 0) == first_12_bit else "valid") for i in range(2)]
    images = (_lib.Image * 2)(a[0].image, a[1].image)
    views = (_lib.View * 2)(a[0].view, a[1].view)
    return a, images, views


def mixed_twice(name, first_12_bit):
    """The mixed resized or tensor call on two_images with out_w = 0."""
    a, images, views = two_images(first_12_bit)
    tail = (a[0].s, None, a[0].p, 192) if "tensor" in name else (a[0].p, 768)
    return getattr(_lib.lib(), name)(None, 2, images, 0, RGB, views, 0, 8, *tail)


def call(name, case, args):
    a = Args(case)
    return getattr(_lib.lib(), name)(None, *args(a))


def orientation_9(a):
    a.orient[0] = 9


def unknown_placement_mode(a):
    a.placement.mode = 7


def non_finite_matrix(a):
    a.matrix6[1] = np.inf


def denominator_changes_sign(a):
    a.matrix9[7] = -1.0                                            # 1 - cy: positive on the canvas's top edge, negative on its bottom


def colour_lo_above_hi(a):
    a.colour.lo = 300.0


def wrong_with_bad_target(name, spoil, case="valid"):
    """`name` with its per-image argument spoilt and a canvas of 0 x 8, on the image of `case`."""
    a = Args(case)
    a.out = (0, 8)
    spoil(a)
    return getattr(_lib.lib(), name)(None, *CALLS[name](a))


# What is spoilt -> the calls that take it: over bytes in memory, over mixed images (those again on a 12-bit image), over files.
SPOILT = {
    "an orientation of 9":
        (orientation_9, "jpeg_amd_resize_oriented_tensor_batch", "jpeg_amd_decode_tensor_oriented_mixed",
         "jpeg_amd_decompress_tensor_oriented_mixed"),
    "an unknown placement mode":
        (unknown_placement_mode, "jpeg_amd_resize_placed_tensor_batch", "jpeg_amd_decode_tensor_placed_mixed",
         "jpeg_amd_decompress_tensor_placed_mixed"),
    "a non-finite warp matrix":
        (non_finite_matrix, "jpeg_amd_warp_tensor_batch", "jpeg_amd_decode_tensor_warped_mixed",
         "jpeg_amd_decompress_tensor_warped_mixed"),
    "a denominator that changes sign":
        (denominator_changes_sign, "jpeg_amd_project_tensor_batch", "jpeg_amd_decode_tensor_projected_mixed",
         "jpeg_amd_decompress_tensor_projected_mixed"),
    "a colour with lo > hi":
        (colour_lo_above_hi, "jpeg_amd_resize_colour_tensor_batch", "jpeg_amd_decode_tensor_colour_mixed",
         "jpeg_amd_decompress_tensor_colour_mixed"),
}
# ... and the statuses of the library before the change: (bytes, mixed, files, mixed on a 12-bit image)
SPOILT_EXPECTED = {
    "an orientation of 9": (EINVAL, EINVAL, EINVAL, ENOSUP),
    "an unknown placement mode": (EINVAL, EINVAL, EINVAL, ENOSUP),
    "a non-finite warp matrix": (EINVAL, EINVAL, EINVAL, EINVAL),
    "a denominator that changes sign": (EINVAL, EINVAL, EINVAL, EINVAL),
    "a colour with lo > hi": (EINVAL, EINVAL, EINVAL, ENOSUP),
}


def spoilt_rows():
    rows = {}
    for what, (spoil, in_memory, mixed, of_files) in SPOILT.items():
        want = SPOILT_EXPECTED[what]
        for name, case, status in ((in_memory, "valid", want[0]), (mixed, "valid", want[1]), (of_files, "valid", want[2]),
                                   (mixed, T12, want[3])):
            title = f"{name[len('jpeg_amd_'):]}, {what} and out_w = 0" + (", 12 bits" if case == T12 else "")
            rows[title] = (lambda name=name, spoil=spoil, case=case: wrong_with_bad_target(name, spoil, case), status)
    return rows


# Calls that are wrong twice, and empty calls: description -> (the call, the status of the library before the change).
T12 = "12-bit layout"
TWICE = {
    **spoilt_rows(),
    "resized batch, 12 bits and out_w = 0":
        (lambda: call("jpeg_amd_decode_resized_batch", T12, lambda a: (a.L, 1, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 0, 8, a.p, 768)), ENOSUP),
    "tensor batch, 12 bits and out_w = 0":
        (lambda: call("jpeg_amd_decode_tensor_batch", T12,
                      lambda a: (a.L, 1, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 0, 8, a.s, None, a.p, 192)), ENOSUP),
    "resized, 12 bits and out_w = 0":
        (lambda: call("jpeg_amd_decode_resized", T12, lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.v, 0, 8, a.p)), ENOSUP),
    "tensor, 12 bits and out_w = 0":
        (lambda: call("jpeg_amd_decode_tensor", T12, lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.v, 0, 8, a.s, 0, a.p)), ENOSUP),
    "tensor batch, 12 bits and a null spec":
        (lambda: call("jpeg_amd_decode_tensor_batch", T12,
                      lambda a: (a.L, 1, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, None, None, a.p, 192)), ENOSUP),
    "tensor, 12 bits and a null spec":
        (lambda: call("jpeg_amd_decode_tensor", T12, lambda a: (a.L, a.pp, a.p, 2, 0, RGB, a.v, 8, 8, None, 0, a.p)), ENOSUP),
    "resized mixed, image 0 of 12 bits and out_w = 0": (lambda: mixed_twice("jpeg_amd_decode_resized_mixed", True), ENOSUP),
    "resized mixed, image 1 of 12 bits and out_w = 0": (lambda: mixed_twice("jpeg_amd_decode_resized_mixed", False), EINVAL),
    "tensor mixed, image 0 of 12 bits and out_w = 0": (lambda: mixed_twice("jpeg_amd_decode_tensor_mixed", True), ENOSUP),
    "tensor mixed, image 1 of 12 bits and out_w = 0": (lambda: mixed_twice("jpeg_amd_decode_tensor_mixed", False), EINVAL),
    "resize batch, empty":
        (lambda: call("jpeg_amd_resize_batch", "valid", lambda a: (0, a.p, 48, a.e, 8, 8, a.p, 192)), EINVAL),
    "resize tensor batch, empty":
        (lambda: call("jpeg_amd_resize_tensor_batch", "valid", lambda a: (0, a.p, 48, a.e, 8, 8, a.s, None, a.p, 192)), EINVAL),
    "resized batch, empty":
        (lambda: call("jpeg_amd_decode_resized_batch", "valid", lambda a: (a.L, 0, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, a.p, 768)), EINVAL),
    "tensor batch, empty":
        (lambda: call("jpeg_amd_decode_tensor_batch", "valid",
                      lambda a: (a.L, 0, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, a.s, None, a.p, 192)), EINVAL),
    # an unknown filter: the target's to refuse, behind the view (a 12-bit layout comes first) and with no image at all
    "resize filter batch, unknown filter":
        (lambda: call("jpeg_amd_resize_filter_batch", "valid", lambda a: (1, a.p, 48, a.e, 8, 8, UNKNOWN_FILTER, a.p, 192)), EINVAL),
    "resize filter batch, unknown filter, empty":
        (lambda: call("jpeg_amd_resize_filter_batch", "valid", lambda a: (0, a.p, 48, a.e, 8, 8, UNKNOWN_FILTER, a.p, 192)), EINVAL),
    "resize filter tensor batch, unknown filter":
        (lambda: call("jpeg_amd_resize_filter_tensor_batch", "valid",
                      lambda a: (1, a.p, 48, a.e, 8, 8, UNKNOWN_FILTER, a.s, None, a.p, 192)), EINVAL),
    "resized filter batch, unknown filter":
        (lambda: call("jpeg_amd_decode_resized_filter_batch", "valid",
                      lambda a: (a.L, 1, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, UNKNOWN_FILTER, a.p, 768)), EINVAL),
    "resized filter batch, 12 bits and an unknown filter":
        (lambda: call("jpeg_amd_decode_resized_filter_batch", T12,
                      lambda a: (a.L, 1, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, UNKNOWN_FILTER, a.p, 768)), ENOSUP),
    "tensor filter batch, unknown filter":
        (lambda: call("jpeg_amd_decode_tensor_filter_batch", "valid",
                      lambda a: (a.L, 1, a.pp, a.sz, a.p, 64, 2, 0, RGB, a.v, 8, 8, UNKNOWN_FILTER, a.s, None, a.p, 192)), EINVAL),
    "resized filter mixed, unknown filter":
        (lambda: call("jpeg_amd_decode_resized_filter_mixed", "valid", lambda a: (1, a.im, 0, RGB, a.v, 8, 8, UNKNOWN_FILTER, a.p, 768)), EINVAL),
    "resized filter mixed, unknown filter, empty":
        (lambda: call("jpeg_amd_decode_resized_filter_mixed", "valid", lambda a: (0, a.im, 0, RGB, a.v, 8, 8, UNKNOWN_FILTER, a.p, 768)), EINVAL),
    "tensor filter mixed, unknown filter":
        (lambda: call("jpeg_amd_decode_tensor_filter_mixed", "valid",
                      lambda a: (1, a.im, 0, RGB, a.v, 8, 8, UNKNOWN_FILTER, a.s, None, a.p, 192)), EINVAL),
    "view mixed, empty":
        (lambda: call("jpeg_amd_decode_view_mixed", "valid", lambda a: (0, a.im, 0, RGB, a.v, a.p, 768)), OK),
    "resized mixed, empty":
        (lambda: call("jpeg_amd_decode_resized_mixed", "valid", lambda a: (0, a.im, 0, RGB, a.v, 8, 8, a.p, 768)), OK),
    "tensor mixed, empty":
        (lambda: call("jpeg_amd_decode_tensor_mixed", "valid", lambda a: (0, a.im, 0, RGB, a.v, 8, 8, a.s, None, a.p, 192)), OK),
}


@pytest.mark.parametrize("what", sorted(TWICE))
def test_status_of_a_call_that_is_wrong_twice_or_empty(what):
    run, want = TWICE[what]
    assert run() == want
