"""What the tests of the mixed calls (jpeg_amd_decode_view_mixed, _resized_mixed, _tensor_mixed) share: the array of
struct jpeg_amd_image and the three calls.  Importing this needs no GPU and no torch."""
import ctypes as C

from _calls import c_views
from jpeg_amd import _lib


def c_images(images):
    """images: (c layout, plane pointers, table pointer, ntables) per image."""
    arr = (_lib.Image * max(len(images), 1))()
    for i, (L, ptrs, quanta, ntables) in enumerate(images):
        arr[i].layout = L
        for p, ptr in enumerate(ptrs):
            arr[i].d_coef[p] = ptr
        arr[i].d_quanta, arr[i].ntables = quanta, ntables
    return arr


def view_mixed(handle, images, cosited, color, views, out_ptr, stride, n=None):
    return _lib.lib().jpeg_amd_decode_view_mixed(handle, len(images) if n is None else n, c_images(images), cosited, color,
                                                 c_views(views), out_ptr, stride)


def resized_mixed(handle, images, cosited, color, views, out_w, out_h, out_ptr, stride, n=None):
    return _lib.lib().jpeg_amd_decode_resized_mixed(handle, len(images) if n is None else n, c_images(images), cosited, color,
                                                    c_views(views), out_w, out_h, out_ptr, stride)


def tensor_mixed(handle, images, cosited, color, views, out_w, out_h, spec, flips, out_ptr, stride, n=None):
    h_flip = None if flips is None else (C.c_uint8 * max(len(flips), 1))(*[1 if f else 0 for f in flips])
    return _lib.lib().jpeg_amd_decode_tensor_mixed(handle, len(images) if n is None else n, c_images(images), cosited, color,
                                                   c_views(views), out_w, out_h, C.byref(spec), h_flip, out_ptr, stride)
