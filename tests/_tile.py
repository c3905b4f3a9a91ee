"""What the tests of the tile decode family (region, scaled, view and mixed decode) share, each stated once: the 8-bit fixtures
with their C layout, the checker of a whole image at a denominator -- independent of the code under test: the oracle's full
decode at denominator 1, _scaled_ref below it -- the crop, and seeded rectangles.  Importing this needs no GPU and no torch."""
import ctypes as C
import glob
import os

import numpy as np

import _scaled_ref as S
import _transform_ref as R
from _golden import GOLDEN
from jpeg_amd import _lib
from oracle import oracle as O

TILE_W, TILE_H = 128, 32                                    # the scaled, view and mixed kernels' tile of output pixels


def _eight_bit(path):
    d = np.fromfile(path, np.uint8)
    i = _lib.FrameInfo()
    return _lib.lib().jpeg_amd_jpeg_inspect(d.ctypes.data, d.size, C.byref(i)) == 0 and i.precision == 8 and i.ncomponents in (1, 3)


# the decode fixtures that the tile kernels' calls take: 8 bits, one or three components
FIXTURES = [p for p in sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg"))) if _eight_bit(p)]


def fixture(path):
    """-> (frame info, C layout, host planes, quanta uint16 [ncomponents, 64]) of a fixture file."""
    info, planes, quanta = R.decode_file(np.fromfile(path, np.uint8))
    nc = info.ncomponents
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes = info.width, info.height, info.precision, nc
    L.scale_x, L.scale_y = info.scale_x, info.scale_y
    for c in range(nc):
        L.factor_x[c], L.factor_y[c] = info.factor_x[c], info.factor_y[c]
        L.units_x[c], L.units_y[c] = info.units_x[c], info.units_y[c]
        L.qi[c] = c
    return info, L, planes, np.ascontiguousarray(quanta, np.uint16)


def reference(L, planes_host, quanta_host, i, denom, cosited):
    """Image i of a batch at `denom`, whole, through the checker -> {color: uint8 [H', W', 3]}.
    planes_host[p] [n, uy, ux, 64], quanta_host [n, ntables, 64]."""
    factors = [(L.factor_x[p], L.factor_y[p]) for p in range(L.nplanes)]
    planes = [pl[i] for pl in planes_host]
    quanta = [quanta_host[i, L.qi[p]] for p in range(L.nplanes)]
    size, scale = (L.width, L.height), (L.scale_x, L.scale_y)
    if denom == 1:
        _, rect = O.decode(planes, quanta, factors, size, cosited=bool(cosited), scale=scale)
    else:
        _, rect = S.interleaved_scaled(planes, quanta, factors, size, denom, bool(cosited), scale)
    w, h = S.scaled_size(size, denom)
    return {_lib.COLOR_RGB8: O.unpack_rgb8(rect, L.nplanes).reshape(h, w, 3),
            _lib.COLOR_YCC8: O.unpack_ycc8(rect, L.nplanes).reshape(h, w, 3)}


def crop(image, r):
    return image[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]


def random_region(rng, W, H, max_w=None, max_h=None):
    """A seeded rectangle inside W x H, at most max_w x max_h."""
    x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
    return x, y, int(rng.integers(1, min(W - x, max_w or W) + 1)), int(rng.integers(1, min(H - y, max_h or H) + 1))
