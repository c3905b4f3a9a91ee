"""The case tables and inputs of tests/test_frame_limit_cpu.py (the references alone, no GPU) and tests/test_gpu_frame_limit.py
(every kernel family on the MI355X): images whose long side is the most a JPEG frame header can say, 65535, or 65529, whose last
8 x 8 block holds a single pixel column (row).  Imports numpy, the oracle and the shared test helpers -- no torch, no GPU.

SHAPES.  65535 leaves 7, 15, 15, 31, 63 and 127 against 8, 16, 24, 32, 64 and 128: a partial last block, MCU and tile of every
kernel.  The short side is one MCU of the layout plus one pixel (9, 17, 25 or 33 for scales 1 to 4): two MCU rows (columns), the
second a single pixel row.  Every case runs "widest" (the long side across) and "tallest" (the long side down).

INPUTS of the 8-bit families (fused decode and encode, tile family, coefficient domain), seeded from the layout and the size: the
recipe of test_extreme_aspect_ratios_at_the_frame_header_limit -- uniform coefficients, strong in the first six zigzag positions
and weak behind them, under the level-1.0 tables -- at an amplitude at which the DECODED image is not mostly clamped: +-20 in the
first six positions and +-1 behind them for the first plane, +-10 and +-1 for the others.  (That test's +-300 decodes to 8 % of
unclamped luma samples: a coordinate error that moves a clamped sample onto another clamped sample is invisible.)
tests/test_frame_limit_cpu.py holds every input to the conditions, and lists the shares it found.

The resample and warp families read pixel sources: _calls.pixel_image("random"), every byte uniform."""
from functools import lru_cache

import numpy as np

import _antialias_ref as A
import _bicubic_ref as B
import _generic_cases as GC
import _project_cubic_ref as Q
import _project_ref as P
import _resize_ref as R
import _warp_ref as W
from _calls import FUSED, c_layout, pixel_image
from _tile import crop, reference
from jpeg_amd import _lib
from oracle import oracle as O

LONGS = (65535, 65529)
ORIENTS = ("widest", "tallest")
WINDOW = 256                                   # the far end: the last 256 columns (rows)
WRAPS = (16384, 32768, 49152)                  # ... must differ from what lies this far in front of it: a coordinate that wraps
LAYOUTS = dict(FUSED, **{"411": [(4, 1), (1, 1), (1, 1)]})
COLORS = {_lib.COLOR_RGB8: "rgb", _lib.COLOR_YCC8: "ycc"}

assert [LONGS[0] % m for m in (8, 16, 24, 32, 64, 128)] == [7, 15, 15, 31, 63, 127] and LONGS[1] % 8 == 1


def scale_of(factors):
    return max(f[0] for f in factors), max(f[1] for f in factors)


def extent(scale, long, orient):
    """(w, h): the long side and one MCU plus one pixel."""
    return (long, 8 * scale[1] + 1) if orient == "widest" else (8 * scale[0] + 1, long)


def along(image, orient):
    """image [H, W, ...] with the long side first."""
    return image.swapaxes(0, 1) if orient == "widest" else image


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the 8-bit inputs ---------------------------------------------------------------------------------------------------------------

def tables():
    """uint16 [2, 64]: the level-1.0 tables."""
    return np.stack([O.compression_quanta("luminance", 1.0), O.compression_quanta("chrominance", 1.0)]).astype(np.uint16)


@lru_cache(maxsize=6)
def image8(name, size, n=1):
    """n images of a LAYOUTS entry -> (host planes [n, uy, ux, 64] per plane, host tables uint16 [n, ntables, 64]); read-only."""
    factors = LAYOUTS[name]
    rng = np.random.default_rng(1000 * size[0] + size[1] + len(name))
    planes = []
    for p, f in enumerate(factors):
        ux, uy = O.plane_units(size, f, scale_of(factors))
        head, tail = (20, 1) if p == 0 else (10, 1)
        c = rng.integers(-head, head + 1, (n, uy, ux, 64)).astype(np.int16)
        c[..., 6:] = rng.integers(-tail, tail + 1, (n, uy, ux, 58))
        planes.append(_frozen(c))
    ntables = 2 if len(factors) == 3 else 1
    return planes, _frozen(np.ascontiguousarray(np.broadcast_to(tables()[:ntables], (n, ntables, 64))))


@lru_cache(maxsize=6)
def decoded8(name, size, denom=1, cosited=0, i=0, n=1):
    """Image i of image8(name, size, n), whole, at `denom`, through _tile.reference -> {color: uint8 [H', W', 3]}; read-only."""
    planes, quanta = image8(name, size, n)
    want = reference(c_layout(size[0], size[1], LAYOUTS[name]), planes, quanta, i, denom, cosited)
    return {k: _frozen(v) for k, v in want.items()}


def encoded8(pixels, size, factors, color):
    """The oracle's coefficient planes of an image uint8 [H, W, 3] under the level-1.0 tables."""
    q = tables()
    quanta = [q[min(p, 1)] for p in range(len(factors))]
    if color == _lib.COLOR_RGB8:
        return O.encode(np.ascontiguousarray(pixels).reshape(-1, 3), size, factors, quanta)
    rect = O.pack_ycc8(np.ascontiguousarray(pixels).reshape(-1, 3), len(factors)).reshape(size[1], size[0], len(factors))
    return [O.fdct_plane(p, t) for p, t in zip(O.decompose(rect, size, factors, scale_of(factors)), quanta)]


# ---- family 1: the fused 8-bit decode and encode of the layouts other than 4:2:0 ---------------------------------------------------------

FUSED8 = [("y8", 0), ("444", 0), ("422", 0), ("422", 1), ("440", 0)]                  # (layout, cosited)
FUSED8_CASES = [(name, cosited, long, orient) for name, cosited in FUSED8 for long in LONGS for orient in ORIENTS]


def fused8_images(long):
    """The images of a call: the 65529 cases are batches of two."""
    return 2 if long == LONGS[1] else 1


# ---- family 2: the generic fused decode and encode ------------------------------------------------------------------------------------

GENERIC = (1, 3, 5, 6, 10)
GENERIC_CASES = [(number, cosite, long, orient) for number in GENERIC for cosite in (False, True) for long in LONGS for orient in ORIENTS]
# launch_generic_fused takes the ticket walk (`walk`) only for 64-row tiles whose subsampled planes all take the exact filter -- a
# factor of 1 in a scale of 2 -- and only when the call has more tiles than workgroups are resident.  NONE of the cases above
# does: each has a plane in thirds or quarters, which the literal filter takes.  The walk's case is 4:2:0 at 12 bits, tallest, as
# a batch of three: 3 x 1024 tiles of 128 x 64, more than the 2048 workgroups of 256 work-items that 256 CUs can hold at all.
WALK = GC.Case(0, ((2, 2), (1, 1), (1, 1)), 12, None, True)
WALK_IMAGES = 3


def generic_case(number):
    return WALK if number == 0 else GC.case(number)


def generic_input(number, size, i=0):
    c = generic_case(number)
    return GC.build_input(c, size, "wide", seed=None if number and i == 0 else 7300 + 10 * number + i)


@lru_cache(maxsize=4)
def generic_rect(number, size, cosite, i=0):
    """The oracle's Rectangular uint16 [H, W, count] of image i of a case under the `wide` input; read-only."""
    if number and i == 0:
        return GC.oracle_rect(number, size, "wide", cosite)
    c = generic_case(number)
    planes, tbl, q = generic_input(number, size, i)
    planar = [O.idct_plane(p, tbl[k], c.precision) for p, k in zip(planes, q)]
    return _frozen(O.interleave(planar, list(c.factors), c.scale, size, cosited=cosite))


def numerators(c, size, cosite):
    """[(plane, axis, factor, scale, the largest a + b t)] of every axis of every plane that is not direct (interleave.hpp)."""
    out = []
    for p, f in enumerate(c.factors):
        if c.count == 1 or f == c.scale:
            continue
        for axis in (0, 1):
            a, b = (0, f[axis]) if cosite else (f[axis] - c.scale[axis], 2 * f[axis])
            out.append((p, axis, f[axis], c.scale[axis], a + b * (size[axis] - 1)))
    return out


# ---- family 3: the tile family ------------------------------------------------------------------------------------------------------------

TILE_LAYOUTS = ("y8", "420", "411")            # 4:1:1 has no tile kernel: k_region_crop and k_idct_scaled
TILE_CASES = [(name, long, orient) for name in TILE_LAYOUTS for long in LONGS for orient in ORIENTS]
DENOMS = (2, 4, 8)


def _flip(r, orient):
    """A rectangle stated for the widest image, for `orient`."""
    return r if orient == "widest" else (r[1], r[0], r[3], r[2])


def far_regions(size, scale, orient):
    """The last 200 columns (rows) whole, the last pixel alone, a window across the last MCU boundary, and one across pixel
    32768, where a 15-bit coordinate wraps: on a centred axis of halves the fraction has period 2 from pixel 1 on and differs
    at pixel 0 alone, so a coordinate taken modulo 2^15 shows in that one column (row) and nowhere else."""
    long, short = (size[0], size[1]) if orient == "widest" else (size[1], size[0])
    mcu = 8 * (scale[0] if orient == "widest" else scale[1])
    seam = (long - 1) // mcu * mcu
    assert seam - 30 < seam < long
    rs = [(long - 200, 0, 200, short), (long - 1, short - 1, 1, 1), (seam - 30, 0, min(45, long - (seam - 30)), short),
          (32768 - 30, 0, 60, short)]
    return [_flip(r, orient) for r in rs]


def wrap_view(size, orient):
    """(1, rectangle): 150 columns (rows) around pixel 32768 at full size, whole across."""
    return 1, _flip((32768 - 75, 0, 150, size[1] if orient == "widest" else size[0]), orient)


def far_view(size, denom, orient, length=150):
    """(denom, rectangle): the last `length` columns (rows) of the image scaled by 1 / denom, whole across."""
    n = 8 // denom
    w, h = (size[0] * n + 7) // 8, (size[1] * n + 7) // 8
    long, short = (w, h) if orient == "widest" else (h, w)
    return denom, _flip((long - length, 0, length, short), orient)


MIXED = [("420", (65535, 17), far_view((65535, 17), 2, "widest")), ("y8", (9, 65535), far_view((9, 65535), 4, "tallest")),
         ("420", (17, 33), (1, (3, 5, 14, 28)))]


# ---- family 4: the coefficient domain ---------------------------------------------------------------------------------------------------

SPECTRAL_CASES = [(name, long, orient) for name in ("y8", "420") for long in LONGS for orient in ORIENTS]


@lru_cache(maxsize=2)
def transform_input(name, size, n=2):
    """-> (planes int16 [n, uy, ux, 64] within +-1900, q_in uint16 [n, ntables, 64] from 1 .. 17 -- no Int16 product overflows --
    q_out, half from 1 .. 255 and half from 256 .. 65535): the inputs of test_gpu_transform_shapes.py."""
    factors = LAYOUTS[name]
    rng = np.random.default_rng(size[0] + 3 * size[1] + len(name))
    planes = [_frozen(rng.integers(-1900, 1901, (n, uy, ux, 64)).astype(np.int16))
              for ux, uy in (O.plane_units(size, f, scale_of(factors)) for f in factors)]
    shape = (n, 2 if len(factors) == 3 else 1, 64)
    q_in = rng.integers(1, 18, shape).astype(np.uint16)
    q_out = np.where(rng.random(shape) < 0.5, rng.integers(1, 256, shape), rng.integers(256, 65536, shape)).astype(np.uint16)
    return planes, _frozen(q_in), _frozen(q_out)


def far_crop(size, scale, orient):
    """A crop region that begins ten MCUs in front of the last MCU boundary and runs to the far end."""
    long = size[0] if orient == "widest" else size[1]
    mcu = 8 * (scale[0] if orient == "widest" else scale[1])
    first = ((long - 1) // mcu - 10) * mcu
    return _flip((first, 0, long - first, size[1] if orient == "widest" else size[0]), orient)


# ---- family 5: the resample and mapped walks from pixel sources ---------------------------------------------------------------------------

SOURCE_SHORT = 9
FILTERS = {"bilinear": (_lib.FILTER_BILINEAR, R.resize, 4096), "antialias": (_lib.FILTER_ANTIALIAS, A.resize, 4096),
           "bicubic": (_lib.FILTER_BICUBIC, B.resize, 8192)}          # (the C constant, the mirror, the strongest reduction's long side)
FILL = (7, 130, 255)
EDGES = {"fill": W.FILL, "replicate": W.REPLICATE}


@lru_cache(maxsize=2)
def source(orient):
    w, h = (LONGS[0], SOURCE_SHORT) if orient == "widest" else (SOURCE_SHORT, LONGS[0])
    return _frozen(pixel_image("random", w, h, 57 * w + h))


def resize_targets(name, orient):
    """(out_w, out_h): the same long side over a larger short side (k = 1 along the long axis), and the strongest reduction
    the filter takes (k just under 16 for the antialiasing filter, just under 8 for the bicubic one) over a smaller short side."""
    return [t if orient == "widest" else t[::-1] for t in ((LONGS[0], 13), (FILTERS[name][2], 5))]


RESIZE_CASES = [(name, orient, k) for name in FILTERS for orient in ORIENTS for k in (0, 1)]


@lru_cache(maxsize=4)
def resized(name, orient, k):
    out_w, out_h = resize_targets(name, orient)[k]
    return _frozen(FILTERS[name][1](source(orient), out_w, out_h))


MAPS = ("translation", "perspective", "quarter-turn")
WINDOW_OUT, WINDOW_SRC = 320, 300


def mapped(name, orient, shift=0):
    """-> (matrix float32 [9], (out_w, out_h)) for source(orient).  translation: a 320-pixel output window over the last 300
    source pixels, so that 20 pixels lie past the image's end; perspective: the same under a seeded four-corner distortion
    (_project_ref.distortion, corners up to 5 % inside and 10 % outside); quarter-turn: the long side turns into the other axis.
    shift: the window that many source pixels in front of the far end (what a wrapped coordinate would read)."""
    h, w = source(orient).shape[:2]
    if name == "quarter-turn":
        return np.array([0, 1, 0, -1, 0, h, 0, 0, 1], np.float32), (h, w)
    short = SOURCE_SHORT
    out = (WINDOW_OUT, short) if orient == "widest" else (short, WINDOW_OUT)
    win = (WINDOW_SRC, short) if orient == "widest" else (short, WINDOW_SRC)
    m = np.eye(3)
    if name == "perspective":
        m = P.distortion(np.random.default_rng(65556), win[0], win[1], out[0], out[1], 0.1, 0.1).astype(np.float64).reshape(3, 3)
    move = np.eye(3)
    move[0 if orient == "widest" else 1, 2] = LONGS[0] - WINDOW_SRC - shift
    return (move @ m).reshape(9).astype(np.float32), out


def affine(m):
    """The six values of jpeg_amd_warp_batch of a 3 x 3 whose last row is (0, 0, 1)."""
    assert m[6:].tolist() == [0, 0, 1]
    return m[:6]


MAP_CASES = [(name, orient, filt, edge) for name in MAPS for orient in ORIENTS for filt in ("bilinear", "bicubic") for edge in EDGES]


@lru_cache(maxsize=4)
def projected(name, orient, filt, edge, shift=0):
    m, (out_w, out_h) = mapped(name, orient, shift)
    mirror = P.project if filt == "bilinear" else Q.project
    return _frozen(mirror(source(orient), m, out_w, out_h, EDGES[edge], FILL))


# the composed case: a far-end view of the widest 4:2:0 image at 1/2, decoded and resampled in one call
COMPOSED = ("420", (65535, 17), far_view((65535, 17), 2, "widest", 300), (64, 5))


@lru_cache(maxsize=1)
def composed():
    name, size, (denom, r), (out_w, out_h) = COMPOSED
    return {k: _frozen(R.resize(crop(v, r), out_w, out_h)) for k, v in decoded8(name, size, denom).items()}
