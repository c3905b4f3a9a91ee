"""The case table and the guarded-buffer helpers of tests/test_buffers_cpu.py (the table alone, no GPU) and tests/test_gpu_buffers.py
(jpeg_amd_decode_batch and jpeg_amd_encode_batch on the MI355X): whole images whose pixel buffer begins at any byte, whose
images lie any number of bytes apart, and whose every byte outside an image is guarded.  Imports numpy and the shared test
helpers -- no torch, no GPU.

WHY.  Each call picks its kernel instantiation from three facts about the caller's pixel buffer (decoder_fast, encoder_fast below:
the launchers' predicates, restated).  On a fresh allocation with a stride of 3 W H bytes they reduce to the width alone, so the
slow instantiations only ever saw widths with a partial last chunk and the fast ones only aligned buffers.  Here every width
class meets every placement.

SHAPES: the smallest at which each store and load mechanism is still taken (SHAPES below, each with its reason).
PLACEMENTS: n = 3 images per call; `lead` bytes from an allocation boundary to image 0; stride = image bytes + gap, the gap the
smallest of at least 16 bytes that gives the stride its residue mod 16; a sentinel tail of 16 bytes.  A stray 16-byte chunk
behind an image therefore cannot reach the next image unseen.

COEFFICIENT PLANES stay where the contract puts them: bases and strides are whole multiples of 8 elements (16 bytes).  The
kernels fetch blocks with 16-byte loads and LDS-DMA, the header states no looser contract, and a misaligned plane could fault
the device: no test may risk that.  The planes' gaps vary in whole blocks only (COEF_LEAD_BLOCKS, coef_gap_blocks)."""
from collections import namedtuple

import numpy as np

from _calls import FUSED, SENTINEL, assert_only_spans_written, out_spans
from test_gpu_quad_shapes import SIZES as QUAD_SIZES

N_IMAGES = 3
TAIL = 16
MIN_GAP = 16
LIMIT = 304                                    # no side of any shape is longer

# ---- the launchers' decisions, restated ---------------------------------------------------------------------------------------------


def decoder_fast(w, base, stride):
    """launch_quad_decode (kernels_quad.hip) and launch_fused_decode (kernels_fused.hip): FAST."""
    return w % 16 == 0 and stride % 16 == 0 and base % 16 == 0


def encoder_fast(w, base, stride):
    """launch_fused_encode (kernels_encode.hip): FASTIN (every width here is below 2^23)."""
    return w % 8 == 0 and stride % 8 == 0 and base % 8 == 0


def luma_units(name, size):
    """Blocks of the first plane: its factor is the scale in every layout here."""
    return -(-size[0] // 8), -(-size[1] // 8)


def strip_blocks(name, size):
    """The strip's width in blocks, 32 (x 2 block rows) or 16 (x 4), that the decoder takes for a short call: quad_cut
    (kernels_quad.hip; the mixed cut needs a call many trips long) for 4:2:0, strip_width (kernels_fused.hip) for the others."""
    ux, uy = luma_units(name, size)
    if name.startswith("420"):
        stacks = lambda cols, by: cols * ((-(-uy // by) + 3) // 4)
        return 16 if stacks(-(-ux // 16), 4) < stacks(-(-ux // 32), 2) else 32
    if name in ("422", "440"):
        return 32 if name == "422" else 16
    return 16 if -(-ux // 16) * -(-uy // 4) < -(-ux // 32) * -(-uy // 2) else 32


def strip_pixels(name, size):
    """(w, h) of a strip in pixels."""
    bx = strip_blocks(name, size)
    return 8 * bx, 8 * (64 // bx)


# ---- the shapes -------------------------------------------------------------------------------------------------------------------

# 4:2:0: the shapes of test_gpu_quad_shapes.SIZES no larger than 304 x 304, each commented there with the mechanism it hits (both
# strip shapes, short last stack, plane ending inside the first strip, one-block image), and three more per strip shape: a
# width that is a multiple of 16 with a partial last strip column, that width + 8 (whole 8-byte rows for the encoder, a partial
# 16-byte chunk for the decoder), that width - 3 (odd).
QUAD_EXTRA = {32: [(288, 52), (296, 52), (285, 52)],      # 32 x 2 strips: two columns of 256 pixels, the second 32, 40, 29 wide
              16: [(272, 116), (280, 116), (269, 116)]}   # 16 x 4 strips: three columns of 128 pixels, the third 16, 24, 13 wide
# The other layouts: W % 16 == 0, W % 16 == 8 and W odd, each more than one strip column wide and not a whole number of strip
# rows high.  4:2:2 is written for the 32 x 2 strip and 4:4:0 for the 16 x 4 one; grey and 4:4:4 share k_luma_fused's two strip
# shapes between them, so that every width class meets both.
SHAPES = {
    "420": [s for s in QUAD_SIZES if max(s) <= LIMIT] + QUAD_EXTRA[32] + QUAD_EXTRA[16],
    "y8": [(288, 12), (296, 52), (285, 12)],               # 32 x 2, 16 x 4, 32 x 2
    "444": [(272, 52), (280, 12), (269, 52)],              # 16 x 4, 32 x 2, 16 x 4
    "422": [(288, 40), (296, 40), (285, 40)],
    "440": [(144, 40), (152, 40), (141, 40)],
}
LAYOUTS = dict(FUSED)
assert list(SHAPES) == ["420", "y8", "444", "422", "440"] and set(SHAPES) == set(FUSED)
# the staged fallbacks of the same entry points: one shape each (odd, more than one MCU either way), three placements
STAGED = {"411": ([(4, 1), (1, 1), (1, 1)], 0, (141, 21)), "420-cosited": (FUSED["420"], 1, (141, 37))}   # (factors, cosited, shape)
STAGED_PLACEMENTS = [(0, 0), (8, 0), (1, 5)]

# ---- the placements ---------------------------------------------------------------------------------------------------------------

PLACEMENTS = [(0, 0),     # control: the fast instantiations, now with guard bytes
              (0, 8),     # aligned base, unaligned stride: image 1 at residue 8
              (8, 0),     # the decoder must leave FAST, the encoder keeps FASTIN
              (4, 0), (1, 5), (15, 8)]   # the general cases
Placed = namedtuple("Placed", "lead gap tail stride nbytes spans")


def place(image_bytes, lead, residue, n=N_IMAGES):
    """n images of image_bytes each, the first `lead` bytes behind an allocation boundary, stride % 16 == residue with the
    smallest gap of at least MIN_GAP bytes, TAIL bytes behind the last image's stride: _calls.out_spans's layout."""
    gap = MIN_GAP + (residue - image_bytes - MIN_GAP) % 16
    stride, nbytes, spans = out_spans([image_bytes] * n, 1, gap, lead, TAIL)
    return Placed(lead, gap, TAIL, stride, nbytes, spans)


def residues(p, m):
    """Where each image begins, modulo m (the buffer begins at an allocation boundary)."""
    return [a % m for a, _ in p.spans]


# ---- the cases --------------------------------------------------------------------------------------------------------------------

QI = [[0, 1, 1], [0, 1, 2], [1, 0, 0], [2, 1, 0]]            # table selectors per plane, three distinct tables
NTABLES = 3
Case = namedtuple("Case", "name factors cosited size qi per_image seed")


def _case(k, name, factors, cosited, size):
    return Case(name, factors, cosited, size, QI[(k // 2) % 4][:len(factors)], k % 2 == 1, 9100 + 10 * k)


CASES = [_case(k, name, LAYOUTS[name], 0, size) for k, (name, size) in enumerate((n, s) for n in SHAPES for s in SHAPES[n])]
STAGED_CASES = [_case(len(CASES) + k, name, f, c, s) for k, (name, (f, c, s)) in enumerate(STAGED.items())]


def case_id(c):
    return "%s-%dx%d" % (c.name, c.size[0], c.size[1])


def placement_id(p):
    return "lead%d-stride%d" % p


def tables(c):
    """uint16 [n, 3, 64] (per-image tables) or [1, 3, 64] (shared): small quanta, 1 at DC and 1 .. 3 elsewhere, so that
    natural_planes_torch's coefficients (DC within +-1024, Laplacian 200 / (1 + k) behind it) decode to mostly unclamped samples;
    the three tables of an image differ in about two thirds of their entries."""
    q = np.random.default_rng(c.seed + 1).integers(1, 4, (N_IMAGES if c.per_image else 1, NTABLES, 64)).astype(np.uint16)
    q[..., 0] = 1
    return q


def image_tables(c, q, i):
    """The table of each plane of image i, as the oracle takes them."""
    return [q[i if c.per_image else 0, t] for t in c.qi]


COEF_LEAD_BLOCKS = 1


def coef_gap_blocks(p):
    """Whole blocks between the images of plane p (and one block in front of the first image, one behind the last)."""
    return 1 + p


# ---- guarded pixel buffers on the host ------------------------------------------------------------------------------------------------

def placed_pixels(images, p, fill):
    """The bytes of a buffer laid out by p: image i at lead + i * stride, `fill` in every other byte (lead, gaps, tail)."""
    buf = np.full(p.nbytes, fill, np.uint8)
    for (a, m), im in zip(p.spans, images):
        buf[a:a + m] = np.asarray(im, np.uint8).reshape(-1)
    return buf


def guard_report(host, p, fill=SENTINEL):
    """'' when every byte of `host` outside the images of p holds `fill`; else which of lead, gap i, tail was touched and where."""
    mine = np.zeros(host.size, bool)
    for a, m in p.spans:
        mine[a:a + m] = True
    stray = np.flatnonzero(~mine & (host != fill))
    if not stray.size:
        return ""
    at = int(stray[0])
    ends = [a + m for a, m in p.spans]
    if at < p.lead:
        where = "the lead, %d bytes in front of image 0" % (p.lead - at)
    else:
        i = max(k for k, (a, _) in enumerate(p.spans) if a <= at)
        where = ("the gap" if i + 1 < len(p.spans) else "the gap and tail") + " behind image %d, %d bytes past its end" % (i, at - ends[i])
    return "%d guard bytes written; the first at byte %d (%s): %d" % (stray.size, at, where, int(host[at]))


def assert_guarded(host, p, fill=SENTINEL):
    assert_only_spans_written(host, p.spans, fill)          # the shared check, and the report that names the place
    report = guard_report(host, p, fill)
    assert not report, report


def first_difference(got, want, size):
    """'' when the bytes of an image (3 per pixel, rows of size[0] pixels) are `want`; else the count and the first differing
    byte's row, column, channel and 16-byte chunk of its row."""
    got, want = np.asarray(got).reshape(-1), np.asarray(want).reshape(-1)
    if got.size != want.size:
        return "%d bytes against %d" % (got.size, want.size)
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return ""
    at = int(bad[0])
    row, rest = divmod(at, 3 * size[0])
    return "%d of %d bytes differ; first at (row %d, column %d, channel %d) [byte %d of its row, chunk %d]: %d != %d" % (
        bad.size, want.size, row, rest // 3, rest % 3, rest, rest // 16, int(got[at]), int(want[at]))


def first_coefficient(got, want):
    """The same for coefficient planes [uy, ux, 64]."""
    for p, (a, b) in enumerate(zip(got, want)):
        a, b = np.asarray(a), np.asarray(b)
        if a.shape != b.shape:
            return "plane %d: %s against %s" % (p, a.shape, b.shape)
        bad = np.argwhere(a != b)
        if len(bad):
            y, x, z = (int(v) for v in bad[0])
            return "plane %d: %d of %d coefficients differ; first at (block x %d, block y %d, zigzag %d): %d != %d" % (
                p, len(bad), b.size, x, y, z, int(a[y, x, z]), int(b[y, x, z]))
    return ""
