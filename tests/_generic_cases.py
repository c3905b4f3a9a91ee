"""The case table and the input builder of tests/test_generic_cases_cpu.py (oracle alone, no GPU) and
tests/test_gpu_generic_shapes.py (k_generic_fused / k_generic_encode against the oracle): custom formats whose planes are a
third or a quarter of the image's scale, on images of several tiles.  Imports numpy and the oracle only -- no torch, no GPU.

SIZES.  A tile of k_generic_fused is 128 pixels wide and 64 or 32 rows high (jpeg_amd/csrc/kernels_generic.hip).  The block
range of a tile on an axis that is neither at the image's scale nor "half of a scale of 2" follows from the tile's column (row):
the tile's first pixel t0 reads sample i0 = (a + b t0) / c (truncating, decode.swift:4240), the tile's first block is i0 >> 3, the
offset of its first sample in that block i0 & 7, and the number of blocks follows from the last pixel's neighbour sample.

  * quarters (factor 1 in a scale of 4): 128 pixels are 32 samples, four whole blocks -- every tile column beyond the first has the
    same (offset, count); the first differs because pixel 0 clamps to sample 0 (centred: a = f - s < 0 truncates to 0).
  * thirds (factor 1 in a scale of 3): 128 pixels are 42 2/3 samples; three tile columns are 384 pixels = 128 samples = 16 whole
    blocks, so (offset, count) cycles with period THREE -- after the first tile, which again differs by the clamp at sample 0.
    The pair therefore takes four values, at tile columns 0, 1, 2 and 3 (cosited, a = 0 and nothing clamps: column 0 equals column
    3, three values); column 4 repeats column 1, and so on for ever.  The same holds for rows with 64-row tiles (3 x 64 rows =
    64 samples = 8 blocks) and 32-row tiles (3 x 32 rows = 32 samples = 4 blocks).
  * 2-in-4 (factor 2 in a scale of 4) is the factor-2 map at c = 8 | 4: whole blocks per tile, one value beyond the first tile.

So an image must span MORE than four tile columns and four tile rows (of the larger tile height: eight of the smaller) to meet
every value of the pair and the first repeat.  LARGE = 517 x 259 is four whole tile columns plus a fifth of 5 pixels -- 5 * count
samples is no multiple of 8 for any count 2 .. 4, so that column also takes the byte-wise store tail -- and four whole 64-row
tiles (eight 32-row ones) plus 3 rows.  SMALL = 129 x 65 has ONE pixel column and ONE pixel row in the second tile column / row
(of 64-row tiles): the narrowest edge tile there is.

INPUTS, both seeded from the case number:
  * wide: the recipe of test_generic_fused_decode_... (tests/test_gpu_parity.py): coefficients uniform in +-2^(P-1), positions 5 and
    later divided by 32, tables drawn from 1 .. 11.  Every channel of the ORACLE's result must reach both clamps (0 and 2^P - 1) and
    at least half of its samples must lie strictly between them (tests/test_generic_cases_cpu.py): an input that only tests the
    clamp would let a filter error through.
  * steps: DC only under an all-8 table -- every block is ONE constant (DC + 2^(P-1)), and the constants cycle through
    0, 2^P - 1, 1, 2^P - 2 and three seeded values, shifted by three from block row to block row: known neighbours, the extremes
    included, across every block seam in both directions, and an index-map or weight error is legible in the failing samples.
"""
from functools import lru_cache
from typing import NamedTuple, Optional, Tuple

import numpy as np

from oracle import oracle as O

TILE_W = 128
TILE_ROWS = (64, 32)          # the two tile heights of k_generic_fused
LARGE = (517, 259)
SMALL = (129, 65)
SIZES = (LARGE, SMALL)
KINDS = ("wide", "steps")

assert LARGE[0] > 4 * TILE_W and LARGE[1] > 4 * max(TILE_ROWS)      # tile columns / rows 0 .. 4: every phase and the first repeat
assert LARGE[0] % TILE_W == 5                                       # the store tail: 5 * count samples, no multiple of 8
assert all((5 * count) % 8 for count in (2, 3, 4))
assert SMALL == (TILE_W + 1, max(TILE_ROWS) + 1)


class Case(NamedTuple):
    number: int
    factors: Tuple[Tuple[int, int], ...]    # the recognised components, in plane order
    precision: int
    extra: Optional[Tuple[int, int]]        # a component the format does not recognise: it takes part in the scale only
    fused: bool                             # generic_fused_supported: False -> the same call takes the staged kernels

    @property
    def scale(self):
        fs = self.factors + ((self.extra,) if self.extra else ())
        return (max(f[0] for f in fs), max(f[1] for f in fs))

    @property
    def count(self):
        return len(self.factors)

    @property
    def q(self):
        """table index per plane (two tables, alternating -- as the layouts of test_generic_fused_decode_...)"""
        return [i & 1 for i in range(self.count)]


_1 = (1, 1)
CASES = (
    # every format is ("custom", precision, count).  Tile rows (a comment only: the tests cannot observe it) = 64 when the host's
    # bound on a 128 x 64 tile's blocks (tile_blocks) is at most 256, else 32.
    Case(1, ((4, 1), _1, _1), 8, None, True),                     # 64  quarters in x through the literal filter; 4:1:1
    Case(2, ((4, 2), _1, _1), 12, None, True),                    # 64  quarters in x, half of a scale of 2 in y; 4:1:0
    Case(3, ((4, 4), _1, _1), 16, None, True),                    # 64  quarters on both axes
    Case(4, ((1, 4), _1, _1), 12, None, True),                    # 64  full x + quarter y: the exact filter with eighths (fourths cosited); 256 blocks
    Case(5, ((3, 3), _1, _1), 12, None, True),                    # 64  thirds on both axes; magic quotient by 6, by 3 cosited
    Case(6, ((1, 3), _1, _1), 16, None, True),                    # 64  full x + thirds in y; 256 blocks
    Case(7, ((3, 1), _1, _1), 8, None, True),                     # 64  thirds in x only
    Case(8, ((3, 2), _1, (3, 1)), 12, None, True),                # 32  three planes over the 64-row bound (266 blocks); one plane full x, half y
    Case(9, ((4, 4), (2, 2), _1, (4, 1)), 12, None, True),        # 32  four planes; 2-in-4 (c = 8, b = 4); full x + quarter y
    Case(10, ((4, 2), (2, 1), (1, 2), (4, 1)), 16, None, True),   # 32  four planes, every plane different
    Case(11, ((4, 1), (1, 4)), 9, None, True),                    # 64  two planes, none direct
    Case(12, (_1, _1, _1), 12, (3, 3), True),                     # 64  every plane in thirds, none direct
    Case(13, ((2, 2),) * 4, 8, (4, 4), True),                     # 64  four planes of 2-in-4, none direct
    Case(14, ((3, 3), (2, 2), _1), 12, None, False),              # n/a 2-in-3: refused by the fused kernel, the staged kernels inside the same call
)
assert [c.number for c in CASES] == list(range(1, 15))
ENCODE_STAGED = (5, 6, 7, 8, 12, 14)     # a box of 3 under decomposed(): the staged encoder inside the same call


def case(number: int) -> Case:
    return CASES[number - 1]


def units(c: Case, size):
    return [O.plane_units(size, f, c.scale) for f in c.factors]


def _frozen(a):
    a.setflags(write=False)
    return a


def step_constants(c: Case, size, precision=None):
    """steps: the constant of every block, per plane [uy, ux] (int32)."""
    P = precision or c.precision
    top = (1 << P) - 1
    rng = np.random.default_rng(8000 + c.number)
    out = []
    for ux, uy in units(c, size):
        by, bx = np.mgrid[0:uy, 0:ux]
        k = (bx + 3 * by) % 7
        seeded = rng.integers(0, top + 1, (uy, ux))
        v = np.choose(np.minimum(k, 4), [np.zeros_like(k), np.full_like(k, top), np.ones_like(k), np.full_like(k, max(top - 1, 0)), seeded])
        out.append(v.astype(np.int32))
    return out


def build_input(c: Case, size, kind: str, precision=None, seed=None):
    """-> (coefficient planes int16 [uy, ux, 64] zigzag, two tables uint16 [64], table index per plane)."""
    P = precision or c.precision
    if kind == "wide":
        # (the seed's base is one under which the ORACLE's result meets the conditions on this input for every case, siting and size --
        # the share of unclamped samples of a plane at the image's scale hangs on the first entries of its table, and lies between
        # 46 % and 75 %; tests/test_generic_cases_cpu.py holds the seeds to the conditions, without the code under test)
        rng = np.random.default_rng(7200 + c.number if seed is None else seed)
        amp = 1 << (P - 1)
        planes = []
        for ux, uy in units(c, size):
            v = rng.integers(-amp, amp, (uy, ux, 64)).astype(np.int32)
            v[..., 5:] //= 32
            planes.append(np.clip(v, -32768, 32767).astype(np.int16))
        tables = [rng.integers(1, 12, 64).astype(np.uint16) for _ in range(2)]
    elif kind == "steps":
        planes = []
        for v in step_constants(c, size, P):
            coef = np.zeros(v.shape + (64,), np.int16)
            coef[..., 0] = v - (1 << (P - 1))          # DC under a quantum of 8: the block is DC + 2^(P-1)
            planes.append(coef)
        tables = [np.full(64, 8, np.uint16) for _ in range(2)]
    else:
        raise ValueError(kind)
    return [_frozen(p) for p in planes], [_frozen(t) for t in tables], c.q


@lru_cache(maxsize=8)
def oracle_planes(number: int, size, kind: str):
    """-> (planes, tables, q, the oracle's Planar) of a case; shared and read-only."""
    c = case(number)
    planes, tables, q = build_input(c, size, kind)
    want_p = [_frozen(O.idct_plane(p, tables[i], c.precision)) for p, i in zip(planes, q)]
    return planes, tables, q, want_p


@lru_cache(maxsize=8)
def oracle_rect(number: int, size, kind: str, cosite: bool):
    """the oracle's Rectangular uint16 [H, W, count] of a case; shared and read-only."""
    c = case(number)
    want_p = oracle_planes(number, size, kind)[3]
    return _frozen(O.interleave(want_p, list(c.factors), c.scale, size, cosited=cosite))


def encode_tables(c: Case):
    """two tables drawn from 16 .. 59 (smaller divisors would push the coefficients of 16-bit samples past Int16, where the
    reference traps), keyed as Rectangular.spectral takes them."""
    rng = np.random.default_rng(9000 + c.number)
    return {k: _frozen(rng.integers(16, 60, 64).astype(np.uint16)) for k in range(2)}


def oracle_encode(c: Case, size, values, tables, precision=None):
    """-> (the oracle's decomposed planes, its coefficient planes) of Rectangular `values`."""
    want_d = O.decompose(values, size, list(c.factors), c.scale)
    want_f = [O.fdct_plane(p, tables[i], precision or c.precision) for p, i in zip(want_d, c.q)]
    return want_d, want_f


def axis_phase(f: int, s: int, cosited: bool, tile: int, index: int):
    """(offset of the first sample in its block, blocks) that tile `index` of `tile` pixels reads on an axis of factor f under a
    scale s: decode.swift:4223-4246, i of the first pixel and i + 1 of the last -- the reasoning of the module comment in numbers."""
    a, b, c = (0, f, s) if cosited else (f - s, 2 * f, 2 * s)
    trunc = lambda n: -((-n) // c) if n < 0 else n // c
    lo = trunc(a + b * tile * index)
    hi = trunc(a + b * (tile * index + tile - 1)) + 1
    return lo & 7, (hi >> 3) - (lo >> 3) + 1
