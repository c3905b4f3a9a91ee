"""Test-side data and models for the encoders' quantiser (tests/test_quantiser_cases_cpu.py, tests/test_gpu_quantiser.py).

1.  A float32 numpy restatement of the reference's encode block path up to the UNROUNDED quotient, written from
    oracle/jpeg_oracle.c (encode.swift:80-99, 123-196, 205-241): min(limit, sample); fdct8 over the rows with the shift
    8 * 2^(P-1), then over the columns; division by the table modulated at scale 8, (r[k] * r[h]) * (8 * Float(Q)).  One
    binary32 operation per statement, in the reference's order.
2.  The tie constructor.  At the four positions whose modulation factor is 1 -- (k, h) in {0, 4}^2, zigzag 0, 10, 14, 39 --
    the transform of integer samples is exact: H = sum phi(x, y) (v - 2^(P-1)) with phi in {1, s(x), s(y), s(x) s(y)},
    s = (+, -, -, +, +, -, -, +), and the divisor is 8 Q exactly.  tie_blocks builds blocks with H = 4 Q m, m odd: the quotient
    is m / 2, which the reference rounds away from zero.
3.  Wrong quantisers as functions of (H, q), for the CPU test to rule out on this data, and an exact model of the kernels'
    own form (reciprocal, one Markstein step, trunc(y1 + copysign(pred(1/2), y1))) with the fused multiply-adds emulated in
    integer arithmetic.
4.  The batches the GPU tests run: one table value Q per image, the image's blocks that Q's ties."""
import math
from functools import lru_cache

import numpy as np

from oracle import oracle as O

F = np.float32
R8 = [F(1.0), F(1.387039845), F(1.306562965), F(1.175875602), F(1.0), F(0.785694958), F(0.541196100), F(0.275899379)]
POSITIONS = ((0, 0), (4, 0), (0, 4), (4, 4))            # (k, h): horizontal, vertical frequency
S4 = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.int64)    # the sign pattern of frequency 4 along one axis
PRED_HALF = F(0.49999997)


def zigzag(k, h):
    """decode.swift:1289-1298."""
    p = 1 if k + h < 8 else 0
    q = (k + h) & 1
    b = 2 * p - 1
    n = b * (k + h) - 14 * p + 15
    return 72 * (p ^ 1) + b * ((n * (n + 1)) >> 1) - q * k - (q ^ 1) * h - 1


ZZ = np.array([[zigzag(k, h) for k in range(8)] for h in range(8)])      # ZZ[h][k]
TIE_ZIGZAG = tuple(int(ZZ[h][k]) for k, h in POSITIONS)
assert sorted(TIE_ZIGZAG) == [0, 10, 14, 39]


# ---- 1. the restatement ------------------------------------------------------------------------------------------------

def modulated(q_zz):
    """float32 [h][k] = (r[k] * r[h]) * (8 * Float(Q[z(k, h)])), left-associative (dct.hpp:30)."""
    q_zz = np.asarray(q_zz, np.uint16).reshape(64)
    out = np.empty((8, 8), F)
    for h in range(8):
        for k in range(8):
            out[h, k] = F(R8[k] * R8[h]) * F(F(8.0) * F(q_zz[ZZ[h][k]]))
    return out


def fdct8(g, shift):
    """encode.swift:123-188 on a list of eight float32 arrays."""
    a0, a1, a2, a3 = g[0] + g[7], g[1] + g[6], g[2] + g[5], g[3] + g[4]
    b0, b1, b2, b3 = a0 + a3, a1 + a2, a1 - a2, a0 - a3
    c = F(0.707106781) * (b2 + b3)
    r0 = (b0 + b1) - shift
    r1, r2, r3 = b3 + c, b0 - b1, b3 - c
    d0, d1, d2, d3 = g[3] - g[4], g[2] - g[5], g[1] - g[6], g[0] - g[7]
    f0, f1, f2 = d0 + d1, d1 + d2, d2 + d3
    k = F(0.707106781) * f1
    l = F(0.382683433) * (f0 - f2)
    m0 = l + f0 * F(0.541196100)
    m1 = l + f2 * F(1.306562965)
    n0, n1 = d3 + k, d3 - k
    out = [r0, n0 + m1, r1, n1 - m0, r2, n1 + m0, r3, n0 - m1]
    assert all(o.dtype == F for o in out)
    return out


def transform(blocks, precision):
    """blocks uint16 [..., 8(y), 8(x)] -> H float32 [..., 8(h), 8(k)], before the division."""
    limit = F(2.0 ** precision - 1.0)
    level = F(2.0 ** (precision - 1) * 8.0)
    g = np.minimum(limit, np.asarray(blocks, np.uint16).astype(F))          # pointwiseMin(limit, v)
    f = np.stack(fdct8([g[..., :, x] for x in range(8)], level), axis=-2)   # [..., k, y]
    return np.stack(fdct8([f[..., :, y] for y in range(8)], F(0.0)), axis=-2)   # [..., h, k]


def quotient(blocks, q_zz, precision):
    """The unrounded quotient, float32 [..., h, k] (one IEEE division), with H and the divisors."""
    H, q = transform(blocks, precision), modulated(q_zz)
    v = H / q
    assert v.dtype == F
    return v, H, q


def round_half_away(v):
    """.toNearestOrAwayFromZero of float32 values, as int64 (exact in float64: |v| < 2^24)."""
    v = np.asarray(v, np.float64)
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def to_zigzag(a):
    """[..., h, k] -> [..., 64] in zigzag order."""
    out = np.empty(a.shape[:-2] + (64,), a.dtype)
    out[..., ZZ.reshape(-1)] = a.reshape(a.shape[:-2] + (64,))
    return out


def coefficients(blocks, q_zz, precision):
    """The restatement's coefficients, int64 [..., 64] zigzag."""
    return to_zigzag(round_half_away(quotient(blocks, q_zz, precision)[0]))


def blocks_of(plane):
    """uint16 [8 uy, 8 ux] -> [uy, ux, 8, 8]."""
    uy, ux = plane.shape[0] // 8, plane.shape[1] // 8
    return plane.reshape(uy, 8, ux, 8).transpose(0, 2, 1, 3)


def plane_of(blocks):
    """[uy, ux, 8, 8] -> [8 uy, 8 ux]."""
    uy, ux = blocks.shape[:2]
    return np.ascontiguousarray(blocks.transpose(0, 2, 1, 3).reshape(8 * uy, 8 * ux))


# ---- 2. the tie constructor --------------------------------------------------------------------------------------------

def phi(position):
    """int64 [8(y), 8(x)]: the basis pattern of an exact position."""
    k, h = position
    sx = S4 if k == 4 else np.ones(8, np.int64)
    sy = S4 if h == 4 else np.ones(8, np.int64)
    return sy[:, None] * sx[None, :]


def tie_multipliers(Q, precision):
    """Every odd m of both signs with H = 4 Q m reachable by moving each sample at most 2^(P-1) - 1 from mid-grey; beyond
    8 bits also |m / 2| < 32767 (the quotient must fit Int16, where the reference traps).  (Samples held constant over
    2 x 2 cells reach the same m: 4 Q |m| is a multiple of 4, spread over 16 cells of four samples.)"""
    top = 64 * (2 ** (precision - 1) - 1) // (4 * Q)
    if precision > 8:
        top = min(top, 65533)
    pos = np.arange(1, top + 1, 2, dtype=np.int64)
    return np.concatenate([pos, -pos])


def _spread(total, n, cap, rng):
    """int64 [len(total), n]: non-negative parts, each <= cap, of every total (total <= n cap), seeded and uneven."""
    total = np.asarray(total, np.int64)
    w = rng.random((len(total), n)) + 0.05
    a = np.minimum(np.floor(total[:, None] * (w / w.sum(1, keepdims=True))).astype(np.int64), cap)
    rem = total - a.sum(1)                                   # what the floor and the cap left over: to the first parts with room
    room = cap - a
    over = np.cumsum(room, 1) - rem[:, None]
    a += np.where(over <= 0, room, np.maximum(0, room - over))
    assert (a.sum(1) == total).all() and a.max(initial=0) <= cap
    return a


def tie_blocks(position, Q, precision, ms=None, cell=1, seed=0):
    """-> (uint16 [n, 8, 8], m int64 [n]): for every m of `ms` (default: tie_multipliers) a block whose H at `position` is
    4 Q m.  From mid-grey, the phi = +1 samples move up and the phi = -1 samples down (m > 0), or the other way (m < 0),
    by amounts that sum to 4 Q |m|."""
    ms = tie_multipliers(Q, precision) if ms is None else np.asarray(ms, np.int64)
    mid, cap = 2 ** (precision - 1), 2 ** (precision - 1) - 1
    rng = np.random.default_rng([seed, Q, precision, position[0], position[1], cell])
    total = 4 * Q * np.abs(ms)
    if cell == 1:
        a = _spread(total, 64, cap, rng).reshape(-1, 8, 8)
    else:
        assert cell == 2 and tuple(position) == (0, 0), "only the DC pattern is constant over 2 x 2 cells"
        a = _spread(total // 4, 16, cap, rng).reshape(-1, 4, 4).repeat(2, axis=1).repeat(2, axis=2)
    v = mid + np.sign(ms)[:, None, None] * phi(position)[None] * a
    assert v.min(initial=mid) >= 0 and v.max(initial=mid) < 2 ** precision
    return v.astype(np.uint16), ms


def table_for(Q, precision, seed=0):
    """uint16 [64] zigzag: Q at the four exact positions.  The other 60 entries are seeded, 1 .. 255, or 17 .. 255 at 16 bits:
    a coefficient is at most sum |v - mid| / 4 <= 16 (2^(P-1) - 1) in magnitude before the table, which stays inside Int16
    under any entry up to 12 bits and under entries >= 17 at 16 (the CPU module asserts it on the data)."""
    rng = np.random.default_rng([seed, Q, precision, 7])
    t = rng.integers(17 if precision > 12 else 1, 256, 64).astype(np.uint16)
    t[list(TIE_ZIGZAG)] = Q
    return t


# ---- 3. quantisers as functions of (H, q) --------------------------------------------------------------------------------

def reference_quantiser(H, q):
    return round_half_away(H / q)


def ties_to_even(H, q):
    return np.rint(H / q).astype(np.int64)


def ties_toward_zero(H, q):
    v = (H / q).astype(np.float64)
    return (np.sign(v) * np.ceil(np.abs(v) - 0.5)).astype(np.int64)


def floor_of_plus_half(H, q):
    return np.floor((H / q).astype(np.float64) + 0.5).astype(np.int64)


def half_without_sign(H, q):
    """trunc(v + pred(1/2)): the kernels' rounding with the half's sign lost."""
    return np.trunc((H / q) + PRED_HALF).astype(np.int64)


def uncorrected_reciprocal(H, q):
    """trunc(H RN(1 / q) + copysign(pred(1/2), .)): the kernels' form without Markstein's correction step (no fused
    operation is left in it)."""
    y0 = H * (F(1.0) / q)
    return np.trunc(y0 + np.copysign(PRED_HALF, y0)).astype(np.int64)


WRONG_QUANTISERS = {"ties to even": ties_to_even, "ties toward zero": ties_toward_zero, "floor(x + 1/2)": floor_of_plus_half,
                    "half without the sign": half_without_sign, "reciprocal without the correction step": uncorrected_reciprocal}


def _fma32(a, b, c):
    """RN(a b + c) for binary32 values held in Python floats: the product and the sum in integers, ONE rounding (to
    nearest, ties to even; normal range)."""
    (ma, ea), (mb, eb), (mc, ec) = math.frexp(a), math.frexp(b), math.frexp(c)
    p, ep = int(ma * 2 ** 24) * int(mb * 2 ** 24), ea + eb - 48          # 24-bit significands: the conversions are exact
    n, en = int(mc * 2 ** 24), ec - 24
    e0 = min(ep, en)
    s = (p << (ep - e0)) + (n << (en - e0))                                # a b + c = s 2^e0, exactly
    sign, s = (-1 if s < 0 else 1), abs(s)
    drop = s.bit_length() - 24
    if drop > 0:
        low, s, half = s & ((1 << drop) - 1), s >> drop, 1 << (drop - 1)
        if low > half or (low == half and s & 1):
            s += 1
        e0 += drop
    return sign * math.ldexp(s, e0)


def kernel_quantiser(H, q):
    """The form k_encode_fused and k_generic_fused compute (quantise.hpp), every operation rounded once: rr = RN(1 / q);
    y0 = RN(H rr); e = RN(H - y0 q) and y1 = RN(y0 + e rr) as FUSED multiply-adds, emulated exactly in integer arithmetic;
    z = RN(y1 + copysign(pred(1/2), y1)); trunc(z)."""
    H, q = np.broadcast_arrays(np.asarray(H, F), np.asarray(q, F))
    rr = F(1.0) / q
    y0 = H * rr
    y1 = np.empty(H.shape, F)
    flat = y1.reshape(-1)
    for i, (hh, qq, r, y) in enumerate(zip(H.reshape(-1).tolist(), q.reshape(-1).tolist(), rr.reshape(-1).tolist(), y0.reshape(-1).tolist())):
        flat[i] = _fma32(_fma32(-y, qq, hh), r, y)
    return np.trunc(y1 + np.copysign(PRED_HALF, y1)).astype(np.int64)


# ---- 4. the batches of the GPU tests ---------------------------------------------------------------------------------

FACTORS = {"grey": [(1, 1)], "444": [(1, 1), (1, 1), (1, 1)], "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)],
           "440": [(1, 2), (1, 1), (1, 1)]}
Q8 = tuple(range(1, 256))


def q16_set(seed=16):
    """The 16-bit table values: the edges, the largest prime below 2^16, and a seeded sample of 1 024."""
    rng = np.random.default_rng(seed)
    fixed = [1, 2, 255, 256, 257, 32767, 32768, 65521, 65535]
    return tuple(sorted(set(fixed) | set(int(v) for v in rng.choice(np.arange(1, 65536), 1024, replace=False))))


def sampled_multipliers(Q, precision, extra=4, seed=0):
    """m = +-1, +-3, the largest +-m, and `extra` seeded others per sign (all of them where there are no more)."""
    ms = tie_multipliers(Q, precision)
    pos = ms[ms > 0]
    if len(pos) <= 3 + extra:
        return ms
    rng = np.random.default_rng([seed, Q, precision, 11])
    pick = np.concatenate([pos[:2], pos[-1:], rng.choice(pos[2:-1], extra, replace=False)])
    return np.concatenate([pick, -pick])


@lru_cache(maxsize=None)
def cases(Q, precision, every_m=True, cell=1):
    """The tie blocks of one table value, the four positions one after the other -> (uint16 [n, 8, 8], position index [n],
    m [n]).  every_m: every multiplier (the 8-bit sets) or sampled_multipliers."""
    blocks, where, ms = [], [], []
    for i, pos in enumerate(POSITIONS if cell == 1 else POSITIONS[:1]):
        m = None if every_m else sampled_multipliers(Q, precision)
        b, m = tie_blocks(pos, Q, precision, m, cell)
        blocks.append(b); where.append(np.full(len(m), i)); ms.append(m)
    return np.concatenate(blocks), np.concatenate(where), np.concatenate(ms)


def has_ties(Q, precision):
    return len(tie_multipliers(Q, precision)) > 0


class Batch:
    """samples uint16 [n, H, W, planes]; tables uint16 [n, ntables, 64] (table 0: luma, table 1: both chroma planes);
    values[i] = (Q of table 0, Q of table 1); blocks[p]: the plane's blocks before the crop, [n, uy, ux, 8, 8]."""

    def __init__(self, name, precision, size, samples, tables, values, blocks):
        self.name, self.precision, self.size = name, precision, size
        self.factors = FACTORS[name]
        self.scale = (max(f[0] for f in self.factors), max(f[1] for f in self.factors))
        self.samples, self.tables, self.values, self.blocks = samples, tables, values, blocks
        self.n = len(samples)

    def plane_tables(self, i):
        return [self.tables[i][min(p, 1)] for p in range(len(self.factors))]

    def planar(self, i):
        """The oracle's decomposed() of image i."""
        return O.decompose(self.samples[i], self.size, self.factors, self.scale)

    def reference(self, i):
        """oracle.decompose + oracle.fdct_plane of image i: int16 [uy, ux, 64] per plane."""
        return [O.fdct_plane(p, t, self.precision) for p, t in zip(self.planar(i), self.plane_tables(i))]


def _take(blocks, n, start):
    return blocks[(start + np.arange(n)) % len(blocks)]


def batch(name, precision, pairs, grid=(40, 12), crop=(0, 0), every_m=True):
    """One image (or, where a value has more ties than an image has blocks, several) per pair (Q of the luma table, Q of
    the chroma table).  The image is grid[0] x grid[1] luma blocks, the blocks that value's ties, repeated to fill it; a
    chroma plane is filled likewise (Cb and Cr take alternate stretches of the chroma value's ties) and every chroma sample
    is replicated over its cell, so the encoder's box mean is exact.  crop: pixels taken off the right and the bottom
    (the last block column and row are then edge-replicated by the encoder)."""
    factors = FACTORS[name]
    sx, sy = max(f[0] for f in factors), max(f[1] for f in factors)
    gx, gy = grid
    assert gx % sx == 0 and gy % sy == 0
    cx, cy = gx // sx, gy // sy
    n_l, n_c = gx * gy, cx * cy
    images, tables, values = [], [], []
    for ql, qc in pairs:
        lum = cases(ql, precision, every_m)[0]
        chroma = cases(qc, precision, every_m)[0] if len(factors) == 3 else lum[:0]
        count = max(-(-len(lum) // n_l), -(-len(chroma) // (2 * n_c)) if len(factors) == 3 else 1)
        for k in range(count):
            planes = [_take(lum, n_l, k * n_l).reshape(gy, gx, 8, 8)]
            if len(factors) == 3:
                planes.append(_take(chroma, n_c, 2 * k * n_c).reshape(cy, cx, 8, 8))
                planes.append(_take(chroma, n_c, (2 * k + 1) * n_c).reshape(cy, cx, 8, 8))
            images.append(planes)
            tables.append(np.stack([table_for(ql, precision), table_for(qc, precision, seed=1)]))
            values.append((ql, qc))
    blocks = [np.stack([im[p] for im in images]) for p in range(len(factors))]
    w, h = 8 * gx - crop[0], 8 * gy - crop[1]
    full = [np.stack([plane_of(b) for b in blocks[0]])]
    for p in range(1, len(factors)):
        full.append(np.stack([plane_of(b) for b in blocks[p]]).repeat(sy, axis=1).repeat(sx, axis=2))
    samples = np.ascontiguousarray(np.stack(full, axis=-1)[:, :h, :w])
    return Batch(name, precision, (w, h), samples, np.stack(tables), values, blocks)


def pairs8():
    """Table 0 takes every Q = 1 .. 255, table 1 the value 256 - Q."""
    return [(q, 256 - q) for q in Q8]


def pairs16(precision):
    """The 16-bit values that admit a tie at this precision, each once in table 0 and once (in reverse order) in table 1."""
    qs = [q for q in q16_set() if has_ties(q, precision)]
    return list(zip(qs, qs[::-1]))


def grey_rgb_map():
    """uint8 [256, 3]: for every Y a near-grey RGB that oracle.pack_rgb8 maps to that Y (plain greys do not all map to
    themselves).  The nearest candidate by summed distance from (Y, Y, Y)."""
    out = np.zeros((256, 3), np.uint8)
    offs = sorted(((a, b, c) for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4)), key=lambda t: (sum(map(abs, t)), t))
    for y in range(256):
        cand = np.clip(np.array(offs) + y, 0, 255).astype(np.uint8)
        got = O.pack_rgb8(cand, 3)[:, 0]
        hit = np.flatnonzero(got == y)
        assert len(hit), y
        out[y] = cand[hit[0]]
    return out


def swing_images():
    """uint8 [n, 48, 80]: 0 / 255 checkerboards and 8-pixel stripes in both axes, in both phases -- the largest magnitudes of
    either sign a transform of 8-bit samples reaches."""
    yy, xx = np.mgrid[0:48, 0:80]
    pats = [(xx + yy) & 1, (xx >> 3) & 1, (yy >> 3) & 1, ((xx >> 3) + (yy >> 3)) & 1, xx & 1, yy & 1, (xx >> 2) & 1, (yy >> 1) & 1]
    return np.stack([p * 255 for p in pats] + [(1 - p) * 255 for p in pats]).astype(np.uint8)


def reduce_batch(denom, grid=(6, 4)):
    """Spectral reduce at 1/8 and 1/4: DC-only inputs under an all-ones table decode to freely chosen samples (one per input
    block at 1/8, a 2 x 2 cell at 1/4: sample = trunc(128.5 + DC / 8)), so the OUTPUT planes are tie blocks under the output
    table.  Per Q = 1 .. 255 one image with m = +-1, +-3 and the largest +-m (at 1/4 only the DC pattern is constant over the
    cells).  -> (coef int16 [255, uy, ux, 64], input size, samples uint16 [255, 8 gy, 8 gx], output tables uint16 [255, 1, 64])."""
    N = 8 // denom
    assert N in (1, 2)
    gx, gy = grid
    planes, tables = [], []
    for Q in Q8:
        blocks = []
        for pos in (POSITIONS if N == 1 else POSITIONS[:1]):
            blocks.append(tie_blocks(pos, Q, 8, sampled_multipliers(Q, 8, extra=0), cell=N)[0])
        planes.append(plane_of(_take(np.concatenate(blocks), gx * gy, 0).reshape(gy, gx, 8, 8)))
        tables.append(table_for(Q, 8)[None])
    samples = np.stack(planes)
    cells = samples[:, ::N, ::N]
    coef = np.zeros(cells.shape + (64,), np.int16)
    coef[..., 0] = 8 * (cells.astype(np.int64) - 128)
    return coef, (8 * cells.shape[2], 8 * cells.shape[1]), samples, np.stack(tables)
