"""Test-side reference of spectral reduce (include/jpeg_amd.h, "spectral reduce"): no arithmetic of its own.  Per plane:
_scaled_ref.idct_plane_scaled (the scaled-decode contract's samples), edge replication to the 8 x units' of the recomputed
layout, oracle.fdct_plane (Spectral.Plane.fdct)."""
import numpy as np

import _scaled_ref as S
from oracle import oracle as O


def _ceil(a, b):
    return -(-a // b)


def reduce_geometry(size, factors, scale, denom):
    """-> ((W', H'), [(ux', uy')]): the scaled size, and the units recomputed from it as jpeg_amd_layout_units does."""
    N = 8 // denom
    w, h = _ceil(size[0] * N, 8), _ceil(size[1] * N, 8)
    return (w, h), [(_ceil(w * fx, 8 * scale[0]), _ceil(h * fy, 8 * scale[1])) for fx, fy in factors]


def replicate(samples, units):
    """samples [N uy, N ux] -> [8 uy', 8 ux']: sample (x, y) = S(min(x, N ux - 1), min(y, N uy - 1))."""
    ux, uy = units
    ys = np.minimum(np.arange(8 * uy), samples.shape[0] - 1)
    xs = np.minimum(np.arange(8 * ux), samples.shape[1] - 1)
    return np.ascontiguousarray(samples[np.ix_(ys, xs)])


def reduced_samples(coef, q_in, denom, units, precision=8):
    """The output plane's samples: uint16 [8 uy', 8 ux']."""
    return replicate(S.idct_plane_scaled(coef, q_in, 8 // denom, precision), units)


def reduce_plane(coef, q_in, denom, units, q_out=None, precision=8):
    """coef int16 [uy, ux, 64] -> int16 [uy', ux', 64]; q_out None = q_in."""
    return O.fdct_plane(reduced_samples(coef, q_in, denom, units, precision), q_in if q_out is None else q_out, precision)


def reduce_image(planes, quanta, factors, scale, size, denom, quanta_out=None, precision=8):
    """planes[p] int16 [uy, ux, 64]; quanta[p]: plane p's table (quanta_out likewise, None = quanta) ->
    ((W', H'), [int16 [uy', ux', 64]])."""
    out_size, units = reduce_geometry(size, factors, scale, denom)
    qo = quanta if quanta_out is None else quanta_out
    return out_size, [reduce_plane(c, q, denom, u, r, precision) for c, q, u, r in zip(planes, quanta, units, qo)]
