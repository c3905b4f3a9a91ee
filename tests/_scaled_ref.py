"""Test-side reference of scaled decode: an independent numpy restatement of the contract in include/jpeg_amd.h
("scaled decode").  float32 arrays, one explicit binary32 operation per statement, in the contract's order -- never
np.sum, whose pairwise order differs.  The interleave and colour stage is the oracle's, on planes padded to whole blocks
by edge replication: orc_interleave_rows clamps the neighbour against the plane it is given, and replication makes
min(i + 1, 8 units' - 1) read the value min(i + 1, N units - 1) reads."""
import numpy as np

from oracle import oracle as O

F = np.float32
R8 = [F(1.0), F(1.387039845), F(1.306562965), F(1.175875602), F(1.0), F(0.785694958), F(0.541196100), F(0.275899379)]


def _zigzag_table():
    """z[h][k]: the zigzag index of horizontal frequency k, vertical frequency h -- the standard walk."""
    z = np.zeros((8, 8), np.int64)
    k = h = 0
    for i in range(64):
        z[h][k] = i
        if (k + h) % 2 == 0:            # moving up-right
            if k == 7:
                h += 1
            elif h == 0:
                k += 1
            else:
                k, h = k + 1, h - 1
        else:                           # moving down-left
            if h == 7:
                k += 1
            elif k == 0:
                h += 1
            else:
                k, h = k - 1, h + 1
    return z


Z = _zigzag_table()


def scaled_size(size, denom):
    n = 8 // denom
    return (size[0] * n + 7) // 8, (size[1] * n + 7) // 8


def table(q_zz, N):
    """q_N[h][k] = (rN[k] * rN[h]) * (0x1p-3 * Float(Q[z(k, h)])), rN[i] = r[8 i / N]."""
    q_zz = np.asarray(q_zz, np.uint16).reshape(64)
    rn = [R8[8 * i // N] for i in range(N)]
    return [[F(F(rn[k] * rn[h]) * F(F(0.125) * F(q_zz[Z[h][k]]))) for k in range(N)] for h in range(N)]


def butterfly(h, shift, N):
    """The contract's N-point butterfly on a list of N float32 arrays."""
    e = shift + h[0]
    if N == 1:
        return [e]
    if N == 2:
        return [e + h[1], e - h[1]]
    a0 = e + h[2]
    a1 = e - h[2]
    b = h[1] + h[3]
    d = h[1] - h[3]
    m = F(1.414213562) * d
    c = m - b
    return [a0 + b, a1 + c, a1 - c, a0 - b]


def idct_plane_scaled(coef, q_zz, N, precision=8):
    """coef int16 [uy, ux, 64] zigzag -> uint16 [N uy, N ux]."""
    coef = np.asarray(coef, np.int16)
    uy, ux, _ = coef.shape
    q = table(q_zz, N)
    level = F(2.0 ** (precision - 1) + 0.5)
    limit = F(2.0 ** precision - 1.0)
    f = []                                              # f[k][y]: arrays [uy, ux]
    for k in range(N):
        h = [q[hh][k] * coef[:, :, Z[hh][k]].astype(F) for hh in range(N)]
        f.append(butterfly(h, F(0.0), N))
    out = np.empty((N * uy, N * ux), np.uint16)
    for y in range(N):
        g = butterfly([f[k][y] for k in range(N)], level, N)
        for x in range(N):
            assert g[x].dtype == F
            out[y::N, x::N] = np.minimum(np.maximum(g[x], F(0.0)), limit).astype(np.uint16)   # clamp, truncate
    return out


def pad_planes(planes):
    """Edge replication up to multiples of 8 samples per axis."""
    return [np.pad(p, ((0, -p.shape[0] % 8), (0, -p.shape[1] % 8)), mode="edge") for p in planes]


def interleaved_scaled(planes, quanta, factors, size, denom, cosited=False, scale=None):
    """-> (the padded scaled planes, uint16 [H', W', count])."""
    N = 8 // denom
    if scale is None:
        scale = (max(f[0] for f in factors), max(f[1] for f in factors))
    padded = pad_planes([idct_plane_scaled(c, q, N) for c, q in zip(planes, quanta)])
    return padded, O.interleave(padded, factors, scale, scaled_size(size, denom), cosited)


def decode_scaled(planes, quanta, factors, size, denom, cosited=False, rgb=True, scale=None):
    """planes[p]: int16 [uy, ux, 64]; quanta[p]: plane p's table -> uint8 [H', W', 3]."""
    _, rect = interleaved_scaled(planes, quanta, factors, size, denom, cosited, scale)
    w, h = scaled_size(size, denom)
    return (O.unpack_rgb8 if rgb else O.unpack_ycc8)(rect, len(planes)).reshape(h, w, 3)


def textbook_plane(coef, q_zz, N, precision=8):
    """float64: (N / 8) x the orthonormal N-point 2-D IDCT of the top-left N x N dequantised coefficients, plus level,
    clamped, truncated.  -> (uint16 [N uy, N ux], the float64 values before clamp and truncation)."""
    coef = np.asarray(coef, np.int16)
    uy, ux, _ = coef.shape
    q = np.asarray(q_zz, np.float64).reshape(64)
    Fq = np.zeros((uy, ux, N, N))                       # [.., h, k]
    for h in range(N):
        for k in range(N):
            Fq[:, :, h, k] = coef[:, :, Z[h][k]].astype(np.float64) * q[Z[h][k]]
    basis = np.zeros((N, N))                            # basis[i][t] = a(i) cos((2 t + 1) i pi / (2 N))
    for i in range(N):
        a = np.sqrt((1.0 if i == 0 else 2.0) / N)
        for t in range(N):
            basis[i][t] = a * np.cos((2 * t + 1) * i * np.pi / (2 * N))
    s = np.einsum("hy,kx,bchk->bcyx", basis, basis, Fq) * (N / 8.0) + (2.0 ** (precision - 1) + 0.5)
    v = s.transpose(0, 2, 1, 3).reshape(N * uy, N * ux)
    return np.floor(np.clip(v, 0.0, 2.0 ** precision - 1.0)).astype(np.uint16), v
