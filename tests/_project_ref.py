"""The projective contract of include/jpeg_amd.h ("projective resample") restated in numpy, float32 throughout: every statement
of the contract is one numpy operation on float32 arrays, so nothing is fused and the result is the contract's, bit for bit
(numpy's float32 division is IEEE's, correctly rounded).  Below it jpeg_amd_project_view restated with Python floats (doubles),
math.floor and one float32 rounding, and the contract's conditioning check.  Independent of the code under test."""
import math

import numpy as np

from _orient import BITS

F = np.float32
FILL, REPLICATE = 0, 1            # JPEG_AMD_EDGE_*


def coordinates(m, w, h, out_w, out_h, flip=False):
    """The clamped source coordinates (sx, sy), float32 [out_h, out_w] each, of the contract."""
    m = np.asarray(m, np.float64).astype(F).reshape(9)
    xs = np.arange(out_w, dtype=np.int32)
    if flip:
        xs = np.int32(out_w - 1) - xs
    xc = (xs.astype(F) + F(0.5))[None, :]
    yc = (np.arange(out_h, dtype=np.int32).astype(F) + F(0.5))[:, None]
    nx = ((m[0] * xc) + (m[1] * yc)) + m[2]
    ny = ((m[3] * xc) + (m[4] * yc)) + m[5]
    nw = ((m[6] * xc) + (m[7] * yc)) + m[8]
    rw = F(1.0) / nw
    sx = nx * rw
    sx = sx - F(0.5)
    sx = np.minimum(np.maximum(sx, F(-1.0)), F(w))
    sy = ny * rw
    sy = sy - F(0.5)
    sy = np.minimum(np.maximum(sy, F(-1.0)), F(h))
    assert sx.dtype == F and sy.dtype == F and rw.dtype == F and sx.shape == (out_h, out_w) and sy.shape == (out_h, out_w)
    assert np.isfinite(sx).all() and np.isfinite(sy).all() and (nw > 0).all()
    return sx, sy


def taps(sx, sy):
    """-> x0, y0 (int32), fx, fy (float32): "warped resample" from fx0 = floorf(sx) on."""
    fx0, fy0 = np.floor(sx), np.floor(sy)
    return fx0.astype(np.int32), fy0.astype(np.int32), sx - fx0, sy - fy0


def project(image, m, out_w, out_h, edge=FILL, fill=(0, 0, 0), flip=False):
    """uint8 [h, w, 3] through the homography m (9 values, rounded to float32 here) -> uint8 [out_h, out_w, 3].  flip: the
    columns are stored mirrored (xs = out_w - 1 - x), which only the tensor calls do."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and edge in (FILL, REPLICATE)
    h, w = image.shape[:2]
    sx, sy = coordinates(m, w, h, out_w, out_h, flip)
    x0, y0, fx, fy = taps(sx, sy)
    x1, y1 = x0 + np.int32(1), y0 + np.int32(1)
    fx, fy = fx[..., None], fy[..., None]
    assert fx.dtype == F and fy.dtype == F
    assert x0.min() >= -1 and x0.max() <= w and y0.min() >= -1 and y0.max() <= h
    img = image.astype(F)
    fill_f = np.asarray(fill, np.uint8).astype(F).reshape(1, 1, 3)

    def tap(yi, xi):
        inside = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        v = img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)]           # REPLICATE: the indices clamped into the image
        return v if edge == REPLICATE else np.where(inside[..., None], v, fill_f)

    a, b, c, d = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    v = top + fy * (bot - top)
    v = np.minimum(np.maximum(v, F(0.0)), F(255.0)) + F(0.5)
    assert v.dtype == F and v.shape == (out_h, out_w, 3)
    return v.astype(np.int32).astype(np.uint8)


def conditioning(m, out_w, out_h):
    """-> (S, min W) of the contract's check, in double, of a matrix of float32 entries."""
    m = [float(v) for v in np.asarray(m, np.float64).astype(F).reshape(9)]
    s = (abs(m[6]) * out_w + abs(m[7]) * out_h) + abs(m[8])
    low = min(m[8], m[6] * out_w + m[8], m[7] * out_h + m[8], (m[6] * out_w + m[7] * out_h) + m[8])
    return s, low


def accepted(m, out_w, out_h):
    m32 = np.asarray(m, np.float64).astype(F).reshape(9)
    if not np.isfinite(m32).all() or np.abs(m32.astype(np.float64)).max() > 2.0 ** 30:
        return False
    s, low = conditioning(m, out_w, out_h)
    return s >= 2.0 ** -30 and low >= s / 16.0


def scaled_size(w, h, denom):
    n = 8 // denom
    return (w * n + 7) // 8, (h * n + 7) // 8


def project_view(w, h, orientation, m, out_w, out_h):
    """jpeg_amd_project_view for a stored image of w x h -> ((denom, x, y, width, height), m_view float32 [9])."""
    m = [float(v) for v in np.asarray(m, np.float64).astype(F).reshape(9)]
    T, fx, fy = BITS[orientation]
    r0, r1, r2 = (m[3:6], m[0:3], m[6:9]) if T else (m[0:3], m[3:6], m[6:9])
    if fx:
        r0 = [float(w) * r2[k] - r0[k] for k in range(3)]
    if fy:
        r1 = [float(h) * r2[k] - r1[k] for k in range(3)]
    points = [(0.0, 0.0), (float(out_w), 0.0), (0.0, float(out_h)), (float(out_w), float(out_h)), (0.5 * out_w, 0.5 * out_h)]
    norms = []
    for px, py in points:
        nw = (m[6] * px + m[7] * py) + m[8]
        X = ((m[0] * px + m[1] * py) + m[2]) / nw
        Y = ((m[3] * px + m[4] * py) + m[5]) / nw
        for c in range(2):
            jx, jy = (m[c] - X * m[6 + c]) / nw, (m[3 + c] - Y * m[6 + c]) / nw
            norms.append(jx * jx + jy * jy)
    step2 = min(norms)
    denom = next((d for d in (8, 4, 2) if float(d * d) <= step2), 1)
    f = float(8 // denom) / 8.0
    r0, r1 = [v * f for v in r0], [v * f for v in r1]
    ws, hs = scaled_size(w, h, denom)
    xsv, ysv = [], []
    for cx, cy in points[:4]:
        nw = (r2[0] * cx + r2[1] * cy) + r2[2]
        xsv.append(((r0[0] * cx + r0[1] * cy) + r0[2]) / nw)
        ysv.append(((r1[0] * cx + r1[1] * cy) + r1[2]) / nw)

    def clamp(v, last):
        return int(min(max(v, 0), last))

    x0, x1 = clamp(math.floor(min(xsv) - 0.5) - 1, ws - 1), clamp(math.floor(max(xsv) - 0.5) + 2, ws - 1)
    y0, y1 = clamp(math.floor(min(ysv) - 0.5) - 1, hs - 1), clamp(math.floor(max(ysv) - 0.5) + 2, hs - 1)
    mv = [r0[k] - float(x0) * r2[k] for k in range(3)] + [r1[k] - float(y0) * r2[k] for k in range(3)] + list(r2)
    return (denom, x0, y0, x1 - x0 + 1, y1 - y0 + 1), np.asarray(mv, np.float64).astype(F)


def homography(src_points, out_points):
    """The 3 x 3 (float64, m22 = 1) that takes the four out_points to the four src_points: eight equations, numpy's solver."""
    a, b = [], []
    for (x, y), (u, v) in zip(out_points, src_points):
        a += [[x, y, 1, 0, 0, 0, -u * x, -u * y], [0, 0, 0, x, y, 1, -v * x, -v * y]]
        b += [u, v]
    return np.append(np.linalg.solve(np.asarray(a, np.float64), np.asarray(b, np.float64)), 1.0).reshape(3, 3)


def distortion(rng, w, h, out_w, out_h, scale=0.5, outside=0.0):
    """A seeded four-corner distortion in torchvision's manner: each corner of the source moves inwards by up to scale / 2 of
    the side (RandomPerspective's distortion_scale), or with `outside` > 0 outwards by up to that share of the side; the
    canvas's corners map to them.  -> float32 [9]."""
    def corner(cx, cy):
        dx = rng.uniform(-outside, scale / 2.0) * w
        dy = rng.uniform(-outside, scale / 2.0) * h
        return (dx if cx == 0 else w - dx, dy if cy == 0 else h - dy)

    src = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]
    out = [(0, 0), (out_w, 0), (out_w, out_h), (0, out_h)]
    return homography(src, out).reshape(9).astype(F)
