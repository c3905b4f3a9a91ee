"""The warp contract of include/jpeg_amd.h ("warped resample") restated in numpy, float32 throughout: every statement of the
contract is one numpy operation on float32 arrays, so nothing is fused and the result is the contract's, bit for bit.  Below
it jpeg_amd_warp_view restated with Python floats (doubles), math.floor and one float32 rounding.  Independent of the code
under test."""
import math

import numpy as np

from _orient import BITS

F = np.float32
FILL, REPLICATE = 0, 1            # JPEG_AMD_EDGE_*


def warp(image, m, out_w, out_h, edge=FILL, fill=(0, 0, 0), flip=False):
    """uint8 [h, w, 3] through the matrix m (6 values, rounded to float32 here) -> uint8 [out_h, out_w, 3].  flip: the columns
    are stored mirrored (xs = out_w - 1 - x), which only the tensor calls do."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and edge in (FILL, REPLICATE)
    h, w = image.shape[:2]
    m = np.asarray(m, np.float64).astype(F).reshape(6)
    xs = np.arange(out_w, dtype=np.int32)
    if flip:
        xs = np.int32(out_w - 1) - xs
    xc = (xs.astype(F) + F(0.5))[None, :]
    yc = (np.arange(out_h, dtype=np.int32).astype(F) + F(0.5))[:, None]
    sx = ((m[0] * xc) + (m[1] * yc)) + m[2]
    sx = sx - F(0.5)
    sx = np.minimum(np.maximum(sx, F(-1.0)), F(w))
    sy = ((m[3] * xc) + (m[4] * yc)) + m[5]
    sy = sy - F(0.5)
    sy = np.minimum(np.maximum(sy, F(-1.0)), F(h))
    assert sx.dtype == F and sy.dtype == F and sx.shape == (out_h, out_w) and sy.shape == (out_h, out_w)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    x0, y0 = fx0.astype(np.int32), fy0.astype(np.int32)
    x1, y1 = x0 + np.int32(1), y0 + np.int32(1)
    fx, fy = (sx - fx0)[..., None], (sy - fy0)[..., None]
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


def scaled_size(w, h, denom):
    n = 8 // denom
    return (w * n + 7) // 8, (h * n + 7) // 8


def warp_view(w, h, orientation, m, out_w, out_h):
    """jpeg_amd_warp_view for a stored image of w x h -> ((denom, x, y, width, height), m_view float32 [6])."""
    m = [float(v) for v in np.asarray(m, np.float64).astype(F).reshape(6)]
    T, fx, fy = BITS[orientation]
    rx, ry = (m[3:6], m[0:3]) if T else (m[0:3], m[3:6])
    if fx:
        rx = [-rx[0], -rx[1], float(w) - rx[2]]
    if fy:
        ry = [-ry[0], -ry[1], float(h) - ry[2]]
    step2 = min(m[0] * m[0] + m[3] * m[3], m[1] * m[1] + m[4] * m[4])
    denom = next((d for d in (8, 4, 2) if float(d * d) <= step2), 1)
    f = float(8 // denom) / 8.0
    s = [v * f for v in list(rx) + list(ry)]
    ws, hs = scaled_size(w, h, denom)
    corners = [(0.0, 0.0), (float(out_w), 0.0), (0.0, float(out_h)), (float(out_w), float(out_h))]
    xsv = [(s[0] * cx + s[1] * cy) + s[2] for cx, cy in corners]
    ysv = [(s[3] * cx + s[4] * cy) + s[5] for cx, cy in corners]

    def clamp(v, last):
        return int(min(max(v, 0), last))

    x0, x1 = clamp(math.floor(min(xsv) - 0.5) - 1, ws - 1), clamp(math.floor(max(xsv) - 0.5) + 2, ws - 1)
    y0, y1 = clamp(math.floor(min(ysv) - 0.5) - 1, hs - 1), clamp(math.floor(max(ysv) - 0.5) + 2, hs - 1)
    s[2] = s[2] - float(x0)
    s[5] = s[5] - float(y0)
    return (denom, x0, y0, x1 - x0 + 1, y1 - y0 + 1), np.asarray(s, np.float64).astype(F)
