"""The bicubic warp contract of include/jpeg_amd.h ("bicubic warp") restated in numpy, float32 throughout: every statement of the
contract is one numpy operation on float32 arrays, so nothing is fused and the result is the contract's, bit for bit.  The
coordinates up to the clamp are "projective resample"'s and are restated here, not imported, because the clamp differs.  Below
it jpeg_amd_project_filter_view restated with Python floats (doubles), math.floor and one float32 rounding: _project_ref's
restatement with the footprint's margin as a parameter.  Independent of the code under test."""
import math

import numpy as np

import _project_ref
from _orient import BITS
from _project_ref import scaled_size

F = np.float32
FILL, REPLICATE = 0, 1            # JPEG_AMD_EDGE_*
BILINEAR, ANTIALIAS, BICUBIC = 0, 1, 3   # JPEG_AMD_FILTER_*


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
    sx = np.minimum(np.maximum(sx, F(-2.0)), F(w) + F(1.0))
    sy = ny * rw
    sy = sy - F(0.5)
    sy = np.minimum(np.maximum(sy, F(-2.0)), F(h) + F(1.0))
    assert sx.dtype == F and sy.dtype == F and rw.dtype == F and sx.shape == (out_h, out_w) and sy.shape == (out_h, out_w)
    assert np.isfinite(sx).all() and np.isfinite(sy).all() and (nw > 0).all()
    return sx, sy


def weight(x):
    """The weight of a distance x >= 0, float32 in and out: "bicubic resample"'s two lines."""
    assert x.dtype == F and (x >= 0).all()
    near = ((F(1.5) * x - F(2.5)) * x) * x + F(1.0)
    far = ((((x - F(5.0)) * x + F(8.0)) * x) - F(4.0)) * F(-0.5)
    w = np.where(x < F(1.0), near, np.where(x < F(2.0), far, F(0.0)))
    assert w.dtype == F
    return w


def axis_weights(f):
    """The four weights of a fraction f (float32 [...]) -> float32 [4, ...]: distances f + 1, f, 1 - f, 2 - f."""
    return [weight(f + F(1.0)), weight(f), weight(F(1.0) - f), weight(F(2.0) - f)]


def project(image, m, out_w, out_h, edge=FILL, fill=(0, 0, 0), flip=False):
    """uint8 [h, w, 3] through the homography m (9 values, rounded to float32 here) with the bicubic filter -> uint8
    [out_h, out_w, 3].  flip: the columns are stored mirrored (xs = out_w - 1 - x), which only the tensor calls do."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3 and edge in (FILL, REPLICATE)
    h, w = image.shape[:2]
    sx, sy = coordinates(m, w, h, out_w, out_h, flip)
    fx0, fy0 = np.floor(sx), np.floor(sy)
    x0, y0 = fx0.astype(np.int32), fy0.astype(np.int32)
    fx, fy = sx - fx0, sy - fy0
    assert fx.dtype == F and fy.dtype == F
    assert x0.min() >= -2 and x0.max() <= w + 1 and y0.min() >= -2 and y0.max() <= h + 1
    wx = [v[..., None] for v in axis_weights(fx)]
    wy = [v[..., None] for v in axis_weights(fy)]
    img = image.astype(F)
    fill_f = np.asarray(fill, np.uint8).astype(F).reshape(1, 1, 3)

    def tap(yi, xi):
        inside = (xi >= 0) & (xi <= w - 1) & (yi >= 0) & (yi <= h - 1)
        v = img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)]           # REPLICATE: the indices clamped into the image
        return v if edge == REPLICATE else np.where(inside[..., None], v, fill_f)

    rows = []
    for j in range(4):
        yi = y0 + np.int32(j - 1)
        t = [tap(yi, x0 + np.int32(i - 1)) for i in range(4)]
        r = wx[0] * t[0]
        r = r + wx[1] * t[1]
        r = r + wx[2] * t[2]
        r = r + wx[3] * t[3]
        assert r.dtype == F
        rows.append(r)
    v = wy[0] * rows[0]
    v = v + wy[1] * rows[1]
    v = v + wy[2] * rows[2]
    v = v + wy[3] * rows[3]
    v = np.minimum(np.maximum(v, F(0.0)), F(255.0)) + F(0.5)
    assert v.dtype == F and v.shape == (out_h, out_w, 3)
    return v.astype(np.int32).astype(np.uint8)


def project_filter(image, m, filter, out_w, out_h, edge=FILL, fill=(0, 0, 0), flip=False):
    """jpeg_amd_project_filter_batch on one image: with BILINEAR the existing call, whose mirror is _project_ref's."""
    assert filter in (BILINEAR, BICUBIC)
    if filter == BILINEAR:
        return _project_ref.project(image, m, out_w, out_h, edge, fill, flip)
    return project(image, m, out_w, out_h, edge, fill, flip)


def taps_inside(m, w, h, out_w, out_h):
    """bool [out_h, out_w]: the pixels all of whose 4 x 4 taps lie inside the image."""
    sx, sy = coordinates(m, w, h, out_w, out_h)
    x0, y0 = np.floor(sx).astype(np.int32), np.floor(sy).astype(np.int32)
    return (x0 - 1 >= 0) & (x0 + 2 <= w - 1) & (y0 - 1 >= 0) & (y0 + 2 <= h - 1)


def project_filter_view(w, h, orientation, m, filter, out_w, out_h):
    """jpeg_amd_project_filter_view for a stored image of w x h -> ((denom, x, y, width, height), m_view float32 [9]).  The
    footprint's margin is 1 + 2 pixels with the bilinear filter and 2 + 3 with the bicubic one; the rest is one text."""
    assert filter in (BILINEAR, BICUBIC)
    wider = 1 if filter == BICUBIC else 0
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

    x0, x1 = clamp(math.floor(min(xsv) - 0.5) - 1 - wider, ws - 1), clamp(math.floor(max(xsv) - 0.5) + 2 + wider, ws - 1)
    y0, y1 = clamp(math.floor(min(ysv) - 0.5) - 1 - wider, hs - 1), clamp(math.floor(max(ysv) - 0.5) + 2 + wider, hs - 1)
    mv = [r0[k] - float(x0) * r2[k] for k in range(3)] + [r1[k] - float(y0) * r2[k] for k in range(3)] + list(r2)
    return (denom, x0, y0, x1 - x0 + 1, y1 - y0 + 1), np.asarray(mv, np.float64).astype(F)
