"""The resample contract of include/jpeg_amd.h ("resized decode") restated in numpy, float32 throughout: every statement of
the contract is one numpy operation on float32 arrays, so nothing is fused and the result is the contract's, bit for bit.
Independent of the code under test."""
import numpy as np

F = np.float32


def axis_taps(n_out, n):
    """-> (i0, i1, f) of every output index of an axis of n source samples resampled to n_out."""
    k = F(n) / F(n_out)
    j = np.arange(n_out, dtype=np.int32).astype(F)
    s = (j + F(0.5)) * k - F(0.5)
    s = np.maximum(s, F(0.0))
    assert s.dtype == F
    i0 = np.minimum(s.astype(np.int32), np.int32(n - 1))
    i1 = np.minimum(i0 + np.int32(1), np.int32(n - 1))
    f = s - i0.astype(F)
    assert f.dtype == F
    return i0, i1, f


def resize(image, out_w, out_h):
    """uint8 [h, w, 3] -> uint8 [out_h, out_w, 3]: the horizontal pass first, then the vertical pass."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3
    h, w = image.shape[:2]
    x0, x1, fx = axis_taps(out_w, w)
    y0, y1, fy = axis_taps(out_h, h)
    img = image.astype(F)
    fx, fy = fx[None, :, None], fy[:, None, None]
    a, b = img[y0][:, x0], img[y0][:, x1]
    c, d = img[y1][:, x0], img[y1][:, x1]
    top = a + fx * (b - a)
    bot = c + fx * (d - c)
    v = top + fy * (bot - top)
    v = np.minimum(np.maximum(v, F(0.0)), F(255.0)) + F(0.5)
    assert v.dtype == F
    return v.astype(np.int32).astype(np.uint8)
