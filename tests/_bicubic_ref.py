"""The bicubic filter of include/jpeg_amd.h ("bicubic resample") restated in numpy, float32 throughout: every statement of
the contract is one numpy operation on float32 values, the totals and the accumulations are explicit ascending loops (no
np.sum, whose order is numpy's), so nothing is fused or reordered and the result is the contract's, bit for bit.
Independent of the code under test (and of _antialias_ref: the passes are written out again here)."""
import numpy as np

F = np.float32
MAX_TAPS = 33          # 4 s + 1 at s = 8
MAX_SCALE = F(8.0)


def weight(u):
    """The Keys cubic with a = -0.5 at u (float32 array), each step one float32 operation in the contract's order."""
    x = np.abs(u)
    assert x.dtype == F
    near = x * F(1.5)
    near = near - F(2.5)
    near = near * x
    near = near * x
    near = near + F(1.0)
    far = x - F(5.0)
    far = far * x
    far = far + F(8.0)
    far = far * x
    far = far - F(4.0)
    far = far * F(-0.5)
    assert near.dtype == F and far.dtype == F
    return np.where(x < F(1.0), near, np.where(x < F(2.0), far, F(0.0))).astype(F)


def axis_table(n_out, n):
    """-> (lo [n_out] int32, count [n_out] int32, W [n_out, taps] float32) of an axis of n source samples resampled to n_out;
    W[j, i] is the normalised weight of tap lo[j] + i, zero behind count[j]."""
    k = F(n) / F(n_out)
    s = np.maximum(k, F(1.0))
    r = F(1.0) / s
    p = F(2.0) * s
    j = np.arange(n_out, dtype=np.int32).astype(F)
    c = (j + F(0.5)) * k
    assert c.dtype == F and r.dtype == F and p.dtype == F
    lo = np.maximum(((c - p) + F(0.5)).astype(np.int32), np.int32(0))
    hi = np.minimum(((c + p) + F(0.5)).astype(np.int32), np.int32(n))
    count = hi - lo
    assert count.min() >= 1 and count.max() <= MAX_TAPS, (n, n_out, int(count.min()), int(count.max()))
    taps = int(count.max())
    w = np.zeros((n_out, taps), F)
    for i in range(taps):
        t = (lo + np.int32(i)).astype(F)
        u = ((t - c) + F(0.5)) * r
        assert u.dtype == F
        w[:, i] = np.where(i < count, weight(u), F(0.0))
    total = w[:, 0].copy()
    for i in range(1, taps):                                # left to right; a tap behind count adds nothing (total + 0 = total)
        total = np.where(i < count, total + w[:, i], total)
    assert total.dtype == F
    W = w / total[:, None]
    assert W.dtype == F
    return lo, count, W


def axis_total(n_out, n):
    """The contract's `total` per output (before the division), for the checks on the reference."""
    lo, count, W = axis_table(n_out, n)
    k = F(n) / F(n_out)
    r = F(1.0) / np.maximum(k, F(1.0))
    c = (np.arange(n_out, dtype=np.int32).astype(F) + F(0.5)) * k
    total = None
    for i in range(W.shape[1]):
        wi = np.where(i < count, weight((((lo + np.int32(i)).astype(F) - c) + F(0.5)) * r), F(0.0))
        total = wi if total is None else np.where(i < count, total + wi, total)
    return total


def _pass(img, lo, count, W, axis):
    """One pass along `axis` of float32 img: out[j] = (...((0 + W[j, 0] img[lo[j]]) + W[j, 1] img[lo[j] + 1]) + ...)."""
    n = img.shape[axis]
    shape = [1, 1, 1]
    shape[axis] = -1
    acc = np.zeros(tuple(len(lo) if a == axis else img.shape[a] for a in range(3)), F)
    for i in range(W.shape[1]):
        live = (i < count).reshape(shape)
        idx = np.minimum(lo + i, n - 1)                     # a tap behind count is not read: its product is dropped below
        prod = W[:, i].reshape(shape) * np.take(img, idx, axis=axis)
        acc = np.where(live, acc + prod, acc)
        assert acc.dtype == F
    return acc


def resize(image, out_w, out_h):
    """uint8 [h, w, 3] -> uint8 [out_h, out_w, 3]: the horizontal pass first, kept as float32, then the vertical pass, then
    the clamp (live here: the weights are negative in the lobes) and the rounding."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3
    h, w = image.shape[:2]
    xlo, xcount, Wx = axis_table(out_w, w)
    ylo, ycount, Wy = axis_table(out_h, h)
    hp = _pass(image.astype(F), xlo, xcount, Wx, 1)
    v = _pass(hp, ylo, ycount, Wy, 0)
    v = np.minimum(np.maximum(v, F(0.0)), F(255.0)) + F(0.5)
    assert v.dtype == F
    return v.astype(np.int32).astype(np.uint8)
