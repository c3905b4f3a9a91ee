"""The colour stage of include/jpeg_amd.h ("colour stage") restated in numpy, float32 throughout and ONE operation per
statement.  The contract is by reference: it takes the BYTES that one of the existing mirrors (_resize_ref, _antialias_ref,
_bicubic_ref, _placed_ref, _warp_ref) defines for an image, mirrors them where the call flips, applies the image's affine map
of (R, G, B) and the clamp, and ends in _tensor_ref's subtraction, multiplication and conversion.  Results are BIT PATTERNS, as
_tensor_ref's.  Independent of the code under test; importing this needs no GPU and no torch."""
import numpy as np

import _tensor_ref as T

F = np.float32
NO_CLAMP = (-np.inf, np.inf)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], F)


def matrix(k):
    """Twelve numbers as the caller of the C ABI rounds them: float32 [3, 4]."""
    return np.asarray(k, np.float64).astype(F).reshape(3, 4)


def permutation(order):
    """Output channel c is input channel order[c]."""
    k = np.zeros((3, 4), F)
    for c, s in enumerate(order):
        k[c, s] = 1
    return k


def mapped(image, k, clamp=NO_CLAMP):
    """uint8 [H, W, 3], float32 [3, 4], (lo, hi) -> q, float32 [H, W, 3]."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    k = np.asarray(k)
    assert k.dtype == F and k.shape == (3, 4)
    lo, hi = F(clamp[0]), F(clamp[1])
    r, g, b = image[..., 0].astype(F), image[..., 1].astype(F), image[..., 2].astype(F)
    out = np.empty(image.shape, F)
    for c in range(3):
        m0 = k[c, 0] * r
        m1 = k[c, 1] * g
        m2 = k[c, 2] * b
        p = m0 + m1
        p = p + m2
        q = p + k[c, 3]
        assert m0.dtype == F and p.dtype == F and q.dtype == F
        q = np.where(q < lo, lo, q)         # two comparisons and selects: -0 is not below +0 and stays
        q = np.where(q > hi, hi, q)
        assert q.dtype == F
        out[..., c] = q
    return out


def convert(q, spec):
    """_tensor_ref.normalise from its subtraction on: float32 [H, W, 3] -> the element bit patterns in spec's layout."""
    t = q - spec.mean
    v = t * spec.scale
    assert t.dtype == F and v.dtype == F
    if spec.dtype == T.F32:
        bits = np.ascontiguousarray(v).view(np.uint32)
    elif spec.dtype == T.F16:
        bits = np.ascontiguousarray(v.astype(np.float16)).view(np.uint16)
    else:
        bits = T.bf16_bits(v)
    return np.ascontiguousarray(bits.transpose(2, 0, 1)) if spec.layout == T.CHW else bits


def normalise(image, k, clamp, spec, flip):
    """The bytes of an existing mirror -> the elements of the colour call: [Ht, Wt, 3] (HWC) or [3, Ht, Wt] (CHW)."""
    image = np.asarray(image)
    if flip:
        image = image[:, ::-1]
    return convert(mapped(image, k, clamp), spec)
