"""The tensor-output contract of include/jpeg_amd.h ("tensor output") restated in numpy: the resampled bytes (_resize_ref),
mirrored, minus mean, times scale -- two float32 operations -- then the dtype's rounding and the layout.  Results are BIT
PATTERNS (uint32 for F32, uint16 for F16 and BF16), so that -0 and the rounding are pinned.  Independent of the code under test."""
import numpy as np

import _resize_ref as R

F = np.float32
F32, F16, BF16 = 0, 1, 2          # JPEG_AMD_F32 ...
HWC, CHW = 0, 1                   # JPEG_AMD_TENSOR_HWC ...
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16}
DTYPES, LAYOUTS = (F32, F16, BF16), (HWC, CHW)

# the constants of the sweeps, in byte units: ImageNet's mean and std times 255
MEAN = (123.675, 116.28, 103.53)
SCALE = tuple(1.0 / s for s in (58.395, 57.12, 57.375))
# exact zeros and -0: (128 - 128) * -1
SIGNED_ZERO = ((0.0, 128.0, 255.0), (1.0, -1.0, 0.5))


class Spec:
    """dtype, layout and the constants rounded to float32 once, as the caller of the C ABI rounds them."""

    def __init__(self, dtype, layout, mean=MEAN, scale=SCALE):
        self.dtype, self.layout = dtype, layout
        self.mean = np.asarray(mean, np.float64).astype(F)
        self.scale = np.asarray(scale, np.float64).astype(F)


def bf16_bits(v):
    """float32 array -> the bfloat16 bit patterns, round to nearest even."""
    bits = np.ascontiguousarray(v, F).view(np.uint32).astype(np.uint64)
    return ((bits + np.uint64(0x7fff) + ((bits >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def normalise(image, spec, flip):
    """uint8 [Ht, Wt, 3] -> the element bit patterns, [Ht, Wt, 3] (HWC) or [3, Ht, Wt] (CHW)."""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3 and image.shape[2] == 3
    if flip:
        image = image[:, ::-1]
    t = image.astype(F) - spec.mean
    v = t * spec.scale
    assert t.dtype == F and v.dtype == F
    if spec.dtype == F32:
        bits = np.ascontiguousarray(v).view(np.uint32)
    elif spec.dtype == F16:
        bits = np.ascontiguousarray(v.astype(np.float16)).view(np.uint16)
    else:
        bits = bf16_bits(v)
    return np.ascontiguousarray(bits.transpose(2, 0, 1)) if spec.layout == CHW else bits


def tensor(image, out_w, out_h, spec, flip):
    """The tensor of a source image uint8 [h, w, 3]."""
    return normalise(R.resize(image, out_w, out_h), spec, flip)
