"""The tensor-source contract of include/jpeg_amd.h ("tensor sources") restated in numpy: an element as float32, times scale,
plus offset -- two float32 operations -- the clamp through fmax / fmin (which return the other operand for a NaN) and the
rounding byte conversion.  Elements travel as BIT PATTERNS (uint32 for F32, uint16 for F16 and BF16, uint8 for U8), so that
NaNs, infinities, -0 and subnormals are pinned.  Independent of the code under test.  Also: the buffers the GPU tests build."""
import numpy as np

import _tensor_ref as T
from _calls import SENTINEL, Out

F = np.float32
F32, F16, BF16, U8 = 0, 1, 2, 3   # JPEG_AMD_F32 ... JPEG_AMD_U8
HWC, CHW = T.HWC, T.CHW
DTYPES, LAYOUTS = (F32, F16, BF16, U8), (HWC, CHW)
BITS = {F32: np.uint32, F16: np.uint16, BF16: np.uint16, U8: np.uint8}
ELEM = {F32: 4, F16: 2, BF16: 2, U8: 1}
DTYPE_NAMES = {F32: "f32", F16: "f16", BF16: "bf16", U8: "u8"}
LAYOUT_NAMES = {HWC: "hwc", CHW: "chw"}

# ImageNet's mean and std in 0 ... 1 units, and the 0 ... 1 convention
IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


class Source:
    """dtype, layout and the constants rounded to float32 once, as the caller of the C ABI rounds them."""

    def __init__(self, dtype, layout, scale=(1.0, 1.0, 1.0), offset=(0.0, 0.0, 0.0)):
        self.dtype, self.layout = dtype, layout
        self.scale = np.asarray(scale, np.float64).astype(F)
        self.offset = np.asarray(offset, np.float64).astype(F)


def inverse(dtype, layout, mean, std):
    """The source that inverts tensor_spec(mean, std): scale = float32(255 std), offset = float32(255 mean), each computed in
    float64 and rounded once."""
    return Source(dtype, layout, [255.0 * s for s in std], [255.0 * m for m in mean])


def forward_spec(dtype, layout, mean, std):
    """_tensor_ref's Spec of the torchvision convention: mean_b = float32(255 mean), scale = float32(1 / (255 std))."""
    return T.Spec(dtype, layout, [255.0 * m for m in mean], [1.0 / (255.0 * s) for s in std])


def values(bits, dtype):
    """Element bit patterns -> their float32 values (exact for every dtype)."""
    bits = np.asarray(bits)
    assert bits.dtype == BITS[dtype]
    if dtype == F32:
        return np.ascontiguousarray(bits).view(F)
    if dtype == F16:
        return np.ascontiguousarray(bits).view(np.float16).astype(F)
    if dtype == BF16:
        return np.ascontiguousarray(bits.astype(np.uint32) << np.uint32(16)).view(F)
    return bits.astype(F)


def to_bits(v, dtype):
    """float32 values -> element bit patterns of dtype, round to nearest even (for making test inputs)."""
    v = np.ascontiguousarray(v, F)
    if dtype == F32:
        return v.view(np.uint32).copy()
    if dtype == F16:
        with np.errstate(over="ignore"):
            return v.astype(np.float16).view(np.uint16).copy()
    if dtype == BF16:
        return T.bf16_bits(v)
    return np.clip(np.nan_to_num(v), 0, 255).astype(np.uint8)


def pixels(bits, src):
    """The element bit patterns of one image, [H, W, 3] (HWC) or [3, H, W] (CHW) -> the contract's bytes uint8 [H, W, 3]."""
    bits = np.asarray(bits)
    assert bits.ndim == 3 and bits.shape[2 if src.layout == HWC else 0] == 3
    if src.layout == CHW:
        bits = bits.transpose(1, 2, 0)
    if src.dtype == U8:
        assert bits.dtype == np.uint8
        return np.ascontiguousarray(bits)
    f = values(bits, src.dtype)
    with np.errstate(invalid="ignore", over="ignore"):
        p = f * src.scale
        s = p + src.offset
        b = np.fmin(np.fmax(s, F(0)), F(255))
        r = b + F(0.5)
    assert p.dtype == F and s.dtype == F and b.dtype == F and r.dtype == F
    return np.ascontiguousarray(r.astype(np.int32).astype(np.uint8))


# ---- special values: (element as float32, the byte under scale 1 and offset 0) --------------------------------------------------
SPECIALS = [(F("nan"), 0), (F("inf"), 255), (F("-inf"), 0), (F(-0.0), 0), (F(0.49999997), 1), (F(254.49998), 254),
            (F(254.5), 255), (F(255.4), 255)]


def random_elements(rng, dtype, shape):
    """Element bit patterns whose values span [-64, 320] in byte units under scale 1, offset 0: both clamps bind."""
    if dtype == U8:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    return to_bits(rng.uniform(-64.0, 320.0, shape).astype(F), dtype)


def with_specials(bits, dtype, layout):
    """`bits` ([H, W, 3] or [3, H, W]) with SPECIALS (as far as the dtype holds them) at the first and the last element of
    rows, channel by channel; a copy."""
    bits = bits.copy()
    if dtype == U8:
        return bits
    hwc = bits if layout == HWC else bits.transpose(1, 2, 0)      # a view: writes go through
    h, w = hwc.shape[:2]
    for k, (v, _) in enumerate(SPECIALS):
        hwc[k % h, 0 if k % 2 == 0 else w - 1, k % 3] = to_bits(np.asarray([v], F), dtype)[0]
        hwc[(k + 1) % h, w - 1 if k % 2 == 0 else 0, (k + 1) % 3] = to_bits(np.asarray([v], F), dtype)[0]
    return bits


# ---- device buffers of the GPU tests ------------------------------------------------------------------------------------------------

class SourceIn:
    """n images of element bit patterns on the device, `gap` elements between them, the first one `lead` elements behind an
    allocation boundary; the elements that belong to no image hold a pattern of their own."""

    def __init__(self, ctx, torch, images, dtype, gap=0, lead=0):
        self.elem = ELEM[dtype]
        n, count = len(images), images[0].size
        self.stride = count + gap
        host = np.full((lead + n * self.stride + 3) * self.elem, 0x5A, np.uint8)
        for i, im in enumerate(images):
            a = (lead + i * self.stride) * self.elem
            host[a:a + count * self.elem] = np.ascontiguousarray(im).reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(host).to(ctx.torch_device)
        assert self.buf.data_ptr() % 256 == 0               # an allocation boundary
        self.ptr = self.buf.data_ptr() + lead * self.elem


class PixelsOut(Out):
    """The output of one front call: n images of 3 w h bytes, `gap` bytes between them, all SENTINEL before the call."""

    def __init__(self, ctx, torch, n, w, h, gap=0, lead=0):
        super().__init__(ctx, torch, [3 * w * h] * n, elem=1, gap=gap, lead=lead, tail=7)
        self.shape = (h, w, 3)

    def images(self):
        return [b.reshape(self.shape) for b in super().images()]


class CoefOut:
    """The coefficient planes of one encode call: per plane an Out of n images of 64 ux uy int16, 8 elements (16 bytes, what
    a block is aligned to) between them."""

    def __init__(self, ctx, torch, L, n):
        self.units = [(L.units_x[p], L.units_y[p]) for p in range(L.nplanes)]
        self.outs = [Out(ctx, torch, [64 * ux * uy] * n, elem=2, gap=8, tail=8) for ux, uy in self.units]

    def ptrs(self):
        return [o.ptr for o in self.outs]

    def strides(self):
        return [o.stride for o in self.outs] + [0] * (4 - len(self.outs))

    def untouched(self):
        return all(o.untouched() for o in self.outs)

    def planes(self):
        """[plane][image] int16 [uy, ux, 64]; asserts the sentinel everywhere else."""
        return [[b.copy().view(np.int16).reshape(uy, ux, 64) for b in o.images()] for o, (ux, uy) in zip(self.outs, self.units)]


assert SENTINEL == 0xA5
