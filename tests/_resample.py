"""What the tests of the resample family share (test_gpu_resize, _tensor, _antialias, _bicubic, _oriented, _resample_family):
the C forms of a spec and of per-image bytes, the packed sources of a raw call, and the exact comparison."""
import ctypes as C

import numpy as np

import _orient as E
import _tensor_ref as T
from jpeg_amd import _lib


def c_spec(spec):
    """A _tensor_ref.Spec as the C struct."""
    s = _lib.TensorSpec()
    s.dtype, s.layout = spec.dtype, spec.layout
    for c in range(3):
        s.mean[c], s.scale[c] = float(spec.mean[c]), float(spec.scale[c])
    return s


def c_bytes(values):
    """Per-image flips or orientations as a C array, or None for NULL."""
    return None if values is None else (C.c_uint8 * max(len(values), 1))(*[int(v) for v in values])


def pack(ctx, torch, images, gap=3):
    """Host images [h, w, 3] in one device allocation, `gap` bytes of 0x5A behind the largest -> (tensor, stride, extents)."""
    n = len(images)
    stride = max(im.size for im in images) + gap
    src = np.full(n * stride, 0x5A, np.uint8)
    for i, im in enumerate(images):
        src[i * stride:i * stride + im.size] = im.reshape(-1)
    return torch.from_numpy(src).to(ctx.torch_device), stride, (_lib.Extent * n)(*[_lib.Extent(im.shape[1], im.shape[0]) for im in images])


def same(got, want, what):
    """got is want: dtype, shape and every value, the first four mismatches in the message.  A flat `got` -- an image as
    _calls.Out hands it out -- has no shape of its own and is compared with want's values in order."""
    got, want = np.asarray(got), np.asarray(want)
    if got.ndim == 1:
        want = want.reshape(-1)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist(), [int(got[tuple(b)]) for b in bad[:4]], [int(want[tuple(b)]) for b in bad[:4]])


def host_bits(b, spec):
    """The bytes of an image of a tensor call, on the host, as bit patterns of spec's dtype."""
    return np.asarray(b).copy().view(T.BITS[spec.dtype])


def tensor_bits(t, torch):
    """A device tensor of a tensor call as bit patterns on the host."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()]).cpu().numpy().view({4: np.uint32, 2: np.uint16}[t.element_size()])


def torch_orient(torch, t, o):
    """A contiguous oriented copy of a device image [h, w, 3], made with torch."""
    transpose, fx, fy = E.BITS[o]
    if fy:
        t = t.flip(0)
    if fx:
        t = t.flip(1)
    if transpose:
        t = t.transpose(0, 1)
    return t.contiguous()
