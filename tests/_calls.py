"""What the tests of the C batch calls (region, scaled, view, resized, tensor and reduce decode) share, each stated once: the
C layout and the argument arrays, the synthetic inputs, the whole-image anchor, and an output buffer that is filled with a
sentinel before a call and checked after it.  Importing this needs no GPU and no torch: torch comes in through the fixture."""
import ctypes as C

import numpy as np
import pytest

import jpeg_amd as J
from jpeg_amd import _lib
from jpeg_amd.synth import natural_planes_torch

SENTINEL = 0xA5
COLORS = (_lib.COLOR_RGB8, _lib.COLOR_YCC8)
# the layouts the fused tile kernels take
FUSED = {"y8": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)],
         "440": [(1, 2), (1, 1), (1, 1)]}


@pytest.fixture(scope="module")
def ctx():
    return J.Context(0)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---- the arguments ------------------------------------------------------------------------------------------------------------

def c_layout(w, h, factors, scale=None, precision=8, qi=None):
    L = _lib.Layout()
    L.width, L.height, L.precision, L.nplanes = w, h, precision, len(factors)
    L.scale_x, L.scale_y = scale or (max(f[0] for f in factors), max(f[1] for f in factors))
    for p, (fx, fy) in enumerate(factors):
        L.factor_x[p], L.factor_y[p] = fx, fy
        L.qi[p] = min(p, 1) if qi is None else qi[p]
    assert _lib.lib().jpeg_amd_layout_units(C.byref(L)) == 0
    return L


def plane_units(L):
    return [(L.units_x[p], L.units_y[p]) for p in range(L.nplanes)]


def plane_factors(L):
    return [(L.factor_x[p], L.factor_y[p]) for p in range(L.nplanes)]


def strides(L, distinct=True):
    """Elements from one image's plane to the next; distinct=False: every image reads image 0."""
    return [64 * ux * uy if distinct else 0 for ux, uy in plane_units(L)] + [0] * (4 - L.nplanes)


def plane_ptrs(planes):
    return _lib.ptr_array([p.data_ptr() for p in planes])


def c_regions(regions):
    arr = (_lib.Region * max(len(regions), 1))()
    for i, r in enumerate(regions):
        arr[i].x, arr[i].y, arr[i].width, arr[i].height = (int(v) for v in r)
    return arr


def c_views(views):
    """views: (denom, (x, y, w, h)) or (denom, x, y, w, h)."""
    arr = (_lib.View * max(len(views), 1))()
    for i, v in enumerate(views):
        arr[i] = _lib.View(v[0], _lib.Region(*(v[1] if len(v) == 2 else v[1:])))
    return arr


# ---- the inputs ---------------------------------------------------------------------------------------------------------------

def synthetic(ctx, torch, L, n, seed, kind="natural"):
    """-> (planes [n, uy, ux, 64] per plane, dq [n, ntables, 64], ntables)."""
    if kind == "natural":
        planes = natural_planes_torch(plane_units(L), n, ctx.torch_device, seed=seed)
    else:                                                # "saturating": every int16, so that the clamp saturates at both ends
        assert kind == "saturating"
        gen = torch.Generator(device=ctx.torch_device).manual_seed(seed)
        planes = [torch.randint(-32768, 32768, (n, uy, ux, 64), dtype=torch.int32, device=ctx.torch_device, generator=gen)
                  .to(torch.int16) for ux, uy in plane_units(L)]
    ntables = 2 if L.nplanes == 3 else 1
    gen = torch.Generator(device=ctx.torch_device).manual_seed(seed + 1)
    dq = torch.randint(1, 24, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen)
    return planes, dq, ntables


def pixel_image(content, w, h, seed):
    """A host image [h, w, 3] of bytes for the resample calls."""
    if content == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "checker":                                # 0 / 255 per sample: both ends of the clamp and of the rounding
        yy, xx, cc = np.mgrid[0:h, 0:w, 0:3]
        return (((xx + yy + cc) & 1) * 255).astype(np.uint8)
    return np.full((h, w, 3), 0 if content == "zero" else 255, np.uint8)


def full_batch(ctx, torch, L, n, planes, coef_stride, dq, q_stride, ntables, cosited, color):
    """The whole images through jpeg_amd_decode_batch: the anchor of the region and scaled tests.  -> uint8 [n, H, W, 3]"""
    out = torch.empty((n, L.height, L.width, 3), dtype=torch.uint8, device=ctx.torch_device)
    assert _lib.lib().jpeg_amd_decode_batch(
        ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(coef_stride), dq.data_ptr(), q_stride, ntables, cosited,
        color, out.data_ptr(), 3 * L.width * L.height) == 0
    return out


# ---- the outputs --------------------------------------------------------------------------------------------------------------

def assert_only_spans_written(host, spans, sentinel=SENTINEL):
    """host: the bytes of a buffer that held `sentinel` everywhere before a call; spans: (first byte, bytes) of each image.
    Every byte that belongs to no image must still hold the sentinel."""
    mine = np.zeros(host.size, bool)
    for a, m in spans:
        mine[a:a + m] = True
    stray = np.flatnonzero(~mine & (host != sentinel))
    assert stray.size == 0, (int(stray.size), stray[:4].tolist())


def out_spans(counts, elem=1, gap=0, lead=0, tail=0):
    """The layout of an output buffer: image i has counts[i] elements of `elem` bytes; the images lie max(counts) + gap
    elements apart, the first one `lead` elements into the buffer, and `tail` elements of room follow the last image's stride.
    -> (stride in elements, bytes of the buffer, (first byte, bytes) of each image)"""
    stride = max(counts) + gap
    return stride, (lead + len(counts) * stride + tail) * elem, [((lead + i * stride) * elem, c * elem) for i, c in enumerate(counts)]


class Out:
    """A device buffer of bytes, all SENTINEL, laid out by out_spans for the n images of one call; it begins at an allocation
    boundary, so the first image lies `lead` elements behind one."""

    def __init__(self, ctx, torch, counts, elem=1, gap=0, lead=0, tail=0):
        self.stride, nbytes, self.spans = out_spans(list(counts), elem, gap, lead, tail)
        self.buf = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
        assert self.buf.data_ptr() % 256 == 0               # an allocation boundary
        self.ptr = self.buf.data_ptr() + lead * elem

    def untouched(self):
        return bool((self.buf == SENTINEL).all().item())

    def device(self, i):
        """The bytes of image i, still on the device; nothing is checked."""
        a, m = self.spans[i]
        return self.buf[a:a + m]

    def images(self):
        """The bytes of the n images on the host; asserts the sentinel in every byte that belongs to none of them."""
        host = self.buf.cpu().numpy()
        assert_only_spans_written(host, self.spans)
        return [host[a:a + m] for a, m in self.spans]


# ---- the resample calls: what the resized and the tensor tests share ----------------------------------------------------------

RESIZE_TILE_W, RESIZE_TILE_H = 64, 32                       # k_resize_bilinear's tile of output pixels
RESIZE_EXTENTS = [(1, 1), (2, 3), (7, 9), (131, 57), (449, 301)]   # (w, h) of the sources of one call
RESIZE_CONTENTS = ["random", "checker", "zero", "full"]
RESIZE_FACTORS = {"y8": FUSED["y8"], "420": FUSED["420"], "420-cosited": FUSED["420"]}
RESIZE_SIZE = (131, 257)
# denominators 1, 2, 4, 8 in one call; the scaled images are 131 x 257, 66 x 129, 33 x 65, 17 x 33
RESIZE_VIEWS = [(2, 3, 5, 60, 100), (1, 10, 20, 100, 200), (8, 0, 0, 17, 33), (4, 1, 1, 30, 60), (2, 65, 128, 1, 1)]


def resize_py_layout(name):
    if name == "y8":
        return J.Layout("y8", {1: J.Component((1, 1), 0)})
    return J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})


def resized_call(ctx, L, planes, dq, ntables, cosited, color, views, out_w, out_h, out_ptr, stride, layout=None):
    return _lib.lib().jpeg_amd_decode_resized_batch(
        ctx.handle, C.byref(layout or L), len(views), plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64,
        ntables, cosited, color, c_views(views), out_w, out_h, out_ptr, stride)
