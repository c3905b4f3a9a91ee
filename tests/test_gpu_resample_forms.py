"""The exported narrow forms that neither a public Python function nor another GPU test reaches any more, on the MI355X: each
is its wide form with NULL for what it lacks (csrc/capi_view.hip, csrc/capi_files.hip), so both are called through ctypes on
the same two images and must leave the same bits: the output tensor inside a sentinel-filled buffer (whose bytes in front of,
between and behind the images are checked) and everything written back to the host -- views, windows, matrices, frame infos,
orientations.  The inputs are the smallest that still cross what can differ: two images of different size and layout, a
10 x 6 canvas, one flip set, orientation 6 on one image, a "fit" placement with a non-zero fill, a small shear for the map."""
import ctypes as C

import numpy as np
import pytest

import _files as F
import jpeg_amd as J
from _calls import Out
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, same
from jpeg_amd import _lib
from jpeg_amd.api import _mixed_args

pytestmark = pytest.mark.gpu

N, OUT_W, OUT_H = 2, 10, 6
FLIPS, ORIENT = [1, 0], [6, 1]
SHEAR = np.array([[1.5, 0.2, 0.5, 0.1, 3.5, 1.0], [1.5, 0.2, 0.0, 0.0, 2.5, 0.5]], np.float32)   # against the UPRIGHT images


@pytest.fixture(scope="module")
def files():
    """4:2:0 at 24 x 16 and 4:4:4 at 16 x 16."""
    return [F.synthetic_file("420", (24, 16), 61)[0], F.synthetic_file("444", (16, 16), 62)[0]]


@pytest.fixture(scope="module")
def spectrals(ctx, files):
    return [J.Spectral.decompress(ctx, d) for d in files]


def room():
    """Where a call writes its results on the host: windows, views, frame infos, matrices, orientations."""
    return {"windows": (_lib.Region * N)(), "views": (_lib.View * N)(), "infos": (_lib.FrameInfo * N)(),
            "matrices": np.full((N, 6), np.nan, np.float32), "applied": (C.c_int32 * N)(-1, -1)}


UNTOUCHED = {key: bytes(r) for key, r in room().items()}


class Call:
    """The arguments both forms of a pair share, a guarded output and the room for what they write back, fresh for each form."""

    def __init__(self, ctx, torch):
        self.spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
        self.target = (C.byref(self.spec), c_bytes(FLIPS))
        self.out = Out(ctx, torch, [3 * OUT_W * OUT_H] * N, elem=2, gap=5, lead=4, tail=7)
        self.dst = (self.out.ptr, self.out.stride)
        self.place = _lib.Placement(_lib.PLACE_FIT, _lib.ANCHOR_CENTRE, None, (C.c_uint8 * 3)(7, 8, 9), 0)
        self.warp = _lib.Warp(_lib.EDGE_FILL, (C.c_uint8 * 3)(3, 4, 5))
        self.room = room()
        self.windows, self.views, self.infos, self.matrices, self.applied = self.room.values()

    def written(self, ctx, status):
        """-> everything the call left behind, as bytes."""
        assert status == 0
        ctx.synchronize()
        return dict({key: bytes(r) for key, r in self.room.items()}, images=self.out.images())


def same_written(narrow, wide, touched):
    for i in range(N):
        same(narrow["images"][i], wide["images"][i], i)
        assert narrow["images"][i].any()                          # (something was decoded: not two empty canvases)
    for key in UNTOUCHED:
        assert narrow[key] == wide[key], key
        assert (key in touched) == (narrow[key] != UNTOUCHED[key]), key


def mixed_head(ctx, spectrals, views):
    vs, h_images, h_views, keep = _mixed_args(ctx, spectrals, views)
    return (ctx.handle, N, h_images, 0, _lib.COLOR_RGB8), h_views, keep


def file_head(ctx, files):
    ptrs = (C.c_void_p * N)(*[d.ctypes.data for d in files])
    return (ctx.handle, ptrs, (C.c_size_t * N)(*[d.size for d in files]), N, 2, 0, _lib.COLOR_RGB8)


def test_decode_tensor_placed_mixed_is_the_colour_form_without_a_colour(ctx, torch, spectrals):
    head, h_views, keep = mixed_head(ctx, spectrals, [(1, 0, 0, 24, 16), (1, 0, 0, 16, 16)])
    L, got = _lib.lib(), []
    for wide in (False, True):
        c = Call(ctx, torch)
        columns = (c_bytes(ORIENT), C.byref(c.place), c.windows)
        args = head + (h_views, OUT_W, OUT_H, _lib.FILTER_BILINEAR) + c.target + columns
        got.append(c.written(ctx, L.jpeg_amd_decode_tensor_colour_mixed(*args, None, *c.dst) if wide else
                             L.jpeg_amd_decode_tensor_placed_mixed(*args, *c.dst)))
    same_written(*got, touched={"windows"})
    assert np.frombuffer(got[0]["windows"], np.int32).reshape(N, 4).tolist() == [[3, 0, 4, 6], [2, 0, 6, 6]]   # 16 x 24 and 16 x 16, fitted


def test_decode_tensor_warped_mixed_is_the_colour_form_without_a_colour(ctx, torch, spectrals):
    head, h_views, keep = mixed_head(ctx, spectrals, np.zeros((N, 5), np.int32))
    L, got = _lib.lib(), []
    for wide in (False, True):
        c = Call(ctx, torch)
        args = head + (c_bytes(ORIENT), SHEAR.ctypes.data, C.byref(c.warp), OUT_W, OUT_H) + c.target + (c.views, c.matrices.ctypes.data)
        got.append(c.written(ctx, L.jpeg_amd_decode_tensor_warped_colour_mixed(*args, None, *c.dst) if wide else
                             L.jpeg_amd_decode_tensor_warped_mixed(*args, *c.dst)))
    same_written(*got, touched={"views", "matrices"})


def test_decompress_tensor_placed_mixed_is_the_colour_form_without_a_colour(ctx, torch, files):
    head = file_head(ctx, files)
    L, got = _lib.lib(), []
    for wide in (False, True):
        c = Call(ctx, torch)
        columns = (c_bytes(ORIENT), C.byref(c.place), c.windows)
        args = head + (None, OUT_W, OUT_H, _lib.FILTER_BILINEAR) + c.target + columns
        tail = c.dst + (c.infos, c.views, c.applied)
        got.append(c.written(ctx, L.jpeg_amd_decompress_tensor_colour_mixed(*args, None, *tail) if wide else
                             L.jpeg_amd_decompress_tensor_placed_mixed(*args, *tail)))
    same_written(*got, touched={"windows", "views", "infos", "applied"})
    assert np.frombuffer(got[0]["applied"], np.int32).tolist() == ORIENT


def test_decompress_tensor_warped_mixed_is_the_colour_form_without_a_colour(ctx, torch, files):
    head = file_head(ctx, files)
    L, got = _lib.lib(), []
    for wide in (False, True):
        c = Call(ctx, torch)
        args = head + (c_bytes(ORIENT), SHEAR.ctypes.data, C.byref(c.warp), OUT_W, OUT_H) + c.target
        tail = c.dst + (c.infos, c.views, c.matrices.ctypes.data, c.applied)
        got.append(c.written(ctx, L.jpeg_amd_decompress_tensor_warped_colour_mixed(*args, None, *tail) if wide else
                             L.jpeg_amd_decompress_tensor_warped_mixed(*args, *tail)))
    same_written(*got, touched={"views", "infos", "matrices", "applied"})
    assert np.frombuffer(got[0]["applied"], np.int32).tolist() == ORIENT
