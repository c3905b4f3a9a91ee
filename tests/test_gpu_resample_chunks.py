"""The resized and tensor decodes across their 1 GiB chunk seam on the MI355X: calls of two and three chunks (resample_chunks in
csrc/capi_view.hip with i0 > 0: the record, ColourRecord and destination offsets of ResampleTarget::launch, a chunk's own stride
in its records' source offsets, the slicing of the images, and a chunk decoded into the buffer the chunk before it was read from).

The limit counts stride x images, so one large view and a hundred small ones cross it while next to nothing is decoded
(_chunk_seam holds the scenarios; test_resample_chunks_cpu checks their splits against the library's own header).  Every
per-image argument varies with the index -- orientation 1 + i % 8, flip i % 2, a random colour matrix, a matrix of its own, tables
of its own -- so that no image of a later chunk is the image at its place in the first.

Two layers, both exact (bit patterns):
  1. split invariance, on every image: the whole call is the same entry point called on each expected chunk's images alone
     (calls of one chunk, which the tests of each entry point hold to the mirrors) -- the pixels and every per-image result;
  2. independent mirrors, on Places.subset() / uniform_subset(): the image's view decoded alone (n = 1), through the numpy mirrors.

Device memory: the context's view buffer grows to 1 GiB (one chunk) and is released with the module's own context; the uniform
calls' 120 distinct y8 images of 2048 x 1536 are 0.76 GB of coefficients; the mixed calls' entries alias eight device images
(22 MB); an output buffer is 95 MB at most, two at a time."""
import ctypes as C

import numpy as np
import pytest

import _antialias_ref as A
import _bicubic_ref as B
import _chunk_seam as S
import _colour_ref as K
import _mixed as M
import _orient as E
import _placed_ref as P
import _project_ref as PR
import _resize_ref as R
import _tensor_ref as T
import _warp_ref as W
import jpeg_amd as J
from _calls import FUSED, Out, c_layout, c_views, plane_ptrs, strides, synthetic
from _calls import torch  # noqa: F401  (the fixture)
from _resample import c_bytes, c_spec, host_bits as bits, same
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
BILINEAR, AA, BICUBIC = _lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS, _lib.FILTER_BICUBIC
COLOR = _lib.COLOR_RGB8
FILL = (7, 130, 255)
CLAMP = (0.0, 255.0)


@pytest.fixture(scope="module")
def ctx():
    """The module's own context: closing it releases the 1 GiB view buffer."""
    c = J.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pool(ctx, torch):
    """The device images of the mixed calls, one per kind, and a table pair per entry of the longest call."""
    kinds = {}
    for k, (name, (what, size)) in enumerate(S.KINDS.items()):
        L = c_layout(size[0], size[1], FUSED[what] if isinstance(what, str) else what)
        planes, _, ntables = synthetic(ctx, torch, L, 1, 900 + 2 * k)
        kinds[name] = (L, planes, ntables)
    gen = torch.Generator(device=ctx.torch_device).manual_seed(77)
    tables = torch.randint(1, 24, (300, 2, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen)
    yield kinds, tables
    kinds.clear()
    del tables
    torch.cuda.empty_cache()


def entries(pool, pl, n=None):
    """The jpeg_amd_image entries of a scenario: entry i aliases the planes of its kind and has the tables i."""
    kinds, tables = pool
    made = []
    for i in range(pl.n if n is None else n):
        L, planes, ntables = kinds[pl.kind(i)]
        made.append((L, [p.data_ptr() for p in planes], tables[i].data_ptr(), ntables))
    return made


def view_alone(ctx, torch, entry, view):
    """The pixels of one entry's view through jpeg_amd_decode_view_mixed with n = 1 -> uint8 [h, w, 3] on the host."""
    w, h = int(view[3]), int(view[4])
    buf = torch.empty(3 * w * h, dtype=torch.uint8, device=ctx.torch_device)
    assert M.view_mixed(ctx.handle, [entry], 0, COLOR, [tuple(int(v) for v in view)], buf.data_ptr(), 0) == 0
    ctx.synchronize()
    return buf.cpu().numpy().reshape(h, w, 3)


def colours(n, seed):
    rng = np.random.default_rng(seed)
    return np.stack([J.colour_matrix(*rng.uniform(0.6, 1.4, 3), rng.uniform(-0.1, 0.1), grey=bool(i % 7 == 3)) for i in range(n)]).astype(F32)


def c_colour(k, clamp):
    keep = np.ascontiguousarray(k, F32).reshape(-1, 12)
    c = _lib.Colour()
    c.h_matrices, c.lo, c.hi = keep.ctypes.data, clamp[0], clamp[1]
    return keep, c


def c_warp(edge):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = FILL
    return w


def c_fit():
    p = _lib.Placement()
    p.mode, p.anchor = P.FIT, P.CENTRE
    p.fill[0], p.fill[1], p.fill[2] = FILL
    return p


class Result:
    """Images [lo, hi) of a cell through its entry point: the bytes of each, and what the call returns per image."""

    def __init__(self, images, windows=None, views=None, matrices=None):
        self.images, self.windows, self.views, self.matrices = images, windows, views, matrices


# ---- the cells --------------------------------------------------------------------------------------------------------------------------

class Cell:
    spec = None                                             # a _tensor_ref.Spec, or None for bytes

    def __init__(self, ctx, torch):
        self.ctx, self.torch = ctx, torch

    def out(self, m):
        elem = 1 if self.spec is None else 4 if self.spec.dtype == T.F32 else 2
        return Out(self.ctx, self.torch, [3 * self.canvas[0] * self.canvas[1]] * m, elem=elem, gap=5, lead=3, tail=7)

    def done(self, status, out, **more):
        assert status == 0
        self.ctx.synchronize()
        return Result(out.images(), **more)

    def got(self, result, j):
        return result.images[j] if self.spec is None else bits(result.images[j], self.spec)


class UniformCell(Cell):
    """jpeg_amd_decode_resized_batch / jpeg_amd_decode_tensor_filter_batch: 120 images of one y8 layout, each with its own
    coefficients and its own table."""
    n = S.UNIFORM_N

    def __init__(self, ctx, torch, data):
        super().__init__(ctx, torch)
        self.L, self.planes, self.dq, self.ntables = data
        self.views = S.uniform_views()
        self.chunks = S.expected_chunks(self.views)
        self.subset = S.uniform_subset()
        self.flips = S.flips(self.n)

    def head(self, lo, hi):
        return (self.ctx.handle, C.byref(self.L), hi - lo, plane_ptrs([p[lo:] for p in self.planes]), _lib.size_array(strides(self.L)),
                self.dq[lo:].data_ptr(), self.ntables * 64, self.ntables, 0, COLOR, c_views(self.views[lo:hi]))

    def pixels(self, i):
        v = self.views[i]
        buf = self.torch.empty(3 * v[3] * v[4], dtype=self.torch.uint8, device=self.ctx.torch_device)
        assert _lib.lib().jpeg_amd_decode_view_batch(*self.head(i, i + 1), buf.data_ptr(), 0) == 0
        self.ctx.synchronize()
        return buf.cpu().numpy().reshape(v[4], v[3], 3)


class UniformBytes(UniformCell):
    canvas = (70, 37)

    def run(self, lo, hi):
        out = self.out(hi - lo)
        return self.done(_lib.lib().jpeg_amd_decode_resized_batch(*self.head(lo, hi), *self.canvas, out.ptr, out.stride), out)

    def mirror(self, i, whole):
        return R.resize(self.pixels(i), *self.canvas)


class UniformAntialias(UniformCell):
    """(The uniform calls take no orientations: their records are the stored ones, here the antialiasing filter's.)"""
    canvas = (130, 97)                                      # 2048 / 130 and 1536 / 97 are below 16
    spec = T.Spec(T.F16, T.CHW)

    def run(self, lo, hi):
        out = self.out(hi - lo)
        cs = c_spec(self.spec)
        return self.done(_lib.lib().jpeg_amd_decode_tensor_filter_batch(*self.head(lo, hi), *self.canvas, AA, C.byref(cs),
                                                                        c_bytes(self.flips[lo:hi]), out.ptr, out.stride), out)

    def mirror(self, i, whole):
        return T.normalise(A.resize(self.pixels(i), *self.canvas), self.spec, self.flips[i])


class MixedCell(Cell):
    """The mixed calls with views: _chunk_seam.MIXED, three chunks."""

    def __init__(self, ctx, torch, pool):
        super().__init__(ctx, torch)
        self.places = S.MIXED
        self.n = self.places.n
        self.views = S.mixed_views()
        self.chunks = S.check_places(self.places, self.views)
        self.subset = self.places.subset()
        self.entries = entries(pool, self.places)
        self.orient, self.flips = S.orientations(self.n), S.flips(self.n)
        self.k = colours(self.n, 11)

    def head(self, lo, hi):
        return (self.ctx.handle, hi - lo, M.c_images(self.entries[lo:hi]), 0, COLOR, c_views(self.views[lo:hi]))

    def pixels(self, i, whole):
        return view_alone(self.ctx, self.torch, self.entries[i], self.views[i])


class MixedBytes(MixedCell):
    canvas = (70, 37)

    def run(self, lo, hi):
        out = self.out(hi - lo)
        return self.done(_lib.lib().jpeg_amd_decode_resized_mixed(*self.head(lo, hi), *self.canvas, out.ptr, out.stride), out)

    def mirror(self, i, whole):
        return R.resize(self.pixels(i, whole), *self.canvas)


class MixedOriented(MixedCell):
    canvas = (130, 129)                                     # 2048 / 129 is below 16, whichever way an orientation turns the view
    spec = T.Spec(T.F32, T.CHW)

    def run(self, lo, hi):
        out = self.out(hi - lo)
        cs = c_spec(self.spec)
        return self.done(_lib.lib().jpeg_amd_decode_tensor_oriented_mixed(*self.head(lo, hi), *self.canvas, AA, C.byref(cs), c_bytes(self.flips[lo:hi]),
                                                                          c_bytes(self.orient[lo:hi]), out.ptr, out.stride), out)

    def mirror(self, i, whole):
        return T.normalise(A.resize(E.orient(self.pixels(i, whole), self.orient[i]), *self.canvas), self.spec, self.flips[i])


class MixedPlaced(MixedCell):
    """Bicubic, fitted windows with a fill, the colour stage with a clamp, bfloat16, the windows written back."""
    canvas = (261, 259)                                     # a 2048 x 1536 view fits at 7.9 to 1, turned or not: below the filter's 8
    spec = T.Spec(T.BF16, T.CHW)

    def window(self, i):
        w, h = E.oriented_size(self.orient[i], self.views[i][3], self.views[i][4])
        return P.place_window(P.FIT, P.CENTRE, w, h, *self.canvas)

    def run(self, lo, hi):
        m = hi - lo
        for i in range(lo, hi):                             # inside the tap limit, every image
            w, h = E.oriented_size(self.orient[i], self.views[i][3], self.views[i][4])
            win = self.window(i)
            assert max(F32(w) / F32(win[2]), F32(h) / F32(win[3])) <= 8.0, i
        out = self.out(m)
        cs, place = c_spec(self.spec), c_fit()
        keep, col = c_colour(self.k[lo:hi], CLAMP)
        wout = (_lib.Region * m)(*[_lib.Region(-7, -7, -7, -7)] * m)
        st = _lib.lib().jpeg_amd_decode_tensor_colour_mixed(*self.head(lo, hi), *self.canvas, BICUBIC, C.byref(cs), c_bytes(self.flips[lo:hi]),
                                                            c_bytes(self.orient[lo:hi]), C.byref(place), wout, C.byref(col), out.ptr, out.stride)
        return self.done(st, out, windows=[(r.x, r.y, r.width, r.height) for r in wout])

    def mirror(self, i, whole):
        win = self.window(i)
        assert whole.windows[i] == win, i
        src = E.orient(self.pixels(i, whole), self.orient[i])
        canvas = P.place(B.resize(src, win[2], win[3]), win, self.canvas, FILL)
        return K.normalise(canvas, self.k[i], CLAMP, self.spec, self.flips[i])


class MappedCell(Cell):
    """The warped and the projected call: the views are the library's (jpeg_amd_warp_view, jpeg_amd_project_view), and
    _chunk_seam's chunks are those of the views the call returns."""
    canvas = S.MAPPED_CANVAS

    def __init__(self, ctx, torch, pool):
        super().__init__(ctx, torch)
        self.scene = S.mapped(self.projective)
        self.places = self.scene.places
        self.n = self.places.n
        self.chunks = S.check_places(self.places, self.scene.views)
        self.subset = self.places.subset()
        self.entries = entries(pool, self.places)
        self.orient, self.flips = self.scene.orient, S.flips(self.n)
        self.k = colours(self.n, 12 + self.projective)

    def run(self, lo, hi):
        m, floats = hi - lo, 9 if self.projective else 6
        out = self.out(m)
        cs, wp = c_spec(self.spec), c_warp(self.edge)
        keep, col = c_colour(self.k[lo:hi], self.clamp)
        mats = np.ascontiguousarray(self.scene.matrices[lo:hi], F32)
        vout, mout = (_lib.View * m)(), np.full((m, floats), -7, F32)
        call = _lib.lib().jpeg_amd_decode_tensor_projected_mixed if self.projective else _lib.lib().jpeg_amd_decode_tensor_warped_colour_mixed
        st = call(self.ctx.handle, m, M.c_images(self.entries[lo:hi]), 0, COLOR, c_bytes(self.orient[lo:hi]), mats.ctypes.data, C.byref(wp),
                  *self.canvas, C.byref(cs), c_bytes(self.flips[lo:hi]), vout, mout.ctypes.data, C.byref(col), out.ptr, out.stride)
        return self.done(st, out, views=[(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in vout], matrices=mout)

    def mirror(self, i, whole):
        L = self.entries[i][0]
        view, m_view = (PR.project_view if self.projective else W.warp_view)(L.width, L.height, self.orient[i], self.scene.matrices[i], *self.canvas)
        assert whole.views[i] == view and np.array_equal(whole.matrices[i], m_view), i
        src = view_alone(self.ctx, self.torch, self.entries[i], view)
        canvas = (PR.project if self.projective else W.warp)(src, m_view, self.canvas[0], self.canvas[1], self.edge, FILL)
        return K.normalise(canvas, self.k[i], self.clamp, self.spec, self.flips[i])


class MixedWarped(MappedCell):
    projective, edge, clamp = False, W.REPLICATE, K.NO_CLAMP
    spec = T.Spec(T.F32, T.HWC)


class MixedProjected(MappedCell):
    projective, edge, clamp = True, W.FILL, CLAMP
    spec = T.Spec(T.F16, T.HWC)


CELLS = {"uniform-stored-bilinear-bytes": UniformBytes, "uniform-stored-antialias-f16-chw": UniformAntialias,
         "mixed-stored-bilinear-bytes": MixedBytes, "mixed-oriented-antialias-f32-chw": MixedOriented,
         "mixed-placed-bicubic-colour-bf16-chw": MixedPlaced, "mixed-warped-colour-f32-hwc": MixedWarped,
         "mixed-projected-colour-f16-hwc": MixedProjected}


@pytest.fixture(scope="module")
def uniform_data(ctx, torch):
    L = c_layout(S.BIG[0], S.BIG[1], FUSED["y8"])
    planes, dq, ntables = synthetic(ctx, torch, L, S.UNIFORM_N, 31)
    assert strides(L)[0] > 0 and ntables * 64 > 0          # with a stride of 0 the chunk's offset into the images could not show
    yield L, planes, dq, ntables
    del planes, dq
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def whole_calls():
    """name -> (the cell, its whole call): each whole call is made once and shared by the two layers."""
    return {}


def cell_and_whole(name, request, ctx, torch, whole_calls):
    if name not in whole_calls:
        data = request.getfixturevalue("uniform_data" if name.startswith("uniform") else "pool")
        cell = CELLS[name](ctx, torch, data)
        assert len(cell.chunks) == (2 if name.startswith("uniform") else 3) and all(i0 > 0 for i0, _, _ in cell.chunks[1:])
        whole_calls[name] = (cell, cell.run(0, cell.n))
    return whole_calls[name]


# ---- 1. split invariance ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CELLS))
def test_the_whole_call_is_the_call_on_each_chunk_alone(request, ctx, torch, whole_calls, name):
    cell, whole = cell_and_whole(name, request, ctx, torch, whole_calls)
    for c, (i0, m, _) in enumerate(cell.chunks):
        part = cell.run(i0, i0 + m)
        for what in ("windows", "views"):
            if getattr(whole, what) is not None:
                assert getattr(whole, what)[i0:i0 + m] == getattr(part, what), (name, c, what)
        if whole.matrices is not None:
            assert np.array_equal(whole.matrices[i0:i0 + m].view(np.uint32), part.matrices.view(np.uint32)), (name, c)
        for j in range(m):
            same(whole.images[i0 + j], part.images[j], (name, "chunk", c, "image", i0 + j))
    # the scenario is not uniform: an image of a later chunk is not the image at its place in the first
    i0 = cell.chunks[1][0]
    assert sum(1 for j in range(cell.chunks[1][1]) if not np.array_equal(whole.images[i0 + j], whole.images[j])) >= cell.chunks[1][1] - 2


# ---- 2. independent mirrors -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CELLS))
def test_the_subset_against_the_mirrors_of_the_view_decoded_alone(request, ctx, torch, whole_calls, name):
    cell, whole = cell_and_whole(name, request, ctx, torch, whole_calls)
    assert len(cell.subset) >= 10
    for i in cell.subset:
        same(cell.got(whole, i), cell.mirror(i, whole), (name, "image", i))


# ---- 3. a call refused for an image of its second chunk ---------------------------------------------------------------------------------

def test_a_view_past_the_tap_limit_in_the_second_chunk_refuses_the_call(ctx, torch, pool):
    views = S.refused_views()
    chunks = S.expected_chunks(views)
    assert len(chunks) == 2 and chunks[1][0] <= S.REFUSED_AT
    made = entries(pool, S.MIXED, S.REFUSED_N)
    cw, ch = S.REFUSED_CANVAS
    over = [i for i, v in enumerate(views) if F32(v[3]) / F32(cw) > 16.0 or F32(v[4]) / F32(ch) > 16.0]
    assert over == [S.REFUSED_AT]

    def call(lo, hi):
        out = Out(ctx, torch, [3 * cw * ch] * (hi - lo), gap=5, lead=3, tail=7)
        st = _lib.lib().jpeg_amd_decode_resized_filter_mixed(ctx.handle, hi - lo, M.c_images(made[lo:hi]), 0, COLOR, c_views(views[lo:hi]), cw, ch, AA,
                                                             out.ptr, out.stride)
        ctx.synchronize()
        return st, out

    st, out = call(0, S.REFUSED_N)
    assert st == _lib.ENOSUP and out.untouched()
    # the context is usable: the first chunk's images alone are inside the limit, the 1920 x 1536 view at exactly 16 to 1
    st, out = call(0, chunks[0][1])
    assert st == 0
    got = out.images()
    for i in (0, S.LARGE0, chunks[0][1] - 1):
        same(got[i], A.resize(view_alone(ctx, torch, made[i], views[i]), cw, ch), ("after the refusal", i))
