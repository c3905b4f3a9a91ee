"""The mixed calls on the MI355X (jpeg_amd_decode_view_mixed, _resized_mixed, _tensor_mixed; k_view_decode_mixed): images of
different sizes and layouts in one call.  The contract is the uniform calls': image i is, byte for byte, what
jpeg_amd_decode_view_batch / _resized_batch / _tensor_batch write for it with n_images = 1 -- which is what every test here
compares with, computed once per module -- and one test anchors three of the images on the oracle as test_gpu_view.py does, so
that the two calls cannot be wrong alike.  Every output buffer is filled with a sentinel before the call, and the bytes between
and behind the images are checked after it."""
import ctypes as C

import numpy as np
import pytest

import _scaled_ref as S
import jpeg_amd as J
from _calls import COLORS, FUSED, SENTINEL, Out, c_layout, c_views, plane_ptrs, strides, synthetic
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _mixed import resized_mixed, tensor_mixed, view_mixed
from _tile import TILE_H, TILE_W, crop, random_region, reference
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

RGB, YCC = _lib.COLOR_RGB8, _lib.COLOR_YCC8
F411 = [(4, 1), (1, 1), (1, 1)]

# The 16 images of the one call: (layout, size, denominator, rectangle of the scaled image or None = the whole of it, or
# "seam" = a seeded rectangle that crosses x = 128 and y = 32 of its tile grid).  Every (N, planes) group holds two images of
# different size and, with three planes, of different sampling; all five fused layouts, all six sizes, the four denominators.
IMAGES = [
    ("y8", (131, 257), 1, "seam"), ("422", (300, 140), 1, "seam"), ("y8", (7, 9), 1, None), ("420", (17, 33), 1, None),
    ("420", (1100, 300), 2, "seam"), ("y8", (300, 140), 2, None), ("444", (131, 257), 2, None), ("y8", (1, 1), 2, None),
    ("440", (300, 140), 4, None), ("y8", (1100, 300), 4, "seam"), ("422", (1100, 300), 4, "seam"), ("y8", (17, 33), 4, (1, 2, 2, 3)),
    ("444", (1100, 300), 8, "seam"), ("y8", (1100, 300), 8, None), ("420", (1, 1), 8, None), ("y8", (7, 9), 8, None),
]
ORACLE = (0, 4, 1)                                           # a grey one, a 4:2:0 at denominator 2, a 4:2:2 at denominator 1


class Image:
    """One image of a call: its layout, its synthetic planes and tables on the device, its view."""

    def __init__(self, ctx, torch, factors, size, denom, rect, seed, rng):
        self.L = c_layout(size[0], size[1], factors)
        self.planes, self.dq, self.ntables = synthetic(ctx, torch, self.L, 1, seed)
        W1, H1 = S.scaled_size(size, denom)
        if rect is None:
            rect = (0, 0, W1, H1)
        elif rect == "seam":
            n = 8 // denom
            x, y = int(rng.integers(1, W1 - TILE_W - 1)), int(rng.integers(1, H1 - TILE_H - 1))
            w, h = int(rng.integers(TILE_W + 1, W1 - x + 1)), int(rng.integers(TILE_H + 1, min(H1 - y, 100) + 1))
            rect = (x, y, w, h)
            assert x % n + w > TILE_W and y % n + h > TILE_H
        self.size, self.denom, self.view = size, denom, (denom, tuple(rect))
        self.area = 3 * rect[2] * rect[3]

    def arg(self):
        return self.L, [p.data_ptr() for p in self.planes], self.dq.data_ptr(), self.ntables

    def uniform_view(self, ctx, torch, cosited, color):
        """jpeg_amd_decode_view_batch with n_images = 1 -> host bytes."""
        out = Out(ctx, torch, [self.area], tail=8)
        assert _lib.lib().jpeg_amd_decode_view_batch(
            ctx.handle, C.byref(self.L), 1, plane_ptrs(self.planes), _lib.size_array(strides(self.L)), self.dq.data_ptr(),
            self.ntables * 64, self.ntables, cosited, color, c_views([self.view]), out.ptr, 0) == 0
        return out.images()[0]

    def uniform_resized(self, ctx, torch, color, out_w, out_h, spec=None, flip=0):
        """jpeg_amd_decode_resized_batch (spec None) or _tensor_batch with n_images = 1 -> host bytes."""
        elem = 1 if spec is None else (4 if spec.dtype == _lib.F32 else 2)
        out = Out(ctx, torch, [3 * out_w * out_h], elem=elem, tail=8)
        head = (ctx.handle, C.byref(self.L), 1, plane_ptrs(self.planes), _lib.size_array(strides(self.L)), self.dq.data_ptr(),
                self.ntables * 64, self.ntables, 0, color, c_views([self.view]), out_w, out_h)
        if spec is None:
            assert _lib.lib().jpeg_amd_decode_resized_batch(*head, out.ptr, 0) == 0
        else:
            assert _lib.lib().jpeg_amd_decode_tensor_batch(*head, C.byref(spec), (C.c_uint8 * 1)(flip), out.ptr, 0) == 0
        return out.images()[0]


class Case:
    """The 16 images and, computed on first use and then kept, what the uniform view call writes for each."""

    def __init__(self, ctx, torch):
        rng = np.random.default_rng(2024)
        self.ctx, self.torch = ctx, torch
        self.images = [Image(ctx, torch, FUSED[name], size, denom, rect, 100 + i, rng)
                       for i, (name, size, denom, rect) in enumerate(IMAGES)]
        self._want = {}

    def want(self, cosited, color):
        key = (cosited, color)
        if key not in self._want:
            self._want[key] = [im.uniform_view(self.ctx, self.torch, cosited, color) for im in self.images]
        return self._want[key]


@pytest.fixture(scope="module")
def case(ctx, torch):
    return Case(ctx, torch)


def _mixed_views(ctx, torch, images, cosited, color, gap=7):
    """One jpeg_amd_decode_view_mixed over `images` -> the host bytes of each; the sentinel is asserted everywhere else."""
    out = Out(ctx, torch, [im.area for im in images], gap=gap, tail=gap)
    assert view_mixed(ctx.handle, [im.arg() for im in images], cosited, color, [im.view for im in images], out.ptr, out.stride) == 0
    return out.images()


def _spec(dtype, layout):
    s = _lib.TensorSpec()
    s.dtype, s.layout = dtype, layout
    for c, (m, k) in enumerate(((123.675, 0.0171247538), (116.28, 0.0175070028), (103.53, 0.0174291939))):
        s.mean[c], s.scale[c] = m, k
    return s


# ---- 1. image by image the uniform call ---------------------------------------------------------------------------------------

def test_the_case_holds_what_it_should(case):
    groups = {}
    for im in case.images:
        groups.setdefault((im.denom, im.L.nplanes), []).append(im)
    assert sorted(groups) == [(d, p) for d in (1, 2, 4, 8) for p in (1, 3)]
    for (denom, nplanes), members in groups.items():
        assert len(members) == 2 and members[0].size != members[1].size
        if nplanes == 3:
            a, b = members
            assert (a.L.scale_x, a.L.scale_y) != (b.L.scale_x, b.L.scale_y)
    assert {name for name, _, _, _ in IMAGES} == set(FUSED)
    assert {size for _, size, _, _ in IMAGES} == {(1, 1), (7, 9), (17, 33), (131, 257), (300, 140), (1100, 300)}
    one_tile = [im for im in case.images if im.view[1][2] <= TILE_W - 8 and im.view[1][3] <= TILE_H - 8]
    assert one_tile and sum(IMAGES[i][3] == "seam" for i in range(len(IMAGES))) == 6


@pytest.mark.parametrize("color", COLORS)
def test_every_image_equals_the_uniform_call(ctx, torch, case, color):
    got = _mixed_views(ctx, torch, case.images, 0, color)
    for i, (g, w) in enumerate(zip(got, case.want(0, color))):
        assert (g == w).all(), (i, IMAGES[i])


# ---- 2. the oracle -------------------------------------------------------------------------------------------------------------

def test_three_images_match_the_oracle(ctx, torch, case):
    assert [(IMAGES[i][0], IMAGES[i][2]) for i in ORACLE] == [("y8", 1), ("420", 2), ("422", 1)]
    got = {color: _mixed_views(ctx, torch, case.images, 0, color) for color in COLORS}
    for i in ORACLE:
        im = case.images[i]
        denom, r = im.view
        want = reference(im.L, [p.cpu().numpy() for p in im.planes], im.dq.cpu().numpy().astype(np.uint16), 0, denom, 0)
        for color in COLORS:
            assert (got[color][i].reshape(r[3], r[2], 3) == crop(want[color], r)).all(), (i, color)


# ---- 3. the index list and the prefix --------------------------------------------------------------------------------------------

def test_permuting_the_images_permutes_the_outputs(ctx, torch, case):
    order = np.random.default_rng(7).permutation(len(case.images)).tolist()
    assert order != sorted(order)
    want = case.want(0, RGB)
    for perm in (order, list(reversed(range(len(case.images))))):
        got = _mixed_views(ctx, torch, [case.images[i] for i in perm], 0, RGB, gap=0)
        for g, i in zip(got, perm):
            assert (g == want[i]).all(), (perm, i)


# ---- 4. one geometry -------------------------------------------------------------------------------------------------------------

def test_eight_images_of_one_geometry_equal_the_uniform_batch_call(ctx, torch):
    L = c_layout(403, 150, FUSED["420"])
    n = 8
    planes, dq, ntables = synthetic(ctx, torch, L, n, 64)
    rng = np.random.default_rng(8)
    views = []
    for i in range(n):
        denom = (1, 2, 4, 8)[i % 4]
        views.append((denom, random_region(rng, *S.scaled_size((403, 150), denom))))
    views[5] = (2,) + ((0, 0) + S.scaled_size((403, 150), 2),)
    areas = [3 * r[2] * r[3] for _, r in views]
    images = [(L, [p[i].data_ptr() for p in planes], dq[i].data_ptr(), ntables) for i in range(n)]
    for color in COLORS:
        uniform, mixed = Out(ctx, torch, areas, gap=3, tail=3), Out(ctx, torch, areas, gap=3, tail=3)
        assert _lib.lib().jpeg_amd_decode_view_batch(
            ctx.handle, C.byref(L), n, plane_ptrs(planes), _lib.size_array(strides(L)), dq.data_ptr(), ntables * 64, ntables, 0,
            color, c_views(views), uniform.ptr, uniform.stride) == 0
        assert view_mixed(ctx.handle, images, 0, color, views, mixed.ptr, mixed.stride) == 0
        for i, (a, b) in enumerate(zip(uniform.images(), mixed.images())):
            assert (a == b).all(), (color, i, views[i])


# ---- 5. the layouts without a tile kernel ----------------------------------------------------------------------------------------

def test_a_411_image_between_fused_ones(ctx, torch, case):
    rng = np.random.default_rng(411)
    odd = [Image(ctx, torch, F411, (131, 65), denom, rect, 411 + denom, rng) for denom, rect in ((1, (3, 5, 120, 40)), (4, None))]
    images = case.images[:3] + odd[:1] + case.images[3:6] + odd[1:]
    for color in COLORS:
        want = case.want(0, color)
        want = want[:3] + [odd[0].uniform_view(ctx, torch, 0, color)] + want[3:6] + [odd[1].uniform_view(ctx, torch, 0, color)]
        for i, (g, w) in enumerate(zip(_mixed_views(ctx, torch, images, 0, color), want)):
            assert (g == w).all(), (color, i)


def test_the_whole_call_cosited(ctx, torch, case):
    """Cosited, only the grey images keep the tile kernel; every three-plane image takes the uniform call."""
    for color in COLORS:
        for i, (g, w) in enumerate(zip(_mixed_views(ctx, torch, case.images, 1, color), case.want(1, color))):
            assert (g == w).all(), (color, i, IMAGES[i])
    assert any((a != b).any() for a, b in zip(case.want(1, RGB), case.want(0, RGB)))   # cosited is another image


# ---- 6. resized and tensor -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("out_size", [(24, 20), (224, 224)], ids=["24x20", "224x224"])
def test_resized_bytes_equal_the_uniform_call(ctx, torch, case, out_size):
    out_w, out_h = out_size
    n = len(case.images)
    for color in COLORS:
        out = Out(ctx, torch, [3 * out_w * out_h] * n, gap=5, tail=5)
        assert resized_mixed(ctx.handle, [im.arg() for im in case.images], 0, color, [im.view for im in case.images], out_w, out_h,
                             out.ptr, out.stride) == 0
        for i, (g, im) in enumerate(zip(out.images(), case.images)):
            assert (g == im.uniform_resized(ctx, torch, color, out_w, out_h)).all(), (color, i, IMAGES[i])


@pytest.mark.parametrize("out_size", [(24, 20), (224, 224)], ids=["24x20", "224x224"])
@pytest.mark.parametrize("form", ["f16-chw", "f32-hwc"])
def test_tensors_equal_the_uniform_call(ctx, torch, case, form, out_size):
    out_w, out_h = out_size
    spec = _spec(_lib.F16, _lib.TENSOR_CHW) if form == "f16-chw" else _spec(_lib.F32, _lib.TENSOR_HWC)
    elem = 2 if form == "f16-chw" else 4
    n = len(case.images)
    flips = [i % 2 for i in range(n)]
    out = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=5, tail=5)
    assert tensor_mixed(ctx.handle, [im.arg() for im in case.images], 0, RGB, [im.view for im in case.images], out_w, out_h, spec,
                        flips, out.ptr, out.stride) == 0
    for i, (g, im) in enumerate(zip(out.images(), case.images)):
        assert (g == im.uniform_resized(ctx, torch, RGB, out_w, out_h, spec, flips[i])).all(), (form, i, IMAGES[i])
    if form == "f32-hwc" and out_size == (24, 20):           # no flips at all is a NULL array
        plain = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem)
        assert tensor_mixed(ctx.handle, [im.arg() for im in case.images], 0, RGB, [im.view for im in case.images], out_w, out_h,
                            spec, None, plain.ptr, plain.stride) == 0
        for i, (g, im) in enumerate(zip(plain.images(), case.images)):
            assert (g == im.uniform_resized(ctx, torch, RGB, out_w, out_h, spec, 0)).all(), i


# ---- 7. refused calls; 8. the empty call -------------------------------------------------------------------------------------------

def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, torch, case):
    images = case.images[2:8]                                 # whole images of 7 x 9 ... and image 4's seam rectangle
    args, views = [im.arg() for im in images], [im.view for im in images]
    out = Out(ctx, torch, [im.area for im in images], gap=4, tail=4)
    spec = _spec(_lib.F32, _lib.TENSOR_HWC)

    def view(a=args, v=views, ptr=out.ptr, stride=out.stride):
        return view_mixed(ctx.handle, a, 0, RGB, v, ptr, stride)

    # image 3 is 17 x 33 whole; image 2's view (denominator 2, inside 550 x 150) lies outside it
    assert view(v=views[:1] + [views[2]] + views[2:]) == _lib.EINVAL
    assert view(v=views[:3] + [(3,) + views[3][1:]] + views[4:]) == _lib.EINVAL
    L12 = c_layout(300, 140, FUSED["y8"], precision=12)
    assert view(a=args[:3] + [(L12,) + args[3][1:]] + args[4:]) == _lib.ENOSUP
    assert view(a=args[:4] + [(args[4][0], [args[4][1][0], None, args[4][1][2]]) + args[4][2:]] + args[5:]) == _lib.EINVAL
    assert view(a=args[:4] + [args[4][:3] + (1,)] + args[5:]) == _lib.EINVAL            # a 4:4:4 image with one table
    assert view(stride=max(im.area for im in images) - 1) == _lib.EINVAL
    assert view(ptr=None) == _lib.EINVAL
    assert view_mixed(ctx.handle, args, 0, RGB, views, out.ptr, out.stride, n=-1) == _lib.EINVAL
    assert resized_mixed(ctx.handle, args, 0, RGB, views, 0, 4, out.ptr, out.stride) == _lib.EINVAL
    assert resized_mixed(ctx.handle, args, 0, RGB, views, 400, 400, out.ptr, out.stride) == _lib.EINVAL   # the stride is too small
    assert tensor_mixed(ctx.handle, args, 0, RGB, views, 4, 4, spec, None, out.ptr + 2, out.stride // 4) == _lib.EINVAL
    assert tensor_mixed(ctx.handle, args, 0, RGB, views[:5] + [(8, (0, 0, 1, 2))], 4, 4, spec, None, out.ptr, out.stride // 4) \
        == _lib.EINVAL                                        # the last image is 1 x 1 at every denominator
    ctx.synchronize()
    assert out.untouched()
    assert view() == 0
    want = case.want(0, RGB)[2:8]
    for i, (g, w) in enumerate(zip(out.images(), want)):
        assert (g == w).all(), i


def test_an_empty_call_is_ok(ctx, torch):
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    spec = _spec(_lib.F16, _lib.TENSOR_CHW)
    lib = _lib.lib()
    assert lib.jpeg_amd_decode_view_mixed(ctx.handle, 0, None, 0, RGB, None, out.data_ptr(), 0) == 0
    assert lib.jpeg_amd_decode_resized_mixed(ctx.handle, 0, None, 0, RGB, None, 4, 4, out.data_ptr(), 0) == 0
    assert lib.jpeg_amd_decode_tensor_mixed(ctx.handle, 0, None, 0, RGB, None, 4, 4, C.byref(spec), None, out.data_ptr(), 0) == 0
    ctx.synchronize()
    assert (out == SENTINEL).all()


# ---- 9. the Python API ---------------------------------------------------------------------------------------------------------------

def test_python_api(ctx, torch):
    ycc = {name: J.Layout("ycc8", {1: J.Component(FUSED[name][0], 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
           for name in ("420", "444")}
    grey = J.Layout("y8", {1: J.Component((1, 1), 0)})
    specs = [("420", ycc["420"], (403, 150)), ("y8", grey, (131, 257)), ("444", ycc["444"], (64, 48))]
    spectrals, batches = [], []
    for i, (name, layout, size) in enumerate(specs):
        L = c_layout(size[0], size[1], FUSED[name])
        planes, dq, ntables = synthetic(ctx, torch, L, 1, 900 + i)
        qh = dq.cpu().numpy().astype(np.uint16)
        q = [0, 1, 1][:L.nplanes]
        spectrals.append(J.Spectral(ctx, size, layout, [p[0] for p in planes], [qh[0, t] for t in range(ntables)], q))
        batches.append((size, layout, planes, dq, q))

    views = [(2, 5, 3, 150, 60), (1, 0, 0, 131, 257), (8, 1, 1, 6, 4)]
    got = J.decode_views_mixed(ctx, spectrals, views, color=J.YCbCr)
    assert len(got) == 3
    for g, sp, v in zip(got, spectrals, views):
        assert tuple(g.shape) == (v[4], v[3], 3)
        assert (g.cpu().numpy() == sp.view(v[1:], v[0], J.YCbCr).cpu().numpy()).all(), v

    resized = J.decode_resized_mixed(ctx, spectrals, views, (24, 20))
    assert tuple(resized.shape) == (3, 20, 24, 3) and resized.dtype == torch.uint8
    for i, (sp, v) in enumerate(zip(spectrals, views)):
        assert (resized[i].cpu().numpy() == sp.view(v[1:], v[0], size=(24, 20)).cpu().numpy()).all(), v

    source = [(10, 7, 380, 140), (3, 9, 100, 200), (0, 0, 64, 48)]
    out_size = (24, 20)
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    flips = [1, 0, 1]
    tensor, chosen = J.decode_crops_tensor_mixed(ctx, spectrals, source, out_size, spec, flips=flips)
    assert tuple(tensor.shape) == (3, 3, 20, 24) and tensor.dtype == torch.float16
    assert chosen.dtype == np.int32 and chosen.shape == (3, 5)
    for i, ((size, layout, planes, dq, q), s) in enumerate(zip(batches, source)):
        denom = J.view_denom(s[2:], out_size)
        assert tuple(chosen[i]) == (denom,) + J.view_of_source(size, denom, s)
        one, one_views = J.decode_crops_tensor(ctx, size, layout, planes, dq, [s], out_size, spec, flips=flips[i:i + 1], q=q)
        assert one_views.tolist() == chosen[i:i + 1].tolist()
        assert (tensor[i].view(torch.int16).cpu().numpy() == one[0].view(torch.int16).cpu().numpy()).all(), i
    assert [int(c[0]) for c in chosen] == [4, 4, 2]          # three sizes, and not one denominator
    same = J.decode_tensors_mixed(ctx, spectrals, chosen, out_size, spec, flips=flips)
    assert (same.view(torch.int16) == tensor.view(torch.int16)).all()
    with pytest.raises(J.JpegAmdError):
        J.decode_views_mixed(ctx, spectrals, [views[0], views[0], views[2]])   # inside image 0 at denominator 2, outside image 1
    with pytest.raises(ValueError):
        J.decode_views_mixed(ctx, spectrals, views[:2])
