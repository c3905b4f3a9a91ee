"""The bicubic warp on the MI355X (jpeg_amd_project_filter_batch, _project_filter_tensor_batch, the *_projected_filter_mixed
decode and file calls; k_mapped_bytes and k_mapped_tensor over ProjectiveMap and CubicTaps): every output is compared byte for byte, or element
for element as a bit pattern, with the numpy mirror of the contract (_project_cubic_ref), and where the contract ties into an
existing call, with that call on the GPU.  The canvas is 70 x 37: two tiles across and two down, the last ones partial, with an
odd width so that runs of 4 straddle out_w.  Every raw call writes into a sentinel-filled buffer whose bytes in front of,
between and behind the images are checked.

The kernels fetch a row's four taps with one 12-byte load where no column or row of the pixel is clamped and the segment ends
four bytes in front of the image's end, and tap by tap elsewhere.  The sources of 17 x 5 (255 bytes), 131 x 67 (26 331) and
1 x 9 (27) have byte counts that are no multiple of 4, and the identity, the shifts and the matrices below read their last
rows and columns: a dword that straddled the image's end and was read as a tap would show as a 0 in the last pixel.  The
131 x 67 source under its mild keystone has whole waves of interior pixels."""
import ctypes as C
import math

import numpy as np
import pytest

import _colour_ref as K
import _files as F
import _orient as E
import _project_cubic_ref as Q
import _project_ref as P
import _tensor_ref as T
import jpeg_amd as J
from _calls import Out, pixel_image
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, c_spec, host_bits as bits, pack, same, tensor_bits
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
CANVAS = (70, 37)
FILL = (7, 130, 255)
EDGES = [Q.FILL, Q.REPLICATE]
EDGE_NAME = {Q.FILL: "fill", Q.REPLICATE: "replicate"}
SIZES = [(1, 1), (1, 9), (9, 1), (17, 5), (64, 32), (131, 67)]          # (w, h); the first three narrower than the four taps
BOX = [(0, 0), (CANVAS[0], 0), (CANVAS[0], CANVAS[1]), (0, CANVAS[1])]
IDENT = [1, 0, 0, 0, 1, 0, 0, 0, 1]


def quad(points):
    """The homography that takes the canvas's corners, clockwise from (0, 0), to four source points, float32 [9]."""
    return P.homography(points, BOX).reshape(9).astype(F32)


def rotation(size, angle, scale, row2=(0.0, 0.0), canvas=CANVAS):
    """A rotation with scale about the centres, times a perspective row (g, k, 1) of the canvas point."""
    a = math.radians(angle)
    lin = scale * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    t = np.array([size[0] / 2.0, size[1] / 2.0]) - lin @ np.array([canvas[0] / 2.0, canvas[1] / 2.0])
    aff = np.array([[lin[0, 0], lin[0, 1], t[0]], [lin[1, 0], lin[1, 1], t[1]], [0, 0, 1.0]])
    return (aff @ np.array([[1, 0, 0], [0, 1, 0], [row2[0], row2[1], 1.0]])).reshape(9).astype(F32)


# one matrix per source: the identity (the canvas runs far past a 1 x 1 source), a shift by (-2, 3), a rotation with scale and
# a perspective row over a source one row high, a footprint that misses its source, a rotation by 25 degrees that leaves the
# corners of the canvas outside, and a mild keystone that keeps most of the canvas inside the largest source
MATRICES = [np.array(IDENT, F32),
            np.array([1, 0, -2, 0, 1, 3, 0, 0, 1], F32),
            rotation(SIZES[2], 33.0, 0.4, (0.002, -0.003)),
            quad([(400.0, -300.0), (420.0, -310.0), (425.0, -280.0), (395.0, -285.0)]),
            rotation(SIZES[4], 25.0, 1.1, (0.001, 0.002)),
            quad([(9.0, 4.0), (125.0, -3.0), (133.0, 69.0), (-2.0, 58.0)])]
# ... and one set of seeded four-corner distortions in which every source about fills the canvas
KEYSTONES = [P.distortion(np.random.default_rng(500 + i), w, h, CANVAS[0], CANVAS[1], 0.5, 0.1) for i, (w, h) in enumerate(SIZES)]


@pytest.fixture(scope="module")
def sources():
    return [pixel_image("checker" if i == 4 else "random", w, h, 59 * w + h) for i, (w, h) in enumerate(SIZES)]


def test_the_cases_are_what_they_are_said_to_be(sources):
    for m in MATRICES + KEYSTONES:
        assert P.accepted(m, *CANVAS)
    assert [s.size % 4 for s in sources] == [3, 3, 3, 3, 0, 3]
    assert set(np.unique(sources[4]).tolist()) == {0, 255}
    # whole waves of interior pixels (a wave: 64 columns of 4 rows): rows 8 .. 27 of the first tile of the largest source
    inside = Q.taps_inside(MATRICES[5], *SIZES[5], *CANVAS)
    assert inside[8:28, :64].all() and not inside.all()
    # the last row and the last column of that source are read, and so is its last pixel by the identity below
    sx, sy = Q.coordinates(MATRICES[5], *SIZES[5], *CANVAS)
    assert (np.floor(sx) + 2 >= SIZES[5][0] - 1).any() and (np.floor(sy) + 2 >= SIZES[5][1] - 1).any()
    fill = np.asarray(FILL, np.uint8)
    assert (Q.project(sources[3], MATRICES[3], CANVAS[0], CANVAS[1], Q.FILL, FILL) == fill).all()          # the footprint that misses
    outside = (Q.project(sources[4], MATRICES[4], CANVAS[0], CANVAS[1], Q.FILL, FILL) == fill).all(axis=2).mean()
    assert 0.02 < outside < 0.5


def c_warp(edge, fill=FILL):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = fill
    return w


def project_call(ctx, torch, images, matrices, canvas, edge, spec=None, flips=None, colour=None, lead=3, gap=5, filter=Q.BICUBIC,
                 plain=False, status=0):
    """jpeg_amd_project_filter_batch (spec: _project_filter_tensor_batch; colour: (k, clamp) or None for NULL; plain: the calls
    without a filter) into a guarded buffer whose first image lies `lead` elements behind an allocation boundary, the images
    3 out_w out_h + gap elements apart -> the images' bytes."""
    out_w, out_h = canvas
    n = len(images)
    d_src, stride, ext = pack(ctx, torch, images)
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=gap, lead=lead, tail=7)
    m = np.ascontiguousarray(matrices, F32).reshape(n, 9)
    wp = c_warp(edge)
    head = (ctx.handle, n, d_src.data_ptr(), stride, ext, m.ctypes.data, C.byref(wp)) + (() if plain else (filter,)) + (out_w, out_h)
    lib = _lib.lib()
    if spec is None:
        st = (lib.jpeg_amd_project_batch if plain else lib.jpeg_amd_project_filter_batch)(*head, out.ptr, out.stride)
    else:
        cs = c_spec(spec)
        col = None
        if colour is not None:
            keep = np.ascontiguousarray(colour[0], F32).reshape(-1, 12)
            col = _lib.Colour()
            col.h_matrices, col.lo, col.hi = keep.ctypes.data, colour[1][0], colour[1][1]
        call = lib.jpeg_amd_project_tensor_batch if plain else lib.jpeg_amd_project_filter_tensor_batch
        st = call(*head, C.byref(cs), c_bytes(flips), None if col is None else C.byref(col), out.ptr, out.stride)
    assert st == status
    ctx.synchronize()
    if status != 0:
        assert out.untouched()
        return None
    return out.images()


# ---- 1. bytes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_six_sources_in_one_launch(ctx, torch, sources, edge):
    """Nonzero record offsets, sources narrower than the taps, whole tiles of fill, whole waves of interior pixels, the images'
    last rows and columns, a strided destination whose gaps are left alone; bit for bit."""
    for matrices in (MATRICES, KEYSTONES):
        got = project_call(ctx, torch, sources, matrices, CANVAS, edge)
        for i, (src, m) in enumerate(zip(sources, matrices)):
            same(got[i], Q.project(src, m, CANVAS[0], CANVAS[1], edge, FILL), (SIZES[i], EDGE_NAME[edge]))


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_the_identity_a_shift_and_the_quarter_turn(ctx, torch, sources, edge):
    """The contract's consequences on the GPU, each on a canvas of its own: the identity at out = (w, h) gives the source bytes
    -- its last pixel included, whose segment ends at the image's end -- a shift the shifted bytes, (0, 1, 0, -1, 0, h, 0, 0, 1)
    to (h, w) the quarter turn."""
    for i in (3, 5, 1):
        src = sources[i]
        h, w = src.shape[:2]
        got = project_call(ctx, torch, [src], [IDENT], (w, h), edge)
        same(got[0], src, ("identity", SIZES[i]))
        shift = [1, 0, 3, 0, 1, -2, 0, 0, 1]
        got = project_call(ctx, torch, [src], [shift], (w, h), edge)
        same(got[0], Q.project(src, shift, w, h, edge, FILL), ("shift", SIZES[i]))
        ys, xs = np.mgrid[0:h, 0:w]
        moved = src[np.clip(ys - 2, 0, h - 1), np.clip(xs + 3, 0, w - 1)]
        if edge == Q.FILL:
            moved = np.where(((ys - 2 >= 0) & (xs + 3 < w))[..., None], moved, np.asarray(FILL, np.uint8))
        same(got[0], moved, ("shifted bytes", SIZES[i]))
        got = project_call(ctx, torch, [src], [[0, 1, 0, -1, 0, h, 0, 0, 1]], (h, w), edge)
        same(got[0], np.ascontiguousarray(src[::-1].transpose(1, 0, 2)), ("quarter turn", SIZES[i]))


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_a_last_row_001_is_warp_with_six_numbers(ctx, torch, sources, edge):
    dev = [torch.from_numpy(s).to(ctx.torch_device) for s in sources]
    nine = [rotation(s, 30.0 + 47.0 * i, 1.3 * max(s[0] / CANVAS[0], s[1] / CANVAS[1])) for i, s in enumerate(SIZES)]
    six = [m[:6] for m in nine]
    assert all(m[6:].tolist() == [0, 0, 1] for m in nine)
    got = J.warp(ctx, dev, six, CANVAS, edge=EDGE_NAME[edge], fill=FILL, filter="bicubic").cpu().numpy()
    same(got, J.project(ctx, dev, nine, CANVAS, edge=EDGE_NAME[edge], fill=FILL, filter="bicubic").cpu().numpy(), "project")
    for i, src in enumerate(sources):
        same(got[i], Q.project(src, nine[i], CANVAS[0], CANVAS[1], edge, FILL), (SIZES[i], "mirror"))
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    flips = [i % 2 for i in range(len(dev))]
    same(tensor_bits(J.warp_tensor(ctx, dev, six, CANVAS, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL, filter="bicubic"), torch),
         tensor_bits(J.project_tensor(ctx, dev, np.array(nine).reshape(-1, 3, 3), CANVAS, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL,
                                      filter="bicubic"), torch), "warp_tensor")
    # and the bicubic filter is not the bilinear one
    assert not np.array_equal(got, J.warp(ctx, dev, six, CANVAS, edge=EDGE_NAME[edge], fill=FILL).cpu().numpy())


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_bilinear_through_the_new_entry_points_is_the_existing_call(ctx, torch, sources, edge):
    for matrices in (MATRICES, KEYSTONES):
        got = project_call(ctx, torch, sources, matrices, CANVAS, edge, filter=Q.BILINEAR)
        want = project_call(ctx, torch, sources, matrices, CANVAS, edge, plain=True)
        for i in range(len(sources)):
            same(got[i], want[i], (SIZES[i], EDGE_NAME[edge]))
    same(got[5], P.project(sources[5], KEYSTONES[5], CANVAS[0], CANVAS[1], edge, FILL), "the bilinear mirror")
    spec = T.Spec(T.F16, T.CHW)
    flips = [i % 2 for i in range(len(sources))]
    got = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, filter=Q.BILINEAR)
    want = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, plain=True)
    for i in range(len(sources)):
        same(got[i], want[i], (SIZES[i], "tensor"))


def test_the_batch_calls_refuse_with_a_context(ctx, torch, sources):
    """With a context the verdicts tell: no images is OK, another filter than the two is EINVAL and writes nothing."""
    assert project_call(ctx, torch, sources, MATRICES, CANVAS, Q.FILL) is not None
    for filter in (1, 2, 4, -1):
        project_call(ctx, torch, sources, MATRICES, CANVAS, Q.FILL, filter=filter, status=-1)
        project_call(ctx, torch, sources, MATRICES, CANVAS, Q.FILL, filter=filter, spec=T.Spec(T.F32, T.HWC), status=-1)
    project_call(ctx, torch, sources, MATRICES, CANVAS, 2, status=-1)
    lib, wp = _lib.lib(), c_warp(Q.FILL)
    assert lib.jpeg_amd_project_filter_batch(ctx.handle, 0, None, 0, None, None, C.byref(wp), Q.BICUBIC, 8, 8, None, 0) == 0
    assert lib.jpeg_amd_project_filter_batch(ctx.handle, 0, None, 0, None, None, C.byref(wp), 1, 8, 8, None, 0) == -1


# ---- 2. the tensor forms ----------------------------------------------------------------------------------------------------------------

COLOURS = np.stack([J.colour_matrix(), J.colour_matrix(order="bgr"), J.colour_matrix(grey=True), J.colour_matrix(1.4, 0.7, 1.8, 0.1),
                    K.matrix([[3, 0, 0, 40], [0, 3, 0, 40], [0, 0, 3, 40]]), K.matrix([[-1, -0.5, 0, 20], [0.25, -2, 0.5, -30], [0, 1, -1, 0]])])


@pytest.mark.parametrize("combo", [(T.F32, T.HWC), (T.F16, T.CHW), (T.BF16, T.CHW)], ids=["f32-hwc", "f16-chw", "bf16-chw"])
@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_tensor_forms_with_and_without_colour(ctx, torch, sources, combo, edge):
    """Into a destination one element behind an allocation boundary, the images 3 * 70 * 37 + 5 elements apart: the sinks'
    unaligned paths; Out.images() checks that the gap elements are left alone."""
    spec = T.Spec(*combo)
    flips = [i % 2 for i in range(len(sources))]
    canvases = [Q.project(src, m, CANVAS[0], CANVAS[1], edge, FILL) for src, m in zip(sources, KEYSTONES)]
    plain = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, lead=1, gap=5)
    for i, (src, m) in enumerate(zip(sources, KEYSTONES)):
        same(bits(plain[i], spec), T.normalise(canvases[i], spec, flips[i]), (SIZES[i], combo, EDGE_NAME[edge], flips[i]))
        # said by the contract's own formula too: the flip moves the taps, xs = out_w - 1 - x
        direct = T.normalise(Q.project(src, m, CANVAS[0], CANVAS[1], edge, FILL, flip=bool(flips[i])), spec, 0)
        same(bits(plain[i], spec), direct, (SIZES[i], "xs"))
    got = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, colour=(COLOURS, (0.0, 255.0)), lead=1, gap=5)
    for i in range(len(sources)):
        same(bits(got[i], spec), K.normalise(canvases[i], COLOURS[i], (0.0, 255.0), spec, flips[i]), (SIZES[i], combo, EDGE_NAME[edge], "colour"))


# ---- 3. one context, call after call ----------------------------------------------------------------------------------------------------

def test_two_calls_through_one_context(ctx, torch, sources):
    other = [pixel_image("random", w, h, 991 * w + h) for w, h in SIZES]
    first = project_call(ctx, torch, sources, KEYSTONES, CANVAS, Q.FILL)
    second = project_call(ctx, torch, other, KEYSTONES, CANVAS, Q.FILL)
    third = project_call(ctx, torch, other, MATRICES, CANVAS, Q.REPLICATE)
    for i in range(len(SIZES)):
        same(first[i], Q.project(sources[i], KEYSTONES[i], CANVAS[0], CANVAS[1], Q.FILL, FILL), ("first", i))
        same(second[i], Q.project(other[i], KEYSTONES[i], CANVAS[0], CANVAS[1], Q.FILL, FILL), ("second", i))
        same(third[i], Q.project(other[i], MATRICES[i], CANVAS[0], CANVAS[1], Q.REPLICATE), ("third", i))


def test_no_images(ctx, torch):
    assert tuple(J.project(ctx, [], np.zeros((0, 9), F32), CANVAS, filter="bicubic").shape) == (0, CANVAS[1], CANVAS[0], 3)
    assert tuple(J.warp(ctx, [], np.zeros((0, 6), F32), CANVAS, filter="bicubic").shape) == (0, CANVAS[1], CANVAS[0], 3)
    spec = J.tensor_spec(layout="chw")
    assert tuple(J.project_tensor(ctx, [], np.zeros((0, 9), F32), CANVAS, spec, filter="bicubic").shape) == (0, 3, CANVAS[1], CANVAS[0])
    out, views, mats = J.decode_warped_mixed(ctx, [], np.zeros((0, 6), F32), CANVAS, filter="bicubic")
    assert tuple(out.shape) == (0, CANVAS[1], CANVAS[0], 3) and views.shape == (0, 5) and mats.shape == (0, 6)
    out, views, mats = J.decompress_resized(ctx, [], CANVAS, warp=np.zeros((0, 9), F32), warp_filter="bicubic")
    assert tuple(out.shape) == (0, CANVAS[1], CANVAS[0], 3) and mats.shape == (0, 9)


# ---- 4. the decode route ----------------------------------------------------------------------------------------------------------------

F311 = [(3, 1), (1, 1), (1, 1)]                               # no tile kernel takes a factor of 3: the one-image fallback
DECODE = [("420", (300, 140)), ("444", (131, 257)), ("y8", (131, 257)), (F311, (150, 90))]
OUT = (48, 32)


@pytest.fixture(scope="module")
def spectrals(ctx):
    sps = []
    for i, (what, size) in enumerate(DECODE):
        name, factors = (what, None) if isinstance(what, str) else (None, what)
        sps.append(J.Spectral.decompress(ctx, F.synthetic_file(name, size, 170 + i, factors=factors)[0]))
    return sps


def upright_keystone(rng, size, o, step, out=OUT):
    """The canvas onto a rectangle of step * out about the centre of the UPRIGHT image, each corner pulled in by up to 7.5 % of
    the rectangle's side: every local step lies between 0.8 and 1.2 times `step`.  float32 [9]"""
    uw, uh = E.oriented_size(o, *size)
    rw, rh = step * out[0], step * out[1]
    x0, y0 = uw / 2.0 - rw / 2.0, uh / 2.0 - rh / 2.0
    d = [(rng.uniform(0, 0.075) * rw, rng.uniform(0, 0.075) * rh) for _ in range(4)]
    src = [(x0 + d[0][0], y0 + d[0][1]), (x0 + rw - d[1][0], y0 + d[1][1]), (x0 + rw - d[2][0], y0 + rh - d[2][1]), (x0 + d[3][0], y0 + rh - d[3][1])]
    return J.perspective_matrix(src, [(0, 0), (out[0], 0), (out[0], out[1]), (0, out[1])]).reshape(9).astype(F32)


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_decode_projected_mixed_is_the_view_decode_and_the_project_call(ctx, torch, spectrals, edge):
    """Denominators 1 and 2 on every image in turn and one matrix that reaches 4; orientations 1, 3, 6, 8 in turn."""
    seen = set()
    rng = np.random.default_rng(407)
    for r in range(4):
        orient = [(1, 3, 6, 8)[(i + r) % 4] for i in range(len(DECODE))]
        want_denoms = [4 if (r, i) == (1, 0) else (1, 2)[(i + r) % 2] for i in range(len(DECODE))]
        matrices = [upright_keystone(rng, size, o, 1.5 * d) for (what, size), o, d in zip(DECODE, orient, want_denoms)]
        got, views, mats = J.decode_projected_mixed(ctx, spectrals, matrices, OUT, orientations=orient, edge=EDGE_NAME[edge], fill=FILL,
                                                    filter="bicubic")
        for i, (what, size) in enumerate(DECODE):
            want_view, want_m = Q.project_filter_view(size[0], size[1], orient[i], matrices[i], Q.BICUBIC, *OUT)
            assert tuple(views[i]) == want_view and np.array_equal(mats[i], want_m), (r, i)
            assert tuple(views[i]) == J.project_view(size, spectrals[i].layout, matrices[i], OUT, orient[i], filter="bicubic")[0]
            assert views[i][0] == want_denoms[i], (r, i)
            seen.add((int(views[i][0]), orient[i]))
        pixels = J.decode_views_mixed(ctx, spectrals, views)
        same(got.cpu().numpy(), J.project(ctx, pixels, mats, OUT, edge=EDGE_NAME[edge], fill=FILL, filter="bicubic").cpu().numpy(), (r, "bytes"))
        same(got[r].cpu().numpy(), Q.project(pixels[r].cpu().numpy(), mats[r], OUT[0], OUT[1], edge, FILL), (r, "mirror"))
        spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
        flips = [i % 2 for i in range(len(DECODE))]
        k = COLOURS[:len(DECODE)] if r % 2 else None
        clamp = (0, 255) if r % 2 else None
        tens, tviews, tmats = J.decode_tensors_projected_mixed(ctx, spectrals, matrices, OUT, spec, flips=flips, orientations=orient,
                                                               edge=EDGE_NAME[edge], fill=FILL, colour=k, colour_clamp=clamp, filter="bicubic")
        assert tviews.tolist() == views.tolist() and np.array_equal(tmats, mats)
        want = J.project_tensor(ctx, pixels, mats, OUT, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL, colour=k, colour_clamp=clamp,
                                filter="bicubic")
        same(tensor_bits(tens, torch), tensor_bits(want, torch), (r, "tensor"))
    assert {d for d, _ in seen} == {1, 2, 4} and {o for _, o in seen} == {1, 3, 6, 8}
    # six numbers per image: the views and the matrices that come back are those of the padded call, [n, 6] again
    six = [rotation(E.oriented_size(o, *size), 20.0, 1.2, canvas=OUT)[:6] for (what, size), o in zip(DECODE, orient)]
    got6, views6, mats6 = J.decode_warped_mixed(ctx, spectrals, six, OUT, orientations=orient, edge=EDGE_NAME[edge], fill=FILL, filter="bicubic")
    nine = [np.concatenate([m, np.array([0, 0, 1], F32)]) for m in six]
    got9, views9, mats9 = J.decode_projected_mixed(ctx, spectrals, nine, OUT, orientations=orient, edge=EDGE_NAME[edge], fill=FILL,
                                                   filter="bicubic")
    assert mats6.shape == (len(DECODE), 6) and np.array_equal(mats6, mats9[:, :6]) and views6.tolist() == views9.tolist()
    same(got6.cpu().numpy(), got9.cpu().numpy(), "six numbers")


# ---- 5. the file route ------------------------------------------------------------------------------------------------------------------

FILES = [("444", (53, 37), "progressive", 0), ("422", (300, 140), "sequential", 5), ("420", (131, 257), "sequential", 0)]
TAGS = [1, 1, 6]


@pytest.fixture(scope="module")
def files():
    datas = []
    for i, (what, size, kind, restart) in enumerate(FILES):
        d = F.synthetic_file(what, size, 180 + i, kind, restart)[0]
        datas.append(d if TAGS[i] == 1 else E.insert(d, E.exif_segment(TAGS[i], big=True)))
    return datas


def test_decompress_with_a_bicubic_warp_is_the_mixed_call_on_the_files_decoded_whole(ctx, torch, files):
    """A progressive, a restart-interval and an EXIF-tagged file, with a homography and with six numbers per file."""
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    rng = np.random.default_rng(411)
    n = len(FILES)
    flips = [1, 0, 1]
    matrices = np.stack([upright_keystone(rng, FILES[i][1], TAGS[i], (0.8, 2.6, 1.5)[i]) for i in range(n)])
    sps = [J.Spectral.decompress(ctx, d) for d in files]
    for edge in ("fill", "replicate"):
        got, views, infos, applied, mats = J.decompress_tensors(ctx, files, OUT, spec, flips=flips, threads=2, orientation="exif",
                                                                warp=matrices.reshape(n, 3, 3), edge=edge, fill=FILL, warp_filter="bicubic")
        assert applied.tolist() == TAGS and mats.shape == (n, 9)
        want, want_views, want_mats = J.decode_tensors_projected_mixed(ctx, sps, matrices, OUT, spec, flips=flips, orientations=TAGS, edge=edge,
                                                                       fill=FILL, filter="bicubic")
        assert views.tolist() == want_views.tolist() and np.array_equal(mats, want_mats)
        same(tensor_bits(got, torch), tensor_bits(want, torch), ("files, tensor", edge))
        for i in range(n):
            assert tuple(views[i]) == Q.project_filter_view(FILES[i][1][0], FILES[i][1][1], TAGS[i], matrices[i], Q.BICUBIC, *OUT)[0]
    raw, raw_views, raw_mats = J.decompress_resized(ctx, files, OUT, threads=2, orientation="exif", warp=matrices, fill=FILL, warp_filter="bicubic")
    want = J.decode_projected_mixed(ctx, sps, matrices, OUT, orientations=TAGS, fill=FILL, filter="bicubic")
    assert raw_views.tolist() == want[1].tolist() and np.array_equal(raw_mats, want[2])
    same(raw.cpu().numpy(), want[0].cpu().numpy(), "files, bytes")
    # the bilinear views are narrower, and the default is the call it was
    plain = J.decompress_resized(ctx, files, OUT, threads=2, orientation="exif", warp=matrices, fill=FILL)
    assert (plain[1][:, 3] <= raw_views[:, 3]).all() and (plain[1][:, 3] < raw_views[:, 3]).any()
    same(plain[0].cpu().numpy(), J.decompress_resized(ctx, files, OUT, threads=2, orientation="exif", warp=matrices, fill=FILL,
                                                      warp_filter="bilinear")[0].cpu().numpy(), "bilinear")
    six = np.stack([rotation(E.oriented_size(TAGS[i], *FILES[i][1]), 15.0, 1.1, canvas=OUT)[:6] for i in range(n)])
    got6 = J.decompress_resized(ctx, files, OUT, orientation="exif", warp=six, fill=FILL, warp_filter="bicubic")
    want6 = J.decode_warped_mixed(ctx, sps, six, OUT, orientations=TAGS, fill=FILL, filter="bicubic")
    assert got6[2].shape == (n, 6) and np.array_equal(got6[2], want6[2]) and got6[1].tolist() == want6[1].tolist()
    same(got6[0].cpu().numpy(), want6[0].cpu().numpy(), "files, six numbers")
