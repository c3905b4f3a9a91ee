"""The projective resample on the MI355X (jpeg_amd_project_batch, _project_tensor_batch, the *_projected_mixed decode and file
calls; k_mapped_bytes and k_mapped_tensor over ProjectiveMap and TwoTaps): every output is compared byte for byte, or element for element as a bit
pattern, with the numpy mirror of the contract (_project_ref) -- which is what holds the kernel's division to the correctly
rounded one -- and where the contract ties into an existing call, with that call on the GPU.  The canvas is 70 x 37: two tiles
across and two down, the last ones partial, with an odd width so that runs of 4 straddle out_w.  Every raw call writes into a
sentinel-filled buffer whose bytes in front of, between and behind the images are checked.  Every matrix passes the
contract's check, and every read the contract defines lies inside its image."""
import ctypes as C
import math

import numpy as np
import pytest

import _colour_ref as K
import _files as F
import _orient as E
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
EDGES = [P.FILL, P.REPLICATE]
EDGE_NAME = {P.FILL: "fill", P.REPLICATE: "replicate"}
SIZES = [(1, 1), (1, 9), (9, 1), (17, 5), (64, 32), (131, 67)]          # (w, h)
BOX = [(0, 0), (CANVAS[0], 0), (CANVAS[0], CANVAS[1]), (0, CANVAS[1])]


def quad(points):
    """The homography that takes the canvas's corners, clockwise from (0, 0), to four source points, float32 [9]."""
    return P.homography(points, BOX).reshape(9).astype(F32)


def near_the_limit(size, share=0.996):
    """A keystone whose denominator falls from 1 at the canvas's left edge towards the right with `share` of the slope at which
    its minimum is S / 16 (S / min W = 15.5 here), composed with the scale that fits its image (x / (1 - a x) over the canvas)
    onto the source."""
    a = share * (15.0 / 17.0) / CANVAS[0]
    far = CANVAS[0] / (1.0 - a * CANVAS[0])
    m = np.diag([size[0] / far, size[1] / CANVAS[1], 1.0]) @ np.array([[1, 0, 0], [0, 1, 0], [-a, 0, 1.0]])
    return m.reshape(9).astype(F32)


def affine(size, angle, scale):
    a = math.radians(angle)
    lin = scale * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    t = np.array([size[0] / 2.0, size[1] / 2.0]) - lin @ np.array([CANVAS[0] / 2.0, CANVAS[1] / 2.0])
    return np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1], 0, 0, 1], np.float64).astype(F32)


# one matrix per source: one with m22 != 1 (a keystone times 2.5 throughout), a map that folds most of the canvas outside its
# source, a footprint that misses its source, a last row (0, 0, 1), one within a few percent of the S / 16 limit, a mild keystone
MATRICES = [(2.5 * quad([(-0.5, -0.4), (1.6, 0.1), (1.2, 1.5), (0.1, 0.9)]).astype(np.float64)).astype(F32),
            quad([(-3.0, -14.0), (5.0, -9.0), (3.5, 30.0), (-4.0, 17.0)]),
            quad([(400.0, -300.0), (420.0, -310.0), (425.0, -280.0), (395.0, -285.0)]),
            affine(SIZES[3], 25.0, 0.3),
            near_the_limit(SIZES[4]),
            quad([(9.0, 4.0), (125.0, -3.0), (133.0, 69.0), (-2.0, 58.0)])]
# ... and one set of seeded four-corner distortions in which every source about fills the canvas
KEYSTONES = [P.distortion(np.random.default_rng(300 + i), w, h, CANVAS[0], CANVAS[1], 0.5, 0.1) for i, (w, h) in enumerate(SIZES)]


def test_the_matrices_are_what_they_are_said_to_be():
    for m in MATRICES + KEYSTONES:
        assert P.accepted(m, *CANVAS)
    s, low = P.conditioning(MATRICES[4], *CANVAS)
    assert 15.0 < s / low < 16.0                                    # within a few percent of the limit, inside it
    assert MATRICES[0][8] == F32(2.5) and MATRICES[3][6:].tolist() == [0, 0, 1]
    assert all(abs(m[6]) + abs(m[7]) > 0 for i, m in enumerate(MATRICES) if i != 3)


@pytest.fixture(scope="module")
def sources():
    return [pixel_image("random", w, h, 57 * w + h) for w, h in SIZES]


def c_warp(edge, fill=FILL):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = fill
    return w


def project_call(ctx, torch, images, matrices, canvas, edge, spec=None, flips=None, colour=None, lead=3, gap=5):
    """jpeg_amd_project_batch (spec: _project_tensor_batch; colour: (k, clamp) or None for NULL) into a guarded buffer whose
    first image lies `lead` elements behind an allocation boundary, the images 3 out_w out_h + gap elements apart -> the
    images' bytes."""
    out_w, out_h = canvas
    n = len(images)
    d_src, stride, ext = pack(ctx, torch, images)
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=gap, lead=lead, tail=7)
    m = np.ascontiguousarray(matrices, F32).reshape(n, 9)
    wp = c_warp(edge)
    head = (ctx.handle, n, d_src.data_ptr(), stride, ext, m.ctypes.data, C.byref(wp), out_w, out_h)
    if spec is None:
        st = _lib.lib().jpeg_amd_project_batch(*head, out.ptr, out.stride)
    else:
        cs = c_spec(spec)
        col = None
        if colour is not None:
            keep = np.ascontiguousarray(colour[0], F32).reshape(-1, 12)
            col = _lib.Colour()
            col.h_matrices, col.lo, col.hi = keep.ctypes.data, colour[1][0], colour[1][1]
        st = _lib.lib().jpeg_amd_project_tensor_batch(*head, C.byref(cs), c_bytes(flips), None if col is None else C.byref(col), out.ptr,
                                                      out.stride)
    assert st == 0
    ctx.synchronize()
    return out.images()


# ---- 1. bytes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_six_sources_in_one_launch(ctx, torch, sources, edge):
    """Nonzero record offsets, taps at -1 and at w, whole tiles of fill, a denominator close to its limit, a strided destination
    whose gaps are left alone; bit for bit, so the division is the correctly rounded one."""
    for matrices in (MATRICES, KEYSTONES):
        got = project_call(ctx, torch, sources, matrices, CANVAS, edge)
        for i, (src, m) in enumerate(zip(sources, matrices)):
            want = P.project(src, m, CANVAS[0], CANVAS[1], edge, FILL)
            same(got[i], want, (SIZES[i], EDGE_NAME[edge]))
    if edge == P.FILL:
        fill = np.asarray(FILL, np.uint8)
        assert (P.project(sources[2], MATRICES[2], CANVAS[0], CANVAS[1], edge, FILL) == fill).all()       # the footprint that misses
        folded = (P.project(sources[1], MATRICES[1], CANVAS[0], CANVAS[1], edge, FILL) == fill).all(axis=2).mean()
        assert 0.5 < folded < 1.0                                                                         # most of the canvas outside
        assert (P.project(sources[5], MATRICES[5], CANVAS[0], CANVAS[1], edge, FILL) != fill).any(axis=2).mean() > 0.9


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_a_last_row_001_is_the_gpu_warp(ctx, torch, sources, edge):
    dev = [torch.from_numpy(s).to(ctx.torch_device) for s in sources]
    six = [affine(s, 30.0 + 47.0 * i, 1.3 * max(s[0] / CANVAS[0], s[1] / CANVAS[1]))[:6] for i, s in enumerate(SIZES)]
    nine = [np.concatenate([m, np.array([0, 0, 1], F32)]) for m in six]
    got = J.project(ctx, dev, nine, CANVAS, edge=EDGE_NAME[edge], fill=FILL).cpu().numpy()
    same(got, J.warp(ctx, dev, six, CANVAS, edge=EDGE_NAME[edge], fill=FILL).cpu().numpy(), "warp")
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    flips = [i % 2 for i in range(len(dev))]
    same(tensor_bits(J.project_tensor(ctx, dev, np.array(nine).reshape(-1, 3, 3), CANVAS, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL), torch),
         tensor_bits(J.warp_tensor(ctx, dev, six, CANVAS, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL), torch), "warp_tensor")


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
    canvases = [P.project(src, m, CANVAS[0], CANVAS[1], edge, FILL) for src, m in zip(sources, KEYSTONES)]
    plain = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, lead=1, gap=5)
    for i, (src, m) in enumerate(zip(sources, KEYSTONES)):
        same(bits(plain[i], spec), T.normalise(canvases[i], spec, flips[i]), (SIZES[i], combo, EDGE_NAME[edge], flips[i]))
        # said by the contract's own formula too: the flip moves the taps, xs = out_w - 1 - x
        direct = T.normalise(P.project(src, m, CANVAS[0], CANVAS[1], edge, FILL, flip=bool(flips[i])), spec, 0)
        same(bits(plain[i], spec), direct, (SIZES[i], "xs"))
    for clamp in ((0.0, 255.0), K.NO_CLAMP):
        got = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, colour=(COLOURS, clamp), lead=1, gap=5)
        for i in range(len(sources)):
            same(bits(got[i], spec), K.normalise(canvases[i], COLOURS[i], clamp, spec, flips[i]), (SIZES[i], combo, EDGE_NAME[edge], clamp))
    # the identity colour is the call without one, and colour = NULL is that call
    ident = project_call(ctx, torch, sources, KEYSTONES, CANVAS, edge, spec=spec, flips=flips, colour=(np.stack([K.IDENTITY] * 6), K.NO_CLAMP),
                         lead=1, gap=5)
    for i in range(len(sources)):
        same(ident[i], plain[i], (SIZES[i], "identity"))


# ---- 3. one context, call after call ----------------------------------------------------------------------------------------------------

def test_two_calls_through_one_context(ctx, torch, sources):
    other = [pixel_image("random", w, h, 991 * w + h) for w, h in SIZES]
    first = project_call(ctx, torch, sources, KEYSTONES, CANVAS, P.FILL)
    second = project_call(ctx, torch, other, KEYSTONES, CANVAS, P.FILL)
    third = project_call(ctx, torch, other, MATRICES, CANVAS, P.REPLICATE)
    for i in range(len(SIZES)):
        same(first[i], P.project(sources[i], KEYSTONES[i], CANVAS[0], CANVAS[1], P.FILL, FILL), ("first", i))
        same(second[i], P.project(other[i], KEYSTONES[i], CANVAS[0], CANVAS[1], P.FILL, FILL), ("second", i))
        same(third[i], P.project(other[i], MATRICES[i], CANVAS[0], CANVAS[1], P.REPLICATE), ("third", i))


def test_no_images(ctx, torch):
    assert tuple(J.project(ctx, [], np.zeros((0, 9), F32), CANVAS).shape) == (0, CANVAS[1], CANVAS[0], 3)
    spec = J.tensor_spec(layout="chw")
    assert tuple(J.project_tensor(ctx, [], np.zeros((0, 9), F32), CANVAS, spec).shape) == (0, 3, CANVAS[1], CANVAS[0])
    out, views, mats = J.decode_projected_mixed(ctx, [], np.zeros((0, 9), F32), CANVAS)
    assert tuple(out.shape) == (0, CANVAS[1], CANVAS[0], 3) and views.shape == (0, 5) and mats.shape == (0, 9)
    out, views, mats = J.decompress_resized(ctx, [], CANVAS, warp=np.zeros((0, 9), F32))
    assert tuple(out.shape) == (0, CANVAS[1], CANVAS[0], 3) and mats.shape == (0, 9)


# ---- 4. the decode route ----------------------------------------------------------------------------------------------------------------

F311 = [(3, 1), (1, 1), (1, 1)]                               # no tile kernel takes a factor of 3: the one-image fallback
DECODE = [("420", (300, 140)), ("444", (131, 257)), ("422", (300, 140)), ("y8", (131, 257)), (F311, (150, 90))]
OUT = (48, 32)


@pytest.fixture(scope="module")
def spectrals(ctx):
    sps = []
    for i, (what, size) in enumerate(DECODE):
        name, factors = (what, None) if isinstance(what, str) else (None, what)
        sps.append(J.Spectral.decompress(ctx, F.synthetic_file(name, size, 70 + i, factors=factors)[0]))
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
    # per image an orientation and a reduction; four rounds so that every image meets every denominator and orientation
    seen = set()
    rng = np.random.default_rng(307)
    for r in range(4):
        orient = [(1, 3, 6, 8)[(i + r) % 4] for i in range(len(DECODE))]
        want_denoms = [(1, 2, 4, 8)[(i + 2 * r + 1) % 4] for i in range(len(DECODE))]
        matrices = [upright_keystone(rng, size, o, 1.5 * d) for (what, size), o, d in zip(DECODE, orient, want_denoms)]
        got, views, mats = J.decode_projected_mixed(ctx, spectrals, matrices, OUT, orientations=orient, edge=EDGE_NAME[edge], fill=FILL)
        for i, (what, size) in enumerate(DECODE):
            want_view, want_m = P.project_view(size[0], size[1], orient[i], matrices[i], *OUT)
            assert tuple(views[i]) == want_view and np.array_equal(mats[i], want_m), (r, i)
            assert tuple(views[i]) == J.project_view(size, spectrals[i].layout, matrices[i], OUT, orient[i])[0]
            assert views[i][0] == want_denoms[i], (r, i)
            seen.add((int(views[i][0]), orient[i]))
        pixels = J.decode_views_mixed(ctx, spectrals, views)
        same(got.cpu().numpy(), J.project(ctx, pixels, mats, OUT, edge=EDGE_NAME[edge], fill=FILL).cpu().numpy(), (r, "bytes"))
        for i, p in enumerate(pixels):                          # ... and the mirror on the decoded view
            same(got[i].cpu().numpy(), P.project(p.cpu().numpy(), mats[i], OUT[0], OUT[1], edge, FILL), (r, i, "mirror"))
        spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
        flips = [i % 2 for i in range(len(DECODE))]
        k = COLOURS[:len(DECODE)] if r % 2 else None
        clamp = (0, 255) if r % 2 else None
        tens, tviews, tmats = J.decode_tensors_projected_mixed(ctx, spectrals, matrices, OUT, spec, flips=flips, orientations=orient,
                                                               edge=EDGE_NAME[edge], fill=FILL, colour=k, colour_clamp=clamp)
        assert tviews.tolist() == views.tolist() and np.array_equal(tmats, mats)
        want = J.project_tensor(ctx, pixels, mats, OUT, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL, colour=k, colour_clamp=clamp)
        same(tensor_bits(tens, torch), tensor_bits(want, torch), (r, "tensor"))
    assert {d for d, _ in seen} == {1, 2, 4, 8} and {o for _, o in seen} == {1, 3, 6, 8}


# ---- 5. the file route ------------------------------------------------------------------------------------------------------------------

FILES = [("420", (300, 140), "sequential", 0), ("y8", (131, 257), "sequential", 3), ("444", (53, 37), "progressive", 0),
         ("422", (300, 140), "sequential", 5), (F311, (150, 90), "sequential", 0), ("420", (131, 257), "dense", 0)]
TAGS = [1, 1, 6, 3, 1, 8]


@pytest.fixture(scope="module")
def files():
    datas = []
    for i, (what, size, kind, restart) in enumerate(FILES):
        name, factors = (what, None) if isinstance(what, str) else (None, what)
        d = F.synthetic_file(name, size, 80 + i, kind, restart, factors=factors)[0]
        datas.append(d if TAGS[i] == 1 else E.insert(d, E.exif_segment(TAGS[i], big=bool(i % 2))))
    return datas


def test_decompress_with_a_homography_is_the_mixed_call_on_the_files_decoded_whole(ctx, torch, files):
    """40 files -- the six, repeated, each with a matrix of its own -- so that the call spans two chunks of the file pipeline
    (32 files each) and the second chunk's mixed call takes the matrices from file 32 on."""
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    reps = 40
    rng = np.random.default_rng(311)
    datas = [files[i % 6] for i in range(reps)]
    tags = [TAGS[i % 6] for i in range(reps)]
    flips = [(i // 3) % 2 for i in range(reps)]
    matrices = np.stack([upright_keystone(rng, FILES[i % 6][1], tags[i], (0.8, 2.6, 1.0, 5.0, 1.5, 13.0)[(i + i // 6) % 6]) for i in range(reps)])
    sps = [J.Spectral.decompress(ctx, d) for d in files]
    sps = [sps[i % 6] for i in range(reps)]
    for edge in ("fill", "replicate"):
        got, views, infos, applied, mats = J.decompress_tensors(ctx, datas, OUT, spec, flips=flips, threads=2, orientation="exif",
                                                                warp=matrices.reshape(reps, 3, 3), edge=edge, fill=FILL)
        assert applied.tolist() == tags and set(views[:, 0].tolist()) == {1, 2, 4, 8} and mats.shape == (reps, 9)
        want, want_views, want_mats = J.decode_tensors_projected_mixed(ctx, sps, matrices, OUT, spec, flips=flips, orientations=tags, edge=edge,
                                                                       fill=FILL)
        assert views.tolist() == want_views.tolist() and np.array_equal(mats, want_mats)
        same(tensor_bits(got, torch), tensor_bits(want, torch), ("files, tensor", edge))
    assert not np.array_equal(tensor_bits(got[32:38], torch), tensor_bits(got[2:8], torch))          # (other matrices, other flips)
    # bytes, and the tensor form with a colour stage, on the six
    raw, raw_views, raw_mats = J.decompress_resized(ctx, files, OUT, threads=2, orientation="exif", warp=matrices[:6], fill=FILL)
    want = J.decode_projected_mixed(ctx, sps[:6], matrices[:6], OUT, orientations=TAGS, fill=FILL)
    assert raw_views.tolist() == want[1].tolist() and np.array_equal(raw_mats, want[2])
    same(raw.cpu().numpy(), want[0].cpu().numpy(), "files, bytes")
    got = J.decompress_tensors(ctx, files, OUT, spec, flips=flips[:6], orientation="exif", warp=matrices[:6], fill=FILL, colour=COLOURS,
                               colour_clamp=(0, 255))
    want = J.decode_tensors_projected_mixed(ctx, sps[:6], matrices[:6], OUT, spec, flips=flips[:6], orientations=TAGS, fill=FILL, colour=COLOURS,
                                            colour_clamp=(0, 255))
    assert got[1].tolist() == want[1].tolist()
    same(tensor_bits(got[0], torch), tensor_bits(want[0], torch), "files, colour")
    # without `orientation` the matrices are taken against the images as they are stored
    stored = J.decompress_resized(ctx, files[2:3], OUT, warp=matrices[2:3], fill=FILL)[0]
    same(stored.cpu().numpy(), J.decode_projected_mixed(ctx, sps[2:3], matrices[2:3], OUT, fill=FILL)[0].cpu().numpy(), "stored")
    for bad in (dict(source_regions=[(0, 0, 8, 8)] * 6), dict(place="fit"), dict(filter="antialias")):
        with pytest.raises(ValueError):
            J.decompress_tensors(ctx, files, OUT, spec, warp=matrices[:6], **bad)
