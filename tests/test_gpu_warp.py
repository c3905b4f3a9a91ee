"""The warped resample on the MI355X (jpeg_amd_warp_batch, _warp_tensor_batch, the *_warped_mixed decode and file calls;
k_mapped_bytes and k_mapped_tensor over AffineMap and TwoTaps): every output is compared byte for byte, or element for element as a bit pattern, with the
numpy mirror of the contract (_warp_ref), and where the contract ties into an existing call, with that call on the GPU.  The
canvas is 70 x 37 -- two tiles across and two down, the last ones partial, with an odd width so that runs of 4 straddle out_w.
Every raw call writes into a sentinel-filled buffer whose bytes in front of, between and behind the images are checked.
Every matrix is valid, and every read the contract defines lies inside its image."""
import ctypes as C
import math

import numpy as np
import pytest

import _files as F
import _orient as E
import _tensor_ref as T
import _warp_ref as W
import jpeg_amd as J
from _calls import Out, pixel_image
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, c_spec, host_bits as bits, pack, same
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

F32 = np.float32
CANVAS = (70, 37)
FILL = (7, 130, 255)
EDGES = [W.FILL, W.REPLICATE]
EDGE_NAME = {W.FILL: "fill", W.REPLICATE: "replicate"}
SIZES = [(1, 1), (1, 9), (9, 1), (17, 5), (64, 32), (131, 67)]          # (w, h)


def centred(size, canvas, angle=0.0, scale=1.0, shear=0.0, offset=(0.0, 0.0)):
    """The matrix whose linear part is scale * rotation(angle, degrees) * shear and which takes the canvas centre to the source
    centre plus `offset`; scale > 1 reduces.  float32 [6]"""
    a = math.radians(angle)
    lin = scale * np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]]) @ np.array([[1.0, shear], [0.0, 1.0]])
    t = np.array([size[0] / 2.0 + offset[0], size[1] / 2.0 + offset[1]]) - lin @ np.array([canvas[0] / 2.0, canvas[1] / 2.0])
    return np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1]], np.float64).astype(F32)


# one matrix per source: a rotation by 30 degrees, one by -135 with scale 1.7, a shear, a reduction by 3.3, an enlargement by 4,
# and one whose footprint misses the source entirely
MATRICES = [centred(SIZES[0], CANVAS, 30.0), centred(SIZES[1], CANVAS, -135.0, 1.7), centred(SIZES[2], CANVAS, shear=0.4),
            centred(SIZES[3], CANVAS, 10.0, 3.3), centred(SIZES[4], CANVAS, 5.0, 0.25), centred(SIZES[5], CANVAS, 20.0, 1.0, offset=(900.0, -700.0))]
# ... and one set in which every source about fills the canvas, each at another angle
ROTATED = [centred(s, CANVAS, 30.0 + 47.0 * i, 1.3 * max(s[0] / CANVAS[0], s[1] / CANVAS[1])) for i, s in enumerate(SIZES)]


@pytest.fixture(scope="module")
def sources():
    return [pixel_image("random", w, h, 57 * w + h) for w, h in SIZES]


def c_warp(edge, fill=FILL):
    w = _lib.Warp()
    w.edge = edge
    w.fill[0], w.fill[1], w.fill[2] = fill
    return w


def warp_call(ctx, torch, images, matrices, canvas, edge, spec=None, flips=None, lead=3, gap=5):
    """jpeg_amd_warp_batch (spec: _warp_tensor_batch) into a guarded buffer whose first image lies `lead` elements behind an
    allocation boundary, the images 3 out_w out_h + gap elements apart -> the images' bytes."""
    out_w, out_h = canvas
    n = len(images)
    d_src, stride, ext = pack(ctx, torch, images)
    elem = 1 if spec is None else (4 if spec.dtype == T.F32 else 2)
    out = Out(ctx, torch, [3 * out_w * out_h] * n, elem=elem, gap=gap, lead=lead, tail=7)
    m = np.ascontiguousarray(matrices, F32).reshape(n, 6)
    wp = c_warp(edge)
    head = (ctx.handle, n, d_src.data_ptr(), stride, ext, m.ctypes.data, C.byref(wp), out_w, out_h)
    if spec is None:
        st = _lib.lib().jpeg_amd_warp_batch(*head, out.ptr, out.stride)
    else:
        cs = c_spec(spec)
        st = _lib.lib().jpeg_amd_warp_tensor_batch(*head, C.byref(cs), c_bytes(flips), out.ptr, out.stride)
    assert st == 0
    ctx.synchronize()
    return out.images()


# ---- 1. bytes ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_six_sources_in_one_launch(ctx, torch, sources, edge):
    """Nonzero record offsets, taps at -1 and at w, whole tiles of fill, a strided destination whose gaps are left alone."""
    for matrices in (MATRICES, ROTATED):
        got = warp_call(ctx, torch, sources, matrices, CANVAS, edge)
        for i, (src, m) in enumerate(zip(sources, matrices)):
            want = W.warp(src, m, CANVAS[0], CANVAS[1], edge, FILL)
            same(got[i], want, (SIZES[i], EDGE_NAME[edge]))
    if edge == W.FILL:
        missed = W.warp(sources[5], MATRICES[5], CANVAS[0], CANVAS[1], edge, FILL)
        assert (missed == np.asarray(FILL, np.uint8)).all()                       # the footprint that misses its source: fill alone
        inside = W.warp(sources[4], MATRICES[4], CANVAS[0], CANVAS[1], edge, FILL)
        assert (inside != np.asarray(FILL, np.uint8)).any(axis=2).mean() > 0.9    # ... and the enlargement shows its source


def test_the_scale_matrix_with_replicate_is_the_gpu_resize(ctx, torch, sources):
    dev = [torch.from_numpy(s).to(ctx.torch_device) for s in sources]
    matrices = [[F32(w) / F32(CANVAS[0]), 0, 0, 0, F32(h) / F32(CANVAS[1]), 0] for w, h in SIZES]
    got = J.warp(ctx, dev, matrices, CANVAS, edge="replicate").cpu().numpy()
    same(got, J.resize(ctx, dev, CANVAS).cpu().numpy(), "resize")


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_identity_and_quarter_turn(ctx, torch, sources, edge):
    src = sources[5]
    h, w = src.shape[:2]
    dev = [torch.from_numpy(src).to(ctx.torch_device)]
    same(J.warp(ctx, dev, [[1, 0, 0, 0, 1, 0]], (w, h), edge=EDGE_NAME[edge], fill=FILL).cpu().numpy()[0], src, "identity")
    same(J.warp(ctx, dev, [[0, 1, 0, -1, 0, h]], (h, w), edge=EDGE_NAME[edge], fill=FILL).cpu().numpy()[0], np.rot90(src, -1), "clockwise")
    same(J.warp(ctx, dev, [J.affine_matrix((w, w), (w, w), angle=90)], (w, w), edge="replicate").cpu().numpy()[0],
         W.warp(src, [0, -1, w, 1, 0, 0], w, w, W.REPLICATE), "affine_matrix(90)")


# ---- 2. the tensor forms ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("combo", [(T.F32, T.HWC), (T.F16, T.CHW), (T.BF16, T.CHW)], ids=["f32-hwc", "f16-chw", "bf16-chw"])
@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_tensor_forms_flip_the_warped_image(ctx, torch, sources, combo, edge):
    """Into a destination one element behind an allocation boundary, the images 3 * 70 * 37 + 5 elements apart: the sinks'
    unaligned paths; Out.images() checks that the gap elements are left alone."""
    spec = T.Spec(*combo)
    flips = [i % 2 for i in range(len(sources))]
    got = warp_call(ctx, torch, sources, ROTATED, CANVAS, edge, spec=spec, flips=flips, lead=1, gap=5)
    for i, (src, m) in enumerate(zip(sources, ROTATED)):
        want = T.normalise(W.warp(src, m, CANVAS[0], CANVAS[1], edge, FILL), spec, flips[i])
        same(bits(got[i], spec), want, (SIZES[i], combo, EDGE_NAME[edge], flips[i]))
        # said by the contract's own formula too: the flip moves the taps, xs = out_w - 1 - x
        direct = T.normalise(W.warp(src, m, CANVAS[0], CANVAS[1], edge, FILL, flip=bool(flips[i])), spec, 0)
        same(bits(got[i], spec), direct, (SIZES[i], "xs"))
    # the fill is normalised like any byte
    got = warp_call(ctx, torch, [sources[5]], [MATRICES[5]], CANVAS, W.FILL, spec=spec, flips=[1], lead=1)
    pad = T.normalise(np.asarray(FILL, np.uint8).reshape(1, 1, 3), spec, 0).reshape(3)
    g = bits(got[0], spec)
    g = g.reshape(3, -1).T if spec.layout == T.CHW else g.reshape(-1, 3)
    assert (g == pad).all()


# ---- 3. one context, call after call ----------------------------------------------------------------------------------------------------

def test_two_calls_through_one_context(ctx, torch, sources):
    other = [pixel_image("random", w, h, 991 * w + h) for w, h in SIZES]
    first = warp_call(ctx, torch, sources, ROTATED, CANVAS, W.FILL)
    second = warp_call(ctx, torch, other, ROTATED, CANVAS, W.FILL)
    third = warp_call(ctx, torch, other, MATRICES, CANVAS, W.REPLICATE)
    for i in range(len(SIZES)):
        same(first[i], W.warp(sources[i], ROTATED[i], CANVAS[0], CANVAS[1], W.FILL, FILL), ("first", i))
        same(second[i], W.warp(other[i], ROTATED[i], CANVAS[0], CANVAS[1], W.FILL, FILL), ("second", i))
        same(third[i], W.warp(other[i], MATRICES[i], CANVAS[0], CANVAS[1], W.REPLICATE), ("third", i))


def test_no_images(ctx, torch):
    assert tuple(J.warp(ctx, [], np.zeros((0, 6), F32), CANVAS).shape) == (0, CANVAS[1], CANVAS[0], 3)
    spec = J.tensor_spec(layout="chw")
    assert tuple(J.warp_tensor(ctx, [], np.zeros((0, 6), F32), CANVAS, spec).shape) == (0, 3, CANVAS[1], CANVAS[0])
    out, views, mats = J.decode_warped_mixed(ctx, [], np.zeros((0, 6), F32), CANVAS)
    assert tuple(out.shape) == (0, CANVAS[1], CANVAS[0], 3) and views.shape == (0, 5) and mats.shape == (0, 6)
    out, views, mats = J.decompress_resized(ctx, [], CANVAS, warp=np.zeros((0, 6), F32))
    assert tuple(out.shape) == (0, CANVAS[1], CANVAS[0], 3)


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


def upright_matrix(size, o, angle, scale, out=OUT):
    """A rotation by `angle` about the centre of the UPRIGHT image that reduces it by `scale` times what fits it to the canvas."""
    uw, uh = E.oriented_size(o, *size)
    return J.affine_matrix((uw, uh), out, angle=angle, scale=1.0 / scale)


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_decode_warped_mixed_is_the_view_decode_and_the_warp(ctx, torch, spectrals, edge):
    # per image an orientation and a reduction; four rounds so that every image meets every denominator and orientation
    seen = set()
    for r in range(4):
        orient = [(1, 3, 6, 8)[(i + r) % 4] for i in range(len(DECODE))]
        want_denoms = [(1, 2, 4, 8)[(i + 2 * r + 1) % 4] for i in range(len(DECODE))]
        matrices = []
        for (what, size), o, d in zip(DECODE, orient, want_denoms):
            uw, uh = E.oriented_size(o, *size)
            fit = min(uw / OUT[0], uh / OUT[1])                 # the smaller step of the crop-resize matrix
            matrices.append(upright_matrix(size, o, 25.0 + 40.0 * r, 1.2 * d / fit))
        got, views, mats = J.decode_warped_mixed(ctx, spectrals, matrices, OUT, orientations=orient, edge=EDGE_NAME[edge], fill=FILL)
        for i, (what, size) in enumerate(DECODE):
            want_view, want_m = W.warp_view(size[0], size[1], orient[i], matrices[i], *OUT)
            assert tuple(views[i]) == want_view and np.array_equal(mats[i], want_m), (r, i)
            assert tuple(views[i]) == J.warp_view(size, spectrals[i].layout, matrices[i], OUT, orient[i])[0]
            seen.add((int(views[i][0]), orient[i]))
        pixels = J.decode_views_mixed(ctx, spectrals, views)
        same(got.cpu().numpy(), J.warp(ctx, pixels, mats, OUT, edge=EDGE_NAME[edge], fill=FILL).cpu().numpy(), (r, "bytes"))
        for i, p in enumerate(pixels):                          # ... and the mirror on the decoded view
            same(got[i].cpu().numpy(), W.warp(p.cpu().numpy(), mats[i], OUT[0], OUT[1], edge, FILL), (r, i, "mirror"))
        spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
        flips = [i % 2 for i in range(len(DECODE))]
        tens, tviews, tmats = J.decode_tensors_warped_mixed(ctx, spectrals, matrices, OUT, spec, flips=flips, orientations=orient,
                                                            edge=EDGE_NAME[edge], fill=FILL)
        assert tviews.tolist() == views.tolist() and np.array_equal(tmats, mats)
        want = J.warp_tensor(ctx, pixels, mats, OUT, spec, flips=flips, edge=EDGE_NAME[edge], fill=FILL)
        same(tens.view(torch.int16).cpu().numpy(), want.view(torch.int16).cpu().numpy(), (r, "tensor"))
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


@pytest.mark.parametrize("edge", EDGES, ids=["fill", "replicate"])
def test_decompress_with_a_warp_is_the_mixed_call_on_the_files_decoded_whole(ctx, torch, files, edge):
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    flips = [0, 1, 0, 1, 1, 0]
    matrices = [upright_matrix(size, o, -20.0 + 35.0 * i, (0.8, 2.6, 1.0, 5.0, 1.5, 9.0)[i]) for i, ((_, size, _, _), o) in enumerate(zip(FILES, TAGS))]
    got, views, infos, applied, mats = J.decompress_tensors(ctx, files, OUT, spec, flips=flips, threads=2, orientation="exif", warp=matrices,
                                                            edge=EDGE_NAME[edge], fill=FILL)
    assert applied.tolist() == TAGS and len(set(views[:, 0].tolist())) >= 3
    sps = [J.Spectral.decompress(ctx, d) for d in files]
    want, want_views, want_mats = J.decode_tensors_warped_mixed(ctx, sps, matrices, OUT, spec, flips=flips, orientations=TAGS,
                                                                edge=EDGE_NAME[edge], fill=FILL)
    assert views.tolist() == want_views.tolist() and np.array_equal(mats, want_mats)
    same(got.view(torch.int16).cpu().numpy(), want.view(torch.int16).cpu().numpy(), "files, tensor")
    raw, raw_views, raw_mats = J.decompress_resized(ctx, files, OUT, threads=2, orientation="exif", warp=matrices, edge=EDGE_NAME[edge], fill=FILL)
    assert raw_views.tolist() == views.tolist() and np.array_equal(raw_mats, mats)
    same(raw.cpu().numpy(), J.decode_warped_mixed(ctx, sps, matrices, OUT, orientations=TAGS, edge=EDGE_NAME[edge], fill=FILL)[0].cpu().numpy(),
         "files, bytes")
    # without `orientation` the matrices are taken against the images as they are stored
    stored = J.decompress_resized(ctx, files[2:3], OUT, warp=matrices[2:3], edge=EDGE_NAME[edge], fill=FILL)[0]
    same(stored.cpu().numpy(), J.decode_warped_mixed(ctx, sps[2:3], matrices[2:3], OUT, edge=EDGE_NAME[edge], fill=FILL)[0].cpu().numpy(), "stored")
    for bad in (dict(source_regions=[(0, 0, 8, 8)] * 6), dict(place="fit"), dict(filter="antialias")):
        with pytest.raises(ValueError):
            J.decompress_tensors(ctx, files, OUT, spec, warp=matrices, **bad)
