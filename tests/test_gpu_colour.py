"""The colour stage on the MI355X (the six *_colour_* calls; k_resize_placed_tensor, k_tables_placed_tensor and k_mapped_tensor with
the Colour flag): every output is compared element for element, as a bit pattern, with the numpy mirror of the contract
(_colour_ref) on the bytes of the existing mirrors, and where the contract ties into an existing call, with that call on the GPU.
The canvas is 70 x 37 -- two tiles across and two down, the last ones partial, an odd width so that runs of 4 straddle out_w --
and the six sources of a launch each have another matrix.  Every raw call writes into a sentinel-filled buffer, 3 elements
behind an allocation boundary and the images 5 elements apart, whose bytes around the images are checked."""
import ctypes as C

import numpy as np
import pytest

import _antialias_ref as A
import _bicubic_ref as B
import _colour_ref as K
import _files as F
import _orient as E
import _placed_ref as P
import _resize_ref as R
import _tensor_ref as T
import _warp_ref as W
import jpeg_amd as J
from _calls import Out, pixel_image
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, c_spec, host_bits as bits, pack, same, tensor_bits
from jpeg_amd import _lib
from test_gpu_warp import ROTATED, upright_matrix

pytestmark = pytest.mark.gpu

F32 = np.float32
BILINEAR, AA, BICUBIC = _lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS, _lib.FILTER_BICUBIC
MIRROR = {BILINEAR: R.resize, AA: A.resize, BICUBIC: B.resize}
NAME = {BILINEAR: "bilinear", AA: "antialias", BICUBIC: "bicubic"}
CANVAS = (70, 37)
FILL = (7, 130, 255)
SIZES = [(1, 1), (1, 9), (9, 1), (17, 5), (64, 32), (131, 67)]          # (w, h)
# identity, BGR, grey, a jitter, one that saturates, one whose q goes below 0
MATRICES = np.stack([J.colour_matrix(), J.colour_matrix(order="bgr"), J.colour_matrix(grey=True), J.colour_matrix(1.4, 0.7, 1.8, 0.1),
                     K.matrix([[3, 0, 0, 40], [0, 3, 0, 40], [0, 0, 3, 40]]), K.matrix([[-1, -0.5, 0, 20], [0.25, -2, 0.5, -30], [0, 1, -1, 0]])])
IDENTITIES = np.stack([K.IDENTITY] * len(SIZES))
CLAMPS = [(0.0, 255.0), K.NO_CLAMP]
COMBOS = [(T.F32, T.CHW), (T.F16, T.HWC), (T.BF16, T.CHW)]
COMBO_IDS = ["f32-chw", "f16-hwc", "bf16-chw"]
FLIPS = [i % 2 for i in range(len(SIZES))]


@pytest.fixture(scope="module")
def sources():
    return [pixel_image("random", w, h, 57 * w + h) for w, h in SIZES]


def c_colour(k, clamp):
    keep = np.ascontiguousarray(k, F32).reshape(-1, 12)
    c = _lib.Colour()
    c.h_matrices, c.lo, c.hi = keep.ctypes.data, clamp[0], clamp[1]
    return keep, c


def c_fit(fill=FILL):
    p = _lib.Placement()
    p.mode, p.anchor = P.FIT, P.CENTRE
    p.fill[0], p.fill[1], p.fill[2] = fill
    return p


def colour_call(ctx, torch, images, spec, flips, colour, filter=BILINEAR, orient=None, place=None, warp=None):
    """jpeg_amd_resize_colour_tensor_batch, or with warp = (matrices, edge) jpeg_amd_warp_colour_tensor_batch, into a guarded
    buffer; colour: (k, clamp), or None for NULL -> (the images' bytes, the windows written)."""
    n = len(images)
    d_src, stride, ext = pack(ctx, torch, images)
    out = Out(ctx, torch, [3 * CANVAS[0] * CANVAS[1]] * n, elem=4 if spec.dtype == T.F32 else 2, gap=5, lead=3, tail=7)
    keep, col = (None, None) if colour is None else c_colour(*colour)
    cs = c_spec(spec)
    wout = (_lib.Region * n)(*[_lib.Region(-7, -7, -7, -7)] * n)
    if warp is None:
        st = _lib.lib().jpeg_amd_resize_colour_tensor_batch(ctx.handle, n, d_src.data_ptr(), stride, ext, CANVAS[0], CANVAS[1], filter,
                                                            C.byref(cs), c_bytes(flips), c_bytes(orient),
                                                            None if place is None else C.byref(place), wout,
                                                            None if col is None else C.byref(col), out.ptr, out.stride)
    else:
        m = np.ascontiguousarray(warp[0], F32).reshape(n, 6)
        wp = _lib.Warp()
        wp.edge = warp[1]
        wp.fill[0], wp.fill[1], wp.fill[2] = FILL
        st = _lib.lib().jpeg_amd_warp_colour_tensor_batch(ctx.handle, n, d_src.data_ptr(), stride, ext, m.ctypes.data, C.byref(wp), CANVAS[0],
                                                          CANVAS[1], C.byref(cs), c_bytes(flips), None if col is None else C.byref(col),
                                                          out.ptr, out.stride)
    assert st == 0
    ctx.synchronize()
    return out.images(), [(r.x, r.y, r.width, r.height) for r in wout]


# ---- 1. against the mirror, per underlying kernel ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def placed_bytes(sources):
    """Per filter the canvases the placed mirror defines for the six sources with place = FIT: computed once."""
    made = {}
    for f in (BILINEAR, AA, BICUBIC):
        made[f] = []
        for (w, h), src in zip(SIZES, sources):
            win = P.place_window(P.FIT, P.CENTRE, w, h, *CANVAS)
            made[f].append((win, P.place(MIRROR[f](src, win[2], win[3]), win, CANVAS, FILL)))
    return made


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("filter", [BILINEAR, AA, BICUBIC], ids=["bilinear", "antialias", "bicubic"])
def test_placed_with_a_fill_against_the_mirror(ctx, torch, sources, placed_bytes, filter, combo):
    spec = T.Spec(*combo)
    assert max(max(w / win[2], h / win[3]) for (w, h), (win, _) in zip(SIZES, placed_bytes[filter])) <= 8.0     # inside every tap limit
    for clamp in CLAMPS:
        got, windows = colour_call(ctx, torch, sources, spec, FLIPS, (MATRICES, clamp), filter=filter, place=c_fit())
        for i, (win, canvas) in enumerate(placed_bytes[filter]):
            assert windows[i] == win
            same(bits(got[i], spec), K.normalise(canvas, MATRICES[i], clamp, spec, FLIPS[i]), (NAME[filter], SIZES[i], combo, clamp))
    # the fill is transformed like any pixel: a corner of the 1 x 9 source's canvas is padding
    win, canvas = placed_bytes[filter][1]
    assert win[0] > 0 and tuple(canvas[0, 0]) == FILL


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
def test_unplaced_with_orientations_against_the_mirror(ctx, torch, sources, combo):
    spec = T.Spec(*combo)
    orient = [1, 3, 6, 8, 6, 3]
    canvases = [R.resize(E.orient(src, o), *CANVAS) for src, o in zip(sources, orient)]
    for clamp in CLAMPS:
        got, windows = colour_call(ctx, torch, sources, spec, FLIPS, (MATRICES, clamp), orient=orient)
        assert windows == [(-7, -7, -7, -7)] * len(SIZES)                    # no placement: none is written
        for i, canvas in enumerate(canvases):
            same(bits(got[i], spec), K.normalise(canvas, MATRICES[i], clamp, spec, FLIPS[i]), (SIZES[i], orient[i], combo, clamp))
    got, _ = colour_call(ctx, torch, sources, spec, FLIPS, (MATRICES, CLAMPS[0]))          # ... and without orientations
    for i, src in enumerate(sources):
        same(bits(got[i], spec), K.normalise(R.resize(src, *CANVAS), MATRICES[i], CLAMPS[0], spec, FLIPS[i]), (SIZES[i], "stored"))


@pytest.mark.parametrize("combo", COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize("edge", [W.FILL, W.REPLICATE], ids=["fill", "replicate"])
def test_warped_against_the_mirror(ctx, torch, sources, edge, combo):
    spec = T.Spec(*combo)
    canvases = [W.warp(src, m, CANVAS[0], CANVAS[1], edge, FILL) for src, m in zip(sources, ROTATED)]
    for clamp in CLAMPS:
        got, _ = colour_call(ctx, torch, sources, spec, FLIPS, (MATRICES, clamp), warp=(ROTATED, edge))
        for i, canvas in enumerate(canvases):
            same(bits(got[i], spec), K.normalise(canvas, MATRICES[i], clamp, spec, FLIPS[i]), (SIZES[i], edge, combo, clamp))


# ---- 2. the identity and NULL against the GPU's own existing calls ------------------------------------------------------------------------

def test_identity_and_null_are_the_existing_calls(ctx, torch, sources):
    spec = T.Spec(T.F16, T.CHW)
    dev = [torch.from_numpy(s).to(ctx.torch_device) for s in sources]
    js = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    orient = [1, 3, 6, 8, 6, 3]
    for kw in (dict(), dict(orientations=orient), dict(filter="antialias", place="fit", fill=FILL), dict(filter="bicubic", orientations=orient)):
        old = J.resize_tensor(ctx, dev, CANVAS, js, flips=FLIPS, **kw)
        new = J.resize_tensor(ctx, dev, CANVAS, js, flips=FLIPS, colour=IDENTITIES, **kw)
        if "place" in kw:
            assert np.array_equal(old[1], new[1])
            old, new = old[0], new[0]
        same(tensor_bits(new, torch), tensor_bits(old, torch), kw)
    for edge in ("fill", "replicate"):
        old = J.warp_tensor(ctx, dev, ROTATED, CANVAS, js, flips=FLIPS, edge=edge, fill=FILL)
        same(tensor_bits(J.warp_tensor(ctx, dev, ROTATED, CANVAS, js, flips=FLIPS, edge=edge, fill=FILL, colour=IDENTITIES), torch),
             tensor_bits(old, torch), edge)
    # colour == NULL through the raw calls: the named calls, bit for bit
    null, _ = colour_call(ctx, torch, sources, spec, FLIPS, None, orient=orient)
    ident, _ = colour_call(ctx, torch, sources, spec, FLIPS, (IDENTITIES, K.NO_CLAMP), orient=orient)
    wnull, _ = colour_call(ctx, torch, sources, spec, FLIPS, None, warp=(ROTATED, W.FILL))
    for i, src in enumerate(sources):
        same(bits(null[i], spec), T.normalise(R.resize(E.orient(src, orient[i]), *CANVAS), spec, FLIPS[i]), (i, "NULL"))
        same(ident[i], null[i], (i, "identity"))
        same(bits(wnull[i], spec), T.normalise(W.warp(src, ROTATED[i], CANVAS[0], CANVAS[1], W.FILL, FILL), spec, FLIPS[i]), (i, "NULL, warp"))
    # a permutation is the call with the channels permuted (the spec's constants are per channel: equal ones here)
    flat = J.tensor_spec(mean=(0.5, 0.5, 0.5), std=(0.25, 0.25, 0.25), layout="chw")
    bgr = J.resize_tensor(ctx, dev, CANVAS, flat, flips=FLIPS, colour=[J.colour_matrix(order="bgr")] * len(dev))
    same(tensor_bits(bgr, torch), tensor_bits(J.resize_tensor(ctx, dev, CANVAS, flat, flips=FLIPS).flip(1), torch), "bgr")


# ---- 3. the decode route ----------------------------------------------------------------------------------------------------------------

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


def test_decode_tensors_mixed_with_colour_is_the_view_decode_and_the_resample(ctx, torch, spectrals):
    """One chunk: the chunk limit of the resized decodes is 2^30 bytes of decoded views, and these views are far below it.
    Calls of two and three chunks -- launch()'s offsets for a chunk that is not the first, the colour records' among them --
    are test_gpu_resample_chunks.py's: the limit counts stride x images, so one large view and a hundred small ones cross it.
    (The file route below does not reach them: each of its chunks of 32 files makes a mixed call of its own, whose per-image
    arrays begin at the chunk's first file.)"""
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    n = len(DECODE)
    views = [(2, 3, 5, 60, 50), (1, 10, 20, 100, 200), (4, 1, 1, 60, 30), (8, 0, 0, 17, 33), (2, 0, 0, 75, 45)]
    flips = [i % 2 for i in range(n)]
    k = MATRICES[[3, 1, 2, 5, 4]]
    pixels = J.decode_views_mixed(ctx, spectrals, views)
    for kw in (dict(), dict(filter="antialias", orientations=[6, 1, 3, 8, 1]), dict(filter="bicubic", place="fit", fill=FILL)):
        got = J.decode_tensors_mixed(ctx, spectrals, views, OUT, spec, flips=flips, colour=k, colour_clamp=(0, 255), **kw)
        want = J.resize_tensor(ctx, pixels, OUT, spec, flips=flips, colour=k, colour_clamp=(0, 255), **kw)
        if "place" in kw:
            assert np.array_equal(got[1], want[1])
            got, want = got[0], want[0]
        same(tensor_bits(got, torch), tensor_bits(want, torch), kw)
        plain = J.decode_tensors_mixed(ctx, spectrals, views, OUT, spec, flips=flips, **kw)
        assert not torch.equal(got, plain[0] if "place" in kw else plain)
    # the warped form
    orient = [1, 3, 6, 8, 1]
    matrices = [upright_matrix(size, o, 25.0 + 40.0 * i, 1.5 + i, OUT) for i, ((_, size), o) in enumerate(zip(DECODE, orient))]
    got, gviews, gmats = J.decode_tensors_warped_mixed(ctx, spectrals, matrices, OUT, spec, flips=flips, orientations=orient, fill=FILL,
                                                       colour=k, colour_clamp=(0, 255))
    pixels = J.decode_views_mixed(ctx, spectrals, gviews)
    want = J.warp_tensor(ctx, pixels, gmats, OUT, spec, flips=flips, fill=FILL, colour=k, colour_clamp=(0, 255))
    same(tensor_bits(got, torch), tensor_bits(want, torch), "warped")
    assert len(set(gviews[:, 0].tolist())) >= 2


# ---- 4. the file route ------------------------------------------------------------------------------------------------------------------

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


def test_decompress_with_colour_is_the_mixed_call_on_the_files_decoded_whole(ctx, torch, files):
    """40 files -- the six, repeated -- so that the call spans two chunks of the file pipeline (32 files each) and the second
    chunk's mixed call takes the matrices from file 32 on."""
    spec = J.tensor_spec(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), layout="chw")
    reps = 40
    datas = [files[i % 6] for i in range(reps)]
    tags = [TAGS[i % 6] for i in range(reps)]
    flips = [(i // 3) % 2 for i in range(reps)]
    rng = np.random.default_rng(11)
    k = np.stack([J.colour_matrix(*rng.uniform(0.6, 1.4, 3), rng.uniform(-0.1, 0.1), grey=bool(i % 7 == 0)) for i in range(reps)])
    sps = [J.Spectral.decompress(ctx, d) for d in files]
    sps = [sps[i % 6] for i in range(reps)]
    got, views, infos, applied = J.decompress_tensors(ctx, datas, OUT, spec, flips=flips, threads=2, orientation="exif", colour=k,
                                                      colour_clamp=(0, 255))
    assert applied.tolist() == tags
    want = J.decode_tensors_mixed(ctx, sps, views, OUT, spec, flips=flips, orientations=tags, colour=k, colour_clamp=(0, 255))
    same(tensor_bits(got, torch), tensor_bits(want, torch), "files")
    assert not np.array_equal(tensor_bits(got[32:38], torch), tensor_bits(got[2:8], torch))          # (other matrices, other flips)
    # placed, and warped
    got = J.decompress_tensors(ctx, files, OUT, spec, flips=flips[:6], orientation="exif", filter="antialias", place="fit", fill=FILL,
                               colour=k[:6])
    want = J.decode_crops_tensor_mixed(ctx, sps[:6], [(0, 0) + E.oriented_size(o, *f[1]) for f, o in zip(FILES, TAGS)], OUT, spec,
                                       flips=flips[:6], filter="antialias", orientations=TAGS, place="fit", fill=FILL, colour=k[:6])
    assert got[1].tolist() == want[1].tolist() and got[4].tolist() == want[2].tolist()
    same(tensor_bits(got[0], torch), tensor_bits(want[0], torch), "files, placed")
    matrices = [upright_matrix(size, o, -20.0 + 35.0 * i, (0.8, 2.6, 1.0, 5.0, 1.5, 9.0)[i], OUT) for i, ((_, size, _, _), o) in enumerate(zip(FILES, TAGS))]
    got = J.decompress_tensors(ctx, files, OUT, spec, flips=flips[:6], orientation="exif", warp=matrices, fill=FILL, colour=k[:6],
                               colour_clamp=(0, 255))
    want = J.decode_tensors_warped_mixed(ctx, sps[:6], matrices, OUT, spec, flips=flips[:6], orientations=TAGS, fill=FILL, colour=k[:6],
                                         colour_clamp=(0, 255))
    assert got[1].tolist() == want[1].tolist()
    same(tensor_bits(got[0], torch), tensor_bits(want[0], torch), "files, warped")
