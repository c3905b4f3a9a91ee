"""jpeg_amd_decompress_tensor_mixed and jpeg_amd_decompress_resized_mixed on the MI355X: JPEG files of mixed sizes and
layouts to one tensor in one call.  The contract is by reference: image i is, bit for bit, what the mixed call writes for the
file decoded by the host into WHOLE planes (Spectral.decompress) with the view the data-loader call chooses -- which is what
every test here compares with.  The file call itself rebuilds only the heads of the blocks of the views' windows in a plane
buffer that the context keeps, so one test runs two sets of files of the same sizes through one context: a read outside the
expanded windows would show the first set's coefficients.  One test anchors three files on the oracle, so that the two routes
cannot be wrong alike.  Every output buffer is filled with a sentinel before the call, and the bytes between and behind the
images are checked after it."""
import ctypes as C

import numpy as np
import pytest

import _files as F
import _scaled_ref as S
import jpeg_amd as J
from _calls import SENTINEL, Out
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from jpeg_amd import _lib
from jpeg_amd.api import _crop_views
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RGB, YCC = _lib.COLOR_RGB8, _lib.COLOR_YCC8
OUT = (24, 16)
F311 = [(3, 1), (1, 1), (1, 1)]                               # no tile kernel takes a factor of 3: the one-image fallback
# (layout name or factors or golden file, size, kind, restart interval, source rectangle or None = the whole image)
FILES = [
    ("420", (300, 140), "sequential", 0, None),
    ("y8", (131, 257), "sequential", 3, None),
    ("444", (17, 33), "progressive", 0, None),
    ("422", (300, 140), "sequential", 5, (236, 100, 64, 40)),      # the bottom right corner
    ("440", (131, 257), "scans", 0, (5, 7, 1, 1)),                 # one pixel
    (F311, (150, 90), "sequential", 0, None),
    ("color-sequential-restart.jpg", None, None, None, None),
    ("grayscale-progressive-1.jpg", None, None, None, None),
    ("y8", (7, 9), "sequential", 0, None),
    ("420", (1, 1), "sequential", 0, None),
    ("444", (300, 140), "sequential", 0, (10, 20, 100, 70)),
    ("420", (131, 257), "sequential", 2, (3, 9, 120, 200)),
    ("440", (300, 140), "sequential", 0, (50, 30, 50, 34)),
    ("422", (17, 33), "sequential", 0, None),
    ("y8", (300, 140), "progressive", 0, None),
    ("420", (300, 140), "sequential", 0, (299, 139, 1, 1)),        # one pixel, the last one
    ("420", (131, 257), "dense", 0, (20, 30, 100, 70)),            # the sparse decoder's arena runs full half way: planes
]
# the same sizes, layouts and kinds with other contents and other rectangles: the second set of the stale-scratch test
OTHER_RECTS = [(150, 70, 150, 70), (0, 100, 131, 157), (3, 3, 9, 20), None, (60, 120, 64, 128), (20, 10, 100, 64), (100, 200, 156, 184),
               (320, 0, 320, 359), None, None, (150, 50, 120, 80), None, (200, 100, 100, 40), (8, 16, 9, 17), (0, 0, 150, 140),
               (0, 0, 200, 139), None]


def make_files(seed, rects=None):
    datas, regions = [], []
    for i, (what, size, kind, restart, rect) in enumerate(FILES):
        if isinstance(what, str) and what.endswith(".jpg"):
            datas.append(F.golden_file(what))
        else:
            name, factors = (what, None) if isinstance(what, str) else (None, what)
            datas.append(F.synthetic_file(name, size, seed + i, kind, restart, factors=factors)[0])
        info = F.inspect(datas[-1])
        rect = rects[i] if rects else rect
        regions.append(rect or (0, 0, info.width, info.height))
    return datas, regions


def spec_of(form):
    s = _lib.TensorSpec()
    s.dtype, s.layout = (_lib.F16, _lib.TENSOR_CHW) if form == "f16-chw" else (_lib.F32, _lib.TENSOR_HWC)
    for c, (m, k) in enumerate(((123.675, 0.0171247538), (116.28, 0.0175070028), (103.53, 0.0174291939))):
        s.mean[c], s.scale[c] = m, k
    return s


def file_call(ctx, datas, regions, out_size, filter, out_ptr, stride, spec=None, flips=None, cosited=0, color=RGB, threads=3,
              whole=False):
    """The tensor call (spec) or the byte call -> (status, views [n, 5], infos)."""
    n = len(datas)
    ptrs = (C.c_void_p * max(n, 1))(*[None if d is None else d.ctypes.data for d in datas])     # (None: a null pointer)
    sizes = (C.c_size_t * max(n, 1))(*[0 if d is None else d.size for d in datas])
    regs = None if whole else (_lib.Region * max(n, 1))(*[_lib.Region(*r) for r in regions])
    infos, views = (_lib.FrameInfo * max(n, 1))(), (_lib.View * max(n, 1))()
    head = (ctx.handle, ptrs, sizes, n, threads, cosited, color, regs, out_size[0], out_size[1], filter)
    if spec is not None:
        h_flip = None if flips is None else (C.c_uint8 * max(n, 1))(*flips)
        st = _lib.lib().jpeg_amd_decompress_tensor_mixed(*head, C.byref(spec), h_flip, out_ptr, stride, infos, views)
    else:
        st = _lib.lib().jpeg_amd_decompress_resized_mixed(*head, out_ptr, stride, infos, views)
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views[:n]], infos


def reference(ctx, torch, datas, regions, out_size, filter, spec=None, flips=None, cosited=False, color=J.RGB):
    """Today's route: every file into whole planes by the host decoder, the data-loader call's views, the mixed call.
    -> (the bytes of every image, the views)"""
    spectrals = [J.Spectral.decompress(ctx, d) for d in datas]
    views = np.stack([_crop_views(s.size, [r], out_size)[0] for s, r in zip(spectrals, regions)])
    name = "antialias" if filter == _lib.FILTER_ANTIALIAS else "bilinear"
    if spec is None:
        got = J.decode_resized_mixed(ctx, spectrals, views, out_size, color=color, cosite=cosited, filter=name)
    else:
        got = J.decode_tensors_mixed(ctx, spectrals, views, out_size, spec, flips=flips, color=color, cosite=cosited, filter=name)
    return [g.contiguous().view(-1).view(torch.uint8).cpu().numpy() for g in got], views


def compare(ctx, torch, datas, regions, out_size, filter, form, flips=None, cosited=0, color=RGB, whole=False, threads=3):
    """One file call into a sentinel-filled buffer with stride gaps and a tail against the reference -> the views."""
    spec = None if form == "bytes" else spec_of(form)
    elem = 1 if spec is None else (2 if spec.dtype == _lib.F16 else 4)
    n = len(datas)
    out = Out(ctx, torch, [3 * out_size[0] * out_size[1]] * n, elem=elem, gap=5, tail=7)
    st, views, infos = file_call(ctx, datas, regions, out_size, filter, out.ptr, out.stride, spec, flips, cosited, color, threads, whole)
    assert st == 0
    want, want_views = reference(ctx, torch, datas, regions, out_size, filter, spec, flips, bool(cosited), J.RGB if color == RGB else J.YCbCr)
    assert views == [tuple(v) for v in want_views.tolist()]
    for i, (g, w) in enumerate(zip(out.images(), want)):               # (images() checks the gaps and the tail)
        assert (g == w).all(), (i, FILES[i] if n == len(FILES) else n, views[i], int((g != w).sum()))
    for i, d in enumerate(datas):
        assert (infos[i].width, infos[i].height, infos[i].process) == (F.inspect(d).width, F.inspect(d).height, F.inspect(d).process)
    return views


@pytest.fixture(scope="module")
def files():
    return make_files(500)


# ---- 1. image by image the mixed call on whole planes -----------------------------------------------------------------------------

def test_the_case_holds_what_it_should(ctx, torch, files):
    datas, regions = files
    out = Out(ctx, torch, [3 * OUT[0] * OUT[1]] * len(datas))
    st, views, infos = file_call(ctx, datas, regions, OUT, _lib.FILTER_BILINEAR, out.ptr, out.stride)
    assert st == 0
    assert {v[0] for v in views} == {1, 2, 4, 8}                      # every denominator, as the call itself chose them
    layouts = {tuple((i.factor_x[c], i.factor_y[c]) for c in range(i.ncomponents)) for i in infos}
    assert {((1, 1),), ((1, 1),) * 3, ((2, 2), (1, 1), (1, 1)), ((2, 1), (1, 1), (1, 1)), ((1, 2), (1, 1), (1, 1)),
            ((3, 1), (1, 1), (1, 1))} <= layouts
    assert sum(i.process == 2 for i in infos) == 3 and sum(i.restart_interval > 0 for i in infos) >= 4
    sparse = [F.decode_sparse(d)[0] == 0 for d in datas]              # both transports are in the call
    assert sum(sparse) >= 10 and not all(sparse)
    assert any(not s and i.process != 2 for s, i in zip(sparse, infos))   # ... and a sequential file that is too dense
    whole = [r == (0, 0, i.width, i.height) for r, i in zip(regions, infos)]
    assert any(whole) and any(r[2:] == (1, 1) for r in regions)
    assert any(r[0] + r[2] == i.width and r[1] + r[3] == i.height and not w for r, i, w in zip(regions, infos, whole))


@pytest.mark.parametrize("filter", [_lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS], ids=["bilinear", "antialias"])
@pytest.mark.parametrize("form", ["f16-chw", "f32-hwc", "bytes"])
def test_every_image_equals_the_mixed_call_on_whole_planes(ctx, torch, files, form, filter):
    datas, regions = files
    flips = None if form == "bytes" else [i % 3 == 1 for i in range(len(datas))]
    compare(ctx, torch, datas, regions, OUT, filter, form, flips, color=RGB if form != "bytes" else YCC)


def test_whole_images_without_rectangles_and_without_helper_threads(ctx, torch, files):
    datas, _ = files
    regions = [(0, 0, F.inspect(d).width, F.inspect(d).height) for d in datas]
    compare(ctx, torch, datas, regions, OUT, _lib.FILTER_BILINEAR, "f16-chw", whole=True, threads=1)


def test_the_whole_call_cosited(ctx, torch, files):
    """Cosited, only the grey files keep the tile kernel; every three-plane file is expanded whole for the fallback."""
    datas, regions = files
    compare(ctx, torch, datas, regions, OUT, _lib.FILTER_BILINEAR, "f32-hwc", flips=[1] * len(datas), cosited=1)


# ---- 2. the oracle ---------------------------------------------------------------------------------------------------------------

def test_three_files_match_the_oracle(ctx, torch):
    """A target of the view's own size resamples nothing ("out_w == w and out_h == h give the source bytes"): the byte call
    then gives the decoded view, which the oracle has -- at denominator 1 for a grey and a 4:2:2 file of 40 x 24, at
    denominator 2 for a 4:2:0 file of 80 x 48."""
    made = [F.synthetic_file("y8", (40, 24), 71, restart=2), F.synthetic_file("420", (80, 48), 72), F.synthetic_file("422", (40, 24), 73)]
    datas = [d for d, _ in made]
    regions = [(0, 0, 40, 24), (0, 0, 80, 48), (0, 0, 40, 24)]
    for color, unpack in ((RGB, O.unpack_rgb8), (YCC, O.unpack_ycc8)):
        out = Out(ctx, torch, [3 * 40 * 24] * 3, gap=3, tail=3)
        st, views, _ = file_call(ctx, datas, regions, (40, 24), _lib.FILTER_BILINEAR, out.ptr, out.stride, color=color)
        assert st == 0 and [v[0] for v in views] == [1, 2, 1] and all(v[1:] == (0, 0, 40, 24) for v in views)
        for (data, L), got, (denom, *_r) in zip(made, out.images(), views):
            info, planes, quanta = F.decode_planes(data)
            factors = [(L.factor_x[p], L.factor_y[p]) for p in range(L.nplanes)]
            tables = [quanta[p] for p in range(L.nplanes)]
            size = (L.width, L.height)
            if denom == 1:
                _, rect = O.decode(planes, tables, factors, size, cosited=False, scale=(L.scale_x, L.scale_y))
            else:
                _, rect = S.interleaved_scaled(planes, tables, factors, size, denom, False, (L.scale_x, L.scale_y))
            assert (got == unpack(rect, L.nplanes).reshape(-1)).all(), (color, size)


# ---- 3. the plane buffer of the context: nothing outside the expanded windows is read -----------------------------------------------

def test_a_second_set_of_files_through_the_same_context(ctx, torch, files):
    datas, regions = files
    compare(ctx, torch, datas, regions, OUT, _lib.FILTER_BILINEAR, "f16-chw")
    other, other_regions = make_files(900, OTHER_RECTS)
    assert [d.size for d in other] != [d.size for d in datas] and other_regions != regions
    views = compare(ctx, torch, other, other_regions, OUT, _lib.FILTER_BILINEAR, "f16-chw")
    assert {v[0] for v in views} == {1, 2, 4, 8}


# ---- 4. two chunks -----------------------------------------------------------------------------------------------------------------

def test_thirty_three_files_are_two_chunks(ctx, torch):
    names = ["420", "y8", "444", "422", "440"]
    datas = [F.synthetic_file(names[i % 5], ((32, 32), (40, 28), (48, 40))[i % 3], 200 + i, restart=i % 4)[0] for i in range(33)]
    regions = [(i % 7, i % 5, 20 + i % 6, 18 + i % 4) for i in range(33)]                 # inside the smallest, 32 x 28
    assert sum(F.decode_sparse(d)[0] == 0 for d in datas) == 33         # the sparse transport, in both chunks
    compare(ctx, torch, datas, regions, (16, 16), _lib.FILTER_BILINEAR, "f16-chw", flips=[i % 2 for i in range(33)])
    compare(ctx, torch, datas, regions, (16, 16), _lib.FILTER_ANTIALIAS, "bytes", threads=1)


# ---- 5. refused calls, damaged files --------------------------------------------------------------------------------------------------

def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, torch, files):
    datas, regions = files
    n = len(datas)
    out = Out(ctx, torch, [3 * OUT[0] * OUT[1]] * n, elem=2, gap=2, tail=2)
    spec = spec_of("f16-chw")

    def call(d=datas, r=regions, out_size=OUT, filter=_lib.FILTER_BILINEAR, ptr=out.ptr, stride=out.stride, spec=spec):
        return file_call(ctx, d, r, out_size, filter, ptr, stride, spec)[0]

    twelve = F.synthetic_file("y8", (16, 16), 4, precision=12)[0]
    assert call(d=datas[:7] + [twelve] + datas[8:]) == _lib.ENOSUP
    assert call(r=regions[:5] + [(100, 60, 51, 30)] + regions[6:]) == _lib.EINVAL       # file 5 is 150 wide
    assert call(r=regions[:5] + [(0, 0, 0, 1)] + regions[6:]) == _lib.EINVAL
    assert call(d=datas[:3] + [np.zeros(100, np.uint8)] + datas[4:]) != 0
    assert call(out_size=(1, 1), filter=_lib.FILTER_ANTIALIAS) == _lib.ENOSUP            # 300 x 140 at 1/8 is 38 x 18
    assert call(filter=5) == _lib.EINVAL
    assert call(stride=3 * OUT[0] * OUT[1] - 1) == _lib.EINVAL
    assert call(ptr=out.ptr + 1) == _lib.EINVAL
    assert call(ptr=None) == _lib.EINVAL
    ctx.synchronize()
    assert out.untouched()
    assert call() == 0
    want, _ = reference(ctx, torch, datas, regions, OUT, _lib.FILTER_BILINEAR, spec)
    for i, (g, w) in enumerate(zip(out.images(), want)):
        assert (g == w).all(), i


def test_a_damaged_file_ends_the_call_and_the_context_stays_usable(ctx, torch, files):
    """A scan header that names Huffman tables the file does not define passes jpeg_amd_jpeg_inspect and fails in the entropy
    decoder: the call has started by then.  (A TRUNCATED entropy segment is no failure for the host decoder -- it decodes
    what is there and leaves the rest zero, status OK -- so for such a file the call's status is OK as well, and its image is
    the reference's for the same bytes.)"""
    datas, regions = files
    grey = datas[1].copy()
    sos = bytes(grey).index(b"\xff\xda")
    assert grey[sos + 4] == 1 and grey[sos + 6] == 0
    grey[sos + 6] = 0x11
    host = F.inspect(grey)
    planes = [np.zeros((host.units_y[0], host.units_x[0], 64), np.int16)]
    want = _lib.lib().jpeg_amd_jpeg_decode_spectral(grey.ctypes.data, grey.size, _lib.ptr_array([planes[0].ctypes.data]),
                                                    np.zeros((4, 64), np.uint16).ctypes.data, None)
    assert want == _lib.EINVAL
    out = Out(ctx, torch, [3 * OUT[0] * OUT[1]] * len(datas), elem=2)
    spec = spec_of("f16-chw")
    for threads in (1, 4):
        assert file_call(ctx, datas[:1] + [grey] + datas[2:], regions, OUT, _lib.FILTER_BILINEAR, out.ptr, out.stride, spec,
                         threads=threads)[0] == want
    cut = datas[0][:datas[0].size * 2 // 3].copy()
    compare(ctx, torch, [cut] + datas[1:], regions, OUT, _lib.FILTER_BILINEAR, "f16-chw")      # the next call, same context


# ---- 5b. the status of the call, fault by fault (files of 16 x 16 to 48 x 32) ---------------------------------------------------------
# Files of other sizes, block counts and subsamplings than file 0 are what the call is for (section 1).  What else a file may
# be, and what the call then returns: the first file that pass 0 (the headers) refuses decides, in front of every fault that
# only shows in the entropy decoder.
MIXED_FAULTS = {
    "null": _lib.EINVAL,                 # pass 0
    "twelve-bit": _lib.ENOSUP,           # pass 0
    "lossless": _lib.ENOSUP,             # pass 0: a frame header that jpeg_amd_jpeg_inspect refuses
    "undefined-tables": _lib.EINVAL,     # the entropy decoder, on a thread of the queue
    "progressive": 0,                    # decoded into planes, among files that travel sparse
}
SMALL = (16, 16)


@pytest.fixture(scope="module")
def small_files():
    shapes = [("420", (32, 32)), ("y8", (48, 32)), ("444", (16, 16)), ("422", (40, 28))]
    good = [F.synthetic_file(name, size, 600 + i, restart=i % 3)[0] for i, (name, size) in enumerate(shapes)]
    faults = {
        "null": None,
        "twelve-bit": F.synthetic_file("y8", (16, 16), 4, precision=12)[0],
        "lossless": F.lossless_marker(good[2]),
        "undefined-tables": F.undefined_tables(good[1]),
        "progressive": F.synthetic_file("420", (48, 32), 610, kind="progressive")[0],
    }
    return good, faults


def _status(ctx, torch, datas, threads):
    out = Out(ctx, torch, [3 * SMALL[0] * SMALL[1]] * len(datas), elem=2)
    return file_call(ctx, datas, None, SMALL, _lib.FILTER_BILINEAR, out.ptr, out.stride, spec_of("f16-chw"), threads=threads, whole=True)[0]


def _whole(datas):
    return [(0, 0, F.inspect(d).width, F.inspect(d).height) for d in datas]


@pytest.mark.parametrize("fault", sorted(MIXED_FAULTS))
def test_status_of_one_fault_behind_file_0(ctx, torch, small_files, fault):
    good, faults = small_files
    datas = [good[0], good[1], faults[fault], good[2], good[3]]
    for threads in (1, 3, 0):
        assert _status(ctx, torch, datas, threads) == MIXED_FAULTS[fault], (fault, threads)
        if MIXED_FAULTS[fault] == 0:
            compare(ctx, torch, datas, _whole(datas), SMALL, _lib.FILTER_BILINEAR, "f16-chw", whole=True, threads=threads)
    compare(ctx, torch, good, _whole(good), SMALL, _lib.FILTER_BILINEAR, "f16-chw", whole=True)      # the context after a refused call


@pytest.mark.parametrize("first, second, want", [
    ("null", "twelve-bit", _lib.EINVAL), ("twelve-bit", "null", _lib.ENOSUP),                  # pass 0: the first file decides
    ("undefined-tables", "lossless", _lib.ENOSUP), ("lossless", "undefined-tables", _lib.ENOSUP),   # pass 0 in front of the decoder
    ("undefined-tables", "null", _lib.EINVAL), ("undefined-tables", "undefined-tables", _lib.EINVAL),
    ("progressive", "twelve-bit", _lib.ENOSUP)])
def test_status_of_two_faults(ctx, torch, small_files, first, second, want):
    good, faults = small_files
    datas = [good[0], faults[first], good[1], faults[second], good[2]]
    for threads in (1, 3, 0):
        assert _status(ctx, torch, datas, threads) == want, (first, second, threads)


def test_a_fault_in_chunk_2_behind_a_progressive_file_in_chunk_1(ctx, torch, small_files):
    """70 files = three chunks: pinned slot 0 is used again and its record cursor reset; a progressive file (planes) in chunk 1,
    a file that fails in the entropy decoder in chunk 2; with 1, 2 and all threads.  Then the clean batch, image by image."""
    good, faults = small_files
    datas = [good[i % 4] for i in range(70)]
    datas[40] = faults["progressive"]
    bad = list(datas)
    bad[66] = faults["undefined-tables"]
    for threads in (1, 2, 0):
        assert _status(ctx, torch, bad, threads) == _lib.EINVAL, threads
    compare(ctx, torch, datas, _whole(datas), SMALL, _lib.FILTER_BILINEAR, "f16-chw", whole=True, threads=2)


# ---- 6. the empty call; the Python functions ------------------------------------------------------------------------------------------

def test_an_empty_call_is_ok(ctx, torch):
    out = torch.full((64,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    assert file_call(ctx, [], [], OUT, _lib.FILTER_BILINEAR, out.data_ptr(), 0, spec_of("f16-chw"))[0] == 0
    assert file_call(ctx, [], [], OUT, _lib.FILTER_BILINEAR, out.data_ptr(), 0)[0] == 0
    ctx.synchronize()
    assert (out == SENTINEL).all()


def test_python_api(ctx, torch, files, tmp_path):
    datas, regions = files
    spec = J.tensor_spec((0.485, 0.456, 0.406), (0.229, 0.224, 0.225), dtype=torch.float16, layout="chw")
    flips = [i % 2 for i in range(len(datas))]
    sources = [d.tobytes() for d in datas]
    path = tmp_path / "file0.jpg"
    path.write_bytes(sources[0])
    sources[0] = str(path)                                             # paths and bytes alike
    tensor, views, infos = J.decompress_tensors(ctx, sources, OUT, spec, source_regions=regions, flips=flips, filter="antialias", threads=2)
    assert tuple(tensor.shape) == (len(datas), 3, OUT[1], OUT[0]) and tensor.dtype == torch.float16
    assert views.dtype == np.int32 and views.shape == (len(datas), 5) and len(infos) == len(datas)
    out = Out(ctx, torch, [3 * OUT[0] * OUT[1]] * len(datas), elem=2)
    st, c_views, _ = file_call(ctx, datas, regions, OUT, _lib.FILTER_ANTIALIAS, out.ptr, out.stride, spec, flips)
    assert st == 0 and [tuple(v) for v in views.tolist()] == c_views
    got = tensor.contiguous().view(len(datas), -1).view(torch.uint8).cpu().numpy()
    for i, w in enumerate(out.images()):
        assert (got[i] == w).all(), i
    assert [(i.width, i.height) for i in infos] == [(F.inspect(d).width, F.inspect(d).height) for d in datas]
    resized = J.decompress_resized(ctx, sources, OUT, source_regions=regions, color=J.YCbCr)
    assert tuple(resized.shape) == (len(datas), OUT[1], OUT[0], 3) and resized.dtype == torch.uint8
    out = Out(ctx, torch, [3 * OUT[0] * OUT[1]] * len(datas))
    assert file_call(ctx, datas, regions, OUT, _lib.FILTER_BILINEAR, out.ptr, out.stride, color=YCC)[0] == 0
    for i, w in enumerate(out.images()):
        assert (resized[i].reshape(-1).cpu().numpy() == w).all(), i
    whole = J.decompress_resized(ctx, sources[:3], OUT)                # no rectangles: the whole images
    assert tuple(whole.shape) == (3, OUT[1], OUT[0], 3)
    with pytest.raises(J.JpegAmdError):
        J.decompress_resized(ctx, sources[:2], OUT, source_regions=[regions[0], (0, 0, 500, 500)])
    with pytest.raises(ValueError):
        J.decompress_resized(ctx, sources[:2], OUT, source_regions=regions[:1])


# ---- a call of two chunks carries every per-file array into its second chunk ---------------------------------------------------

@pytest.fixture(scope="module")
def files_33():
    """33 small files, one more than a chunk holds: 4:2:0 and grey in turn, none larger than 48 x 32."""
    sizes = [(48, 32), (31, 17), (16, 16), (9, 29), (40, 8)]
    return [F.synthetic_file("420" if i % 2 else "y8", sizes[i % len(sizes)], 900 + i)[0].tobytes() for i in range(33)]


@pytest.mark.parametrize("case", ["placed", "warped"])
def test_a_call_of_two_chunks_is_its_chunks_side_by_side(ctx, torch, files_33, case):
    """Orientations 1 .. 8 in turn, flips on the odd files and a colour per file, with (placed) a fitted window, the antialiasing
    filter and a float16 CHW tensor, or (warped) an affine map per file: the call on all 33 files is, bit for bit and in every
    per-file result it returns, the call on files [0, 32) and the call on file 32 alone."""
    n = len(files_33)
    rng = np.random.Generator(np.random.PCG64(33))
    colour = np.tile(np.eye(3, 4, dtype=np.float32), (n, 1, 1)) + rng.uniform(-0.2, 0.2, (n, 3, 4)).astype(np.float32)
    colour[:, :, 3] = rng.uniform(-20, 20, (n, 3))
    orient = [1 + i % 8 for i in range(n)]
    flips = [i % 2 for i in range(n)]
    if case == "placed":
        spec = spec_of("f16-chw")
        kw = dict(filter="antialias", place="fit", fill=(9, 8, 7))
    else:
        spec = spec_of("f32-hwc")
        angle = rng.uniform(-0.5, 0.5, n)
        zoom = rng.uniform(0.8, 1.6, n)
        warp = np.stack([zoom * np.cos(angle), -zoom * np.sin(angle), rng.uniform(-3, 3, n),
                         zoom * np.sin(angle), zoom * np.cos(angle), rng.uniform(-3, 3, n)], axis=1).astype(np.float32)
        kw = dict(edge="replicate")

    def call(lo, hi):
        more = dict(kw, warp=warp[lo:hi]) if case == "warped" else kw
        got = J.decompress_tensors(ctx, files_33[lo:hi], OUT, spec, flips=flips[lo:hi], orientation=orient[lo:hi],
                                   colour=colour[lo:hi], colour_clamp=(0.0, 255.0), threads=2, **more)
        tensor, views, infos, applied, last = got                       # (last: the windows, or the matrices applied)
        return tensor.contiguous().view(hi - lo, -1).view(torch.uint8).cpu().numpy(), views, applied, np.asarray(last)

    whole, head, tail = call(0, n), call(0, 32), call(32, n)
    for w, h, t in zip(whole, head, tail):
        assert w.shape[0] == n and (w == np.concatenate([h, t])).all()
    assert whole[2].tolist() == orient
    assert len({tuple(v) for v in whole[1].tolist()}) > 1 and whole[0].any()
