"""The host side of the oriented resample (include/jpeg_amd.h, "oriented resample") -- no GPU: jpeg_amd_jpeg_orientation on
APP1 segments built byte by byte (known answers, and every way a segment can be broken gives orientation 1 and OK),
jpeg_amd_orient_region against numpy on every small extent and rectangle, and what the six oriented calls refuse, and in
which order, with a NULL context in the manner of test_status_order_cpu.py."""
import ctypes as C
import io
import itertools
import struct

import numpy as np
import pytest

import _files as F
import _golden as G
import _orient as E
import jpeg_amd as J
from _calls import c_layout
from jpeg_amd import _lib

OK, EINVAL, ENOSUP = 0, -1, -5
BILINEAR, ANTIALIAS = _lib.FILTER_BILINEAR, _lib.FILTER_ANTIALIAS
RGB = _lib.COLOR_RGB8


def orientation(data, nbytes=None):
    data = np.ascontiguousarray(data, np.uint8)
    o = C.c_int32(-7)
    st = _lib.lib().jpeg_amd_jpeg_orientation(data.ctypes.data, data.size if nbytes is None else nbytes, C.byref(o))
    return st, o.value


@pytest.fixture(scope="module")
def plain():
    """A small sequential 4:2:0 file without any APPn segment."""
    return F.synthetic_file("420", (40, 24), 11)[0]


def pil_orientation(data):
    Image = pytest.importorskip("PIL.Image")
    return Image.open(io.BytesIO(bytes(data))).getexif().get(E.TAG, 1)


# ---- the parser: known answers -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("big", [False, True], ids=["II", "MM"])
@pytest.mark.parametrize("type", [E.SHORT, E.LONG], ids=["short", "long"])
def test_every_value_in_both_byte_orders_and_both_types(plain, big, type):
    assert orientation(plain) == (OK, 1)
    for value in range(1, 9):
        data = E.insert(plain, E.exif_segment(value, big, type))
        assert orientation(data) == (OK, value)
        assert J.exif_orientation(data) == value and J.exif_orientation(bytes(data)) == value
        assert F.inspect(data).width == 40                     # the file still decodes


@pytest.mark.parametrize("big", [False, True], ids=["II", "MM"])
def test_pil_agrees_on_the_well_formed_segments(plain, big):
    for value, type in itertools.product(range(1, 9), (E.SHORT, E.LONG)):
        data = E.insert(plain, E.exif_segment(value, big, type, before=2, after=0))
        assert pil_orientation(data) == value == orientation(data)[1]
    assert pil_orientation(plain) == 1


def test_where_the_tag_stands_in_the_directory(plain):
    for before, after in ((0, 0), (0, 3), (3, 0), (5, 2)):
        assert orientation(E.insert(plain, E.exif_segment(6, False, before=before, after=after))) == (OK, 6)
    absent = E.app1(b"Exif\0\0" + E.tiff([E.entry(0x010f, E.SHORT, 1, 6, True), E.entry(0x011a, E.LONG, 1, 8, True)], True))
    assert orientation(E.insert(plain, absent)) == (OK, 1)
    # an IFD0 that does not start right behind the header
    far = E.app1(b"Exif\0\0" + E.tiff([E.entry(E.TAG, E.SHORT, 1, 8, False)], False, ifd_offset=26))
    assert orientation(E.insert(plain, far)) == (OK, 8)


@pytest.mark.parametrize("big", [False, True], ids=["II", "MM"])
def test_values_types_and_counts_that_do_not_count(plain, big):
    for value in (0, 9, 65535):
        assert orientation(E.insert(plain, E.exif_segment(value, big))) == (OK, 1)
        assert orientation(E.insert(plain, E.exif_segment(value, big, E.LONG))) == (OK, 1)
    assert orientation(E.insert(plain, E.exif_segment(0x60000, big, E.LONG))) == (OK, 1)      # 6 in the other half of the LONG
    assert orientation(E.insert(plain, E.exif_segment(6, big, count=2))) == (OK, 1)
    assert orientation(E.insert(plain, E.exif_segment(6, big, count=0))) == (OK, 1)
    ascii = E.app1(b"Exif\0\0" + E.tiff([E.entry(E.TAG, E.ASCII, 1, 0, big, b"6\0\0\0")], big))
    assert orientation(E.insert(plain, ascii)) == (OK, 1)
    # a SHORT is read from the START of the value field, in the file's byte order: the other two bytes do not matter
    e = ">" if big else "<"
    short = E.app1(b"Exif\0\0" + E.tiff([E.entry(E.TAG, E.SHORT, 1, 0, big, struct.pack(e + "HH", 3, 0xffff))], big))
    assert orientation(E.insert(plain, short)) == (OK, 3)


def test_which_segment_is_read(plain):
    exif = E.exif_segment(5, True)
    assert orientation(E.insert(plain, E.XMP + exif)) == (OK, 5)              # an XMP APP1 in front
    assert orientation(E.insert(plain, exif + E.exif_segment(7))) == (OK, 5)   # the first Exif segment
    assert orientation(E.insert(plain, b"\xff\xe0\x00\x04ab" + b"\xff\xfe\x00\x03c" + exif)) == (OK, 5)
    assert orientation(E.insert_behind_sos(plain, exif)) == (OK, 1)           # behind the SOS: ignored
    assert orientation(E.insert(plain, E.app1(b"Exif\0" + b"x" * 30))) == (OK, 1)
    assert orientation(E.insert(plain, E.app1(b"Exif\0\0" + b"XX*\0" + b"\0" * 30))) == (OK, 1)
    assert orientation(E.insert(plain, E.app1(b"Exif\0\0II"))) == (OK, 1)      # no room for a TIFF header


@pytest.mark.parametrize("big", [False, True], ids=["II", "MM"])
def test_offsets_counts_and_lengths_that_leave_their_container(plain, big):
    one = [E.entry(E.TAG, E.SHORT, 1, 6, big)]
    body = E.tiff(one, big)
    assert orientation(E.insert(plain, E.app1(b"Exif\0\0" + body))) == (OK, 6)
    for off in (len(body) - 1, len(body), len(body) + 1, 0x7fffffff, 0xffffffff):    # the IFD offset past the segment
        assert orientation(E.insert(plain, E.app1(b"Exif\0\0" + E.tiff(one, big)[:4] + struct.pack((">" if big else "<") + "I", off)
                                                  + body[8:]))) == (OK, 1)
    for count in (2, 3, 0xffff):                                                     # an entry count that overruns it
        assert orientation(E.insert(plain, E.app1(b"Exif\0\0" + E.tiff(one, big, count=count)[:8 + 2 + 12]))) == (OK, 1)
    seg = E.exif_segment(6, big)
    for length in (len(seg) - 2 + 400000 // 8, 0xffff):                               # a segment length past the file
        data = E.insert(plain[:60], b"\xff\xe1" + struct.pack(">H", min(length, 0xffff)) + seg[4:])
        assert data.size < min(length, 0xffff) and orientation(data) == (OK, 1)
    assert orientation(E.insert(plain, b"\xff\xe1\x00\x01" + seg[4:])) == (OK, 1)    # a length below its own two bytes


def test_nbytes_cut_at_every_byte_of_the_segment(plain):
    """No byte at or beyond nbytes is read: the buffer handed over ends exactly at nbytes (a copy of that size), and the answer
    is 6 exactly from the byte on at which the whole segment lies inside."""
    seg = E.exif_segment(6, False, before=1, after=0)
    data = E.insert(plain, seg)
    end = 2 + len(seg)
    for n in range(0, end + 6):
        cut = data[:n].copy()
        st, o = orientation(cut) if n else orientation(np.zeros(1, np.uint8), 0)
        assert st == OK and o == (6 if n >= end else 1), n
    assert orientation(data, end) == (OK, 6) and orientation(data, end - 1) == (OK, 1)


def test_null_pointers_and_buffers_that_are_no_jpeg(plain):
    o = C.c_int32()
    assert _lib.lib().jpeg_amd_jpeg_orientation(None, 10, C.byref(o)) == EINVAL
    assert _lib.lib().jpeg_amd_jpeg_orientation(plain.ctypes.data, plain.size, None) == EINVAL
    rng = np.random.default_rng(5)
    for data in (np.zeros(64, np.uint8), rng.integers(0, 256, 500, dtype=np.uint8), np.frombuffer(b"\x89PNG\r\n\x1a\n" + b"\0" * 40, np.uint8),
                 np.frombuffer(E.exif_segment(6), np.uint8), np.frombuffer(b"\xff\xd8", np.uint8), np.full(300, 0xff, np.uint8)):
        assert orientation(data) == (OK, 1)


GOLDEN = {"decode/color-sequential-restart.jpg": True, "decode/color-progressive-restart.jpg": True, "decode/karlie-oscars-2017.jpg": True,
          "encode/karlie-2011.jpg.jpg": True, "decode/karlie-2019.jpg": False}


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_the_golden_files_that_carry_an_exif_segment(name):
    """The reference's own fixtures: four name orientation 1 in their Exif segment, one has a segment without the tag."""
    data = np.fromfile(G.path(name), np.uint8)
    raw = bytes(data)
    at = raw.index(b"Exif\0\0")
    assert raw[at - 4:at - 2] == b"\xff\xe1" and at < raw.index(b"\xff\xda")
    big = raw[at + 6:at + 8] == b"MM"
    tag = struct.pack(">H" if big else "<H", E.TAG)
    ifd = at + 6 + struct.unpack(">I" if big else "<I", raw[at + 10:at + 14])[0]
    count = struct.unpack(">H" if big else "<H", raw[ifd:ifd + 2])[0]
    assert (tag in [raw[ifd + 2 + 12 * i:ifd + 4 + 12 * i] for i in range(count)]) == GOLDEN[name]
    assert orientation(data) == (OK, 1)
    # ... and the same segment with its value replaced says what it is made to say
    if GOLDEN[name]:
        i = [raw[ifd + 2 + 12 * i:ifd + 4 + 12 * i] for i in range(count)].index(tag)
        changed = data.copy()
        changed[ifd + 2 + 12 * i + 8:ifd + 2 + 12 * i + 10] = np.frombuffer(struct.pack(">H" if big else "<H", 8), np.uint8)
        assert orientation(changed) == (OK, 8)


def test_pil_agrees_on_the_golden_files():
    for name in GOLDEN:
        data = np.fromfile(G.path(name), np.uint8)
        assert pil_orientation(data) == orientation(data)[1] == 1


# ---- the rectangle mapping, exhaustively ---------------------------------------------------------------------------------------

def region(o, w, h, rect):
    r = _lib.Region()
    st = _lib.lib().jpeg_amd_orient_region(o, w, h, None if rect is None else C.byref(_lib.Region(*rect)), C.byref(r))
    return st, (r.x, r.y, r.width, r.height)


def test_every_rectangle_of_every_small_extent():
    """The mask of the stored rectangle, oriented with numpy, is the mask of the oriented rectangle."""
    for o, w, h in itertools.product(range(1, 9), range(1, 7), range(1, 6)):
        ow, oh = E.oriented_size(o, w, h)
        assert region(o, w, h, None) == (OK, (0, 0, w, h))
        for x, y in itertools.product(range(ow), range(oh)):
            for rw, rh in itertools.product(range(1, ow - x + 1), range(1, oh - y + 1)):
                st, (sx, sy, sw, sh) = region(o, w, h, (x, y, rw, rh))
                assert st == OK and (sx, sy, sw, sh) == E.stored_rect(o, w, h, (x, y, rw, rh)) == J.orient_region(o, (w, h), (x, y, rw, rh))
                assert 0 <= sx and sx + sw <= w and 0 <= sy and sy + sh <= h
                stored = np.zeros((h, w), bool)
                stored[sy:sy + sh, sx:sx + sw] = True
                want = np.zeros((oh, ow), bool)
                want[y:y + rh, x:x + rw] = True
                assert (E.orient(stored, o) == want).all(), (o, w, h, x, y, rw, rh)


def test_rectangles_and_orientations_the_mapping_refuses():
    assert region(6, 6, 5, (0, 0, 5, 6))[0] == OK                     # the oriented image is 5 x 6
    for rect in ((0, 0, 6, 5), (0, 0, 6, 6), (1, 0, 5, 6), (0, 1, 5, 6), (-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, 0, 3), (0, 0, 3, 0),
                 (5, 0, 1, 1), (0, 6, 1, 1), (2**31 - 1, 0, 2, 1), (0, 0, -1, -1)):
        assert region(6, 6, 5, rect)[0] == EINVAL, rect
    for o in (0, 9, -1, 255):
        assert region(o, 6, 5, None)[0] == EINVAL
    assert region(1, 0, 5, None)[0] == EINVAL and region(1, 5, 0, None)[0] == EINVAL
    assert _lib.lib().jpeg_amd_orient_region(1, 6, 5, None, None) == EINVAL
    with pytest.raises(J.JpegAmdError):
        J.orient_region(9, (6, 5), None)


def test_numpy_orientation_is_exif_transpose():
    Image = pytest.importorskip("PIL.Image")
    ImageOps = pytest.importorskip("PIL.ImageOps")
    w, h = 6, 5
    labelled = (np.arange(h * w * 3) * 3 % 251).astype(np.uint8).reshape(h, w, 3)
    for o in range(1, 9):
        im = Image.fromarray(labelled)
        exif = im.getexif()
        exif[E.TAG] = o
        im.info["exif"] = exif.tobytes()
        buf = io.BytesIO()
        im.save(buf, "PNG", exif=exif.tobytes())
        upright = np.asarray(ImageOps.exif_transpose(Image.open(io.BytesIO(buf.getvalue()))))
        assert upright.shape == E.orient(labelled, o).shape and (upright == E.orient(labelled, o)).all(), o


# ---- refusals and their order, with a NULL context ---------------------------------------------------------------------------------
# A call that passes every check reaches the context, which is NULL: EINVAL.  So the verdict that shows how far a call came is
# the tap limit's ENOSUP, which is given last and before the context is looked at: an antialias call over the limit that is
# refused for anything else says EINVAL, one that is refused for nothing else says ENOSUP.

class Resize:
    def __init__(self, w=600, h=40, out=(32, 40)):
        self.buf = np.zeros(16, np.uint8)
        self.p = self.buf.ctypes.data
        self.extents = (_lib.Extent * 2)(_lib.Extent(w, h), _lib.Extent(w, h))
        self.spec = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
        self.out = out
        self.stride = 3 * w * h

    def bytes(self, orient, filter=ANTIALIAS, n=2, out=None):
        o = None if orient is None else (C.c_uint8 * 2)(*orient)
        ow, oh = out or self.out
        return _lib.lib().jpeg_amd_resize_oriented_batch(None, n, self.p, self.stride, self.extents, ow, oh, filter, o, self.p, 3 * 64 * 64)

    def tensor(self, orient, filter=ANTIALIAS, n=2, out=None, spec=True):
        o = None if orient is None else (C.c_uint8 * 2)(*orient)
        ow, oh = out or self.out
        return _lib.lib().jpeg_amd_resize_oriented_tensor_batch(None, n, self.p, self.stride, self.extents, ow, oh, filter,
                                                                C.byref(self.spec) if spec else None, None, o, self.p, 3 * 64 * 64)


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_resize_calls_judge_the_limit_last_and_on_the_oriented_factors(form):
    r = Resize()                                                       # 600 x 40 -> 32 x 40: kx = 18.75 as stored, 1.25 transposed
    call = getattr(r, form)
    assert call(None) == ENOSUP and call([1, 1]) == ENOSUP and call([2, 3]) == ENOSUP and call([1, 6]) == ENOSUP
    assert call([6, 5]) == EINVAL                                     # inside the limit: the call reaches the (NULL) context
    assert call([6, 8], out=(2, 40)) == ENOSUP                        # ky = 600 / 40 = 15 is inside, kx = 40 / 2 is not
    assert call(None, BILINEAR) == EINVAL and call([1, 6], BILINEAR) == EINVAL
    for bad in ([0, 1], [1, 9], [255, 1]):                             # a bad value in front of the limit, in either place
        assert call(bad) == EINVAL
    assert call([1, 9], n=1) == ENOSUP                                # ... and only of the call's own images
    assert call([1, 1], out=(0, 40)) == EINVAL and call([9, 1], out=(0, 40)) == EINVAL      # a bad target
    assert call([1, 1], filter=7) == EINVAL
    if form == "tensor":
        assert call([1, 1], spec=False) == EINVAL


def mixed_args(precisions=(8, 8), size=(600, 40)):
    buf = np.zeros(16, np.uint16)
    images = (_lib.Image * 2)()
    for i, precision in enumerate(precisions):
        images[i].layout = c_layout(size[0], size[1], [(1, 1)] * 3, precision=precision)
        for c in range(3):
            images[i].d_coef[c] = buf.ctypes.data
        images[i].d_quanta, images[i].ntables = buf.ctypes.data, 2
    views = (_lib.View * 2)(_lib.View(1, _lib.Region(0, 0, size[0], size[1])), _lib.View(1, _lib.Region(0, 0, size[0], size[1])))
    return buf, images, views


@pytest.mark.parametrize("form", ["bytes", "tensor"])
def test_the_mixed_calls_judge_an_orientation_with_its_image(form):
    spec = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))

    def call(orient, precisions=(8, 8), out=(32, 40), filter=ANTIALIAS, n=2):
        buf, images, views = mixed_args(precisions)
        o = None if orient is None else (C.c_uint8 * 2)(*orient)
        if form == "bytes":
            return _lib.lib().jpeg_amd_decode_resized_oriented_mixed(None, n, images, 0, RGB, views, out[0], out[1], filter, o, buf.ctypes.data,
                                                                     3 * 64 * 64)
        return _lib.lib().jpeg_amd_decode_tensor_oriented_mixed(None, n, images, 0, RGB, views, out[0], out[1], filter, C.byref(spec), None, o,
                                                                buf.ctypes.data, 3 * 64 * 64)

    assert call(None) == ENOSUP and call([1, 1]) == ENOSUP and call([4, 6]) == ENOSUP
    assert call([6, 7]) == EINVAL                                     # inside the limit: the (NULL) context
    assert call([0, 1]) == EINVAL and call([1, 9]) == EINVAL           # a bad value in front of the limit
    assert call([1, 9], (12, 8)) == ENOSUP                            # image 0's layout is judged in front of image 1's orientation
    assert call([9, 1], (8, 12)) == EINVAL                            # ... and image 0's orientation in front of image 1's layout
    assert call([9, 1], (12, 8)) == ENOSUP                            # ... and behind image 0's own layout
    assert call([6, 6], out=(0, 40)) == EINVAL
    assert call([9, 9], n=0) == OK and call(None, n=0) == OK           # an empty call judges no image


def test_the_calls_without_orientations_refuse_what_the_old_calls_refuse():
    """h_orient == NULL and an array of ones, against the *_filter_* calls, over argument sets that are wrong in one way each."""
    L = _lib.lib()
    spec = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
    ones = (C.c_uint8 * 2)(1, 1)
    r = Resize()
    seen = set()
    for n, out, filter, stride, src in itertools.product((2, 0, -1, 70000), ((32, 40), (0, 40), (32, 2**30 + 1), (600, 40)),
                                                         (BILINEAR, ANTIALIAS, 7), (r.stride, 5), (r.p, None)):
        old = L.jpeg_amd_resize_filter_batch(None, n, src, stride, r.extents, out[0], out[1], filter, r.p, 3 * 640 * 64)
        for o in (None, ones):
            assert L.jpeg_amd_resize_oriented_batch(None, n, src, stride, r.extents, out[0], out[1], filter, o, r.p, 3 * 640 * 64) == old
        old_t = L.jpeg_amd_resize_filter_tensor_batch(None, n, src, stride, r.extents, out[0], out[1], filter, C.byref(spec), None, r.p,
                                                      3 * 640 * 64)
        for o in (None, ones):
            assert L.jpeg_amd_resize_oriented_tensor_batch(None, n, src, stride, r.extents, out[0], out[1], filter, C.byref(spec), None, o,
                                                           r.p, 3 * 640 * 64) == old_t
        seen |= {old, old_t}
    for n, out, filter, precisions in itertools.product((2, 0, -1), ((32, 40), (0, 40), (600, 40)), (BILINEAR, ANTIALIAS, 7),
                                                        ((8, 8), (8, 12), (12, 8))):
        buf, images, views = mixed_args(precisions)
        old = L.jpeg_amd_decode_resized_filter_mixed(None, n, images, 0, RGB, views, out[0], out[1], filter, buf.ctypes.data, 3 * 640 * 64)
        old_t = L.jpeg_amd_decode_tensor_filter_mixed(None, n, images, 0, RGB, views, out[0], out[1], filter, C.byref(spec), None,
                                                      buf.ctypes.data, 3 * 640 * 64)
        for o in (None, ones):
            assert L.jpeg_amd_decode_resized_oriented_mixed(None, n, images, 0, RGB, views, out[0], out[1], filter, o, buf.ctypes.data,
                                                            3 * 640 * 64) == old
            assert L.jpeg_amd_decode_tensor_oriented_mixed(None, n, images, 0, RGB, views, out[0], out[1], filter, C.byref(spec), None, o,
                                                           buf.ctypes.data, 3 * 640 * 64) == old_t
        seen |= {old, old_t}
    assert seen == {OK, EINVAL, ENOSUP}


# ---- the file calls -----------------------------------------------------------------------------------------------------------------

def file_call(datas, orient, regions=None, out=(2, 2), filter=ANTIALIAS, tensor=False, oriented=True):
    """-> (status, the views written, the orientations written); -7 where nothing was written."""
    n = len(datas)
    ptrs = (C.c_void_p * n)(*[d.ctypes.data for d in datas])
    sizes = (C.c_size_t * n)(*[d.size for d in datas])
    regs = None if regions is None else (_lib.Region * n)(*[_lib.Region(*r) for r in regions])
    o = None if orient is None else (C.c_uint8 * n)(*orient)
    infos, views, applied = (_lib.FrameInfo * n)(), (_lib.View * n)(), (C.c_int32 * n)(*[-7] * n)
    for v in views:
        v.denom = -7
    buf = np.zeros(16, np.uint8)
    spec = _lib.TensorSpec(_lib.F32, _lib.TENSOR_HWC, (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1))
    head = (None, ptrs, sizes, n, 1, 0, RGB, regs, out[0], out[1], filter)
    if not oriented:
        st = (_lib.lib().jpeg_amd_decompress_tensor_mixed(*head, C.byref(spec), None, buf.ctypes.data, 12, infos, views) if tensor else
              _lib.lib().jpeg_amd_decompress_resized_mixed(*head, buf.ctypes.data, 12, infos, views))
    elif tensor:
        st = _lib.lib().jpeg_amd_decompress_tensor_oriented_mixed(*head, C.byref(spec), None, o, buf.ctypes.data, 12, infos, views, applied)
    else:
        st = _lib.lib().jpeg_amd_decompress_resized_oriented_mixed(*head, o, buf.ctypes.data, 12, infos, views, applied)
    return st, [(v.denom, v.region.x, v.region.y, v.region.width, v.region.height) for v in views], list(applied)


@pytest.fixture(scope="module")
def wide():
    """600 x 40: at out (2, 2) the view's denominator is 8 and kx = 75 / 2 is over the antialias limit."""
    return F.synthetic_file("444", (600, 40), 21)[0]


@pytest.mark.parametrize("tensor", [False, True], ids=["bytes", "tensor"])
def test_the_file_calls_resolve_and_judge_orientations_in_pass_0(wide, plain, tensor):
    tagged = E.insert(wide, E.exif_segment(6, True))
    # the limit, last: every call here passes everything else
    st, views, applied = file_call([wide, tagged], [0, 0], tensor=tensor)
    assert st == ENOSUP and applied == [1, 6] and [v[0] for v in views] == [8, 8]
    assert file_call([wide, tagged], None, tensor=tensor)[0] == ENOSUP
    assert file_call([wide, tagged], None, tensor=tensor)[2] == [1, 1]         # no orientations named: the images as stored
    assert file_call([tagged, tagged], [3, 0], tensor=tensor)[2] == [3, 6]     # a forced value overrides the tag
    # the limit is judged on the ORIENTED factors: 600 x 40 to 4 x 60 is kx = 150 stored and 10 = 40 / 4, 10 = 600 / 60 transposed
    assert file_call([tagged], [1], out=(4, 60), tensor=tensor)[0] == ENOSUP
    assert file_call([tagged], [0], out=(4, 60), tensor=tensor)[0] == EINVAL    # ... which reaches the (NULL) context
    # a value above 8: EINVAL, behind the file's own verdict
    assert file_call([wide, wide], [1, 9], tensor=tensor) == (EINVAL, [(8, 0, 0, 75, 5), (-7, 0, 0, 0, 0)], [1, -7])
    assert file_call([F.lossless_marker(wide)], [9], tensor=tensor)[0] == ENOSUP
    assert file_call([wide[:30]], [9], tensor=tensor)[0] == file_call([wide[:30]], None, tensor=tensor)[0] != OK
    # a broken EXIF block fails nothing: orientation 1
    broken = E.insert(wide, E.app1(b"Exif\0\0MM\0*\xff\xff\xff\xff"))
    assert file_call([broken], [0], tensor=tensor)[::2] == (ENOSUP, [1])


def test_source_rectangles_are_rectangles_of_the_oriented_image(wide):
    # oriented 40 x 600: a rectangle that fits the stored frame only is outside it
    assert file_call([wide], [6], [(0, 0, 600, 40)])[0] == EINVAL
    assert file_call([wide], [1], [(0, 0, 600, 40)])[0] == ENOSUP
    assert file_call([wide], [6], [(0, 0, 40, 600)])[0] == ENOSUP
    assert file_call([wide], None, [(0, 0, 40, 600)])[0] == EINVAL
    # the view reported is the STORED one: the oriented rectangle (8, 16, 16, 512) of orientation 6 is stored (16, 16, 512, 16)
    assert E.stored_rect(6, 600, 40, (8, 16, 16, 512)) == (16, 16, 512, 16)
    # and the denominator is chosen for the ORIENTED rectangle: 16 x 512 to 2 x 32 takes 8 (the stored 512 x 16 would take 1)
    st, views, applied = file_call([wide], [6], [(8, 16, 16, 512)], out=(2, 32), filter=BILINEAR)
    assert st == EINVAL and applied == [6]                            # (the context)
    assert views == [(8, 2, 2, 64, 2)]
    assert file_call([wide], [1], [(16, 16, 512, 16)], out=(2, 32), filter=BILINEAR)[1] == [(1, 16, 16, 512, 16)]


@pytest.mark.parametrize("o", range(1, 9))
def test_whole_images_choose_the_denominator_for_the_oriented_extent(wide, o):
    """h_source_regions == NULL is the whole ORIENTED image: the same views, statuses and orientations as naming that
    rectangle, for targets that are not square -- where the stored and the oriented extent choose different denominators."""
    ow, oh = E.oriented_size(o, 600, 40)
    for tensor in (False, True):
        for out in ((4, 60), (60, 4), (2, 32), (32, 2), (7, 7)):
            none = file_call([wide], [o], None, out=out, filter=BILINEAR, tensor=tensor)
            named = file_call([wide], [o], [(0, 0, ow, oh)], out=out, filter=BILINEAR, tensor=tensor)
            assert none == named and none[0] == EINVAL and none[2] == [o]          # (EINVAL: the NULL context, behind everything)
            denom = J.view_denom((ow, oh), out)
            assert none[1] == [(denom,) + J.view_of_source((600, 40), denom, (0, 0, 600, 40))], (o, out)
    # the known answers: 40 x 600 to 4 x 60 is an eighth; to 60 x 4 nothing smaller than the image itself will do
    if o >= 5:
        assert file_call([wide], [o], None, out=(4, 60), filter=BILINEAR)[1] == [(8, 0, 0, 75, 5)]
        assert file_call([wide], [o], None, out=(60, 4), filter=BILINEAR)[1] == [(1, 0, 0, 600, 40)]
    else:
        assert file_call([wide], [o], None, out=(60, 4), filter=BILINEAR)[1] == [(8, 0, 0, 75, 5)]
        assert file_call([wide], [o], None, out=(4, 60), filter=BILINEAR)[1] == [(1, 0, 0, 600, 40)]
