"""Every kernel of the resample family once, on the MI355X: 3 filters x {stored, oriented} records x {bytes, three dtypes in two
layouts} is the table that launch_resample picks a kernel from, and each case below reaches one cell of it through one call of
jpeg_amd_resize_oriented_batch or jpeg_amd_resize_oriented_tensor_batch (h_orient NULL: the stored records).  Expected values
are the numpy mirrors (_resize_ref, _antialias_ref, _bicubic_ref, _tensor_ref) applied to _orient's copy of each source, compared
exactly, as bit patterns; the bytes around the images are checked through _calls.Out."""
import ctypes as C
import functools

import pytest

import _antialias_ref as A
import _bicubic_ref as B
import _orient as E
import _resize_ref as R
import _tensor_ref as T
from _calls import Out, pixel_image
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _resample import c_bytes, c_spec, host_bits, pack, same
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

MIRROR = {_lib.FILTER_BILINEAR: R.resize, _lib.FILTER_ANTIALIAS: A.resize, _lib.FILTER_BICUBIC: B.resize}
FILTER_IDS = {_lib.FILTER_BILINEAR: "bilinear", _lib.FILTER_ANTIALIAS: "antialias", _lib.FILTER_BICUBIC: "bicubic"}
EXTENTS = [(150, 90), (61, 45), (97, 120)]                 # (w, h) as stored: factors 2.1, 0.87, 1.4 across and 2.4, 1.2, 3.2 down
OUT_W, OUT_H = 70, 37                                      # two tile columns and two tile rows, both partial
ORIENT = {"stored": None, "oriented": [1, 3, 6]}           # as stored, both flips, a transposing one: in one launch
FLIPS = [0, 1, 1]
MEAN, SCALE = (10.5, 100.25, 200.0), (0.5, -0.03125, 3.0)   # neither 0 nor 1
SINKS = [None] + [(d, l) for d in T.DTYPES for l in T.LAYOUTS]
SINK_IDS = ["bytes"] + ["%s-%s" % ({T.F32: "f32", T.F16: "f16", T.BF16: "bf16"}[d], {T.HWC: "hwc", T.CHW: "chw"}[l]) for d, l in SINKS[1:]]


def _sources():
    return [pixel_image("random", w, h, 1000 * w + h) for w, h in EXTENTS]


@functools.lru_cache(maxsize=None)
def _resampled(filter, records):
    """The byte images of the contract: computed once per filter and record kind, shared by the seven sinks, never written to."""
    orient = ORIENT[records] or [1] * len(EXTENTS)
    out = tuple(MIRROR[filter](E.orient(im, o), OUT_W, OUT_H) for im, o in zip(_sources(), orient))
    for o in out:
        o.setflags(write=False)
    return out


def test_the_three_filters_differ_on_these_sources():
    for records in ORIENT:
        u = {f: _resampled(f, records) for f in MIRROR}
        for i in range(len(EXTENTS)):
            assert (u[_lib.FILTER_BICUBIC][i] != u[_lib.FILTER_BILINEAR][i]).any() and (u[_lib.FILTER_BICUBIC][i] != u[_lib.FILTER_ANTIALIAS][i]).any()
        assert (u[_lib.FILTER_BILINEAR][0] != u[_lib.FILTER_ANTIALIAS][0]).any()
    for f in MIRROR:
        assert any((a != b).any() for a, b in zip(_resampled(f, "stored"), _resampled(f, "oriented")))
    assert all(max(w, h) / min(OUT_W, OUT_H) < 8 for w, h in EXTENTS)      # under the cubic's limit on either axis, transposed or not


@pytest.mark.parametrize("sink", SINKS, ids=SINK_IDS)
@pytest.mark.parametrize("records", list(ORIENT))
@pytest.mark.parametrize("filter", list(MIRROR), ids=list(FILTER_IDS.values()))
def test_every_cell_of_the_launch_table(ctx, torch, filter, records, sink):
    n = len(EXTENTS)
    d_src, stride, ext = pack(ctx, torch, _sources())
    head = (ctx.handle, n, d_src.data_ptr(), stride, ext, OUT_W, OUT_H, filter)
    want = _resampled(filter, records)
    if sink is None:
        out = Out(ctx, torch, [3 * OUT_W * OUT_H] * n, gap=5, lead=4, tail=7)
        assert _lib.lib().jpeg_amd_resize_oriented_batch(*head, c_bytes(ORIENT[records]), out.ptr, out.stride) == 0
        for i, g in enumerate(out.images()):
            same(g.reshape(OUT_H, OUT_W, 3), want[i], (FILTER_IDS[filter], records, "bytes", i))
        return
    spec = T.Spec(*sink, mean=MEAN, scale=SCALE)
    out = Out(ctx, torch, [3 * OUT_W * OUT_H] * n, elem=4 if spec.dtype == T.F32 else 2, gap=5, lead=4, tail=7)
    cs = c_spec(spec)
    assert _lib.lib().jpeg_amd_resize_oriented_tensor_batch(*head, C.byref(cs), c_bytes(FLIPS), c_bytes(ORIENT[records]), out.ptr,
                                                            out.stride) == 0
    shape = (3, OUT_H, OUT_W) if spec.layout == T.CHW else (OUT_H, OUT_W, 3)
    for i, g in enumerate(out.images()):
        same(host_bits(g, spec).reshape(shape), T.normalise(want[i], spec, FLIPS[i]), (FILTER_IDS[filter], records, sink, i))
