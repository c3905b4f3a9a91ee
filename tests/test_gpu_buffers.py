"""jpeg_amd_decode_batch and jpeg_amd_encode_batch -- k_quad420, k_luma_fused, k_encode_fused and the staged fallbacks of the same
entry points -- on pixel buffers that begin at any byte, with images any number of bytes apart and a guard around every image,
on the MI355X.  The launchers pick FAST (16-byte chunks that are whole or outside, no store_tail) and FASTIN (vector loads for
inner blocks) from the width, the base and the stride; tests/_buffers.py holds the table that brings every width class to every
placement, tests/test_buffers_cpu.py holds that table to its claims without a GPU.

Every comparison is exact: every byte against the oracle's decode + unpack, every coefficient against the
oracle's encode, every byte outside an image against its sentinel.  Three images per call, inputs from natural_planes_torch under
small tables (mostly unclamped: asserted), three distinct tables per image through four selector patterns, per-image and shared.
The coefficient planes keep 16-byte bases and strides (see _buffers.py) and have whole-block gaps.  A failing assertion names the
layout, shape, placement, colour and image, and the first differing byte's row, column, channel and chunk."""
import ctypes as C

import numpy as np
import pytest

import _buffers as B
from _calls import SENTINEL, Out, c_layout, plane_units
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from jpeg_amd import _lib
from jpeg_amd.synth import natural_planes_torch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

RGB, YCC = _lib.COLOR_RGB8, _lib.COLOR_YCC8
COLORS = {RGB: "rgb", YCC: "ycc"}
N = B.N_IMAGES
FUSED_PLACED = [(c, p) for c in B.CASES for p in B.PLACEMENTS]
STAGED_PLACED = [(c, p) for c in B.STAGED_CASES for p in B.STAGED_PLACEMENTS]
_placed_ids = lambda cases: ["%s-%s" % (B.case_id(c), B.placement_id(p)) for c, p in cases]
_case_ids = lambda cases: [B.case_id(c) for c in cases]


# ---- the inputs and the oracle's results: once per (layout, shape), read-only -------------------------------------------------------

class Inputs:
    def __init__(self, ctx, torch, c):
        self.case, self.L = c, c_layout(c.size[0], c.size[1], c.factors, qi=c.qi)
        self.units = plane_units(self.L)
        self.planes = [_frozen(p.cpu().numpy()) for p in natural_planes_torch(self.units, N, ctx.torch_device, seed=c.seed)]
        self.tables = _frozen(B.tables(c))
        self.d_tables = torch.from_numpy(self.tables.view(np.int16).copy()).to(ctx.torch_device)
        self.q_stride = 64 * B.NTABLES if c.per_image else 0
        self.pixels = {RGB: [], YCC: []}                      # [color][image]: uint8 [H * W, 3]
        for i in range(N):
            _, rect = O.decode([p[i] for p in self.planes], B.image_tables(c, self.tables, i), c.factors, c.size, cosited=bool(c.cosited))
            self.pixels[RGB].append(_frozen(O.unpack_rgb8(rect, len(c.factors))))
            self.pixels[YCC].append(_frozen(O.unpack_ycc8(rect, len(c.factors))))
        # the inputs' condition: a stray or a missing store must not hide behind a clamp
        for color, px in self.pixels.items():
            free = np.mean([((v > 0) & (v < 255)).mean() for v in px])
            assert free > 0.5, (B.case_id(c), COLORS[color], free)
        self._coefficients = {}

    def coefficients(self, color, i):
        """The oracle's encode of pixels[color][i] under the tables of image i."""
        if (color, i) not in self._coefficients:
            c, quanta = self.case, B.image_tables(self.case, self.tables, i)
            if color == RGB:
                want = O.encode(self.pixels[color][i], c.size, c.factors, quanta)
            else:
                scale = (max(f[0] for f in c.factors), max(f[1] for f in c.factors))
                rect = O.pack_ycc8(self.pixels[color][i], len(c.factors)).reshape(c.size[1], c.size[0], len(c.factors))
                want = [O.fdct_plane(p, t) for p, t in zip(O.decompose(rect, c.size, c.factors, scale), quanta)]
            self._coefficients[color, i] = [_frozen(w) for w in want]
        return self._coefficients[color, i]


def _frozen(a):
    a.setflags(write=False)
    return a


_inputs = {}


def inputs(ctx, torch, c):
    key = B.case_id(c)
    if key not in _inputs:
        _inputs[key] = Inputs(ctx, torch, c)
    return _inputs[key]


def _what(c, placement, color, *more):
    """One line (a tuple would be abbreviated in the report)."""
    return ", ".join(str(v) for v in (c.name, "%d x %d" % c.size, "lead %d and stride %% 16 == %d" % placement, COLORS[color]) + more)


class CoefIn:
    """The coefficient planes of the N images on the device, plane p with coef_gap_blocks(p) blocks of `filler` between the images,
    COEF_LEAD_BLOCKS in front of the first and one gap behind the last: bases and strides are whole blocks."""

    def __init__(self, ctx, torch, inp, filler=0):
        self.host, self.bufs, self.ptrs, self.strides = [], [], [], []
        for p, (plane, (ux, uy)) in enumerate(zip(inp.planes, inp.units)):
            blocks, gap = ux * uy, B.coef_gap_blocks(p)
            room = np.empty((N, blocks + gap, 64), np.int16)
            room[:, :blocks] = plane.reshape(N, blocks, 64)
            room[:, blocks:] = filler if np.isscalar(filler) else filler(room[:, blocks:].shape)
            lead = np.empty((B.COEF_LEAD_BLOCKS, 64), np.int16)
            lead[:] = room[0, blocks:][:1]
            host = np.concatenate([lead.reshape(-1), room.reshape(-1)])
            buf = torch.from_numpy(host).to(ctx.torch_device)
            assert buf.data_ptr() % 256 == 0
            self.host.append(host)
            self.bufs.append(buf)
            self.ptrs.append(buf.data_ptr() + 2 * 64 * B.COEF_LEAD_BLOCKS)
            self.strides.append(64 * (blocks + gap))
        assert all(ptr % 16 == 0 for ptr in self.ptrs) and all(s % 8 == 0 for s in self.strides)

    def unchanged(self):
        return all((b.cpu().numpy() == h).all() for b, h in zip(self.bufs, self.host))


def _extremes(shape):
    """+-32767, alternating: what a block read from a gap would bring."""
    return np.where(np.indices(shape).sum(0) & 1, 32767, -32767).astype(np.int16)


def decode(ctx, torch, inp, coef, placement, color, coef_strides=None, q_stride=None):
    """One jpeg_amd_decode_batch call into an Out placed by `placement` -> (Placed, the buffer's bytes on the host)."""
    c = inp.case
    p = B.place(3 * c.size[0] * c.size[1], *placement)
    out = Out(ctx, torch, [3 * c.size[0] * c.size[1]] * N, gap=p.gap, lead=p.lead, tail=p.tail)
    assert out.spans == p.spans and out.stride == p.stride and out.ptr % 16 == p.lead % 16
    strides = coef.strides if coef_strides is None else coef_strides
    status = _lib.lib().jpeg_amd_decode_batch(
        ctx.handle, C.byref(inp.L), N, _lib.ptr_array(coef.ptrs), _lib.size_array(strides + [0] * (4 - len(strides))), inp.d_tables.data_ptr(),
        inp.q_stride if q_stride is None else q_stride, B.NTABLES, c.cosited, color, out.ptr, out.stride)
    assert status == 0, _what(c, placement, color, "status", status)
    return p, out.buf.cpu().numpy()


def _images(host, p):
    return [host[a:a + m] for a, m in p.spans]


# ---- 1. decode into placed buffers ---------------------------------------------------------------------------------------------------

def _decode_into_placed(ctx, torch, c, placement):
    inp = inputs(ctx, torch, c)
    coef = CoefIn(ctx, torch, inp)
    for color in (RGB, YCC):
        p, host = decode(ctx, torch, inp, coef, placement, color)
        for i, got in enumerate(_images(host, p)):
            report = B.first_difference(got, inp.pixels[color][i], c.size)
            assert not report, _what(c, placement, color, "image", i, "at residue %d" % (p.spans[i][0] % 16), report)
        report = B.guard_report(host, p)
        assert not report, _what(c, placement, color, report)
        B.assert_guarded(host, p)


@pytest.mark.parametrize("c,placement", FUSED_PLACED, ids=_placed_ids(FUSED_PLACED))
def test_decode_into_placed_buffers(ctx, torch, c, placement):
    """Image i is the oracle's bytes exactly; the lead, the gaps and the tail keep their sentinel."""
    _decode_into_placed(ctx, torch, c, placement)


# ---- 2. decode is placement-independent ----------------------------------------------------------------------------------------------

def _decode_placement_independent(ctx, torch, c, placements):
    inp = inputs(ctx, torch, c)
    coef = CoefIn(ctx, torch, inp)
    for color in (RGB, YCC):
        p0, host0 = decode(ctx, torch, inp, coef, (0, 0), color)
        anchor = _images(host0, p0)
        for placement in placements:
            if placement == (0, 0):
                continue
            p, host = decode(ctx, torch, inp, coef, placement, color)
            for i, got in enumerate(_images(host, p)):
                report = B.first_difference(got, anchor[i], c.size)
                assert not report, _what(c, placement, color, "image", i, "against the aligned placement", report)


@pytest.mark.parametrize("c", B.CASES, ids=_case_ids(B.CASES))
def test_decode_is_placement_independent(ctx, torch, c):
    """The bytes from every placement are those from (0, 0): an anchor that does not pass through the oracle."""
    _decode_placement_independent(ctx, torch, c, B.PLACEMENTS)


# ---- 3. decode reads only its own coefficients ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,c", list(enumerate(B.CASES)), ids=_case_ids(B.CASES))
def test_decode_reads_only_its_own_coefficients(ctx, torch, k, c):
    """Whole-block gaps between the images' planes, filled with 0 in one run and with +-32767 in the other: the same pixels, planes
    and gaps unchanged; coef_stride = 0 gives N copies of image 0.  (The placement walks through the table with the case.)"""
    inp = inputs(ctx, torch, c)
    placement = B.PLACEMENTS[k % len(B.PLACEMENTS)]
    quiet, loud = CoefIn(ctx, torch, inp, 0), CoefIn(ctx, torch, inp, _extremes)
    assert all((h == 0).sum() < (g == 0).sum() for h, g in zip(loud.host, quiet.host))
    for color in (RGB, YCC):
        p, a = decode(ctx, torch, inp, quiet, placement, color)
        _, b = decode(ctx, torch, inp, loud, placement, color)
        for i, (ga, gb) in enumerate(zip(_images(a, p), _images(b, p))):
            report = B.first_difference(gb, ga, c.size)
            assert not report, _what(c, placement, color, "image", i, "gaps of +-32767 against gaps of 0", report)
            report = B.first_difference(ga, inp.pixels[color][i], c.size)
            assert not report, _what(c, placement, color, "image", i, report)
        B.assert_guarded(b, p)
        assert quiet.unchanged() and loud.unchanged(), _what(c, placement, color, "the call wrote to its coefficient planes")
        p, same = decode(ctx, torch, inp, loud, placement, color, coef_strides=[0] * len(loud.strides), q_stride=0)
        for i, got in enumerate(_images(same, p)):
            report = B.first_difference(got, inp.pixels[color][0], c.size)
            assert not report, _what(c, placement, color, "coef_stride 0, image", i, "against image 0", report)
        B.assert_guarded(same, p)


# ---- 4. encode from placed pixels ----------------------------------------------------------------------------------------------------

COEF_FILL = 0x5A5A


def _dense_planes(ctx, torch, inp):
    return [torch.full((N, 64 * ux * uy), COEF_FILL, dtype=torch.int16, device=ctx.torch_device) for ux, uy in inp.units]


def _encode(ctx, inp, px, p, color, ptrs, strides):
    status = _lib.lib().jpeg_amd_encode_batch(
        ctx.handle, C.byref(inp.L), N, px.data_ptr() + p.lead, p.stride, color, inp.d_tables.data_ptr(), inp.q_stride, B.NTABLES,
        _lib.ptr_array(ptrs), _lib.size_array(strides + [0] * (4 - len(strides))))
    assert status == 0, (B.case_id(inp.case), status)


def _encode_from_placed(ctx, torch, c, placement):
    inp = inputs(ctx, torch, c)
    p = B.place(3 * c.size[0] * c.size[1], *placement)
    for color in (RGB, YCC):
        runs = {}
        for fill in (0x00, 0xFF):
            host = B.placed_pixels(inp.pixels[color], p, fill)
            px = torch.from_numpy(host).to(ctx.torch_device)
            assert px.data_ptr() % 256 == 0 and (px.data_ptr() + p.lead) % 16 == p.lead % 16
            outs = _dense_planes(ctx, torch, inp)
            _encode(ctx, inp, px, p, color, [o.data_ptr() for o in outs], [o.shape[1] for o in outs])
            runs[fill] = [o.cpu().numpy() for o in outs]
            assert (px.cpu().numpy() == host).all(), _what(c, placement, color, "the call wrote to its pixels")
        for i in range(N):
            got = {fill: [o[i].reshape(uy, ux, 64) for o, (ux, uy) in zip(planes, inp.units)] for fill, planes in runs.items()}
            report = B.first_coefficient(got[0xFF], got[0x00])
            assert not report, _what(c, placement, color, "image", i, "0xFF around the images against 0x00", report)
            report = B.first_coefficient(got[0x00], inp.coefficients(color, i))
            assert not report, _what(c, placement, color, "image", i, "at residue %d" % (p.spans[i][0] % 16), report)


@pytest.mark.parametrize("c,placement", FUSED_PLACED, ids=_placed_ids(FUSED_PLACED))
def test_encode_from_placed_pixels(ctx, torch, c, placement):
    """The pixels are the oracle's decode; every byte outside them is 0x00 in one run and 0xFF in the other.  Both give the
    oracle's coefficients: the padding of a right or bottom edge block replicates the image's own last column or row, never
    what lies behind it.  The pixel buffer is unchanged."""
    _encode_from_placed(ctx, torch, c, placement)


# ---- 5. encode into guarded planes ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k,c", list(enumerate(B.CASES)), ids=_case_ids(B.CASES))
def test_encode_into_guarded_planes(ctx, torch, k, c):
    """One guarded buffer per plane, whole blocks of lead and gap (as test_gpu_frame_limit._coef_outs): the oracle's
    coefficients, and the sentinel in every element outside the planes."""
    inp = inputs(ctx, torch, c)
    placement = B.PLACEMENTS[(k + 3) % len(B.PLACEMENTS)]
    p = B.place(3 * c.size[0] * c.size[1], *placement)
    for color in (RGB, YCC):
        px = torch.from_numpy(B.placed_pixels(inp.pixels[color], p, SENTINEL)).to(ctx.torch_device)
        outs = [Out(ctx, torch, [64 * ux * uy] * N, elem=2, gap=64 * (q + 1), lead=64, tail=8) for q, (ux, uy) in enumerate(inp.units)]
        _encode(ctx, inp, px, p, color, [o.ptr for o in outs], [o.stride for o in outs])
        planes = [o.images() for o in outs]                  # asserts the sentinel outside the planes
        for i in range(N):
            got = [pl[i].view(np.int16).reshape(uy, ux, 64) for pl, (ux, uy) in zip(planes, inp.units)]
            report = B.first_coefficient(got, inp.coefficients(color, i))
            assert not report, _what(c, placement, color, "image", i, report)


# ---- 6. the staged fallbacks of the same entry points --------------------------------------------------------------------------------

@pytest.mark.parametrize("c,placement", STAGED_PLACED, ids=_placed_ids(STAGED_PLACED))
def test_staged_decode_into_placed_buffers(ctx, torch, c, placement):
    """4:1:1 and cosited 4:2:0 take staged_decode inside jpeg_amd_decode_batch."""
    _decode_into_placed(ctx, torch, c, placement)


@pytest.mark.parametrize("c", B.STAGED_CASES, ids=_case_ids(B.STAGED_CASES))
def test_staged_decode_is_placement_independent(ctx, torch, c):
    _decode_placement_independent(ctx, torch, c, B.STAGED_PLACEMENTS)


@pytest.mark.parametrize("c,placement", STAGED_PLACED, ids=_placed_ids(STAGED_PLACED))
def test_staged_encode_from_placed_pixels(ctx, torch, c, placement):
    """4:1:1 takes staged_encode inside jpeg_amd_encode_batch; the cosited decode's pixels go through k_encode_fused (the encoder
    has no cosited form)."""
    _encode_from_placed(ctx, torch, c, placement)
