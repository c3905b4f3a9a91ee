"""Spectral reduce on the MI355X (jpeg_amd_spectral_reduce_batch, k_spectral_reduce): coefficient for coefficient the contract
of include/jpeg_amd.h ("spectral reduce") as _reduce_ref composes it from the scaled-decode reference and the oracle's fdct --
every layout kind at sizes that give a partial last block, N units not a multiple of 8, a one-block output and tile seams in
both axes -- the one launch against the staged route, other output tables, batches with stride gaps, unread coefficients, the
argument checks, and JPEG file to JPEG file."""
import ctypes as C
import os

import numpy as np
import pytest

import _golden as G
import _reduce_ref as R
import _scaled_ref as S
import _transform_ref as T
import jpeg_amd as J
from _calls import c_layout, plane_factors, plane_ptrs, plane_units
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _golden import GOLDEN
from jpeg_amd import _lib
from jpeg_amd.synth import natural_planes_torch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

DENOMS = (2, 4, 8)
FILL = 0x5A5A                                               # what every int16 of an output buffer holds before a call


def _reduce_layout(L, denom):
    out = _lib.Layout()
    assert _lib.lib().jpeg_amd_reduce_layout(C.byref(L), denom, C.byref(out)) == 0
    return out


def _synthetic(ctx, torch, L, n, seed, ntables=None):
    """Natural planes, a tenth of the blocks with DC = +-2000 (the clamp is hit on both sides), and n table sets."""
    planes = natural_planes_torch(plane_units(L), n, ctx.torch_device, seed=seed)
    gen = torch.Generator(device=ctx.torch_device).manual_seed(seed + 1)
    for p in planes:
        pick = torch.rand(p.shape[:3], generator=gen, device=ctx.torch_device)
        dc = torch.where(pick < 0.05, torch.full_like(p[..., 0], 2000), p[..., 0])
        p[..., 0] = torch.where(pick > 0.95, torch.full_like(dc, -2000), dc)
    ntables = ntables or max(L.qi[p] for p in range(L.nplanes)) + 1
    dq = torch.randint(1, 24, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen)
    return planes, dq, ntables


def _out_planes(ctx, torch, O_, n, gap=0):
    """Per plane one int16 buffer [n * (samples + gap) + gap] filled with FILL, and the strides."""
    strides = [64 * ux * uy + gap for ux, uy in plane_units(O_)]
    return [torch.full((n * s + gap,), FILL, dtype=torch.int16, device=ctx.torch_device) for s in strides], strides


def _batch(ctx, L, n, denom, in_ptrs, in_strides, dq, q_stride, ntables, dqo, out_ptrs, out_strides):
    return _lib.lib().jpeg_amd_spectral_reduce_batch(
        ctx.handle, C.byref(L), n, denom, _lib.ptr_array(in_ptrs), _lib.size_array(in_strides),
        dq.data_ptr() if dq is not None else None, q_stride, ntables, dqo.data_ptr() if dqo is not None else None,
        _lib.ptr_array(out_ptrs), _lib.size_array(out_strides))


def _reduce_batch(ctx, torch, L, n, planes, dq, ntables, denom, dqo=None):
    """-> per plane int16 numpy [n, uy', ux', 64]."""
    O_ = _reduce_layout(L, denom)
    outs, strides = _out_planes(ctx, torch, O_, n)
    assert _batch(ctx, L, n, denom, [p.data_ptr() for p in planes], [p[0].numel() for p in planes], dq, ntables * 64, ntables,
                  dqo, [o.data_ptr() for o in outs], strides) == 0
    return [o.cpu().numpy().reshape(n, uy, ux, 64) for o, (ux, uy) in zip(outs, plane_units(O_))]


def _reference(L, planes_host, q_host, i, denom, qo_host=None):
    """Image i of a batch through _reduce_ref: planes_host[p] [n, uy, ux, 64], q_host [n, ntables, 64]."""
    qi = [L.qi[p] for p in range(L.nplanes)]
    size, planes = R.reduce_image([pl[i] for pl in planes_host], [q_host[i, t] for t in qi], plane_factors(L), (L.scale_x, L.scale_y),
                                  (L.width, L.height), denom, None if qo_host is None else [qo_host[i, t] for t in qi], L.precision)
    return planes


# ---- every layout kind against the reference -----------------------------------------------------------------------------

LAYOUTS = {"y8": [(1, 1)], "444": [(1, 1)] * 3, "420": [(2, 2), (1, 1), (1, 1)], "422": [(2, 1), (1, 1), (1, 1)],
           "440": [(1, 2), (1, 1), (1, 1)], "411": [(4, 1), (1, 1), (1, 1)]}
# a partial last block, N units not a multiple of 8, a one-block output, tile seams in both axes (at every denominator:
# test_tile_seams_at_every_denominator)
SIZES = [(1, 1), (9, 15), (7, 65), (131, 257), (257, 131)]


def _check_against_reference(ctx, torch, L, seed, with_qout):
    n = 2
    planes, dq, ntables = _synthetic(ctx, torch, L, n, seed)
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    gen = torch.Generator(device=ctx.torch_device).manual_seed(seed + 2)
    dqo = torch.randint(1, 40, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen) if with_qout else None
    qoh = dqo.cpu().numpy().astype(np.uint16) if with_qout else None
    before = [p.clone() for p in planes]
    for denom in DENOMS:
        O_ = _reduce_layout(L, denom)
        got = _reduce_batch(ctx, torch, L, n, planes, dq, ntables, denom, dqo)
        for i in range(n):
            want = _reference(L, ph, qh, i, denom, qoh)
            for p in range(L.nplanes):
                assert want[p].shape == (O_.units_y[p], O_.units_x[p], 64)
                assert (got[p][i] == want[p]).all(), (denom, i, p)
    assert all(torch.equal(a, b) for a, b in zip(planes, before))


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_synthetic_batches_match_the_reference(ctx, torch, name, size):
    L = c_layout(size[0], size[1], LAYOUTS[name])
    _check_against_reference(ctx, torch, L, size[0] * 31 + size[1], with_qout=(size[0] + len(name)) % 2 == 0)


@pytest.mark.parametrize("name", ["y8", "420"])
def test_tile_seams_at_every_denominator(ctx, torch, name):
    """The kernel's tiles are 16 x 16 output blocks at denominators 2 and 4 and 8 x 8 at 8: 531 x 523 gives more than one
    tile in both axes at each of them (34 x 33, 17 x 17 and 9 x 9 luma blocks), with partial tiles at the far edges."""
    L = c_layout(531, 523, LAYOUTS[name])
    _check_against_reference(ctx, torch, L, 531, with_qout=False)


def test_a_factor_that_does_not_divide_the_scale(ctx, torch):
    """3 in 4 at width 85: the output has a block column with no source sample of its own, replicated whole."""
    L = c_layout(85, 15, [(4, 1), (3, 1), (1, 1)])
    sl = _lib.Layout()
    larger = False
    for denom in DENOMS:
        assert _lib.lib().jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(sl)) == 0
        larger |= _reduce_layout(L, denom).units_x[1] > sl.units_x[1]
    assert larger
    _check_against_reference(ctx, torch, L, 85, with_qout=False)


def test_the_12_bit_four_plane_layout(ctx, torch):
    """The layout of examples/custom-color: precision 12, four planes, a table per plane."""
    _, _, factors, _, _, m = G.custom_color()
    assert len(factors) == 4
    L = c_layout(131, 65, factors, precision=12, qi=[0, 1, 2, 3])
    _check_against_reference(ctx, torch, L, 12, with_qout=True)


# ---- the one launch against the staged route --------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [(9, 15), (131, 257)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_one_launch_equals_the_staged_route(ctx, torch, name, size):
    """jpeg_amd_spectral_idct_scaled planes -> jpeg_amd_planar_fdct under jpeg_amd_scaled_layout's layout (the factors divide
    the scale, so its units are the reduced layout's)."""
    lib = _lib.lib()
    L = c_layout(size[0], size[1], LAYOUTS[name])
    planes, dq, ntables = _synthetic(ctx, torch, L, 1, size[0] + 7 * size[1])
    one = [p[0] for p in planes]
    qh = np.ascontiguousarray(dq[0].cpu().numpy().astype(np.uint16))
    for denom in DENOMS:
        sl = _lib.Layout()
        assert lib.jpeg_amd_scaled_layout(C.byref(L), denom, C.byref(sl)) == 0
        O_ = _reduce_layout(L, denom)
        assert plane_units(sl) == plane_units(O_) and (sl.width, sl.height) == (O_.width, O_.height)
        samples = [torch.full((64 * ux * uy,), -1, dtype=torch.int16, device=ctx.torch_device) for ux, uy in plane_units(sl)]
        assert lib.jpeg_amd_spectral_idct_scaled(ctx.handle, C.byref(L), plane_ptrs(one), qh.ctypes.data, ntables, denom,
                                                 plane_ptrs(samples)) == 0
        staged = [torch.full((64 * ux * uy,), FILL, dtype=torch.int16, device=ctx.torch_device) for ux, uy in plane_units(sl)]
        assert lib.jpeg_amd_planar_fdct(ctx.handle, C.byref(sl), plane_ptrs(samples), qh.ctypes.data, ntables, plane_ptrs(staged)) == 0
        fused = [torch.full((64 * ux * uy,), FILL, dtype=torch.int16, device=ctx.torch_device) for ux, uy in plane_units(O_)]
        assert lib.jpeg_amd_spectral_reduce(ctx.handle, C.byref(L), denom, plane_ptrs(one), qh.ctypes.data, ntables, None,
                                            plane_ptrs(fused)) == 0
        for p in range(L.nplanes):
            assert torch.equal(staged[p], fused[p]), (name, size, denom, p)


# ---- output tables ------------------------------------------------------------------------------------------------------------

def test_other_output_tables_and_the_null_default(ctx, torch):
    """Luminance level 0.5 in, 2.0 out; NULL = the input tables."""
    lib = _lib.lib()
    L = c_layout(131, 257, LAYOUTS["420"], qi=[0, 0, 0])
    planes, _, _ = _synthetic(ctx, torch, L, 1, 5)
    one = [p[0] for p in planes]
    ph = [p.cpu().numpy() for p in planes]
    q_in = np.ascontiguousarray(O.compression_quanta("luminance", 0.5))
    q_out = np.ascontiguousarray(O.compression_quanta("luminance", 2.0))
    assert (q_in != q_out).any()
    for denom in DENOMS:
        O_ = _reduce_layout(L, denom)
        results = []
        for qo in (q_out, None):
            outs = [torch.full((64 * ux * uy,), FILL, dtype=torch.int16, device=ctx.torch_device) for ux, uy in plane_units(O_)]
            assert lib.jpeg_amd_spectral_reduce(ctx.handle, C.byref(L), denom, plane_ptrs(one), q_in.ctypes.data, 1,
                                                qo.ctypes.data if qo is not None else None, plane_ptrs(outs)) == 0
            want = _reference(L, ph, q_in[None, None, :], 0, denom, None if qo is None else qo[None, None, :])
            for p in range(3):
                assert (outs[p].cpu().numpy().reshape(want[p].shape) == want[p]).all(), (denom, qo is None, p)
            results.append(outs)
        assert not torch.equal(results[0][0], results[1][0])


# ---- batches --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["420", "411"])
def test_batch_of_64_with_stride_gaps_and_against_single_calls(ctx, torch, name):
    L = c_layout(33, 17, LAYOUTS[name])
    n, gap = 64, 48
    planes, dq, ntables = _synthetic(ctx, torch, L, n, 64)
    qh = np.ascontiguousarray(dq.cpu().numpy().astype(np.uint16))
    # the inputs at a stride with a gap as well
    in_strides = [p[0].numel() + gap for p in planes]
    spaced = []
    for p, s in zip(planes, in_strides):
        buf = torch.full((n, s), 12345, dtype=torch.int16, device=ctx.torch_device)
        buf[:, :p[0].numel()] = p.reshape(n, -1)
        spaced.append(buf)
    for denom in DENOMS:
        O_ = _reduce_layout(L, denom)
        outs, strides = _out_planes(ctx, torch, O_, n, gap=gap)
        # the outputs start `gap` elements into their buffers: a gap on both sides of every image
        assert _batch(ctx, L, n, denom, [b.data_ptr() for b in spaced], in_strides, dq, ntables * 64, ntables, None,
                      [o.data_ptr() + 2 * gap for o in outs], strides) == 0
        for p, (ux, uy) in enumerate(plane_units(O_)):
            m = 64 * ux * uy
            host = outs[p].cpu().numpy()
            assert (host[:gap] == FILL).all()
            body = host[gap:].reshape(n, strides[p])
            assert (body[:, m:] == FILL).all()
            assert (body[:, :m] != FILL).any()
        for i in range(n):
            single = [torch.full((64 * ux * uy,), FILL, dtype=torch.int16, device=ctx.torch_device) for ux, uy in plane_units(O_)]
            assert _lib.lib().jpeg_amd_spectral_reduce(ctx.handle, C.byref(L), denom, plane_ptrs([p[i] for p in planes]),
                                                       qh[i].ctypes.data, ntables, None, plane_ptrs(single)) == 0
            for p in range(L.nplanes):
                m = single[p].numel()
                assert torch.equal(single[p], outs[p][gap + i * strides[p]:gap + i * strides[p] + m]), (name, denom, i, p)


@pytest.mark.parametrize("name", ["y8", "420", "411"])
def test_unread_coefficients_do_not_matter(ctx, torch, name):
    L = c_layout(131, 65, LAYOUTS[name])
    planes, dq, ntables = _synthetic(ctx, torch, L, 2, 99)
    for denom in DENOMS:
        N = 8 // denom
        unread = torch.ones(64, dtype=torch.bool, device=ctx.torch_device)
        unread[torch.as_tensor(sorted(int(S.Z[h][k]) for h in range(N) for k in range(N)), device=ctx.torch_device)] = False
        zeroed, poisoned = [], []
        for p in planes:
            z = p.clone()
            z[..., unread] = 0
            r = torch.full_like(p, 32767)
            r[:, 1::2] = -32767
            r[:, :, 1::2] *= -1
            zeroed.append(z)
            poisoned.append(torch.where(unread, r, p).contiguous())
        a = _reduce_batch(ctx, torch, L, 2, zeroed, dq, ntables, denom)
        b = _reduce_batch(ctx, torch, L, 2, poisoned, dq, ntables, denom)
        assert all((x == y).all() for x, y in zip(a, b)), (name, denom)


def test_an_empty_batch_is_ok(ctx, torch):
    L = c_layout(33, 17, LAYOUTS["420"])
    assert _lib.lib().jpeg_amd_spectral_reduce_batch(ctx.handle, C.byref(L), 0, 2, None, None, None, 0, 2, None, None, None) == 0
    planes, dq, ntables = _synthetic(ctx, torch, L, 1, 4)
    outs, strides = _out_planes(ctx, torch, _reduce_layout(L, 2), 1)
    assert _batch(ctx, L, 0, 2, [p.data_ptr() for p in planes], [p[0].numel() for p in planes], dq, ntables * 64, ntables, None,
                  [o.data_ptr() for o in outs], strides) == 0
    ctx.synchronize()
    assert all((o == FILL).all() for o in outs)


def test_invalid_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    lib = _lib.lib()
    L = c_layout(33, 17, LAYOUTS["420"])
    n = 2
    planes, dq, ntables = _synthetic(ctx, torch, L, n, 3)
    qh = np.ascontiguousarray(dq.cpu().numpy().astype(np.uint16))
    O_ = _reduce_layout(L, 2)
    outs, strides = _out_planes(ctx, torch, O_, n)
    in_ptrs, in_strides = [p.data_ptr() for p in planes], [p[0].numel() for p in planes]
    out_ptrs = [o.data_ptr() for o in outs]

    def call(n_images=n, denom=2, ins=in_ptrs, outp=out_ptrs, q=dq, nt=ntables):
        return _batch(ctx, L, n_images, denom, ins, in_strides, q, ntables * 64, nt, None, outp, strides)

    for denom in (1, 0, 3, 16, -1):
        assert call(denom=denom) == _lib.EINVAL
    assert call(ins=[in_ptrs[0], None, in_ptrs[2]]) == _lib.EINVAL
    assert call(outp=[out_ptrs[0], out_ptrs[1], None]) == _lib.EINVAL
    assert call(q=None) == _lib.EINVAL
    assert call(nt=1) == _lib.EINVAL                     # plane 1 uses table 1
    assert call(n_images=65536) == _lib.EINVAL
    # every block on a 16-byte boundary: pointers multiples of 16 bytes, strides multiples of 8 elements
    assert call(ins=[in_ptrs[0] + 2, in_ptrs[1], in_ptrs[2]]) == _lib.EINVAL
    assert call(outp=[out_ptrs[0], out_ptrs[1] + 8, out_ptrs[2]]) == _lib.EINVAL
    assert _batch(ctx, L, n, 2, in_ptrs, in_strides, dq, ntables * 64, ntables, None, out_ptrs,
                  [strides[0] + 4, strides[1], strides[2]]) == _lib.EINVAL
    assert call(n_images=-1) == _lib.EINVAL

    def single(denom=2, q=qh[1], qo=None, ins=None):
        return lib.jpeg_amd_spectral_reduce(ctx.handle, C.byref(L), denom,
                                            _lib.ptr_array(ins or [p[1].data_ptr() for p in planes]), q.ctypes.data, ntables,
                                            qo.ctypes.data if qo is not None else None,
                                            _lib.ptr_array([o.data_ptr() + 2 * s for o, s in zip(outs, strides)]))

    zero_out = qh[1].copy()
    zero_out[1, 63] = 0
    assert single(qo=zero_out) == _lib.EINVAL
    assert single(q=zero_out) == _lib.EINVAL              # NULL output tables = the input's: the same zero divisor
    assert single(denom=1) == _lib.EINVAL
    assert single(ins=[planes[0][1].data_ptr(), None, planes[2][1].data_ptr()]) == _lib.EINVAL
    ctx.synchronize()
    assert all((o == FILL).all() for o in outs)
    # the context still works
    assert call() == 0
    assert single() == 0
    want = _reference(L, [p.cpu().numpy() for p in planes], qh, 1, 2)
    for p in range(3):
        assert (outs[p].cpu().numpy().reshape(n, *want[p].shape)[1] == want[p]).all()


# ---- file to file ---------------------------------------------------------------------------------------------------------------

def _reduce_file(ctx, data, denom, requant=None, sizing=False):
    n = C.c_size_t()
    info = _lib.FrameInfo()
    out = np.zeros(2 * data.size + (1 << 16), np.uint8)
    st = _lib.lib().jpeg_amd_reduce(ctx.handle, data.ctypes.data, data.size, denom,
                                    requant.ctypes.data if requant is not None else None, 2,
                                    None if sizing else out.ctypes.data, 0 if sizing else out.size, C.byref(n), C.byref(info))
    return st, out[:n.value].copy(), n.value, info


@pytest.mark.parametrize("denom", [2, 8])
@pytest.mark.parametrize("name", ["color-sequential-1.jpg", "color-progressive-1.jpg"])
def test_file_to_file(ctx, name, denom):
    """A baseline and a progressive fixture: geometry, process, ids, script, and the coefficients of the output file."""
    data = np.fromfile(os.path.join(GOLDEN, "decode", name), np.uint8)
    info, planes, quanta = T.decode_file(data)
    nc = info.ncomponents
    factors = [(info.factor_x[c], info.factor_y[c]) for c in range(nc)]
    st, scans, keys, meta = T.c_script(data)
    assert st == 0
    # a table per component; the two chroma components share a key
    assert keys[1] == keys[2] != keys[0]
    requant = np.ascontiguousarray(np.stack([O.compression_quanta("luminance", 2.0), O.compression_quanta("chrominance", 2.0),
                                             O.compression_quanta("chrominance", 2.0)]))
    for rq in (None, requant):
        st, out, nbytes, oinfo = _reduce_file(ctx, data, denom, rq)
        assert st == 0 and nbytes == out.size > 0
        assert _reduce_file(ctx, data, denom, rq, sizing=True)[2] == nbytes
        got = J.inspect(out.tobytes())
        size, want = R.reduce_image(planes, list(quanta), factors, (info.scale_x, info.scale_y), (info.width, info.height), denom,
                                    None if rq is None else list(rq))
        assert (got.width, got.height) == size == (oinfo.width, oinfo.height)
        assert (got.process, got.precision, got.ncomponents, got.restart_interval) == \
            (info.process, info.precision, nc, info.restart_interval)
        for c in range(nc):
            assert (got.id[c], got.factor_x[c], got.factor_y[c]) == (info.id[c], info.factor_x[c], info.factor_y[c])
            assert (got.units_x[c], got.units_y[c]) == (want[c].shape[1], want[c].shape[0]) == (oinfo.units_x[c], oinfo.units_y[c])
        st, oscans, okeys, ometa = T.c_script(out)
        assert st == 0 and oscans == scans and okeys == keys and ometa == meta
        _, oplanes, oquanta = T.decode_file(out)
        assert (oquanta == (quanta if rq is None else rq)).all()
        for c in range(nc):
            assert (oplanes[c] == want[c]).all(), (name, denom, rq is not None, c)
    # components of one key must get equal tables
    unequal = requant.copy()
    unequal[2, 5] += 1
    assert _reduce_file(ctx, data, denom, unequal)[0] == _lib.EINVAL
    assert _reduce_file(ctx, data, 1)[0] == _lib.EINVAL


# ---- the Python mirror ------------------------------------------------------------------------------------------------------------

def test_python_api(ctx, torch):
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 1)})
    size = (131, 65)
    L = c_layout(size[0], size[1], LAYOUTS["420"])
    planes, dq, ntables = _synthetic(ctx, torch, L, 1, 11)
    ph = [p.cpu().numpy() for p in planes]
    qh = dq.cpu().numpy().astype(np.uint16)
    sp = J.Spectral(ctx, size, layout, [p[0] for p in planes], [qh[0, 0], qh[0, 1]], [0, 1, 1])
    for denom in DENOMS:
        w, h = S.scaled_size(size, denom)
        assert J.reduce_layout(size, layout, denom) == R.reduce_geometry(size, LAYOUTS["420"], (2, 2), denom)
        small = sp.reduce(denom)
        assert small.size == (w, h) and small.q == sp.q
        want = _reference(L, ph, qh, 0, denom)
        for p in range(3):
            assert (small.planes[p].cpu().numpy() == want[p]).all()
        px = small.decode(J.RGB)
        assert tuple(px.shape) == (w * h, 3)
        rq = {0: O.compression_quanta("luminance", 2.0), 1: O.compression_quanta("chrominance", 2.0)}
        other = sp.reduce(denom, quanta=rq)
        qo = np.stack([rq[0], rq[1]])[None]
        want = _reference(L, ph, qh, 0, denom, qo)
        for p in range(3):
            assert (other.planes[p].cpu().numpy() == want[p]).all()
        assert all((a == b).all() for a, b in zip(other.quanta, [rq[0], rq[1]]))
    with pytest.raises(J.JpegAmdError):
        sp.reduce(1)
    data = np.fromfile(os.path.join(GOLDEN, "decode", "color-sequential-1.jpg"), np.uint8)
    out = J.reduce(data.tobytes(), 4, ctx=ctx)
    info = J.inspect(out)
    assert (info.width, info.height) == S.scaled_size((319, 480), 4)
