"""Lossless spectral transforms on the MI355X (kernels_transform.hip): rotate, flip, crop, requantise.

Pins: the reference's own rotated files (examples/rotate: karlie-kwk-wwdc-2017-{ii,iii,iv}.jpg) and its requantised file
(examples/recompress/recompressed-requantized.jpg), the numpy restatement of examples/rotate/main.swift in _transform_ref,
and the float64 requantisation expression of examples/recompress/main.swift:52-56."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

import _transform_ref as R
import jpeg_amd as J
from _calls import ctx  # noqa: F401  (the fixture)
from _golden import GOLDEN
from jpeg_amd import _lib
from jpeg_amd.api import _metadata_array, _scan_array, Scan
from test_entropy_encode_cpu import _script, _sorted_dht

pytestmark = pytest.mark.gpu

SOURCE = R.xpath("karlie-kwk-wwdc-2017.jpg")
ROTATED = {"ii": 5, "iii": 6, "iv": 3}
CASES = (sorted(glob.glob(os.path.join(GOLDEN, "decode", "*.jpg"))) +
         [os.path.join(GOLDEN, "encode", f) for f in ("karlie-milan-sp12-2011-4-2-2-1.0.jpg",
                                                      "karlie-milan-sp12-2011-4-4-0-1.0.jpg", "custom-color-output.jpg")])


def _bytes(path):
    return np.fromfile(path, np.uint8)


def _decoded(data):
    info, planes, quanta = R.decode_file(data)
    return info, planes, quanta


@pytest.mark.parametrize("name", sorted(ROTATED))
def test_rotations_reproduce_the_references_files(ctx, name):
    out = J.transform(SOURCE, name, ctx=ctx)
    gold = _bytes(R.xpath(f"karlie-kwk-wwdc-2017-{name}.jpg")).tobytes()
    assert len(out) == len(gold)
    assert _sorted_dht(out) == _sorted_dht(gold)
    info_a, planes_a, q_a = _decoded(np.frombuffer(out, np.uint8))
    info_b, planes_b, q_b = _decoded(np.frombuffer(gold, np.uint8))
    assert (info_a.width, info_a.height) == (info_b.width, info_b.height)
    for a, b in zip(planes_a, planes_b):
        assert a.shape == b.shape and (a == b).all()
    assert (q_a == q_b).all()


def _encode_with_script(info, planes, tables_by_component, data):
    """jpeg_amd_jpeg_encode_spectral with the script (scans, keys, metadata) of `data`."""
    process, metadata, scans, keys, tkeys, _ = _script(data)
    tables = np.stack([tables_by_component[keys.index(k)] for k in tkeys]).astype(np.uint16)
    qkey = (C.c_int32 * len(keys))(*keys)
    tk = (C.c_int32 * len(tkeys))(*tkeys)
    sarr = _scan_array(scans)
    marr, nmeta, _keep = _metadata_array(metadata)
    n = C.c_size_t()
    args = [C.byref(info), qkey, _lib.ptr_array([p.ctypes.data for p in planes]), tables.ctypes.data, tk, len(tkeys),
            sarr, len(scans), marr, nmeta]
    assert _lib.lib().jpeg_amd_jpeg_encode_spectral(*args, None, 0, C.byref(n)) == 0
    out = np.empty(n.value, np.uint8)
    assert _lib.lib().jpeg_amd_jpeg_encode_spectral(*args, out.ctypes.data, out.size, C.byref(n)) == 0
    return out.tobytes()


def test_requantisation_reproduces_the_references_coefficients(ctx):
    src = _bytes(R.xpath("original.jpg"))
    info, planes, quanta = _decoded(src)
    # examples/recompress/main.swift:36-39: DC kept, AC min(3 q, 255)
    req = [np.concatenate([q[:1], np.minimum(q[1:].astype(np.int64) * 3, 255)]).astype(np.uint16) for q in quanta]
    out = J.transform(src, "none", requantize=req, ctx=ctx)
    gold = _bytes(os.path.join(GOLDEN, "encode", "recompressed-requantized.jpg"))
    ginfo, gplanes, gq = _decoded(gold)
    oinfo, oplanes, oq = _decoded(np.frombuffer(out, np.uint8))
    for a, b in zip(oplanes, gplanes):
        assert a.shape == b.shape and (a == b).all()
    assert (oq == gq).all()
    # written with the gold's own scan script, keys and metadata, the planes give the gold back (up to DHT order)
    again = _encode_with_script(ginfo, oplanes, oq, gold)
    assert len(again) == gold.size
    assert _sorted_dht(again) == _sorted_dht(gold.tobytes())
    # the device-to-device form gives the same planes
    sp = J.Spectral.decompress(ctx, src)
    rq = sp.transform("none", requantize={c.qi: req[p] for p, c in enumerate(sp.layout.planes)})
    for a, b in zip(rq.host_planes(), gplanes):
        assert (a == b).all()


def _ref_planes(planes, quanta, info, op, region):
    factors = [(info.factor_x[c], info.factor_y[c]) for c in range(info.ncomponents)]
    ow, oh, ofac, units, cropped, origin = R.layout_ref(info.width, info.height, factors, op, region)
    m, _ = R.mapping_arrays(op)
    out = [R.transform_plane(p, op, cropped[c], origin[c]) for c, p in enumerate(planes)]
    return (ow, oh), ofac, out, [q[m] for q in quanta]


@pytest.mark.parametrize("path", CASES, ids=os.path.basename)
def test_every_op_against_the_numpy_restatement(ctx, path):
    data = _bytes(path)
    info, planes, quanta = _decoded(data)
    _, scans0, keys0, meta0 = R.c_script(data)
    sx, sy = info.scale_x, info.scale_y
    region = (8 * sx, 8 * sy, max(info.width - 8 * sx - 5, 1), max(info.height // 2, 1))
    sp = J.Spectral.decompress(ctx, data)
    for op in range(8):
        for reg in (None, region):
            size, ofac, want, wq = _ref_planes(planes, quanta, info, op, reg)
            # device to device
            t = sp.transform(op, reg)
            assert t.size == size
            assert [c.factor for c in t.layout.planes] == ofac
            for a, b in zip(t.host_planes(), want):
                assert a.shape == b.shape and (a.astype(np.int64) == b).all(), (op, reg)
            for p in range(len(planes)):
                assert (t.quanta[t.q[p]] == wq[p]).all()
            # file to file
            out = J.transform(data, op, reg, ctx=ctx)
            oinfo, oplanes, oq = _decoded(np.frombuffer(out, np.uint8))
            assert (oinfo.width, oinfo.height) == size
            assert oinfo.process == info.process and oinfo.nscans == info.nscans
            assert [(oinfo.factor_x[c], oinfo.factor_y[c]) for c in range(oinfo.ncomponents)] == ofac
            for a, b in zip(oplanes, want):
                assert a.shape == b.shape and (a.astype(np.int64) == b).all(), (op, reg)
            assert (oq == np.stack(wq)).all()
            _, scans1, keys1, meta1 = R.c_script(np.frombuffer(out, np.uint8))
            assert scans1 == scans0 and keys1 == keys0 and meta1 == meta0


def _synthetic(ctx, size, factors, seed):
    rng = np.random.default_rng(seed)
    layout = J.Layout("ycc8", {k + 1: J.Component(f, min(k, 1)) for k, f in enumerate(factors)})
    units = layout.units(size)
    planes = [rng.integers(-2000, 2000, (uy, ux, 64)).astype(np.int16) for ux, uy in units]
    quanta = [rng.integers(1, 255, 64).astype(np.uint16) for _ in range(2)]
    return J.Spectral.from_host(ctx, size, layout, planes, quanta)


def _same(a, b):
    assert a.size == b.size
    assert all((x == y).all() for x, y in zip(a.host_planes(), b.host_planes()))
    assert all((a.quanta[a.q[p]] == b.quanta[b.q[p]]).all() for p in range(a.layout.count))


@pytest.mark.parametrize("factors", [[(2, 2), (1, 1), (1, 1)], [(2, 1), (1, 1), (1, 1)], [(1, 1)] * 3])
def test_group_identities(ctx, factors):
    sp = _synthetic(ctx, (256, 128), factors, 3)
    r = sp
    for _ in range(4):
        r = r.transform("rot_ccw")
    _same(r, sp)
    _same(sp.transform("rot_ccw").transform("rot_cw"), sp)
    _same(sp.transform("transpose").transform("transpose"), sp)
    _same(sp.transform("flip_v").transform("flip_h"), sp.transform("rot_180"))
    _same(sp.transform("transverse").transform("transverse"), sp)


def test_batch_equals_single_calls(ctx):
    import torch
    lib = _lib.lib()
    size, factors = (200, 136), [(2, 2), (1, 1), (1, 1)]
    L = R.c_layout(*size, factors)
    L.qi[2] = 1
    op, region = 5, (16, 16, 150, 100)
    st, out = R.c_transform_layout(L, op, region)
    assert st == 0
    rng = np.random.default_rng(11)
    n = 3
    in_units = [(L.units_x[p], L.units_y[p]) for p in range(3)]
    out_units = [(out.units_x[p], out.units_y[p]) for p in range(3)]
    pad_in, pad_out = [64 * 5, 64 * 17, 64 * 2], [64 * 3, 64, 64 * 9]
    in_stride = [64 * ux * uy + pad_in[p] for p, (ux, uy) in enumerate(in_units)]
    out_stride = [64 * ux * uy + pad_out[p] for p, (ux, uy) in enumerate(out_units)]
    host = [rng.integers(-300, 300, n * s).astype(np.int16) for s in in_stride]
    d_in = [ctx.upload(h) for h in host]
    sentinel = -23131                                             # 0xA5A5: the kernel writes zero blocks by design
    d_out = [torch.full((n * s,), sentinel, dtype=torch.int16, device=ctx.torch_device) for s in out_stride]
    q_in = rng.integers(1, 100, (n, 2, 64)).astype(np.uint16)
    q_out = rng.integers(1, 200, (n, 2, 64)).astype(np.uint16)
    d_q, d_qo = ctx.upload(q_in), ctx.upload(q_out)
    flag = torch.zeros(1, dtype=torch.int32, device=ctx.torch_device)
    reg = _lib.Region(*region)
    assert lib.jpeg_amd_spectral_transform_batch(
        ctx.handle, C.byref(L), n, op, C.byref(reg), _lib.ptr_array([t.data_ptr() for t in d_in]), _lib.size_array(in_stride),
        d_q.data_ptr(), 128, 2, d_qo.data_ptr(), _lib.ptr_array([t.data_ptr() for t in d_out]), _lib.size_array(out_stride),
        flag.data_ptr()) == 0
    ctx.synchronize()
    assert int(flag.item()) == 0
    batch = [t.cpu().numpy() for t in d_out]
    for i in range(n):
        singles = [torch.zeros(64 * ux * uy, dtype=torch.int16, device=ctx.torch_device) for ux, uy in out_units]
        ins = [d_in[p][i * in_stride[p]:] for p in range(3)]
        assert lib.jpeg_amd_spectral_transform(
            ctx.handle, C.byref(L), op, C.byref(reg), _lib.ptr_array([t.data_ptr() for t in ins]),
            q_in[i].ctypes.data, 2, q_out[i].ctypes.data, _lib.ptr_array([t.data_ptr() for t in singles])) == 0
        for p, (ux, uy) in enumerate(out_units):
            got = batch[p][i * out_stride[p]:i * out_stride[p] + 64 * ux * uy]
            assert (got == singles[p].cpu().numpy()).all()
            # and the numpy restatement
            plane = host[p][i * in_stride[p]:i * in_stride[p] + 64 * in_units[p][0] * in_units[p][1]].reshape(
                in_units[p][1], in_units[p][0], 64)
            _, _, _, _, cropped, origin = R.layout_ref(*size, factors, op, region)
            t = R.transform_plane(plane, op, cropped[p], origin[p])
            m, _ = R.mapping_arrays(op)
            want, trapped = R.requantize_ref(t, q_in[i, L.qi[p]][m], q_out[i, L.qi[p]])
            assert not trapped
            assert (got.reshape(want.shape) == want).all()
        # the padding between images is left alone
        for p, (ux, uy) in enumerate(out_units):
            assert (batch[p][i * out_stride[p] + 64 * ux * uy:(i + 1) * out_stride[p]] == sentinel).all()


@pytest.mark.parametrize("name,k", [("rot_ccw", 1), ("rot_180", 2), ("rot_cw", 3)])
def test_orientation_in_pixel_space(ctx, name, k):
    sp = J.Spectral.decompress(ctx, SOURCE)
    full = sp.rectangular().host_values().astype(np.int32)            # [H, W, 3]
    t = sp.transform(name)
    W, H = sp.size
    sx, sy = sp.layout.scale
    op = _lib.XFORM[name]
    w = W - W % (8 * sx) if op in (5, 6) else W
    h = H - H % (8 * sy) if op in (3, 6) else H
    want = np.rot90(full[:h, :w], k=k, axes=(0, 1))
    got = t.rectangular().host_values().astype(np.int32)
    assert got.shape == want.shape
    d = np.abs(got - want)
    assert d.max() <= 2
    assert (d != 0).mean() < 1e-3


def _rounding_ref(v, q):
    r = v.astype(np.float64) / q.astype(np.float64)
    return np.trunc(r + 0.3 * np.where(r < 0, -1.0, 1.0)).astype(np.int64)


def _requant_batch(ctx, plane, q_out_tables):
    """op NONE, q_in = 1, image i requantised with q_out_tables[i] (the input plane shared: stride 0)."""
    import torch
    lib = _lib.lib()
    nblocks = plane.shape[0]
    L = R.c_layout(8, 8 * nblocks, [(1, 1)])
    n = len(q_out_tables)
    d_in = ctx.upload(plane.reshape(-1))
    d_out = torch.empty(n * nblocks * 64, dtype=torch.int16, device=ctx.torch_device)
    d_q = ctx.upload(np.ones((n, 64), np.uint16))
    d_qo = ctx.upload(np.stack(q_out_tables).astype(np.uint16))
    flag = torch.zeros(1, dtype=torch.int32, device=ctx.torch_device)
    assert lib.jpeg_amd_spectral_transform_batch(
        ctx.handle, C.byref(L), n, 0, None, _lib.ptr_array([d_in.data_ptr()]), _lib.size_array([0]), d_q.data_ptr(), 64, 1,
        d_qo.data_ptr(), _lib.ptr_array([d_out.data_ptr()]), _lib.size_array([nblocks * 64]), flag.data_ptr()) == 0
    ctx.synchronize()
    assert int(flag.item()) == 0
    return d_out.cpu().numpy().reshape(n, nblocks, 64)


def test_requantisation_rounding_exhaustive_over_8_bit_tables(ctx):
    v = np.arange(-32768, 32768, dtype=np.int64)
    plane = v.astype(np.int16).reshape(1024, 64)
    qs = np.arange(1, 256)
    out = _requant_batch(ctx, plane, [np.full(64, q, np.uint16) for q in qs])
    for i, q in enumerate(qs):
        assert (out[i].reshape(-1) == _rounding_ref(v, np.int64(q))).all(), q


def test_requantisation_rounding_sampled_16_bit_tables(ctx):
    rng = np.random.default_rng(5)
    v = np.arange(-32768, 32768, dtype=np.int64)
    plane = np.repeat(v.astype(np.int16)[:, None], 64, axis=1)       # every coefficient of block b is v[b]
    for chunk in range(4):
        tables = [rng.integers(1, 65536, 64).astype(np.uint16) for _ in range(16)]
        out = _requant_batch(ctx, plane, tables)
        for i, t in enumerate(tables):
            assert (out[i] == _rounding_ref(v[:, None], t[None, :].astype(np.int64))).all()


def test_requantisation_traps_are_einval(ctx):
    import torch
    lib = _lib.lib()
    L = R.c_layout(16, 8, [(1, 1)])
    plane = np.zeros((1, 2, 64), np.int16)
    plane[0, 1, 5] = 20000
    d_in = ctx.upload(plane.reshape(-1))
    d_out = torch.zeros(128, dtype=torch.int16, device=ctx.torch_device)

    def run(q_in, q_out, op=0, data=d_in):
        return lib.jpeg_amd_spectral_transform(ctx.handle, C.byref(L), op, None, _lib.ptr_array([data.data_ptr()]),
                                               np.ascontiguousarray(q_in, np.uint16).ctypes.data, 1,
                                               None if q_out is None else np.ascontiguousarray(q_out, np.uint16).ctypes.data,
                                               _lib.ptr_array([d_out.data_ptr()]))
    ones = np.ones(64, np.uint16)
    assert run(ones, ones) == 0
    assert run(np.full(64, 2, np.uint16), ones) == _lib.EINVAL             # 2 * 20000 overflows Int16
    zero_out = ones.copy(); zero_out[7] = 0
    assert run(ones, zero_out) == _lib.EINVAL                               # q_out = 0
    big = ones.copy(); big[0] = 40000
    assert run(big, ones) == _lib.EINVAL                                    # Int16(q_in) traps
    assert run(big, None) == 0                                              # without requantisation tables are not read
    # a negated Int16.min traps in the example's `* multiplier`, with or without requantisation
    m = np.zeros((1, 2, 64), np.int16); m[0, 0, 1] = -32768                 # zigzag 1 = (k 1, h 0): FLIP_H negates it
    d_m = ctx.upload(m.reshape(-1))
    assert run(ones, None, op=2, data=d_m) == _lib.EINVAL
    assert run(ones, None, op=4, data=d_m) == 0                             # FLIP_V leaves odd k alone
    with pytest.raises(J.JpegAmdError):
        J.Spectral.from_host(ctx, (16, 8), J.Layout("y8", {1: J.Component((1, 1), 0)}), [m.reshape(1, 2, 64)],
                             [ones]).transform("flip_h")


def test_set_width_height_crops_and_zero_pads(ctx):
    sp = _synthetic(ctx, (100, 60), [(2, 2), (1, 1), (1, 1)], 9)
    before = sp.host_planes()
    sp.set(width=250)
    sp.set(height=20)
    assert sp.size == (250, 20)
    assert sp.units == [(32, 3), (16, 2), (16, 2)]
    for a, b in zip(sp.host_planes(), before):
        uy, ux = a.shape[:2]
        want = np.zeros_like(a)
        want[:min(uy, b.shape[0]), :min(ux, b.shape[1])] = b[:uy, :ux]
        assert (a == want).all()
    with pytest.raises(J.JpegAmdError):
        sp.set(width=0)
