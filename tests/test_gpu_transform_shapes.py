"""k_spectral_transform<op, requantise> (kernels_transform.hip) on synthetic shapes: every op, with and without
requantisation, across the seams of its workgroups (256 x 1 output blocks for the ops that keep the axes, 32 x 8 for the
transposing ones), on regions that crop and that grow, in planes of one block, with strided batches in buffers that held a
sentinel, and the overflow flag from any block, plane and image.

Every call is jpeg_amd_spectral_transform_batch itself; every comparison is integer equality with the numpy restatement
(_transform_ref.transform_plane, requantize_ref), which test_transform_cpu anchors in pixel space.  The layouts, sizes and
regions are _transform_ref.LAYOUTS, seam_sizes and seam_regions.  Strides, gaps and the lead of the buffers are multiples of 8
elements: the kernel moves blocks in 16-byte pieces."""
import ctypes as C

import numpy as np
import pytest

import _transform_ref as R
import jpeg_amd as J
from _calls import Out, c_layout, ctx, torch  # noqa: F401  (the fixtures)
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

N = 3
CASES = [(name, size) for name in R.LAYOUTS for size in R.seam_sizes(name)]
IDS = [f"{name}-{w}x{h}" for name, (w, h) in CASES]
LEAD, TAIL = 24, 40                                       # elements of the output buffers before and after the images


def _gap(p, out):
    return 8 * (2 * p + (5 if out else 3))                # differs per plane, and between input and output


class Batch:
    """n images of a layout on the host: plane p is one int16 array, image i at i * stride[p], random in the gaps too."""

    def __init__(self, name, size, rng, lo, hi, n=N):
        self.name, self.size, self.n = name, size, n
        self.factors = R.LAYOUTS[name]
        self.qi, self.ntables = R.layout_tables(name)
        self.L = c_layout(*size, self.factors, qi=self.qi)
        self.units = [(self.L.units_x[p], self.L.units_y[p]) for p in range(len(self.factors))]
        self.stride = [64 * ux * uy + _gap(p, False) for p, (ux, uy) in enumerate(self.units)]
        self.host = [rng.integers(lo, hi + 1, n * s).astype(np.int16) for s in self.stride]

    def copy(self):
        other = object.__new__(Batch)
        other.__dict__.update(self.__dict__)
        other.host = [h.copy() for h in self.host]
        return other

    def plane(self, i, p):
        """Image i of plane p as [uy, ux, 64], a view."""
        ux, uy = self.units[p]
        return self.host[p][i * self.stride[p]:i * self.stride[p] + 64 * ux * uy].reshape(uy, ux, 64)

    def kept_last(self, op, p):
        """The last block of plane p that op keeps when it trims the whole image; None where it keeps none."""
        lay = R.layout_ref(*self.size, self.factors, op)
        return None if lay is None else (lay[4][p][1] - 1, lay[4][p][0] - 1)

    def upload(self, ctx):
        return [ctx.upload(h) for h in self.host]


def _positions(op):
    """The source zigzag positions whose coefficient op negates, and the others."""
    m, sign = R.mapping_arrays(op)
    neg = np.sort(m[sign < 0])
    return neg, np.setdiff1d(np.arange(64), neg)


def _legal(batch, op):
    """A copy of `batch` that the reference transforms without a trap: -32768 stays only where op does not negate.  The
    extremes that must not raise the flag are planted in the last block of the last plane of the last image, and in the
    last block of it that op keeps (ROT_CCW, say, trims the last block column away)."""
    b = batch.copy()
    neg, keep = _positions(op)
    last = len(b.factors) - 1
    for i in range(b.n):
        for p in range(len(b.factors)):
            v = b.plane(i, p)
            sub = v[..., neg]
            sub[sub == -32768] = -32767
            v[..., neg] = sub
    v = b.plane(b.n - 1, last)
    for at in {(v.shape[0] - 1, v.shape[1] - 1), b.kept_last(op, last)} - {None}:
        v[at][keep[-1]] = -32768
        if neg.size:
            v[at][neg[0]], v[at][neg[-1]] = 32767, -32767
    return b


def _expected(batch, op, region, q_in=None, q_out=None, shared=False):
    """-> (per plane int64 [n, ouy, oux, 64], trapped) by the restatement, or None where the layout is refused.
    shared: every image reads image 0 and its tables (strides of 0)."""
    lay = R.layout_ref(*batch.size, batch.factors, op, region)
    if lay is None:
        return None
    _, _, _, units, cropped, origin = lay
    m, _ = R.mapping_arrays(op)
    want, trapped = [], False
    for p in range(len(batch.factors)):
        images = []
        for i in range(1 if shared else batch.n):
            t = R.transform_plane(batch.plane(i, p), op, cropped[p], origin[p])
            assert t.shape == (units[p][1], units[p][0], 64)
            if q_out is not None:
                t, trap = R.requantize_ref(t, q_in[i, batch.qi[p]][m], q_out[i, batch.qi[p]])
                trapped |= trap
            images.append(t.astype(np.int64))
        want.append(np.stack(images * batch.n if shared else images))
    return want, trapped


def _run(ctx, torch, batch, d_in, op, region, want, d_q=None, d_qo=None, shared=False):
    """One call into sentinel buffers.  -> (status, flag, per plane int16 [n, ouy, oux, 64] or None); asserts that nothing
    outside the images' spans was written."""
    nplanes = len(batch.factors)
    shapes = [w.shape[1:] for w in want] if want is not None else [(1, 1, 64)] * nplanes
    outs = [Out(ctx, torch, [int(s[0] * s[1] * 64)] * batch.n, elem=2, gap=_gap(p, True), lead=LEAD, tail=TAIL)
            for p, s in enumerate(shapes)]
    flag = torch.zeros(1, dtype=torch.int32, device=ctx.torch_device)
    reg = None if region is None else _lib.Region(*region)
    st = _lib.lib().jpeg_amd_spectral_transform_batch(
        ctx.handle, C.byref(batch.L), batch.n, op, None if reg is None else C.byref(reg),
        _lib.ptr_array([t.data_ptr() for t in d_in]), _lib.size_array([0] * nplanes if shared else batch.stride),
        None if d_q is None else d_q.data_ptr(), 0 if shared else 64 * batch.ntables, batch.ntables,
        None if d_qo is None else d_qo.data_ptr(), _lib.ptr_array([o.ptr for o in outs]),
        _lib.size_array([o.stride for o in outs]), flag.data_ptr())
    ctx.synchronize()
    if want is None:
        assert all(o.untouched() for o in outs)
        return st, int(flag.item()), None
    got = [np.stack([img.view(np.int16).reshape(s) for img in o.images()]) for o, s in zip(outs, shapes)]
    return st, int(flag.item()), got


def _tables(batch, rng):
    """q_in from 1 .. 17 (with coefficients within +-1900 no Int16 product overflows); q_out half from 1 .. 255, half from
    256 .. 65535; per image."""
    shape = (batch.n, batch.ntables, 64)
    q_in = rng.integers(1, 18, shape).astype(np.uint16)
    q_out = np.where(rng.random(shape) < 0.5, rng.integers(1, 256, shape), rng.integers(256, 65536, shape)).astype(np.uint16)
    return q_in, q_out


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_every_op_and_region_matches_the_restatement(ctx, torch, name, size):
    base = Batch(name, size, np.random.default_rng(101), -32768, 32767)
    for op in range(8):
        batch = _legal(base, op)
        d_in = batch.upload(ctx)
        for region in R.seam_regions(*size, batch.factors):
            exp = _expected(batch, op, region)
            st, flag, got = _run(ctx, torch, batch, d_in, op, region, exp and exp[0])
            if exp is None:
                assert st == _lib.EINVAL, (op, region)
                continue
            assert st == 0 and flag == 0, (op, region, st, flag)
            for p, (g, w) in enumerate(zip(got, exp[0])):
                assert np.array_equal(g, w), (op, region, p)      # the zero blocks of a grown region included


@pytest.mark.parametrize("name,size", CASES, ids=IDS)
def test_every_op_requantises_like_the_restatement(ctx, torch, name, size):
    rng = np.random.default_rng(202)
    batch = Batch(name, size, rng, -1900, 1900)
    q_in, q_out = _tables(batch, rng)
    d_in, d_q, d_qo = batch.upload(ctx), ctx.upload(q_in), ctx.upload(q_out)
    for op in range(8):
        for region in R.seam_regions(*size, batch.factors):
            exp = _expected(batch, op, region, q_in, q_out)
            st, flag, got = _run(ctx, torch, batch, d_in, op, region, exp and exp[0], d_q, d_qo)
            if exp is None:
                assert st == _lib.EINVAL, (op, region)
                continue
            assert not exp[1]                                     # the restatement does not trap on these inputs
            assert st == 0 and flag == 0, (op, region, st, flag)
            for p, (g, w) in enumerate(zip(got, exp[0])):
                assert np.array_equal(g, w), (op, region, p)


def test_requantising_batch_with_strides_of_zero_reads_image_0(ctx, torch):
    """in_stride = 0 and quanta_stride = 0: every image is image 0 with the tables of image 0."""
    rng = np.random.default_rng(303)
    batch = Batch("420", (150, 600), rng, -1900, 1900)
    q_in, q_out = _tables(batch, rng)
    d_in, d_q, d_qo = batch.upload(ctx), ctx.upload(q_in), ctx.upload(q_out)
    for op in range(8):
        want, trapped = _expected(batch, op, None, q_in, q_out, shared=True)
        assert not trapped
        st, flag, got = _run(ctx, torch, batch, d_in, op, None, want, d_q, d_qo, shared=True)
        assert st == 0 and flag == 0, (op, st, flag)
        for p, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), (op, p)
            assert all(np.array_equal(g[i], g[0]) for i in range(1, batch.n))


def _workgroup(op, x, y, oux):
    """The workgroup, within its plane, of output block (x, y)."""
    gw, gh = (32, 8) if op & 1 else (256, 1)
    return (y // gh) * -(-oux // gw) + x // gw


@pytest.mark.parametrize("op", [2, 5])
def test_traps_are_flagged_from_any_block_plane_and_image(ctx, torch, op):
    name, size = "420", (4133, 37)
    neg, keep = _positions(op)
    legal = _legal(Batch(name, size, np.random.default_rng(404), -32768, 32767), op)
    last = len(legal.factors) - 1
    # -- a single negated -32768, without requantisation: in the last kept block of the last plane of the last image, and in
    #    that plane's first block, which the mirror sends past the plane's first workgroup
    for at in (legal.kept_last(op, last), (0, 0)):
        batch = legal.copy()
        batch.plane(N - 1, last)[at][neg[3]] = -32768
        want, _ = _expected(batch, op, None)
        st, flag, got = _run(ctx, torch, batch, batch.upload(ctx), op, None, want)
        assert st == 0 and flag != 0, (at, st, flag)
        for p, (g, w) in enumerate(zip(got, want)):
            free = w == 32768                                     # where the reference traps the value is unspecified
            assert int(free.sum()) == (p == last)
            assert np.array_equal(g[~free], w[~free]), (at, p)
        i, y, x, _ = (int(v[0]) for v in np.nonzero(want[last] == 32768))
        assert i == N - 1
        if at == (0, 0):
            assert _workgroup(op, x, y, want[last].shape[2]) > 0
    st, flag, got = _run(ctx, torch, legal, legal.upload(ctx), op, None, _expected(legal, op, None)[0])
    assert st == 0 and flag == 0                                  # the same input without the planted coefficient
    # -- with requantisation: q_in * c at the edges of Int16, in a luma block past the first workgroup, at a position the op
    #    negates and at one it does not
    rng = np.random.default_rng(505)
    base = Batch(name, size, rng, -1900, 1900)
    q_base, q_out = _tables(base, rng)
    d_qo = ctx.upload(q_out)
    cropped0 = R.layout_ref(*size, base.factors, op)[4][0]
    block = (base.units[0][1] - 1, 0)                             # the first block of the last row of luma, image 1
    marker = np.zeros_like(base.plane(1, 0))
    for product, q, c in ((32767, 7, 4681), (-32768, 8, -4096), (32768, 8, 4096), (-32769, 3, -10923)):
        assert q * c == product
        for pos in (int(neg[5]), int(keep[5])):
            batch, q_in = base.copy(), q_base.copy()
            q_in[1, 0, pos] = q
            batch.plane(1, 0)[block][pos] = -c if pos in neg else c
            want, trapped = _expected(batch, op, None, q_in, q_out)
            assert trapped == (not -32768 <= product <= 32767)
            # where the planted coefficient lands: past the plane's first workgroup
            marker[:] = 0
            marker[block][pos] = 1
            y, x, z = (int(v[0]) for v in np.nonzero(R.transform_plane(marker, op, cropped0, (0, 0))))
            assert _workgroup(op, x, y, want[0].shape[2]) > 0
            st, flag, got = _run(ctx, torch, batch, batch.upload(ctx), op, None, want, ctx.upload(q_in), d_qo)
            assert st == 0 and (flag != 0) == trapped, (product, pos, st, flag)
            for p, (g, w) in enumerate(zip(got, want)):
                same = g == w
                if trapped and p == 0:
                    same[1, y, x, z] = True                       # where the reference traps the value is unspecified
                assert same.all(), (product, pos, p)


@pytest.mark.parametrize("name", ["420", "411"])
def test_python_api_at_a_seam_shape(ctx, name):
    size, factors = (4133, 37), R.LAYOUTS[name]
    rng = np.random.default_rng(606)
    layout = J.Layout("ycc8", {k + 1: J.Component(f, min(k, 1)) for k, f in enumerate(factors)})
    planes = [rng.integers(-32767, 32768, (uy, ux, 64)).astype(np.int16) for ux, uy in layout.units(size)]
    quanta = [rng.integers(1, 255, 64).astype(np.uint16) for _ in range(2)]
    sp = J.Spectral.from_host(ctx, size, layout, planes, quanta)
    for op in range(8):
        ow, oh, ofac, units, cropped, origin = R.layout_ref(*size, factors, op)
        t = sp.transform(op)
        assert t.size == (ow, oh) and t.units == units
        assert [c.factor for c in t.layout.planes] == ofac
        m, _ = R.mapping_arrays(op)
        for p, got in enumerate(t.host_planes()):
            assert np.array_equal(got, R.transform_plane(planes[p], op, cropped[p], origin[p])), (op, p)
            assert (t.quanta[t.q[p]] == quanta[min(p, 1)][m]).all()

    def same(a, b):
        assert a.size == b.size
        assert all(np.array_equal(x, y) for x, y in zip(a.host_planes(), b.host_planes()))
        assert all((a.quanta[a.q[p]] == b.quanta[b.q[p]]).all() for p in range(a.layout.count))

    # a rotation trims the edge it moves to the top or left to whole MCUs: on the image cropped to whole MCUs nothing is lost
    sx, sy = layout.scale
    whole = sp.transform("none", (0, 0, size[0] - size[0] % (8 * sx), size[1] - size[1] % (8 * sy)))
    assert whole.size == (4128, 32)
    r = whole
    for _ in range(4):
        r = r.transform("rot_ccw")
    same(r, whole)
    same(sp.transform("flip_v").transform("flip_h"), sp.transform("rot_180"))
