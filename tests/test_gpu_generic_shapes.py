"""k_generic_fused (jpeg_amd_spectral_rectangular[_batch]) and k_generic_encode (jpeg_amd_rectangular_spectral[_batch]) on the
layouts with a factor of 3 or 4 -- 4:1:1, 4:1:0, thirds, quarters, 2-in-4 -- on images of several tiles: the per-tile block range
at every phase of its period, the magic-multiply quotient by 3 and 6, the literal filter over whole tile interiors, the exact
filter with vertical weights in eighths, both tile heights, tiles of exactly 256 blocks, the store tail of a 5-pixel tile column.
The reference holds no gold for these layouts: the oracle (its literal formulas on the CPU) is the checker, sample for sample,
and the staged kernels a second one.  The cases, sizes and inputs are in tests/_generic_cases.py; tests/test_generic_cases_cpu.py
checks the inputs themselves without a GPU."""
import ctypes as C

import numpy as np
import pytest

import _generic_cases as GC
from oracle import oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def J():
    import jpeg_amd
    return jpeg_amd


@pytest.fixture(scope="module")
def ctx(J):
    return J.Context(0)


def _layout(J, c, precision=None):
    comps = {i + 1: J.Component(f, i & 1) for i, f in enumerate(c.factors)}
    if c.extra is not None:
        comps[99] = J.Component(c.extra, 0)      # not recognised: takes part in the scale only (decode.swift:2181-2190)
    layout = J.Layout(("custom", precision or c.precision, c.count), comps)
    assert layout.scale == c.scale and [p.factor for p in layout.planes] == list(c.factors)
    return layout


def _differences(got, want, what):
    """'' when equal; else the count and the first positions with their tile -- the tile index is what identifies the fault."""
    if got.shape == want.shape and (got == want).all():
        return ""
    if got.shape != want.shape:
        return f"{what}: shape {got.shape} against {want.shape}"
    bad = np.argwhere(got != want)
    lines = [f"{what}: {len(bad)} of {want.size} samples differ; first (x, y, plane) [tile column x / 128; tile row y / 64 | y / 32]: got != want"]
    for y, x, p in bad[:8]:
        lines.append(f"  ({x}, {y}, {p}) [column {x // GC.TILE_W}; row {y // 64} | {y // 32}]: {int(got[y, x, p])} != {int(want[y, x, p])}")
    cols = sorted({int(x) // GC.TILE_W for _, x, _ in bad}); rows = sorted({int(y) // 32 for y, _, _ in bad}); pl = sorted({int(p) for _, _, p in bad})
    lines.append(f"  tile columns {cols}, 32-row bands {rows}, planes {pl}")
    return "\n".join(lines)


def _coefficient_differences(got, want, what):
    """the same for coefficient planes [uy, ux, 64]: (block x, block y, zigzag index)."""
    out = []
    for p, (a, b) in enumerate(zip(got, want)):
        if a.shape != b.shape:
            out.append(f"{what}: plane {p}: shape {a.shape} against {b.shape}")
        elif not (a == b).all():
            bad = np.argwhere(a != b)
            first = ", ".join(f"({bx}, {by}, {z}): {int(a[by, bx, z])} != {int(b[by, bx, z])}" for by, bx, z in bad[:6])
            out.append(f"{what}: plane {p}: {len(bad)} of {b.size} coefficients differ; first (block x, block y, zigzag): {first}")
    return "\n".join(out)


_copy = lambda a: np.array(a)      # the shared inputs are read-only; torch.from_numpy wants a writable array


_name = lambda size: f"{size[0]}x{size[1]}"
DECODE = [(c.number, cosite, size, kind) for c in GC.CASES for size in GC.SIZES for kind in GC.KINDS for cosite in (False, True)]
ENCODE = [(c.number, cosite, size) for c in GC.CASES for size in GC.SIZES for cosite in (False, True)]


@pytest.mark.parametrize("number,cosite,size,kind", DECODE,
                         ids=[f"case{n}-{'cosited' if s else 'centred'}-{_name(z)}-{k}" for n, s, z, k in DECODE])
def test_generic_decode_factor_3_and_4_layouts_across_tile_seams(J, ctx, number, cosite, size, kind):
    """Spectral.rectangular(cosite:) == the oracle's idct + interleaved == the staged kernels, every sample (case 14 is refused by
    generic_fused_supported: the same call takes the staged kernels and must still agree)."""
    c = GC.case(number)
    planes, tables, q, want_p = GC.oracle_planes(number, size, kind)
    want = GC.oracle_rect(number, size, kind, cosite)
    spectral = J.Spectral.from_host(ctx, size, _layout(J, c), [_copy(p) for p in planes], tables, q=q)
    got = spectral.rectangular(cosite=cosite).host_values()
    staged = spectral.idct().interleaved(cosite=cosite).host_values()
    report = _differences(got, want, "one call against the oracle")
    assert not report, report
    report = _differences(got, staged, "one call against the staged kernels")
    assert not report, report


@pytest.mark.parametrize("number,cosite,size", ENCODE, ids=[f"case{n}-{'cosited' if s else 'centred'}-{_name(z)}" for n, s, z in ENCODE])
def test_generic_encode_factor_3_and_4_layouts_across_tile_seams(J, ctx, number, cosite, size):
    """Rectangular.spectral(quanta) == the oracle's decomposed + fdct == the staged kernels on the oracle's interleaved samples of
    the `wide` input.  The cases with a box of 3 (GC.ENCODE_STAGED) take the staged encoder inside the same call: the dispatch is
    part of what is tested."""
    c = GC.case(number)
    values = GC.oracle_rect(number, size, "wide", cosite)
    tables = GC.encode_tables(c)
    _, want = GC.oracle_encode(c, size, values, tables)
    assert max(int(np.abs(w.astype(np.int32)).max()) for w in want) < 32000      # where the reference would trap
    rect = J.Rectangular.from_host(ctx, size, _layout(J, c), _copy(values))
    got = rect.spectral(tables).host_planes()
    report = _coefficient_differences(got, want, "one call against the oracle")
    assert not report, report
    staged = rect.decomposed().fdct(tables).host_planes()
    report = _coefficient_differences(got, staged, "one call against the staged kernels")
    assert not report, report


def test_generic_batch_411_twelve_bit_strides_and_sentinels(J, ctx):
    """jpeg_amd_spectral_rectangular_batch and jpeg_amd_rectangular_spectral_batch on case 1 (4:1:1: quarters in x through the literal
    filter) at 12 bits: three images of 517 x 259 with their own table sets -- the grid of tiles x images, which has so far run as a
    batch for 4:2:0 only -- and an image stride with a gap.  Every image equals its own single call and the oracle; the gaps and the
    tail keep their sentinel."""
    import torch
    from jpeg_amd import _lib
    c, P, n, size, gap = GC.case(1), 12, 3, GC.LARGE, 24
    layout = _layout(J, c, P)
    units = layout.units(size)
    L = layout.c_layout(size, units, c.q)
    factors = list(c.factors)
    npx = size[0] * size[1] * c.count
    inputs = [GC.build_input(c, size, "wide", precision=P, seed=7700 + i) for i in range(n)]
    host = [planes for planes, _, _ in inputs]
    tables = np.stack([np.stack(t) for _, t, _ in inputs])                     # [n, 2, 64]
    assert not (tables[0] == tables[1]).all() and not (tables[1] == tables[2]).all()
    dev = ctx.torch_device
    lib = _lib.lib()

    # ---- decode ----
    d_planes = [torch.from_numpy(np.stack([host[i][p] for i in range(n)])).to(dev) for p in range(c.count)]
    d_q = torch.from_numpy(tables.view(np.int16)).to(dev)
    sentinel = 0x5a5a
    out = torch.full((n, npx + gap), sentinel, dtype=torch.int16, device=dev)
    st = lib.jpeg_amd_spectral_rectangular_batch(ctx.handle, C.byref(L), n, _lib.ptr_array([p.data_ptr() for p in d_planes]),
                                                 _lib.size_array([64 * a * b for a, b in units]), d_q.data_ptr(), 128, 2, 0,
                                                 out.data_ptr(), npx + gap)
    assert st == 0
    got = out.cpu().numpy().view(np.uint16)
    wants = []
    for i in range(n):
        want_p = [O.idct_plane(host[i][p], tables[i][c.q[p]], P) for p in range(c.count)]
        want = O.interleave(want_p, factors, c.scale, size, cosited=False)
        wants.append(want)
        report = _differences(got[i, :npx].reshape(want.shape), want, f"image {i} of the batch against the oracle")
        assert not report, report
        single = J.Spectral.from_host(ctx, size, layout, [_copy(p) for p in host[i]], list(tables[i]), q=c.q).rectangular(cosite=False).host_values()
        report = _differences(got[i, :npx].reshape(want.shape), single, f"image {i} of the batch against its own single call")
        assert not report, report
        assert (got[i, npx:] == sentinel).all(), f"the gap behind image {i} was written"

    # ---- encode: the oracle's samples of each image, tables from 16 .. 59 per image ----
    rng = np.random.default_rng(7800)
    etables = rng.integers(16, 60, (n, 2, 64)).astype(np.uint16)
    d_rect = torch.full((n, npx + gap), sentinel, dtype=torch.int16, device=dev)
    d_rect[:, :npx] = torch.from_numpy(np.stack([w.reshape(-1) for w in wants]).view(np.int16)).to(dev)
    d_eq = torch.from_numpy(etables.view(np.int16)).to(dev)
    cgap = 64
    outs = [torch.full((n, 64 * a * b + cgap), 99, dtype=torch.int16, device=dev) for a, b in units]
    st = lib.jpeg_amd_rectangular_spectral_batch(ctx.handle, C.byref(L), n, d_rect.data_ptr(), npx + gap, d_eq.data_ptr(), 128, 2,
                                                 _lib.ptr_array([o.data_ptr() for o in outs]),
                                                 _lib.size_array([64 * a * b + cgap for a, b in units]))
    assert st == 0
    h_outs = [o.cpu().numpy() for o in outs]
    for i in range(n):
        _, want_f = GC.oracle_encode(c, size, wants[i], list(etables[i]), precision=P)
        assert max(int(np.abs(w.astype(np.int32)).max()) for w in want_f) < 32000
        got_f = [h_outs[p][i, :want_f[p].size].reshape(want_f[p].shape) for p in range(c.count)]
        report = _coefficient_differences(got_f, want_f, f"image {i} of the batch against the oracle")
        assert not report, report
        single = J.Rectangular.from_host(ctx, size, layout, wants[i]).spectral({k: etables[i][k] for k in range(2)}).host_planes()
        report = _coefficient_differences(got_f, single, f"image {i} of the batch against its own single call")
        assert not report, report
        for p in range(c.count):
            assert (h_outs[p][i, want_f[p].size:] == 99).all(), f"the gap behind plane {p} of image {i} was written"
