"""Entropy decoding on the GPU: jpeg_amd_jpeg_decode_spectral_device (k_huffman_intervals, one restart interval per work-item)
against jpeg_amd_jpeg_decode_spectral -- exact equality of planes, tables, frame infos and statuses -- on the inputs that
tests/test_entropy_device_cpu.py has cleared on the host: every sequential fixture, the files written from constructed planes
and the seeded damage.  Each group goes through ONE call (files of any mix of geometries), so the whole file is a handful of
launches."""
import ctypes as C

import numpy as np
import pytest

import jpeg_amd as J
import _entropy_device as E
from _calls import ctx, torch  # noqa: F401  (fixtures)
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu
SENTINEL = -23131


def device_decode(ctx, torch, files):
    """One call for `files` -> (status of the call, per-file statuses, planes per file as numpy, quanta [n, 4, 64], infos).
    The planes hold SENTINEL before the call."""
    n = len(files)
    infos = [J.inspect(f) for f in files]
    planes = [[torch.full((i.units_y[c], i.units_x[c], 64), SENTINEL, dtype=torch.int16, device=ctx.torch_device)
               for c in range(i.ncomponents)] for i in infos]
    coef = (C.c_void_p * (4 * max(n, 1)))()
    for k, ps in enumerate(planes):
        for c, t in enumerate(ps):
            coef[4 * k + c] = t.data_ptr()
    quanta = np.zeros((max(n, 1), 4, 64), np.uint16)
    out_info, status = (_lib.FrameInfo * max(n, 1))(), (C.c_int32 * max(n, 1))(*([-99] * max(n, 1)))
    st = _lib.lib().jpeg_amd_jpeg_decode_spectral_device(
        ctx.handle, n, (C.c_void_p * max(n, 1))(*[f.ctypes.data for f in files]), (C.c_size_t * max(n, 1))(*[f.size for f in files]),
        coef, quanta.ctypes.data, out_info, status)
    torch.cuda.synchronize()
    return st, list(status)[:n], [[t.cpu().numpy() for t in ps] for ps in planes], quanta, out_info


def check_group(ctx, torch, named):
    """Every file of `named` [(name, bytes)] in one call, each compared with the host decoder."""
    files = [d for _, d in named]
    st, status, planes, quanta, infos = device_decode(ctx, torch, files)
    want = [E.host_decode(d) for d in files]
    first_bad = next((w[0] for w in want if w[0] != E.OK), E.OK)
    assert st == first_bad
    for k, (name, _) in enumerate(named):
        hs, hinfo, hplanes, hquanta = want[k]
        assert status[k] == hs, name
        if hs != E.OK:
            continue                                   # (the planes of such a file are unspecified)
        assert bytes(infos[k]) == bytes(hinfo), name
        assert (quanta[k] == hquanta).all(), name
        for c, (a, b) in enumerate(zip(planes[k], hplanes)):
            assert (a == b).all(), (name, c)


def test_counter_and_empty_call(ctx, torch):
    count = C.c_int64(-1)
    assert _lib.lib().jpeg_amd_ctx_device_entropy_files(ctx.handle, C.byref(count)) == 0
    before = count.value
    assert device_decode(ctx, torch, [])[0] == E.OK
    data = E.constructed_file("420-64x48-row")[0]
    check_group(ctx, torch, [("a", data), ("b", data)])
    assert _lib.lib().jpeg_amd_ctx_device_entropy_files(ctx.handle, C.byref(count)) == 0
    assert count.value == before + 2


def test_sequential_fixtures(ctx, torch):
    named = [(n, d) for n, d, _ in E.fixture_files() if E.plan(d)[0] == E.OK]
    assert len(named) >= 8 and any("restart" in n for n, _ in named)
    check_group(ctx, torch, named)


def test_constructed_files(ctx, torch):
    check_group(ctx, torch, [(n, E.constructed_file(n)[0]) for n in sorted(E.CONSTRUCTED)])


def test_seeded_damage(ctx, torch):
    named = [(n, d) for n, d, verdict in E.damaged_files() if verdict == E.OK]
    assert len(named) >= 40
    check_group(ctx, torch, named)


def test_three_geometries_in_one_call(ctx, torch):
    named = [(n, E.constructed_file(n)[0]) for n in ("grey-257-intervals", "411-70x30-row", "four-12bit-35x19-ri2")]
    check_group(ctx, torch, named)


@pytest.mark.parametrize("bad", ["progressive", "marker-removed", "undefined-tables"])
def test_a_refused_file_ends_the_call_with_nothing_written(ctx, torch, bad):
    import _files as F
    good = E.constructed_file("420-64x48-row")[0]
    other, verdict = {"progressive": (F.golden_file("color-progressive-1.jpg"), E.ENOSUP),
                      "marker-removed": (next(d for n, d, _ in E.damaged_files() if n.endswith("420-64x48-row/marker-removed")), E.ENOSUP),
                      "undefined-tables": (F.undefined_tables(good), E.EINVAL)}[bad]
    st, status, planes, _, _ = device_decode(ctx, torch, [good, other, good])
    assert st == verdict
    assert status == [-99, -99, -99]
    for ps in planes:
        for p in ps:
            assert (p == SENTINEL).all()


def test_null_pointers_and_misaligned_planes(ctx, torch):
    data = E.constructed_file("grey-17x17-ri1")[0]
    lib = _lib.lib()
    info = J.inspect(data)
    plane = torch.full((info.units_y[0] * info.units_x[0] * 64 + 8,), SENTINEL, dtype=torch.int16, device=ctx.torch_device)
    quanta, out_info, status = np.zeros((1, 4, 64), np.uint16), (_lib.FrameInfo * 1)(), (C.c_int32 * 1)()
    files, sizes = (C.c_void_p * 1)(data.ctypes.data), (C.c_size_t * 1)(data.size)

    def call(ptr, files=files, h=ctx.handle):
        coef = (C.c_void_p * 4)(ptr)
        return lib.jpeg_amd_jpeg_decode_spectral_device(h, 1, files, sizes, coef, quanta.ctypes.data, out_info, status)

    assert call(plane.data_ptr() + 2) == E.EINVAL           # not 16-byte aligned
    assert call(None) == E.EINVAL
    assert call(plane.data_ptr(), files=(C.c_void_p * 1)(None)) == E.EINVAL
    assert call(plane.data_ptr(), h=None) == E.EINVAL
    torch.cuda.synchronize()
    assert (plane.cpu().numpy() == SENTINEL).all()
    assert call(plane.data_ptr()) == E.OK


def test_python_entry_points(ctx, torch):
    data = E.constructed_file("420-35x19-ri1")[0]
    info, nscans, nintervals = J.plan_intervals(data)
    assert (info.width, info.height, nscans, nintervals) == (35, 19, 1, 6)
    with pytest.raises(J.JpegAmdError):
        J.plan_intervals(np.fromfile(E.G.path("decode/color-progressive-1.jpg"), np.uint8))
    host = J.Spectral.decompress(ctx, data)
    dev = J.Spectral.decompress(ctx, data, entropy="device")
    many = J.decompress_spectrals(ctx, [data, E.constructed_file("grey-17x17-ri1")[0]])
    assert len(many) == 2 and many[1].size == (17, 17)
    for s in (dev, many[0]):
        assert s.size == host.size and s.q == host.q
        assert all((a == b).all() for a, b in zip(s.quanta, host.quanta))
        assert all(torch.equal(a, b) for a, b in zip(s.planes, host.planes))
    assert torch.equal(dev.decode(J.RGB), host.decode(J.RGB))
    assert J.decompress_spectrals(ctx, []) == []


# ---- routing: JPEG_AMD_CTX_DEVICE_ENTROPY in the batch file calls ----------------------------------------------------------------

@pytest.fixture(scope="module")
def flagged():
    return J.Context(0, device_entropy=True)


def _batch_device(c, torch, batch, size):
    """jpeg_amd_decompress_batch_device on one context -> (pixels uint8 [n, h * w * 3] on the host, files that took the device route)."""
    n, npx = len(batch), size[0] * size[1] * 3
    out = torch.zeros(n * npx, dtype=torch.uint8, device=c.torch_device)
    ptrs, sizes = (C.c_void_p * n)(*[f.ctypes.data for f in batch]), (C.c_size_t * n)(*[f.size for f in batch])
    before = c.device_entropy_files
    st = _lib.lib().jpeg_amd_decompress_batch_device(c.handle, ptrs, sizes, n, 4, 0, J.RGB.code, out.data_ptr(), 0, None)
    assert st == 0, st
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, npx), c.device_entropy_files - before


@pytest.mark.parametrize("name", ["color-sequential-restart.jpg", "grayscale-sequential-restart.jpg"])
def test_routed_batch_of_a_restart_fixture(ctx, flagged, torch, name):
    e = E.G.entry(name)
    data = np.fromfile(E.G.path(e["file"]), np.uint8)
    batch = [data.copy() for _ in range(5)]
    want, none = _batch_device(ctx, torch, batch, (e["width"], e["height"]))
    got, routed = _batch_device(flagged, torch, batch, (e["width"], e["height"]))
    assert (none, routed) == (0, 5)
    assert (got == want).all()
    if e["gold"]:
        assert E.G.sha(got[0]) == e["gold"]["rgb_sha256"]


def test_routed_batch_crosses_the_chunk_of_32(ctx, flagged, torch):
    """33 files of one 4:2:0 geometry: 31 with restart intervals (seeds differ), one without DRI (eligible: one interval) and a
    progressive one, which takes the host route in the first chunk."""
    import _files as F
    L = F.c_layout(160, 96, E.LAYOUTS["420"], qi=[0, 1, 2])
    batch = [F.write_file(L, E.crafted_planes(F.plane_units(L), 300 + i), F.tables(3, 300 + i), "sequential", 10) for i in range(31)]
    batch.insert(7, F.write_file(L, E.crafted_planes(F.plane_units(L), 400), F.tables(3, 400), "progressive"))
    batch.append(F.write_file(L, E.crafted_planes(F.plane_units(L), 401), F.tables(3, 401), "sequential", 0))
    assert len(batch) == 33 and [E.plan(f)[0] for f in batch].count(E.OK) == 32
    want, none = _batch_device(ctx, torch, batch, (160, 96))
    got, routed = _batch_device(flagged, torch, batch, (160, 96))
    assert (none, routed) == (0, 32)
    assert (got == want).all()


def test_routed_files_to_tensors_on_a_mixed_list(ctx, flagged, torch):
    """decompress_tensors at 32 x 32: a restart file, a baseline file without DRI, a grey file, a progressive file (host route
    in the same chunk) and a 4:1:1 file; tensors equal bit for bit, and exactly the eligible files took the device route."""
    import _files as F
    files = [E.constructed("420", (160, 96), 500, 10)[0], F.golden_file("color-sequential-1.jpg"), E.constructed("grey", (150, 99), 501, 7)[0],
             F.golden_file("color-progressive-1.jpg"), E.constructed("411", (170, 90), 502, 6)[0]]
    eligible = [E.plan(f)[0] == E.OK for f in files]
    assert eligible == [True, True, True, False, True]
    spec = J.tensor_spec()
    before = (ctx.device_entropy_files, flagged.device_entropy_files)
    want = J.decompress_tensors(ctx, files, (32, 32), spec, threads=2)
    got = J.decompress_tensors(flagged, files, (32, 32), spec, threads=2)
    torch.cuda.synchronize()
    assert (ctx.device_entropy_files - before[0], flagged.device_entropy_files - before[1]) == (0, 4)
    assert torch.equal(got[0].cpu(), want[0].cpu())
    assert (got[1] == want[1]).all()
    resized = [J.decompress_resized(c, files, (32, 32), threads=2)[0].cpu() for c in (ctx, flagged)]
    assert torch.equal(resized[0], resized[1])


def test_an_invalid_interval_is_the_files_status_in_the_standalone_call(ctx, torch):
    """Files built to hold a DC symbol above 16 (E.dc_symbol_17) among good ones: h_status is EINVAL for exactly those, the
    call returns the first of them, and the good files' planes are the host decoder's."""
    good = [E.constructed_file(n)[0] for n in ("420-64x48-row", "grey-35x19-ri2", "four-12bit-35x19-ri2")]
    bad = [E.dc_symbol_17(g) for g in good]
    named = [("good0", good[0]), ("bad1", bad[1]), ("good1", good[1]), ("bad0", bad[0]), ("bad2", bad[2]), ("good2", good[2])]
    assert [E.plan(d)[0] for _, d in named] == [E.OK] * 6
    assert [E.host_decode(d)[0] for _, d in named] == [E.OK, E.EINVAL, E.OK, E.EINVAL, E.EINVAL, E.OK]
    check_group(ctx, torch, named)                   # (statuses, the call's status and the good files' planes)


def test_a_damaged_device_file_ends_the_routed_call_with_its_status(ctx, flagged, torch):
    """A file the planner takes with a DC symbol above 16 in some interval, among good files of its geometry: EINVAL from
    the call on both routes, on the flagged context through the device route, and the context is usable afterwards."""
    good = E.constructed("420", (160, 96), 600, 10)[0]
    bad = E.dc_symbol_17(good)
    assert E.plan(bad)[0] == E.OK and E.host_decode(bad)[0] == E.EINVAL
    n, batch = 3, [good, bad, good]
    out = torch.zeros(n * 160 * 96 * 3, dtype=torch.uint8, device=ctx.torch_device)
    ptrs, sizes = (C.c_void_p * n)(*[f.ctypes.data for f in batch]), (C.c_size_t * n)(*[f.size for f in batch])
    before = flagged.device_entropy_files
    for c in (ctx, flagged):
        assert _lib.lib().jpeg_amd_decompress_batch_device(c.handle, ptrs, sizes, n, 2, 0, J.RGB.code, out.data_ptr(), 0, None) == E.EINVAL
    assert flagged.device_entropy_files - before == 3                            # all three went up: the status came from the device
    want, _ = _batch_device(ctx, torch, [good, good], (160, 96))
    got, routed = _batch_device(flagged, torch, [good, good], (160, 96))          # the context is usable afterwards
    assert routed == 2 and (got == want).all()


def test_the_one_file_calls_stay_on_the_host_route(ctx, flagged, torch):
    """jpeg_amd_decompress and jpeg_amd_decompress_rectangular decode on the host whatever the flag says: the counter of a
    flagged context stays put, for a file the batch call would route."""
    data = E.constructed("420", (160, 96), 601, 10)[0]
    assert _batch_device(flagged, torch, [data], (160, 96))[1] == 1               # (eligible, and it fits)
    lib, before = _lib.lib(), flagged.device_entropy_files
    px = [np.zeros(160 * 96 * 3, np.uint8) for _ in range(2)]
    rect = [np.zeros(160 * 96 * 3, np.uint16) for _ in range(2)]
    for k, c in enumerate((ctx, flagged)):
        assert lib.jpeg_amd_decompress(c.handle, data.ctypes.data, data.size, 0, J.RGB.code, px[k].ctypes.data, px[k].size, None) == 0
        assert lib.jpeg_amd_decompress_rectangular(c.handle, data.ctypes.data, data.size, 0, 0, 2, rect[k].ctypes.data, rect[k].size, None) == 0
    assert flagged.device_entropy_files == before
    assert (px[0] == px[1]).all() and (rect[0] == rect[1]).all() and px[0].any()
