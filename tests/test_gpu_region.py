"""Region decode on the MI355X (jpeg_amd_decode_region_batch, k_region_decode): every case is bit for bit the full decode of
the same image, cropped -- against jpeg_amd_decode[_batch] on the device and, for the fixtures, against the oracle's full
decode on the host as well."""
import ctypes as C
import os

import numpy as np
import pytest

import jpeg_amd as J
from _calls import SENTINEL, Out, c_layout, c_regions, full_batch, plane_ptrs, plane_units
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _golden import GOLDEN
from _tile import FIXTURES, fixture, random_region
from jpeg_amd import _lib
from jpeg_amd.synth import natural_planes_torch
from oracle import oracle as O

pytestmark = pytest.mark.gpu

def _region_batch(ctx, L, planes, coef_stride, dq, q_stride, ntables, cosited, color, regions, out, stride):
    return _lib.lib().jpeg_amd_decode_region_batch(
        ctx.handle, C.byref(L), len(regions), plane_ptrs(planes), _lib.size_array(coef_stride),
        dq.data_ptr(), q_stride, ntables, cosited, color, c_regions(regions), out.data_ptr() if out is not None else None,
        stride)


def _decode_regions(ctx, torch, L, planes, coef_stride, dq, q_stride, ntables, cosited, color, regions, gap=0):
    """-> the output buffer, filled with SENTINEL before the call: nothing behind the last image's stride."""
    out = Out(ctx, torch, [3 * r[2] * r[3] for r in regions], gap=gap)
    assert _region_batch(ctx, L, planes, coef_stride, dq, q_stride, ntables, cosited, color, regions, out.buf, out.stride) == 0
    return out


def _crop(out, i, r):
    """Image i, still on the device."""
    x, y, w, h = r
    return out.device(i).view(h, w, 3)


def _fixture_regions(W, H, sx, sy, rng, k=20):
    mw, mh = 8 * sx, 8 * sy
    regs = [(0, 0, W, H), (1, 0, W - 1, H) if W > 1 else (0, 0, W, H), (0, 1, W, H - 1) if H > 1 else (0, 0, W, H),
            (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1), (0, 0, min(mw, W), min(mh, H))]
    for ox, oy, w, h in ((mw - 3, mh - 5, 7, 11), (mw + 1, 2 * mh - 1, 2 * mw + 3, mh + 3), (3, 5, 3 * mw - 1, 2 * mh + 1)):
        if ox < W and oy < H:
            regs.append((ox, oy, min(w, W - ox), min(h, H - oy)))
    for k16 in (1, 2, 5):
        for c in (16 * k16 - 1, 16 * k16, 16 * k16 + 1):
            if c < W:
                regs.append((c, 0, 1, H))
            if c < H:
                regs.append((0, c, W, 1))
    lx, ly = (W - 1) // mw * mw, (H - 1) // mh * mh      # the last (partial) MCU column / row
    regs += [(lx, 0, W - lx, H), (0, ly, W, H - ly), (lx, ly, W - lx, H - ly)]
    return regs + [random_region(rng, W, H) for _ in range(k)]


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p) for p in FIXTURES])
def test_fixture_regions_match_the_full_decode_and_the_oracle(ctx, torch, path):
    info, L, planes, quanta = fixture(path)
    W, H, nc = info.width, info.height, info.ncomponents
    dev = [ctx.upload(p) for p in planes]
    dq = ctx.upload(quanta)
    regs = _fixture_regions(W, H, info.scale_x, info.scale_y, np.random.default_rng(W * 7 + H))
    factors = [(info.factor_x[c], info.factor_y[c]) for c in range(nc)]
    for cosited in (0, 1):
        _, rect = O.decode(planes, list(quanta), factors, (W, H), cosited=bool(cosited), scale=(info.scale_x, info.scale_y))
        for color in (_lib.COLOR_RGB8, _lib.COLOR_YCC8):
            want = (O.unpack_rgb8 if color == _lib.COLOR_RGB8 else O.unpack_ycc8)(rect, nc).reshape(H, W, 3)
            full = full_batch(ctx, torch, L, 1, dev, [0] * 4, dq, 0, nc, cosited, color)[0].cpu().numpy()
            assert (full == want).all()
            host = _decode_regions(ctx, torch, L, dev, [0] * 4, dq, 0, nc, cosited, color, regs).images()
            for i, (x, y, w, h) in enumerate(regs):
                got = host[i].reshape(h, w, 3)
                assert (got == want[y:y + h, x:x + w]).all(), (os.path.basename(path), cosited, color, (x, y, w, h))
            # the single-image entry point, and a call whose only region is the whole image (the batch path)
            r = regs[5]
            one = torch.full((3 * r[2] * r[3],), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
            reg = _lib.Region(*r)
            assert _lib.lib().jpeg_amd_decode_region(ctx.handle, C.byref(L), plane_ptrs(dev), quanta.ctypes.data, nc, cosited, color,
                                                     C.byref(reg), one.data_ptr()) == 0
            assert (one.cpu().numpy().reshape(r[3], r[2], 3) == want[r[1]:r[1] + r[3], r[0]:r[0] + r[2]]).all()
            whole = _decode_regions(ctx, torch, L, dev, [0] * 4, dq, 0, nc, cosited, color, [(0, 0, W, H)])
            assert (whole.images()[0].reshape(H, W, 3) == want).all()


SYNTH_LAYOUTS = {"444": [(1, 1)] * 3, "422": [(2, 1), (1, 1), (1, 1)], "440": [(1, 2), (1, 1), (1, 1)],
                 "420": [(2, 2), (1, 1), (1, 1)], "y8": [(1, 1)]}
SYNTH_SIZES = [(1, 1), (7, 9), (17, 33), (1919, 1079), (4095, 17), (4096, 4096)]


def _random_regions(rng, W, H, n):
    return [random_region(rng, W, H) for _ in range(n)]


def _check_against_batch(ctx, torch, L, planes, coef_stride, dq, ntables, cosited, color, regs, chunk=16):
    out = _decode_regions(ctx, torch, L, planes, coef_stride, dq, ntables * 64, ntables, cosited, color, regs)
    n = len(regs)
    for i0 in range(0, n, chunk):
        m = min(chunk, n - i0)
        sub = [p[i0:] if s else p for p, s in zip(planes, coef_stride)]
        full = full_batch(ctx, torch, L, m, sub, coef_stride, dq[i0:], ntables * 64, ntables, cosited, color)
        for i in range(i0, i0 + m):
            x, y, w, h = regs[i]
            assert torch.equal(_crop(out, i, regs[i]), full[i - i0, y:y + h, x:x + w]), (i, regs[i])


@pytest.mark.parametrize("size", SYNTH_SIZES, ids=["%dx%d" % s for s in SYNTH_SIZES])
@pytest.mark.parametrize("name", sorted(SYNTH_LAYOUTS))
def test_synthetic_batch_of_200_regions(ctx, torch, name, size):
    W, H = size
    factors = SYNTH_LAYOUTS[name]
    L = c_layout(W, H, factors)
    units = plane_units(L)
    n = 200
    per_image = sum(64 * ux * uy for ux, uy in units)
    distinct = per_image * n * 2 <= (1 << 30)              # else all images share one set of coefficients (stride 0)
    planes = natural_planes_torch(units, n if distinct else 1, ctx.torch_device, seed=W * 31 + H)
    coef_stride = [64 * ux * uy if distinct else 0 for ux, uy in units] + [0] * (4 - len(units))
    ntables = 2 if L.nplanes == 3 else 1
    gen = torch.Generator(device=ctx.torch_device).manual_seed(W + H)
    dq = torch.randint(1, 24, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen)
    regs = _random_regions(np.random.default_rng(W * H + len(name)), W, H, n)
    color = _lib.COLOR_YCC8 if name == "440" else _lib.COLOR_RGB8
    _check_against_batch(ctx, torch, L, planes, coef_stride, dq, ntables, 0, color, regs)


@pytest.mark.parametrize("factors,cosited", [([(2, 2), (1, 1), (1, 1)], 1), ([(3, 1), (1, 1), (1, 1)], 0),
                                             ([(4, 2), (1, 1), (2, 1)], 0), ([(3, 3), (1, 1), (1, 1)], 0)],
                         ids=["420-cosited", "chroma-third", "chroma-quarter", "chroma-third-both"])
def test_fallback_layouts(ctx, torch, factors, cosited):
    W, H = 301, 187
    L = c_layout(W, H, factors)
    units = plane_units(L)
    n = 40
    planes = natural_planes_torch(units, n, ctx.torch_device, seed=11)
    coef_stride = [64 * ux * uy for ux, uy in units] + [0]
    gen = torch.Generator(device=ctx.torch_device).manual_seed(3)
    dq = torch.randint(1, 24, (n, 2, 64), dtype=torch.int16, device=ctx.torch_device, generator=gen)
    regs = _random_regions(np.random.default_rng(5), W, H, n - 2) + [(0, 0, W, H), (1, 0, W - 1, H)]
    _check_against_batch(ctx, torch, L, planes, coef_stride, dq, 2, cosited, _lib.COLOR_RGB8, regs)
    # and the oracle for image 0, region 0
    host = [p[0].cpu().numpy() for p in planes]
    q = dq[0].cpu().numpy().view(np.uint16)
    _, rect = O.decode(host, [q[min(p, 1)] for p in range(3)], factors, (W, H), cosited=bool(cosited))
    want = O.unpack_rgb8(rect, 3).reshape(H, W, 3)
    out = _decode_regions(ctx, torch, L, [p[0] for p in planes], [0] * 4, dq[0:1], 128, 2, cosited, _lib.COLOR_RGB8, regs[:1])
    x, y, w, h = regs[0]
    assert (_crop(out, 0, regs[0]).cpu().numpy() == want[y:y + h, x:x + w]).all()


@pytest.mark.parametrize("factors,cosited", [([(2, 2), (1, 1), (1, 1)], 0), ([(2, 2), (1, 1), (1, 1)], 1), ([(1, 1)], 0)],
                         ids=["420", "420-cosited-fallback", "y8"])
def test_batch_of_64_leaves_the_stride_gaps_alone(ctx, torch, factors, cosited):
    W, H = 333, 251
    L = c_layout(W, H, factors)
    units = plane_units(L)
    n = 64
    planes = natural_planes_torch(units, n, ctx.torch_device, seed=17)
    coef_stride = [64 * ux * uy for ux, uy in units] + [0] * (4 - len(units))
    ntables = 2 if L.nplanes == 3 else 1
    dq = torch.randint(1, 24, (n, ntables, 64), dtype=torch.int16, device=ctx.torch_device,
                       generator=torch.Generator(device=ctx.torch_device).manual_seed(9))
    regs = _random_regions(np.random.default_rng(19), W, H, n)
    out = _decode_regions(ctx, torch, L, planes, coef_stride, dq, ntables * 64, ntables, cosited, _lib.COLOR_RGB8, regs, gap=97)
    full = full_batch(ctx, torch, L, n, planes, coef_stride, dq, ntables * 64, ntables, cosited, _lib.COLOR_RGB8)
    for i, (x, y, w, h) in enumerate(regs):
        assert torch.equal(_crop(out, i, regs[i]), full[i, y:y + h, x:x + w])
    out.images()                                            # the sentinel in every byte of the stride gaps


def test_zero_images(ctx, torch):
    L = c_layout(64, 64, [(2, 2), (1, 1), (1, 1)])
    lib = _lib.lib()
    assert lib.jpeg_amd_decode_region_batch(ctx.handle, C.byref(L), 0, None, None, None, 0, 2, 0, _lib.COLOR_RGB8, None,
                                            None, 0) == 0


def test_invalid_calls_write_nothing_and_the_context_stays_usable(ctx, torch):
    W, H = 130, 77
    L = c_layout(W, H, [(2, 2), (1, 1), (1, 1)])
    units = plane_units(L)
    planes = natural_planes_torch(units, 4, ctx.torch_device, seed=23)
    coef_stride = [64 * ux * uy for ux, uy in units] + [0]
    dq = torch.randint(1, 24, (4, 2, 64), dtype=torch.int16, device=ctx.torch_device,
                       generator=torch.Generator(device=ctx.torch_device).manual_seed(1))
    good = [(3, 5, 40, 20), (0, 0, W, H), (W - 1, H - 1, 1, 1), (64, 1, 33, 70)]
    stride = 3 * W * H
    bad_sets = [
        good[:3] + [(-1, 0, 4, 4)], good[:3] + [(0, -1, 4, 4)], good[:3] + [(0, 0, 0, 4)], good[:3] + [(0, 0, 4, 0)],
        good[:3] + [(W - 3, 0, 4, 4)], good[:3] + [(0, H - 3, 4, 4)], good[:3] + [(5, 0, 2 ** 31 - 1, 4)],
        good[:3] + [(0, 5, 4, 2 ** 31 - 1)], [(-5, 0, 10, 10)] + good[1:],
    ]
    out = torch.full((4 * stride,), SENTINEL, dtype=torch.uint8, device=ctx.torch_device)
    for regs in bad_sets:
        for cosited in (0, 1):
            assert _region_batch(ctx, L, planes, coef_stride, dq, 128, 2, cosited, _lib.COLOR_RGB8, regs, out, stride) == \
                _lib.EINVAL, regs
    # a pixel stride below one image's bytes
    assert _region_batch(ctx, L, planes, coef_stride, dq, 128, 2, 0, _lib.COLOR_RGB8, good, out, 3 * W * H - 1) == _lib.EINVAL
    ctx.synchronize()
    assert bool((out == SENTINEL).all())
    # the next valid call on the same context
    got = _decode_regions(ctx, torch, L, planes, coef_stride, dq, 128, 2, 0, _lib.COLOR_RGB8, good)
    full = full_batch(ctx, torch, L, 4, planes, coef_stride, dq, 128, 2, 0, _lib.COLOR_RGB8)
    for i, (x, y, w, h) in enumerate(good):
        assert torch.equal(_crop(got, i, good[i]), full[i, y:y + h, x:x + w])


def test_8192_420_region_of_4096_at_1237_901(ctx, torch):
    W = H = 8192
    L = c_layout(W, H, [(2, 2), (1, 1), (1, 1)])
    units = plane_units(L)
    planes = natural_planes_torch(units, 1, ctx.torch_device, seed=29)
    dq = torch.randint(1, 24, (1, 2, 64), dtype=torch.int16, device=ctx.torch_device,
                       generator=torch.Generator(device=ctx.torch_device).manual_seed(2))
    r = (1237, 901, 4096, 4096)
    for color in (_lib.COLOR_RGB8, _lib.COLOR_YCC8):
        out = _decode_regions(ctx, torch, L, [p[0] for p in planes], [0] * 4, dq, 128, 2, 0, color, [r])
        full = full_batch(ctx, torch, L, 1, [p[0] for p in planes], [0] * 4, dq, 128, 2, 0, color)
        assert torch.equal(_crop(out, 0, r), full[0, 901:901 + 4096, 1237:1237 + 4096])


def test_python_api(ctx, torch):
    info, L, planes, quanta = fixture(os.path.join(GOLDEN, "decode", "color-sequential-1.jpg"))
    W, H = info.width, info.height
    layout = J.Layout("ycc8", {1: J.Component((2, 2), 0), 2: J.Component((1, 1), 1), 3: J.Component((1, 1), 2)})
    spectral = J.Spectral.from_host(ctx, (W, H), layout, planes, list(quanta), q=[0, 1, 2])
    for color in (J.RGB, J.YCbCr):
        for cosite in (False, True):
            full = spectral.decode(color, cosite).view(H, W, 3)
            for r in ((0, 0, W, H), (17, 3, 100, 41), (W - 1, H - 1, 1, 1)):
                got = spectral.decode(color, cosite, region=r)
                x, y, w, h = r
                assert got.shape == (w * h, 3)
                assert torch.equal(got.view(h, w, 3), full[y:y + h, x:x + w])
    with pytest.raises(J.JpegAmdError):
        spectral.decode(region=(W - 1, 0, 2, 1))
    # decode_regions: n images of one layout, per-image tables
    n = 5
    dev = [torch.stack([ctx.upload(p)] * n) for p in planes]
    qn = np.stack([quanta] * n)
    regs = [(0, 0, W, H), (1, 2, 3, 4), (100, 200, 150, 77), (W - 20, H - 30, 20, 30), (5, 5, 1, 1)]
    outs = J.decode_regions(ctx, (W, H), layout, dev, qn, regs, q=[0, 1, 2])
    full = spectral.decode(J.RGB).view(H, W, 3)
    assert len(outs) == n
    for o, (x, y, w, h) in zip(outs, regs):
        assert tuple(o.shape) == (h, w, 3)
        assert torch.equal(o, full[y:y + h, x:x + w])
    # an empty batch is no images, from decode_regions as from decode_views
    none = [p[:0] for p in dev]
    assert J.decode_regions(ctx, (W, H), layout, none, qn[:0], np.zeros((0, 4)), q=[0, 1, 2]) == []
    assert J.decode_views(ctx, (W, H), layout, none, qn[:0], np.zeros((0, 5)), q=[0, 1, 2]) == []
