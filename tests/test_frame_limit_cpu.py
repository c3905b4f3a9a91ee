"""The inputs of tests/test_gpu_frame_limit.py, checked with the references alone (no GPU): a GPU test at the 65535-pixel frame
limit proves something only if the far end of its expected output is neither clamped nor a copy of what a wrapped coordinate
would read.  For every decode and resample case of tests/_frame_limit.py:

  * INTERIOR SHARE: of the last 256 columns (widest) or rows (tallest) of the reference output, at least half of the samples lie
    strictly between 0 and the precision's maximum;
  * WRAPPED POSITIONS: that window differs in more than 90 % of its samples from the reference output 16384, 32768 and 49152
    positions in front of it along the long side.  Where the output is shorter than the source along that side (scaled decode,
    the reductions) the three distances shrink with it -- they stay the same distances in the source; the 320-pixel windows
    of the translation and the perspective map are compared with the same map moved by the three distances;
  * the case tables hold what the issue lists, and the generic cases' coordinates are as large as the frame allows.

A single-plane image decodes to r = g = b = y and cb = cr = 128: its one informative channel is checked.

The shares found, the smallest over the cases of a family (interior share, differing share; each test prints its own):
  fused 8-bit decode, RGB      0.654  0.931   (4:4:4 widest)
  fused 8-bit decode, YCbCr    0.782  0.970   (y8)
  generic, `wide` inputs       0.687  0.931   (case 6 centred, 65535 x 25)
  generic, the walk's 4:2:0    0.727  0.942
  tile family, RGB             0.704  0.946   (4:1:1 widest, denominator 1)
  tile family, YCbCr           0.793  0.961
  resize                       0.979  0.964   (random source bytes; the antialiased reduction to 5 x 4096 differs least)
  warp and projective maps     0.966  0.993
"""
import numpy as np
import pytest

import _frame_limit as FL
import _generic_cases as GC
import _project_ref as P


def far_end(image, orient, top):
    """-> (interior share of the far-end window, the smallest share of samples that differ from a wrapped position)."""
    a = FL.along(np.asarray(image), orient)
    long = a.shape[0]
    far = a[long - FL.WINDOW:]
    interior = float(((far > 0) & (far < top)).mean())
    wraps = [int(round(k * long / 65536.0)) for k in FL.WRAPS]
    assert FL.WINDOW <= wraps[0] and wraps[2] + FL.WINDOW <= long
    differ = min(float((far != a[long - FL.WINDOW - s:long - s]).mean()) for s in wraps)
    return interior, differ


def hold(family, what, interior, differ):
    print(f"{family}: {what}: interior {interior:.3f}, differing {differ:.3f}")
    assert interior >= 0.5, (family, what, interior)
    assert differ > 0.9, (family, what, differ)


def test_the_case_tables_hold_what_the_issue_lists():
    assert FL.LONGS == (65535, 65529) and FL.ORIENTS == ("widest", "tallest")
    assert [65535 % m for m in (8, 16, 24, 32, 64, 128)] == [7, 15, 15, 31, 63, 127] and 65529 % 8 == 1
    assert [FL.extent((s, s), 65535, "widest")[1] for s in (1, 2, 3, 4)] == [9, 17, 25, 33]
    assert FL.extent((4, 1), 65529, "tallest") == (33, 65529) and FL.extent((4, 1), 65529, "widest") == (65529, 9)
    assert FL.FUSED8 == [("y8", 0), ("444", 0), ("422", 0), ("422", 1), ("440", 0)] and len(FL.FUSED8_CASES) == 20
    assert any(FL.fused8_images(long) == 2 for long in FL.LONGS)
    assert FL.GENERIC == (1, 3, 5, 6, 10) and len(FL.GENERIC_CASES) == 40
    assert [(GC.case(n).scale, GC.case(n).precision) for n in FL.GENERIC] == [((4, 1), 8), ((4, 4), 16), ((3, 3), 12), ((1, 3), 16), ((4, 2), 16)]
    assert FL.TILE_LAYOUTS == ("y8", "420", "411") and FL.DENOMS == (2, 4, 8) and len(FL.TILE_CASES) == 12
    assert len(FL.SPECTRAL_CASES) == 8 and {name for name, _, _ in FL.SPECTRAL_CASES} == {"y8", "420"}
    assert {name: f[2] for name, f in FL.FILTERS.items()} == {"bilinear": 4096, "antialias": 4096, "bicubic": 8192}
    assert len(FL.RESIZE_CASES) == 12 and len(FL.MAP_CASES) == 3 * 2 * 2 * 2
    assert FL.source("widest").shape == (9, 65535, 3) and FL.source("tallest").shape == (65535, 9, 3)


def _informative(name, image):
    return image[..., :1] if name == "y8" else image


@pytest.mark.parametrize("name,cosited,long,orient", FL.FUSED8_CASES, ids=lambda v: str(v))
def test_fused_8_bit_inputs(name, cosited, long, orient):
    size = FL.extent(FL.scale_of(FL.LAYOUTS[name]), long, orient)
    n = FL.fused8_images(long)
    for i in range(n):
        for color, image in FL.decoded8(name, size, 1, cosited, i, n).items():
            assert image.shape == (size[1], size[0], 3)
            hold("fused", (name, cosited, size, i, FL.COLORS[color]), *far_end(_informative(name, image), orient, 255))
    if n == 2:
        a, b = (FL.decoded8(name, size, 1, cosited, i, n) for i in range(2))
        assert all((a[k] != b[k]).mean() > 0.9 or name == "y8" for k in a)


@pytest.mark.parametrize("number,cosite,long,orient", FL.GENERIC_CASES, ids=lambda v: str(v))
def test_generic_inputs_and_numerators(number, cosite, long, orient):
    c = GC.case(number)
    size = FL.extent(c.scale, long, orient)
    hold("generic", (number, cosite, size), *far_end(FL.generic_rect(number, size, cosite), orient, (1 << c.precision) - 1))
    # the coordinates: a centred axis of thirds or quarters reaches a + b t = 2 * 65534 - 2 = 131066 (65528: 131054) along the long
    # side; a cosited one a + b t = t, which the frame bounds by 65534 -- more than 100 000 cannot be asked of it
    axis = 0 if orient == "widest" else 1
    found = [n for _, ax, f, s, n in FL.numerators(c, size, cosite) if ax == axis and f != s and s in (3, 4)]
    if c.scale[axis] in (3, 4):
        assert found, (number, orient)
    for n in found:
        assert n > (65000 if cosite else 100000), (number, cosite, orient, n)
        assert n < 1 << 26                                    # the range div_trunc_small's comment claims


def test_the_walk_case_inputs():
    size = FL.extent(FL.WALK.scale, FL.LONGS[0], "tallest")
    assert size == (17, 65535) and FL.WALK_IMAGES * -(-size[1] // 64) * -(-size[0] // 128) > 2048
    for i in range(FL.WALK_IMAGES):
        hold("generic walk", i, *far_end(FL.generic_rect(0, size, False, i), "tallest", 4095))


@pytest.mark.parametrize("name,long,orient", FL.TILE_CASES, ids=lambda v: str(v))
def test_tile_family_inputs(name, long, orient):
    scale = FL.scale_of(FL.LAYOUTS[name])
    size = FL.extent(scale, long, orient)
    for denom in (1,) + FL.DENOMS:
        for color, image in FL.decoded8(name, size, denom).items():
            hold("tile", (name, size, denom, FL.COLORS[color]), *far_end(_informative(name, image), orient, 255))
    W, H = size
    for x, y, w, h in FL.far_regions(size, scale, orient):
        assert 0 <= x and 0 <= y and w >= 1 and h >= 1 and x + w <= W and y + h <= H
    last, pixel, seam, wrap = FL.far_regions(size, scale, orient)
    assert (last[0] + last[2], last[1] + last[3]) == size and 200 in last[2:]
    assert pixel == (W - 1, H - 1, 1, 1)
    axis = 0 if orient == "widest" else 1
    assert wrap[axis] < 32768 < wrap[axis] + wrap[axis + 2] and FL.wrap_view(size, orient)[1][axis] < 32768
    mcu = 8 * scale[axis]
    assert seam[axis] // mcu < (seam[axis] + seam[axis + 2] - 1) // mcu == (size[axis] - 1) // mcu
    for denom in (1,) + FL.DENOMS:
        d, (x, y, w, h) = FL.far_view(size, denom, orient)
        n = 8 // d
        assert (x + w, y + h) == ((W * n + 7) // 8, (H * n + 7) // 8) and max(w, h) == 150      # across a 128-pixel tile seam


def test_the_mixed_and_the_composed_case():
    assert [size for _, size, _ in FL.MIXED] == [(65535, 17), (9, 65535), (17, 33)]
    for name, size, (denom, (x, y, w, h)) in FL.MIXED:
        n = 8 // denom
        assert x + w <= (size[0] * n + 7) // 8 and y + h <= (size[1] * n + 7) // 8
    name, size, (denom, r), (out_w, out_h) = FL.COMPOSED
    assert r[0] + r[2] == (size[0] * (8 // denom) + 7) // 8 and r[2] == 300
    for color, image in FL.composed().items():
        assert image.shape == (out_h, out_w, 3)
        assert ((image > 0) & (image < 255)).mean() >= 0.5


@pytest.mark.parametrize("name,orient,k", FL.RESIZE_CASES, ids=lambda v: str(v))
def test_resize_inputs(name, orient, k):
    out_w, out_h = FL.resize_targets(name, orient)[k]
    src = FL.source(orient)
    long_out, long_src = max(out_w, out_h), max(src.shape[:2])
    assert long_src == 65535 and (long_out == 65535 if k == 0 else long_out == FL.FILTERS[name][2])
    ratio = np.float32(long_src) / np.float32(long_out)
    assert ratio == 1 or {"antialias": 15.9 < ratio < 16, "bicubic": 7.9 < ratio < 8, "bilinear": ratio > 15.9}[name]
    hold("resize", (name, orient, (out_w, out_h)), *far_end(FL.resized(name, orient, k), orient, 255))


@pytest.mark.parametrize("name,orient,filt,edge", FL.MAP_CASES, ids=lambda v: str(v))
def test_map_inputs(name, orient, filt, edge):
    m, (out_w, out_h) = FL.mapped(name, orient)
    assert P.accepted(m, out_w, out_h)
    want = FL.projected(name, orient, filt, edge)
    if name == "quarter-turn":
        assert max(out_w, out_h) == 65535 and (out_w > out_h) == (orient == "tallest")
        hold("maps", (name, orient, filt, edge), *far_end(want, "widest" if out_w > out_h else "tallest", 255))
        return
    interior = float(((want > 0) & (want < 255)).mean())
    differ = min(float((want != FL.projected(name, orient, filt, edge, shift)).mean()) for shift in FL.WRAPS)
    hold("maps", (name, orient, filt, edge), interior, differ)
    # FILL and REPLICATE both bind: the window runs past the image's end
    other = FL.projected(name, orient, filt, "replicate" if edge == "fill" else "fill")
    assert (want != other).any()
    sx, sy = P.coordinates(m, FL.source(orient).shape[1], FL.source(orient).shape[0], out_w, out_h)
    far = sx if orient == "widest" else sy
    assert far.max() >= 65535 and far.min() > 65535 - 400
