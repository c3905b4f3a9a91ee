"""What the tests of the chunk seam of the resized and tensor decodes share (test_resample_chunks_cpu, test_gpu_resample_chunks):
the chunk rule restated, and the scenarios -- calls whose compact views pass 2^30 bytes while next to nothing is decoded, because
the rule counts stride x images and one large view sets the stride of its whole chunk.  Importing this needs no GPU, no torch and
no library: the views of the mapped calls come from the Python mirrors of jpeg_amd_warp_view and jpeg_amd_project_view.

The rule (include/jpeg_amd.h, "resized decode" and "mixed calls": "each view compact, the views of a chunk at a stride of the
chunk's largest, chunks of consecutive images of at most 1 GiB"): a chunk takes the consecutive images that fit, and one at least.

A scenario keeps three things in step with its chunks, so that a host that plans chunk c from the images of chunk 0 (a dropped
`+ i0`) still stays inside every buffer: the image at place j of EVERY chunk has the plane count of the image at place j of the
first chunk, it takes the one-image fallback only where that one does, and its denominator is no smaller (a view of a smaller
scaled image lies inside the larger one).  What differs is what such a host gets wrong: the pixels."""
import math

import numpy as np

import _orient as E
import _project_ref as P
import _warp_ref as W

F32 = np.float32
LIMIT = 1 << 30                                             # kResizeChunkBytes
BIG = (2048, 1536)
F311 = [(3, 1), (1, 1), (1, 1)]                             # no tile kernel takes a factor of 3: the one-image fallback
# the device images a mixed call's entries alias: name -> (the layout's name in _calls.FUSED or its factors, (w, h))
KINDS = {"A": ("y8", BIG), "B": ("420", BIG), "y8": ("y8", (131, 257)), "444": ("444", (200, 120)), "422": ("422", (300, 140)),
         "440": ("440", (157, 93)), "420": ("420", (300, 140)), "311": (F311, (150, 90))}
TAIL = 4                                                    # images of the last chunk
LARGE0, LARGE1_AT, FALLBACK_AT = 60, 4, 17                  # the first large view; the place of the second and of the fallback images in their chunks


def expected_chunks(views, limit=LIMIT):
    """views: (denom, x, y, width, height) per image -> [(i0, m, stride)]."""
    size = [3 * int(v[3]) * int(v[4]) for v in views]
    chunks, i0 = [], 0
    while i0 < len(size):
        m, stride = 1, size[i0]
        while i0 + m < len(size) and max(stride, size[i0 + m]) * (m + 1) <= limit:
            stride = max(stride, size[i0 + m])
            m += 1
        chunks.append((i0, m, stride))
        i0 += m
    return chunks


def scaled(size, denom):
    return (size[0] + denom - 1) // denom, (size[1] + denom - 1) // denom


class Places:
    """The images of a call of three chunks whose first two hold one large view each, of s0 and of s1 bytes: chunk c begins at
    starts[c], the large views are images `large`, the last chunk's largest is image `third`."""

    def __init__(self, s0, s1):
        per0, per1 = LIMIT // s0, LIMIT // s1
        assert per0 > LARGE0 and FALLBACK_AT < per1 <= per0       # (no chunk is longer than the first: every place of one is a place of it)
        self.starts = (0, per0, per0 + per1)
        self.n = self.starts[2] + TAIL
        self.large = (LARGE0, per0 + LARGE1_AT)
        self.third = self.starts[2]
        self.fallback = (FALLBACK_AT, per0 + FALLBACK_AT)   # the second one is the fallback image of a chunk that is not the first

    def chunk(self, i):
        return sum(1 for s in self.starts[1:] if i >= s)

    def kind(self, i):
        """Which device image entry i aliases: by its place j in its chunk, one plane where j % 5 == 0 and three elsewhere."""
        if i == self.large[0] or i == self.third:
            return "A"
        if i == self.large[1]:
            return "B"
        if i in self.fallback:
            return "311"
        j = i - self.starts[self.chunk(i)]
        return (("A", "y8", "A")[i % 3], "444", "422", "440", ("B", "420")[i % 2])[j % 5]

    def denom(self, i):
        """1, 2, 4, 8 by the place in the chunk, doubled per chunk: never smaller than at the same place of the first chunk."""
        if i in self.large:
            return 1
        if i == self.third:
            return 2
        c = self.chunk(i)
        return min(8, (1, 2, 4, 8)[(i - self.starts[c]) % 4] << c)

    def subset(self):
        """The images of the independent mirrors: the first and the last of every chunk, both large views, the fallback image
        of the second chunk, every image of the last chunk."""
        ends = [s - 1 for s in self.starts[1:]] + [self.n - 1]
        return sorted(set(self.starts) | set(ends) | set(self.large) | {self.fallback[1]} | set(range(self.starts[2], self.n)))


def orientations(n):
    return [1 + i % 8 for i in range(n)]


def flips(n):
    return [i % 2 for i in range(n)]


# ---- the mixed calls with views ---------------------------------------------------------------------------------------------------------

NEARLY = (1, 0, 3, BIG[0], BIG[1] - 6)                      # 9 400 320 bytes: 114 of them fit, 115 do not
WHOLE = (1, 0, 0, BIG[0], BIG[1])                           # 9 437 184 bytes: 113 fit, 114 do not
MIXED = Places(3 * NEARLY[3] * NEARLY[4], 3 * WHOLE[3] * WHOLE[4])


def mixed_view(pl, i):
    """Nearly a whole view at the first large image, the whole one at the second, the whole image at 1/2 at the head of the last chunk;
    else a rectangle of at most 160 x 60 somewhere in the scaled image."""
    if i in pl.large:
        return NEARLY if i == pl.large[0] else WHOLE
    d = pl.denom(i)
    ws, hs = scaled(KINDS[pl.kind(i)][1], d)
    if i == pl.third:
        return (d, 0, 0, ws, hs)
    w, h = min(ws, 20 + (37 * i) % 141), min(hs, 8 + (11 * i) % 53)
    return (d, (53 * i) % (ws - w + 1), (29 * i) % (hs - h + 1), w, h)


def mixed_views(pl=MIXED):
    return [mixed_view(pl, i) for i in range(pl.n)]


# ---- the refused call: two chunks, the only view past the antialiasing filter's 16 in the second ------------------------------------------

REFUSED_CANVAS = (120, 96)
REFUSED_N, REFUSED_AT = 140, 128                            # (image 128 is a "B" by Places.kind)


def refused_views():
    """MIXED's small views; image 60 is 1920 x 1536 (16 times the canvas on both axes: inside the limit; 121 of them fit), and
    image 128 the whole 2048 x 1536 (17.07 times: past it)."""
    views = [mixed_view(MIXED, i) for i in range(REFUSED_N)]
    views[LARGE0] = (1, 64, 0, 1920, 1536)
    views[MIXED.large[1]] = (1, 100, 100, 150, 50)
    assert MIXED.kind(REFUSED_AT) == "B"
    views[REFUSED_AT] = WHOLE
    return views


# ---- the uniform calls ------------------------------------------------------------------------------------------------------------------

UNIFORM_N = 120


def uniform_views():
    """One y8 layout of 2048 x 1536: the whole view at image 60, the whole image at 1/2 at image 118, small rectangles elsewhere:
    [0, 113) and [113, 120)."""
    views = []
    for i in range(UNIFORM_N):
        d = (1, 2, 4, 8)[i % 4]
        ws, hs = scaled(BIG, d)
        w, h = 20 + (37 * i) % 141, 8 + (11 * i) % 53
        views.append((d, (53 * i) % (ws - w + 1), (29 * i) % (hs - h + 1), w, h))
    views[LARGE0] = WHOLE
    views[118] = (2, 0, 0) + scaled(BIG, 2)
    return views


def uniform_subset():
    return [0, LARGE0, 112] + list(range(113, UNIFORM_N))


# ---- the mapped calls: the view is the canvas's footprint ---------------------------------------------------------------------------------

MAPPED_CANVAS = (1300, 8)                                   # long and thin: laid on a diagonal its footprint is most of the image


def _rotation(angle):
    a = math.radians(angle)
    return np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])


def affine(upright, angle, step, canvas=MAPPED_CANVAS):
    """The canvas centre onto the centre of the upright image, rotated by `angle` degrees, `step` source pixels per output
    pixel.  float32 [6]"""
    lin = step * _rotation(angle)
    t = np.array([upright[0] / 2.0, upright[1] / 2.0]) - lin @ np.array([canvas[0] / 2.0, canvas[1] / 2.0])
    return np.array([lin[0, 0], lin[0, 1], t[0], lin[1, 0], lin[1, 1], t[1]], np.float64).astype(F32)


def keystone(upright, angle, step, pulls, canvas=MAPPED_CANVAS):
    """The canvas onto the rectangle of step * canvas about the centre of the upright image, rotated by `angle`, each corner
    pulled towards the centre by pulls[k] (at most 0.075) of its distance from it: a mild keystone, whose smallest local step
    stays above two thirds of `step` (Mapped checks the denominators it leads to).  float32 [9]"""
    rot, centre = _rotation(angle), np.array([upright[0] / 2.0, upright[1] / 2.0])
    half = [(-0.5, -0.5), (0.5, -0.5), (0.5, 0.5), (-0.5, 0.5)]
    src = [tuple(centre + (1.0 - pulls[k]) * (rot @ np.array([hx * step * canvas[0], hy * step * canvas[1]]))) for k, (hx, hy) in enumerate(half)]
    out = [(0, 0), (canvas[0], 0), (canvas[0], canvas[1]), (0, canvas[1])]
    return P.homography(src, out).reshape(9).astype(F32)


class Mapped:
    """A warped (projective=False) or a projected call of three chunks.  The two large views are the footprints of the canvas
    along the diagonal of a 2048 x 1536 image at a step of 1.9 (denominator 1), the first one 4 degrees off it; the head of the
    last chunk reads the image at 1/2; every other image reads a thin, slightly tilted strip at its place's denominator."""

    def __init__(self, projective):
        self.projective = projective
        rng = np.random.default_rng(41 if projective else 40)
        self.pulls = rng.uniform(0.0, 0.075, (1024, 4))
        first = self._view("A", orientations(LARGE0 + 1)[LARGE0], self._large(LARGE0, -4.0))
        per0 = LIMIT // (3 * first[3] * first[4])
        at = per0 + LARGE1_AT
        second = self._view("B", orientations(at + 1)[at], self._large(at, 0.0))
        self.places = Places(3 * first[3] * first[4], 3 * second[3] * second[4])
        assert self.places.large == (LARGE0, at)
        pl = self.places
        self.orient = orientations(pl.n)
        self.matrices = np.stack([self._matrix(i) for i in range(pl.n)])
        self.views = [self._view(pl.kind(i), self.orient[i], self.matrices[i]) for i in range(pl.n)]
        assert [v[0] for v in self.views] == [pl.denom(i) for i in range(pl.n)]

    def _make(self, upright, angle, step, i):
        return keystone(upright, angle, step, self.pulls[i]) if self.projective else affine(upright, angle, step)

    def _large(self, i, off):
        uw, uh = E.oriented_size(orientations(i + 1)[i], *BIG)
        return self._make((uw, uh), math.degrees(math.atan2(uh, uw)) + off, 1.9, i)

    def _matrix(self, i):
        pl = self.places
        if i in pl.large:
            return self._large(i, -4.0 if i == pl.large[0] else 0.0)
        upright = E.oriented_size(self.orient[i], *KINDS[pl.kind(i)][1])
        if i == pl.third:
            return self._make(upright, 20.0, 2.4 if not self.projective else 3.0, i)
        return self._make(upright, float((7 * i) % 15 - 7), (1.5 if self.projective else 1.2) * pl.denom(i), i)

    def _view(self, kind, o, m):
        w, h = KINDS[kind][1]
        mirror = P.project_view if self.projective else W.warp_view
        return mirror(w, h, o, m, *MAPPED_CANVAS)[0]


_MAPPED = {}


def mapped(projective):
    if projective not in _MAPPED:
        _MAPPED[projective] = Mapped(projective)
    return _MAPPED[projective]


def check_places(pl, views):
    """What every test of a three-chunk scenario assumes of it: the split, the strides that differ pairwise, each set by the
    view it is meant to be set by, and the three things a scenario keeps in step with its chunks."""
    chunks = expected_chunks(views)
    assert [(i0, m) for i0, m, _ in chunks] == [(pl.starts[0], pl.starts[1]), (pl.starts[1], pl.starts[2] - pl.starts[1]), (pl.starts[2], TAIL)], chunks
    strides = [s for _, _, s in chunks]
    assert len(set(strides)) == 3 and strides == [3 * views[i][3] * views[i][4] for i in pl.large + (pl.third,)], strides
    assert pl.chunk(pl.large[0]) == 0 and pl.chunk(pl.large[1]) == 1 and pl.chunk(pl.fallback[1]) == 1
    planes = lambda i: 1 if KINDS[pl.kind(i)][0] == "y8" else 3
    for c in (1, 2):
        for i in range(pl.starts[c], pl.n if c == 2 else pl.starts[c + 1]):
            j = i - pl.starts[c]
            assert planes(i) == planes(j) and (pl.kind(i) != "311" or pl.kind(j) == "311") and views[i][0] >= views[j][0], (i, j)
    assert {v[0] for v in views} == {1, 2, 4, 8}
    return chunks
