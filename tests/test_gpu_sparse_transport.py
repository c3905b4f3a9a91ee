"""The sparse coefficient transport on the MI355X, kernel by kernel: k_sparsify through jpeg_amd_spectral_sparsify_batch against
the numpy statement of the writer's contract (_sparse_ref.py, which test_sparse_ref_cpu.py holds against both host coders), and
k_expand_sparse and k_expand_mixed on records CONSTRUCTED on the host -- rows in reversed and shuffled arena order, poison
between them, 64-entry rows, the value 0x8000, absent blocks -- against the numpy readers (_sparse.expand,
_files.expand_mirror).  Three images per call, every stride larger than needed, and a sentinel in every word the kernels must
leave alone: descriptors, arenas, counts, planes and the gaps between the images are compared whole.

THE ORDER RULE of the round trips: a record the device wrote is copied to the host and passes the host comparison BEFORE a
device reader is given it.  A wrong record then fails an assert; it never sends a reader walking for a flag that is not there."""
import ctypes as C
import functools

import numpy as np
import pytest

import _files as F
import _sparse
import _sparse_ref as R
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from _calls import plane_units
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

N = 3                                                          # images per call
LEAD, GAP = 64, 192                                            # int16 in front of a plane buffer's first image / behind every image
DESC_LEAD, DESC_GAP, ARENA_LEAD, ARENA_GAP = 5, 5, 3, 7        # uint32, likewise
HEADS = (1, 4, 8)
NAMES = list(R.LAYOUTS)


@functools.lru_cache(maxsize=None)
def images_of(name, safe=False, equal=False):
    """(the planes of the three images, their reference rows); shared, and left as they are."""
    images = R.three_images(name, 20, safe, equal)
    return images, [R.sparsify_rows(p) for p in images]


def total(rows):
    return sum(r.size for r in rows)


def to_device(ctx, torch, host):
    return torch.from_numpy(host.view(np.int32 if host.dtype == np.uint32 else host.dtype)).to(ctx.torch_device)


class Planes:
    """Per plane one device buffer of int16: LEAD sentinels, then the three images GAP sentinels apart."""

    def __init__(self, ctx, torch, L, images=None):
        self.units = plane_units(L)
        self.stride = [64 * ux * uy + GAP for ux, uy in self.units]
        self.dev = [to_device(ctx, torch, h) for h in self.host(images)]
        self.ptrs = [d.data_ptr() + 2 * LEAD for d in self.dev]
        assert all(p % 128 == 0 for p in self.ptrs)

    def host(self, images):
        """What the buffers hold with `images` in place (None: nothing but the sentinel)."""
        out = []
        for p, ((ux, uy), stride) in enumerate(zip(self.units, self.stride)):
            h = np.full(LEAD + N * stride, F.SENTINEL16, np.int16)
            for i in range(N if images is not None else 0):
                h[LEAD + i * stride:LEAD + i * stride + 64 * ux * uy] = images[i][p].ravel()
            out.append(h)
        return out

    def image_ptrs(self, i):
        return [ptr + 2 * i * stride for ptr, stride in zip(self.ptrs, self.stride)]

    def assert_hold(self, images, what):
        for p, (d, w) in enumerate(zip(self.dev, self.host(images))):
            g = d.cpu().numpy()
            assert (g == w).all(), (what, "plane", p, np.flatnonzero(g != w)[:4].tolist())


class Record:
    """One device buffer of uint32 with the records of the three images: DESC_LEAD sentinels, the descriptors of the images
    desc_stride apart, ARENA_LEAD sentinels, their arenas entries_stride apart -- and the counts in a buffer of their own,
    a sentinel on either side."""

    def __init__(self, ctx, torch, blocks, capacity, desc=None, arenas=None):
        self.blocks, self.capacity = blocks, capacity
        self.desc_stride, self.entries_stride = blocks + DESC_GAP, capacity + ARENA_GAP
        self.desc_at = [DESC_LEAD + i * self.desc_stride for i in range(N)]
        first = DESC_LEAD + N * self.desc_stride + ARENA_LEAD
        self.entries_at = [first + i * self.entries_stride for i in range(N)]
        self.before = np.full(first + N * self.entries_stride, R.SENTINEL32, np.uint32)
        for i in range(N if desc is not None else 0):
            self.before[self.desc_at[i]:self.desc_at[i] + blocks] = desc[i]
            self.before[self.entries_at[i]:self.entries_at[i] + arenas[i].size] = arenas[i]
        self.dev = to_device(ctx, torch, self.before)
        self.dev_count = to_device(ctx, torch, np.full(N + 2, R.SENTINEL32, np.uint32))
        self.ptr = self.dev.data_ptr()
        self.desc_ptr, self.entries_ptr = self.ptr + 4 * self.desc_at[0], self.ptr + 4 * self.entries_at[0]
        self.count_ptr = self.dev_count.data_ptr() + 4

    def download(self):
        self.now = self.dev.cpu().numpy().view(np.uint32)
        counts = self.dev_count.cpu().numpy().view(np.uint32)
        assert counts[0] == R.SENTINEL32 and counts[-1] == R.SENTINEL32
        self.counts = [int(c) for c in counts[1:-1]]
        # nothing outside the descriptors and the arenas [0, capacity) of the three images is changed
        mine = np.zeros(self.now.size, bool)
        for i in range(N):
            mine[self.desc_at[i]:self.desc_at[i] + self.blocks] = True
            mine[self.entries_at[i]:self.entries_at[i] + self.capacity] = True
        stray = np.flatnonzero(~mine & (self.now != self.before))
        assert stray.size == 0, ("written outside the records", stray[:4].tolist())
        return self

    def desc(self, i):
        return self.now[self.desc_at[i]:self.desc_at[i] + self.blocks]

    def arena(self, i):
        return self.now[self.entries_at[i]:self.entries_at[i] + self.capacity]

    def assert_complete(self, i, want):
        """Image i's record is what the contract promises of an image that fits."""
        count, desc, arena = self.counts[i], self.desc(i), self.arena(i)
        assert count == total(want), (i, count, total(want))
        assert count <= self.capacity
        got = R.rows_of(desc, arena[:count])
        bad = [b for b, (g, w) in enumerate(zip(got, want)) if g is None or not np.array_equal(g, w)]
        assert not bad, (i, "blocks", bad[:4], [(got[b], want[b]) for b in bad[:1]])
        R.assert_tiles(desc, got, count)
        assert (arena[count:] == R.SENTINEL32).all(), (i, "written behind the count")


def sparsify(ctx, torch, L, images, capacity):
    """jpeg_amd_spectral_sparsify_batch on the three images -> the Record, downloaded, its guards checked."""
    src = Planes(ctx, torch, L, images)
    rec = Record(ctx, torch, R.blocks_of(L), capacity)
    st = _lib.lib().jpeg_amd_spectral_sparsify_batch(ctx.handle, C.byref(L), N, _lib.ptr_array(src.ptrs), _lib.size_array(src.stride),
                                                     rec.desc_ptr, rec.desc_stride, rec.entries_ptr, rec.entries_stride, capacity,
                                                     rec.count_ptr)
    assert st == 0
    ctx.synchronize()
    src.assert_hold(images, "the source")
    return rec.download()


def checked_record(ctx, torch, name, safe=False):
    """The device's record of images_of(name) at capacity 64 * blocks, every image through the host comparison: what the
    round trips may hand to a reader."""
    L = R.layout(name)
    images, rows = images_of(name, safe)
    rec = sparsify(ctx, torch, L, images, 64 * R.blocks_of(L))
    for i in range(N):
        rec.assert_complete(i, rows[i])
    return L, images, rec


def expand_batch(ctx, torch, L, rec):
    out = Planes(ctx, torch, L)
    st = _lib.lib().jpeg_amd_spectral_expand_batch(ctx.handle, C.byref(L), N, rec.desc_ptr, rec.desc_stride, rec.entries_ptr,
                                                   rec.entries_stride, None, _lib.ptr_array(out.ptrs), _lib.size_array(out.stride))
    assert st == 0
    ctx.synchronize()
    return out


def expand_mixed(ctx, torch, L, rec, heads):
    """One launch over the three images, image i at heads[i], whole windows."""
    out = Planes(ctx, torch, L)
    items = (_lib.ExpandItem * N)()
    for i, it in enumerate(items):
        it.layout, it.head, it.desc_at, it.entries_at = L, heads[i], rec.desc_at[i], rec.entries_at[i]
        for p, (w, ptr) in enumerate(zip(F.whole_windows(L), out.image_ptrs(i))):
            it.d_coef[p], it.window[p] = ptr, _lib.Region(*w)
    assert _lib.lib().jpeg_amd_spectral_expand_mixed(ctx.handle, N, items, rec.ptr) == 0
    ctx.synchronize()
    return out


# ---- the writer ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_writer_with_room_to_spare(ctx, torch, name):
    L = R.layout(name)
    images, rows = images_of(name)
    rec = sparsify(ctx, torch, L, images, 64 * R.blocks_of(L))
    for i in range(N):
        rec.assert_complete(i, rows[i])


@pytest.mark.parametrize("name", NAMES)
def test_writer_at_the_exact_fit(ctx, torch, name):
    L = R.layout(name)
    images, rows = images_of(name, equal=True)
    cap = total(rows[0])
    assert [total(r) for r in rows] == [cap] * N
    rec = sparsify(ctx, torch, L, images, cap)
    assert rec.counts == [cap] * N
    for i in range(N):
        rec.assert_complete(i, rows[i])


@pytest.mark.parametrize("name", NAMES)
def test_writer_with_an_image_that_overflows_between_two_that_fit(ctx, torch, name):
    L = R.layout(name)
    fit, rows = images_of(name, equal=True)
    cap = total(rows[0])
    over = R.top_up([p.copy() for p in fit[1]], 1)                 # one more nonzero coefficient than the arena holds
    images, rows = [fit[0], over, fit[2]], [rows[0], R.sparsify_rows(over), rows[2]]
    rec = sparsify(ctx, torch, L, images, cap)                     # (download: nothing at or beyond cap is changed)
    assert rec.counts == [cap, cap + 1, cap]
    rec.assert_complete(0, rows[0])
    rec.assert_complete(2, rows[2])
    desc, arena = rec.desc(1), rec.arena(1)
    unwritten = 0
    for b, (at, want) in enumerate(zip(desc, rows[1])):
        if at == R.SENTINEL32:
            unwritten += 1
            continue
        assert int(at) + want.size <= cap, (b, int(at))
        assert np.array_equal(arena[at:at + want.size], want), b
    assert unwritten >= 1
    # what is written tiles nothing twice: the written rows are pairwise disjoint
    spans = sorted((int(at), int(at) + want.size) for at, want in zip(desc, rows[1]) if at != R.SENTINEL32)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


# ---- the readers, on constructed records ----------------------------------------------------------------------------------------

def constructed(ctx, torch, name, order, gap):
    """Records of images_of(name) with block b absent where b % 7 == 3, rows placed as `order` says with `gap` poison words
    between them.  -> (L, Record on the device, per image the host record [descriptors, arena])"""
    L = R.layout(name)
    _, rows = images_of(name)
    desc, arenas = [], []
    for i in range(N):
        mine = [None if b % 7 == 3 else r for b, r in enumerate(rows[i])]
        blocks = list(range(len(mine)))
        if order == "reversed":
            blocks.reverse()
        else:
            np.random.Generator(np.random.PCG64(50 + i)).shuffle(blocks)
        d, a = R.record(mine, blocks, gap)
        desc.append(d)
        arenas.append(a)
    rec = Record(ctx, torch, len(rows[0]), max(a.size for a in arenas), desc, arenas)
    return L, rec, [(d, a) for d, a in zip(desc, arenas)]


ORDERS = [("reversed", 0), ("reversed", 3), ("shuffled", 0), ("shuffled", 3)]


def test_constructed_records_hold_what_they_should():
    _, rows = images_of("420 300x140")
    assert any(r.size == 64 for r in rows[0]) and any((r & 0xFFFF == 0x8000).any() for r in rows[0])
    assert {int(r[-1] >> 19) & 7 for b, r in enumerate(rows[0]) if b % 7 != 3} == set(range(8))   # a last entry in every octet


@pytest.mark.parametrize("order,gap", ORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_expand_batch_reads_constructed_records(ctx, torch, name, order, gap):
    L, rec, host = constructed(ctx, torch, name, order, gap)
    out = expand_batch(ctx, torch, L, rec)
    out.assert_hold([_sparse.expand(F.frame_info(L), d, a) for d, a in host], (name, order, gap))


@pytest.mark.parametrize("order,gap", ORDERS)
@pytest.mark.parametrize("name", NAMES)
def test_expand_mixed_reads_constructed_records(ctx, torch, name, order, gap):
    L, rec, host = constructed(ctx, torch, name, order, gap)
    for turn in range(len(HEADS)):                                 # every image at every head
        heads = [HEADS[(i + turn) % len(HEADS)] for i in range(N)]
        out = expand_mixed(ctx, torch, L, rec, heads)
        want = [F.expand_mirror(L, np.concatenate([d, a]), F.whole_windows(L), h) for (d, a), h in zip(host, heads)]
        out.assert_hold(want, (name, order, gap, heads))


# ---- round trips -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_sparsify_then_expand_batch_gives_the_planes_back(ctx, torch, name):
    L, images, rec = checked_record(ctx, torch, name)
    expand_batch(ctx, torch, L, rec).assert_hold(images, name)


@pytest.mark.parametrize("name", NAMES)
def test_sparsify_then_expand_mixed_gives_the_leading_coefficients_back(ctx, torch, name):
    """The ascending-order promise of sparse_format.hpp, kept by the device writer: the reader that stops at the first entry
    at or behind its head loses nothing in front of it."""
    L, images, rec = checked_record(ctx, torch, name)
    for turn in range(len(HEADS)):
        heads = [HEADS[(i + turn) % len(HEADS)] for i in range(N)]
        want = []
        for planes, head in zip(images, heads):
            want.append([np.concatenate([p[..., :8 * head], np.full_like(p[..., 8 * head:], F.SENTINEL16)], axis=-1) for p in planes])
        expand_mixed(ctx, torch, L, rec, heads).assert_hold(want, (name, heads))


@pytest.mark.parametrize("name", NAMES)
def test_sparsify_then_the_host_writer_writes_the_file_of_the_planes(ctx, torch, name):
    L, images, rec = checked_record(ctx, torch, name, safe=True)
    for i, (interleaved, restart) in enumerate([(True, 0), (False, 5), (True, 5)]):
        dense, sparse = R.write_files(L, images[i], rec.desc(i), rec.arena(i)[:rec.counts[i]], interleaved, restart)
        assert dense == sparse, (name, i)


# ---- refused calls ---------------------------------------------------------------------------------------------------------------

def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, torch):
    lib = _lib.lib()
    name = "420 300x140"
    L = R.layout(name)
    images, rows = images_of(name)
    src, out = Planes(ctx, torch, L, images), Planes(ctx, torch, L)
    cap = 64 * R.blocks_of(L)
    rec = Record(ctx, torch, R.blocks_of(L), cap)

    def write(layout=L, n=N, coef=_lib.ptr_array(src.ptrs), strides=_lib.size_array(src.stride), desc=rec.desc_ptr, entries=rec.entries_ptr,
              count=rec.count_ptr):
        return lib.jpeg_amd_spectral_sparsify_batch(ctx.handle, C.byref(layout) if layout else None, n, coef, strides, desc,
                                                    rec.desc_stride, entries, rec.entries_stride, cap, count)

    def read(layout=L, n=N, desc=rec.desc_ptr, entries=rec.entries_ptr, coef=_lib.ptr_array(out.ptrs), strides=_lib.size_array(out.stride)):
        return lib.jpeg_amd_spectral_expand_batch(ctx.handle, C.byref(layout) if layout else None, n, desc, rec.desc_stride, entries,
                                                  rec.entries_stride, None, coef, strides)

    for call in (write, read):
        for wrong in ({"layout": None}, {"n": -1}, {"n": 65536}, {"coef": None}, {"strides": None}, {"desc": None}, {"entries": None},
                      {"coef": _lib.ptr_array(src.ptrs[:2] + [None])}):
            assert call(**wrong) == _lib.EINVAL, (call.__name__, wrong)
    assert write(count=None) == _lib.EINVAL
    assert lib.jpeg_amd_spectral_sparsify_batch(None, C.byref(L), N, _lib.ptr_array(src.ptrs), _lib.size_array(src.stride), rec.desc_ptr,
                                                rec.desc_stride, rec.entries_ptr, rec.entries_stride, cap, rec.count_ptr) == _lib.EINVAL
    # four planes of 2^30 blocks: each passes the layout's check, their sum wraps 32 bits to zero.  (Refused: the made-up
    # pointers are never used.)
    huge = _lib.Layout()
    huge.width = huge.height = 1 << 18
    huge.precision, huge.nplanes, huge.scale_x, huge.scale_y = 8, 4, 1, 1
    for p in range(4):
        huge.factor_x[p] = huge.factor_y[p] = 1
        huge.units_x[p] = huge.units_y[p] = 1 << 15
    made_up = _lib.ptr_array([4096] * 4)
    assert write(layout=huge, coef=made_up) == _lib.EINVAL
    assert read(layout=huge, coef=made_up) == _lib.EINVAL
    ctx.synchronize()
    out.assert_hold(None, "refused reads")
    rec.download()
    assert (rec.now == rec.before).all() and rec.counts == [R.SENTINEL32] * N
    # an empty call is no error, and the context works afterwards
    assert write(n=0) == 0 and read(n=0) == 0
    assert write() == 0
    ctx.synchronize()
    rec.download()
    for i in range(N):
        rec.assert_complete(i, rows[i])
    assert read() == 0
    ctx.synchronize()
    out.assert_hold(images, "after the refusals")
