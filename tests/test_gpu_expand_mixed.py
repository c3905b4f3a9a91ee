"""jpeg_amd_spectral_expand_mixed on the MI355X (k_expand_mixed): sparse records of ten images of different sizes and
layouts into windows of their planes, at heads of 1, 4 and 8 octets, in ONE launch.  The contract is
jpeg_amd_spectral_expand_batch's bytes inside the windows' heads and nothing else: the planes hold a sentinel before the call
and EVERY coefficient of every plane is compared with the numpy mirror of that contract (_files.expand_mirror, which
test_file_tensor_cpu.py checks against the host decoder) -- written ones and untouched ones alike.  One test sends the same
records through jpeg_amd_spectral_expand_batch itself, so that mirror and kernel cannot be wrong alike."""
import ctypes as C

import numpy as np
import pytest

import _files as F
from _calls import FUSED, c_layout, plane_units
from _calls import ctx, torch  # noqa: F401  (the fixtures)
from jpeg_amd import _lib

pytestmark = pytest.mark.gpu

WG = 256                                                       # octets per workgroup: 256 / head blocks
# (layout, size, head, windows): "whole", "one" = a single block, "edge" = up to the last block column and row from (1, 1)
# or (0, 0), or a window per plane.  Units: 300 x 140 4:2:0 is 38 x 18 and 19 x 9 blocks, 131 x 257 grey 17 x 33.
IMAGES = [
    ("y8", (1, 1), 8, "whole"),
    ("440", (7, 9), 1, "whole"),
    ("420", (17, 33), 4, "edge"),
    ("y8", (131, 257), 8, [(3, 2, 5, 20)]),                   # 100 blocks of 32 a workgroup: a boundary at row 6, column 2
    ("420", (300, 140), 1, [(1, 1, 37, 17), (0, 0, 19, 9), (18, 8, 1, 1)]),   # 629 + 171 + 1 blocks of 256 a workgroup
    ("422", (300, 140), 4, [(5, 3, 13, 7), (2, 1, 9, 11), (0, 17, 19, 1)]),   # 91 + 99 + 19 of 64: planes meet inside one
    ("444", (131, 257), 8, "one"),
    ("444", (17, 33), 1, [(0, 0, 3, 5), (0, 0, 0, 0), (2, 4, 1, 1)]),         # a plane with nothing to write
    ("y8", (300, 140), 4, "whole"),
    ("440", (131, 257), 8, "edge"),
]


def _windows(L, spec):
    units = plane_units(L)
    if spec == "whole":
        return F.whole_windows(L)
    if spec == "one":
        return [(ux // 2, uy // 2, 1, 1) for ux, uy in units]
    if spec == "edge":
        return [(min(1, ux - 1), min(1, uy - 1), ux - min(1, ux - 1), uy - min(1, uy - 1)) for ux, uy in units]
    return spec


class Case:
    """The ten images: records (packed one behind the other with gaps, on the device), windows and heads."""

    def __init__(self, ctx, torch):
        self.ctx, self.torch = ctx, torch
        self.L, self.records, self.windows, self.heads, self.at = [], [], [], [], []
        packed, at = [], 5                                     # (the first record does not begin the buffer)
        for i, (name, size, head, spec) in enumerate(IMAGES):
            data, L = F.synthetic_file(name, size, 40 + i, kind="sequential" if i % 2 else "scans", restart=(0, 4)[i % 3 == 0])
            st, info, record = F.decode_sparse(data)
            assert st == 0
            blocks = sum(ux * uy for ux, uy in plane_units(L))
            if blocks > 4:                                     # blocks no scan reached: every fifth one
                record[:blocks][2::5] = F.ABSENT
            self.L.append(L); self.records.append(record); self.windows.append(_windows(L, spec)); self.heads.append(head)
            self.at.append((at, at + blocks))
            packed += [np.zeros(at - sum(p.size for p in packed), np.uint32), record]
            at += record.size + 3 + i
        self.d_records = torch.from_numpy(np.concatenate(packed).view(np.int32)).to(ctx.torch_device)

    def planes(self, i):
        return [self.torch.full((uy, ux, 64), int(F.SENTINEL16), dtype=self.torch.int16, device=self.ctx.torch_device)
                for ux, uy in plane_units(self.L[i])]

    def items(self, planes, order=None):
        order = list(range(len(IMAGES))) if order is None else order
        items = (_lib.ExpandItem * len(order))()
        for it, i in zip(items, order):
            it.layout, it.head = self.L[i], self.heads[i]
            for p, w in enumerate(self.windows[i]):
                it.d_coef[p] = planes[i][p].data_ptr()
                it.window[p] = _lib.Region(*w)
            it.desc_at, it.entries_at = self.at[i]
        return items


@pytest.fixture(scope="module")
def case(ctx, torch):
    return Case(ctx, torch)


def test_the_case_holds_what_it_should(case):
    assert {name for name, _, _, _ in IMAGES} == set(FUSED)
    assert {size for _, size, _, _ in IMAGES} == {(1, 1), (7, 9), (17, 33), (131, 257), (300, 140)}
    assert {head for _, _, head, _ in IMAGES} == {1, 4, 8}
    counts = [[w * h for _, _, w, h in ws] for ws in case.windows]
    assert any(sum(c) * head % WG for c, head in zip(counts, case.heads))          # a last workgroup that is not full
    # a workgroup boundary in the middle of a window's row, and one block windows, and windows up to both far edges
    assert any((WG // head) % ws[0][2] and ws[0][2] * ws[0][3] > WG // head for ws, head in zip(case.windows, case.heads))
    assert any(w == 1 and h == 1 for ws in case.windows for _, _, w, h in ws)
    assert any(x > 0 and y > 0 and x + w == ux and y + h == uy
               for ws, L in zip(case.windows, case.L) for (x, y, w, h), (ux, uy) in zip(ws, plane_units(L)))
    for record, L in zip(case.records, case.L):
        blocks = sum(ux * uy for ux, uy in plane_units(L))
        pos = (record[blocks:] >> 16) & 63
        if blocks > 100:
            assert (record[:blocks] == F.ABSENT).any() and (pos >= 32).any() and (pos == 63).any()


@pytest.mark.parametrize("order", ["as listed", "reversed"])
def test_one_launch_writes_the_heads_of_the_windows_and_nothing_else(ctx, torch, case, order):
    order = list(range(len(IMAGES))) if order == "as listed" else list(reversed(range(len(IMAGES))))
    planes = [case.planes(i) for i in range(len(IMAGES))]
    items = case.items(planes, order)
    assert _lib.lib().jpeg_amd_spectral_expand_mixed(ctx.handle, len(order), items, case.d_records.data_ptr()) == 0
    ctx.synchronize()
    for i in range(len(IMAGES)):
        want = F.expand_mirror(case.L[i], case.records[i], case.windows[i], case.heads[i])
        for p, (g, w) in enumerate(zip(planes[i], want)):
            g = g.cpu().numpy()
            assert (g == w).all(), (IMAGES[i], p, np.argwhere(g != w)[:4].tolist())


def test_whole_planes_at_head_8_are_the_uniform_expand(ctx, torch, case):
    """jpeg_amd_spectral_expand_batch on the same records: the reference of the contract itself."""
    lib = _lib.lib()
    for i in (4, 5, 9):
        L, record = case.L[i], case.records[i]
        blocks = sum(ux * uy for ux, uy in plane_units(L))
        d_rec = torch.from_numpy(record.view(np.int32).copy()).to(ctx.torch_device)
        uniform, mixed = case.planes(i), case.planes(i)
        strides = _lib.size_array([p.numel() for p in uniform])
        assert lib.jpeg_amd_spectral_expand_batch(ctx.handle, C.byref(L), 1, d_rec.data_ptr(), 0, d_rec.data_ptr() + 4 * blocks, 0, None,
                                                  _lib.ptr_array([p.data_ptr() for p in uniform]), strides) == 0
        item = (_lib.ExpandItem * 1)()
        item[0].layout, item[0].head, item[0].desc_at, item[0].entries_at = L, 8, 0, blocks
        for p, w in enumerate(F.whole_windows(L)):
            item[0].d_coef[p], item[0].window[p] = mixed[p].data_ptr(), _lib.Region(*w)
        assert lib.jpeg_amd_spectral_expand_mixed(ctx.handle, 1, item, d_rec.data_ptr()) == 0
        ctx.synchronize()
        for a, b in zip(uniform, mixed):
            assert bool((a == b).all().item()), IMAGES[i]


def test_refused_calls_write_nothing_and_leave_the_context_usable(ctx, torch, case):
    lib = _lib.lib()
    planes = [case.planes(i) for i in range(len(IMAGES))]
    rec = case.d_records.data_ptr()

    def call(change=None, n=len(IMAGES), records=rec):
        items = case.items(planes)
        if change:
            change(items)
        return lib.jpeg_amd_spectral_expand_mixed(ctx.handle, n, items, records)

    def window(i, p, w):
        def change(items):
            items[i].window[p] = _lib.Region(*w)
        return change

    def head(h):
        def change(items):
            items[6].head = h
        return change

    def pointer(i, p, value):
        def change(items):
            items[i].d_coef[p] = value
        return change

    assert call(window(4, 0, (1, 1, 38, 17))) == _lib.EINVAL           # one column past the plane's 38
    assert call(window(4, 1, (0, 1, 19, 9))) == _lib.EINVAL            # one row past its 9
    assert call(window(9, 0, (-1, 0, 2, 2))) == _lib.EINVAL
    assert call(window(9, 0, (0, 0, -2, 2))) == _lib.EINVAL
    for h in (0, 2, 3, 16):
        assert call(head(h)) == _lib.EINVAL
    assert call(pointer(5, 2, None)) == _lib.EINVAL
    assert call(pointer(5, 2, planes[5][2].data_ptr() + 2)) == _lib.EINVAL   # not 16-byte aligned
    assert call(n=-1) == _lib.EINVAL
    assert call(records=None) == _lib.EINVAL
    assert lib.jpeg_amd_spectral_expand_mixed(ctx.handle, len(IMAGES), None, rec) == _lib.EINVAL
    assert lib.jpeg_amd_spectral_expand_mixed(ctx.handle, 65536, case.items(planes), rec) == _lib.EINVAL
    # more workgroups than a grid holds: 64 planes of 2^30 blocks at head 8 are 2^31 workgroups (refused: the made-up
    # pointers are never used)
    huge = c_layout(1 << 18, 1 << 18, FUSED["y8"])
    assert plane_units(huge) == [(1 << 15, 1 << 15)]
    items = (_lib.ExpandItem * 64)()
    for it in items:
        it.layout, it.head, it.d_coef[0], it.window[0] = huge, 8, 4096, _lib.Region(0, 0, 1 << 15, 1 << 15)
    assert lib.jpeg_amd_spectral_expand_mixed(ctx.handle, 64, items, rec) == _lib.EINVAL
    ctx.synchronize()
    for ps in planes:
        for p in ps:
            assert bool((p == int(F.SENTINEL16)).all().item())
    assert lib.jpeg_amd_spectral_expand_mixed(ctx.handle, 0, None, None) == 0
    assert call() == 0
    ctx.synchronize()
    want = F.expand_mirror(case.L[4], case.records[4], case.windows[4], case.heads[4])
    assert all((g.cpu().numpy() == w).all() for g, w in zip(planes[4], want))
