"""The numpy statement of the sparse record (_sparse_ref.py) against the two host coders, and the conditions the device tests
(test_gpu_sparse_transport.py) rely on of its planes -- no GPU.  The reference is sound before any kernel is measured with
it: its rows are jpeg_amd_jpeg_decode_sparse's, and jpeg_amd_jpeg_encode_sparse reads them in the order the device writes."""
import numpy as np
import pytest

import _files as F
import _sparse_ref as R
from _calls import FUSED, plane_units

SIZES = [(1, 1), (7, 9), (17, 33), (131, 257)]
FORMS = [("sequential", 0), ("scans", 0), ("sequential", 5)]                    # (kind, restart interval)


@pytest.mark.parametrize("name", sorted(FUSED))
def test_reference_rows_are_the_host_decoders(name):
    for s, size in enumerate(SIZES):
        for f, (kind, restart) in enumerate(FORMS):
            data, L = F.synthetic_file(name, size, 11 * s + f, kind=kind, restart=restart)
            st, info, rec = F.decode_sparse(data)
            assert st == 0
            _, planes, _ = F.decode_planes(data)
            blocks = R.blocks_of(L)
            desc, entries = rec[:blocks], rec[blocks:]
            want = R.sparsify_rows(planes)
            got = R.rows_of(desc, entries)
            assert R.same_rows(got, want), (name, size, kind, restart)
            R.assert_tiles(desc, got, entries.size)                              # the arena has no holes


@pytest.mark.parametrize("restart", [0, 5])
@pytest.mark.parametrize("interleaved", [True, False], ids=["one scan", "scan per component"])
@pytest.mark.parametrize("name", ["y8 131x257", "420 300x140", "four planes 17x33", "one block"])
def test_host_writer_reads_rows_in_the_order_the_device_writes_them(name, interleaved, restart):
    """jpeg_amd_jpeg_encode_sparse on the reference's rows in runs of 256 blocks, the runs shuffled, writes the bytes of
    jpeg_amd_jpeg_encode_spectral on the planes."""
    L = R.layout(name)
    planes = R.pattern_planes(plane_units(L), 5, safe=True)
    rows = R.sparsify_rows(planes)
    assert any(r.size == 1 and r[0] == R.LAST for r in rows)                     # an all-zero block
    order = R.group_shuffled(len(rows), 9)
    assert len(rows) <= R.WG or order != sorted(order)
    desc, arena = R.record(rows, order, 0)
    dense, sparse = R.write_files(L, planes, desc, arena, interleaved, restart)
    assert dense == sparse


def test_record_places_rows_as_told_and_rows_of_reads_them_back():
    planes = R.pattern_planes([(5, 4)], 2)
    rows = R.sparsify_rows(planes)
    rows[3] = None
    order = list(reversed(range(len(rows))))
    desc, arena = R.record(rows, order, 3)
    assert desc[3] == R.ABSENT and desc[len(rows) - 1] == 3 and (arena[:3] == R.POISON).all() and (arena[-3:] == R.POISON).all()
    assert R.same_rows(R.rows_of(desc, arena), rows)
    live = [b for b in order if rows[b] is not None]
    assert all(desc[a] + rows[a].size + 3 == desc[b] for a, b in zip(live, live[1:]))
    assert int((arena == R.POISON).sum()) == 3 * (len(live) + 1)
    with pytest.raises(AssertionError):
        R.assert_tiles(desc, rows, arena.size)                                  # the gaps are holes
    desc0, arena0 = R.record(rows, order, 0)
    R.assert_tiles(desc0, rows, arena0.size)


def test_top_up_adds_exactly_what_it_is_told():
    for name in R.LAYOUTS:
        images = R.three_images(name, 1, equal=True)
        counts = [R.entry_count(p) for p in images]
        assert counts[0] == counts[1] == counts[2]
        assert R.entry_count(R.top_up(images[1], 1)) == counts[1] + 1


@pytest.mark.parametrize("safe", [False, True], ids=["full range", "huffman safe"])
def test_pattern_planes_hold_what_the_device_tests_rely_on(safe):
    for name in ("y8 131x257", "420 300x140"):
        planes = R.pattern_planes(plane_units(R.layout(name)), 1, safe)
        frame = np.concatenate([p.reshape(-1, 64) for p in planes]).astype(np.int32)
        rows = R.sparsify_rows(planes)
        counts = np.array([r.size for r in rows])
        nz = (frame != 0).sum(1)
        b = np.arange(len(rows))
        pat = b % R.PATTERNS
        # every pattern is what it says
        assert (nz[pat == 0] == 0).all() and (counts[pat == 0] == 1).all()
        assert (frame[pat == 1, 0] == (-1000 if safe else -32768)).all() and (nz[pat == 1] == 1).all()
        assert (frame[pat == 2, 63] == (1000 if safe else 32767)).all() and (counts[pat == 2] == 2).all()   # a DC of zero in front
        assert (frame[pat == 3, 1] != 0).all() and (nz[pat == 3] == 1).all()
        assert (counts[pat == 4] == 64).all() and (np.sign(frame[pat == 4]) == np.where(np.arange(64) % 2 == 0, 1, -1)).all()
        assert (nz[pat == 5] == 32).all() and (frame[pat == 5, 1::2] == 0).all()
        assert (nz[pat == 6] == 32).all() and (frame[pat == 6, 0::2] == 0).all() and (counts[pat == 6] == 33).all()
        assert (nz[pat == 7] == 24).all()
        assert (nz[pat == 8] == 8).all() and (frame[pat == 8, 7::8] != 0).all()
        assert (np.abs(frame).max() <= 1000) == safe
        # all ten patterns in every wave of a k_sparsify workgroup (256 blocks, four waves of 64), first workgroup and last
        for wave in range(R.WG // R.WAVE):
            assert set(pat[(b % R.WG) // R.WAVE == wave]) == set(range(R.PATTERNS))
        # a wave's first and last lane, whose prefix sums start and end the wave's, see short rows and long ones
        for lane in (0, R.WAVE - 1):
            assert counts[b % R.WAVE == lane].min() <= 2 and counts[b % R.WAVE == lane].max() >= 32
        # the counts differ from wave to wave inside every workgroup, and the last workgroup is not full
        waves = [int(counts[a:a + R.WAVE].sum()) for a in range(0, len(rows), R.WAVE)]
        for a in range(0, len(waves), R.WG // R.WAVE):
            group = waves[a:a + R.WG // R.WAVE]
            assert len(set(group)) == len(group), group
        assert len(rows) % R.WG and len(rows) % R.WAVE
        # the mean stays under the 24 entries per block of the batch paths' arena
        assert counts.mean() < 24
        # a last entry in every octet (the readers' walk ends there), the value 0x8000, 64-entry rows
        assert {int(r[-1] >> 19) & 7 for r in rows} == set(range(8))
        assert safe or any((r & 0xFFFF == 0x8000).any() for r in rows)
        assert any(r.size == 64 for r in rows)
