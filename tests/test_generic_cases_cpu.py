"""The inputs of tests/test_gpu_generic_shapes.py, checked with the oracle alone (no GPU): the sizes span every phase of the
per-tile block range, the `wide` input drives every channel to both clamps while at least half of its samples stay strictly
inside the range, and the `steps` input gives block-constant planes with the chosen constants."""
import numpy as np
import pytest

import _generic_cases as GC

CASE_SITING = [(c.number, cosite) for c in GC.CASES for cosite in (False, True)]
_ids = lambda v: f"case{v[0]}-{'cosited' if v[1] else 'centred'}"


def test_case_table_counts_precisions_scales_and_dispatch():
    assert len(GC.CASES) == 14
    assert [c.count for c in GC.CASES] == [3, 3, 3, 3, 3, 3, 3, 3, 4, 4, 2, 3, 4, 3]
    assert [c.precision for c in GC.CASES] == [8, 12, 16, 12, 12, 16, 8, 12, 12, 16, 9, 12, 8, 12]
    assert [c.scale for c in GC.CASES] == [(4, 1), (4, 2), (4, 4), (1, 4), (3, 3), (1, 3), (3, 1), (3, 2), (4, 4), (4, 2), (4, 4),
                                            (3, 3), (4, 4), (3, 3)]
    assert [c.number for c in GC.CASES if not c.fused] == [14]
    # a box of 3 under decomposed() <=> the staged encoder
    box3 = [c.number for c in GC.CASES if any(c.scale[0] // f[0] == 3 or c.scale[1] // f[1] == 3 for f in c.factors) or not c.fused]
    assert tuple(box3) == GC.ENCODE_STAGED


def test_sizes_span_every_phase_of_the_block_range():
    W, H = GC.LARGE
    assert W > 4 * GC.TILE_W and H > 4 * 64 and H > 8 * 32
    assert W % GC.TILE_W == 5 and all((5 * n) % 8 for n in (2, 3, 4))       # the byte-wise store tail of the last tile column
    assert GC.SMALL == (GC.TILE_W + 1, 65)                                   # one pixel column / row in the second tile
    for cosited in (False, True):
        for tile in (GC.TILE_W, 64, 32):
            # thirds: period three beyond the first tile, checked far beyond the sizes used.  Centred, the first tile differs (the
            # clamp at sample 0): four values at tiles 0 .. 3; cosited (a = 0) it is part of the cycle: three values
            ph = [GC.axis_phase(1, 3, cosited, tile, i) for i in range(4096)]
            assert len(set(ph[:4])) == (3 if cosited else 4), (cosited, tile, ph[:4])
            assert len(set(ph[1:4])) == 3
            assert all(ph[i] == ph[i - 3] for i in range(4, 4096))
            # quarters and 2-in-4: one value beyond the first tile, which differs (the clamp at sample 0) when centred
            for f in (1, 2):
                ph = [GC.axis_phase(f, 4, cosited, tile, i) for i in range(4096)]
                assert all(p == ph[1] for p in ph[1:])
                assert cosited or ph[0] != ph[1]
    # the tiles of LARGE: columns 0 .. 4, rows 0 .. 4 (64-row tiles) -- every value and the first repeat
    assert (W - 1) // GC.TILE_W == 4 and (H - 1) // 64 == 4 and (H - 1) // 32 == 8


@pytest.mark.parametrize("cs", CASE_SITING, ids=_ids)
@pytest.mark.parametrize("size", GC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_wide_input_reaches_both_clamps_and_stays_inside_for_half_the_samples(cs, size):
    number, cosite = cs
    c = GC.case(number)
    want = GC.oracle_rect(number, size, "wide", cosite)
    top = (1 << c.precision) - 1
    assert want.shape == (size[1], size[0], c.count)
    for ch in range(c.count):
        v = want[..., ch]
        share = float(((v > 0) & (v < top)).mean())
        print(f"case {number} {'cosited' if cosite else 'centred'} {size[0]}x{size[1]} channel {ch}: min {int(v.min())} max {int(v.max())} "
              f"interior share {share:.4f}")
        assert int(v.min()) == 0 and int(v.max()) == top, (number, cosite, size, ch)
        assert share >= 0.5, (number, cosite, size, ch, share)


@pytest.mark.parametrize("number", [c.number for c in GC.CASES])
@pytest.mark.parametrize("size", GC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_steps_planes_are_block_constant_with_the_chosen_constants(number, size):
    c = GC.case(number)
    top = (1 << c.precision) - 1
    planes, tables, q, want_p = GC.oracle_planes(number, size, "steps")
    for p, (plane, consts) in enumerate(zip(want_p, GC.step_constants(c, size))):
        uy, ux = consts.shape
        blocks = plane.reshape(uy, 8, ux, 8)
        assert (blocks == blocks[:, :1, :, :1]).all(), (number, p)            # block-constant in the oracle's idct_plane
        assert (blocks[:, 0, :, 0] == consts).all(), (number, p)              # ... at DC + 2^(P-1)
        # the extremes lie next to each other across block seams, in both directions
        if ux >= 7 and uy >= 3:
            assert {0, 1, top - 1, top} <= set(np.unique(consts[:3]).tolist())
            assert ((consts[:, :-1] == 0) & (consts[:, 1:] == top)).any()
            assert ((consts[:-1] == 0) & (consts[1:] == top - 1)).any()
    for cosite in (False, True):
        want = GC.oracle_rect(number, size, "steps", cosite)
        assert int(want.min()) == 0 and int(want.max()) == top


@pytest.mark.parametrize("cs", CASE_SITING, ids=_ids)
def test_encode_inputs_stay_where_the_reference_does_not_trap(cs):
    number, cosite = cs
    c = GC.case(number)
    for size in GC.SIZES:
        values = GC.oracle_rect(number, size, "wide", cosite)
        tables = GC.encode_tables(c)
        _, want_f = GC.oracle_encode(c, size, values, tables)
        assert max(int(np.abs(w.astype(np.int32)).max()) for w in want_f) < 32000
        assert any(int(np.abs(w[..., 1:]).max()) > 0 for w in want_f)        # not DC alone
