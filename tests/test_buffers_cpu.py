"""tests/_buffers.py held to what it claims, without a GPU: the table of tests/test_gpu_buffers.py must not quietly shrink into
the aligned case again -- every width class in every layout, every placement at the residues it states, the launchers' predicates
false (true) exactly where the table says so, guard bytes around every image, and guard helpers that do see a stray byte."""
import numpy as np
import pytest

import _buffers as B
from _calls import FUSED, SENTINEL, assert_only_spans_written


def _placements(c):
    return [(p, B.place(3 * c.size[0] * c.size[1], *p)) for p in B.PLACEMENTS]


def test_every_fused_layout_has_every_width_class():
    assert set(B.SHAPES) == set(FUSED)
    for name, shapes in B.SHAPES.items():
        widths = [w for w, _ in shapes]
        assert any(w % 16 == 0 for w in widths) and any(w % 16 == 8 for w in widths) and any(w % 2 == 1 for w in widths), name
        assert all(max(s) <= B.LIMIT for s in shapes), name


def test_420_takes_the_listed_shapes_and_three_per_strip_shape():
    from test_gpu_quad_shapes import SIZES
    small = [s for s in SIZES if max(s) <= 304]
    assert len(small) == 9 and all(s in B.SHAPES["420"] for s in small)
    assert {B.strip_blocks("420", s) for s in small} == {16, 32}
    for bx, extra in B.QUAD_EXTRA.items():
        assert all(s in B.SHAPES["420"] for s in extra)
        (w0, h), (w1, _), (w2, _) = extra
        assert w0 % 16 == 0 and w1 == w0 + 8 and w2 == w0 - 3 and w2 % 2 == 1
        for s in extra:
            assert B.strip_blocks("420", s) == bx, s
            assert s[0] > 8 * bx and s[0] % (8 * bx) != 0, s          # more than one strip column, the last one partial


def test_other_layouts_span_strip_columns_and_end_inside_a_strip_row():
    for name in ("y8", "444", "422", "440"):
        assert len(B.SHAPES[name]) == 3
        for s in B.SHAPES[name]:
            sw, sh = B.strip_pixels(name, s)
            assert s[0] > sw and s[1] % sh != 0, (name, s)
    # grey and 4:4:4 are one kernel template: between them every width class meets both strip shapes
    met = {(B.strip_blocks(name, s), 0 if s[0] % 16 == 0 else 8 if s[0] % 16 == 8 else 1) for name in ("y8", "444") for s in B.SHAPES[name]}
    assert met == {(bx, k) for bx in (16, 32) for k in (0, 8, 1)}
    assert all(B.strip_blocks("422", s) == 32 for s in B.SHAPES["422"]) and all(B.strip_blocks("440", s) == 16 for s in B.SHAPES["440"])


def test_placements_are_the_six_pairs_at_their_residues():
    assert B.PLACEMENTS == [(0, 0), (0, 8), (8, 0), (4, 0), (1, 5), (15, 8)] and B.N_IMAGES == 3
    for c in B.CASES + B.STAGED_CASES:
        for (lead, r), p in _placements(c):
            assert p.lead == lead and p.stride % 16 == r and p.stride == 3 * c.size[0] * c.size[1] + p.gap
            assert [a for a, _ in p.spans] == [lead + i * p.stride for i in range(3)]
            assert B.residues(p, 16) == [(lead + i * r) % 16 for i in range(3)]
            assert B.residues(p, 8) == [(lead + i * r) % 8 for i in range(3)]
            assert 16 <= p.gap < 32 and p.tail >= 16
            assert p.nbytes == p.spans[-1][0] + p.stride + p.tail             # gap and tail behind the last image
    p = B.place(3 * 17 * 17, 0, 8)
    assert B.residues(p, 16) == [0, 8, 0]                                     # image 1 at residue 8
    p = B.place(3 * 17 * 17, 1, 5)
    assert B.residues(p, 16) == [1, 6, 11]


def test_every_layout_has_a_case_with_every_image_at_another_residue():
    for name in B.SHAPES:
        assert any(len(set(B.residues(p, 16))) == 3 for c in B.CASES if c.name == name for _, p in _placements(c)), name


def test_the_predicates_fall_where_the_table_says():
    for c in B.CASES:
        w = c.size[0]
        for (lead, r), p in _placements(c):
            fast = B.decoder_fast(w, lead, p.stride)
            assert fast == ((lead, r) == (0, 0) and w % 16 == 0)
            assert B.encoder_fast(w, lead, p.stride) == (w % 8 == 0 and (lead, r) in [(0, 0), (0, 8), (8, 0)])
    for name in B.SHAPES:        # each layout reaches: fast; not fast on whole chunks for base alone, stride alone; FASTIN with FAST lost
        whole = [c for c in B.CASES if c.name == name and c.size[0] % 16 == 0]
        assert whole
        for c in whole:
            img = 3 * c.size[0] * c.size[1]
            assert B.decoder_fast(c.size[0], 0, B.place(img, 0, 0).stride)
            assert not B.decoder_fast(c.size[0], 0, B.place(img, 0, 8).stride) and B.encoder_fast(c.size[0], 0, B.place(img, 0, 8).stride)
            assert not B.decoder_fast(c.size[0], 8, B.place(img, 8, 0).stride) and B.encoder_fast(c.size[0], 8, B.place(img, 8, 0).stride)
        half = [c for c in B.CASES if c.name == name and c.size[0] % 16 == 8]
        assert half and all(B.encoder_fast(c.size[0], 8, B.place(3 * c.size[0] * c.size[1], 8, 0).stride) for c in half)


def test_settings_are_spread_over_the_cases():
    cases = B.CASES
    per = sum(c.per_image for c in cases)
    assert abs(2 * per - len(cases)) <= 1
    assert B.QI == [[0, 1, 1], [0, 1, 2], [1, 0, 0], [2, 1, 0]]
    for name in ("420", "444", "422", "440"):
        mine = [c for c in cases if c.name == name]
        assert {c.per_image for c in mine} == {False, True} and len({tuple(c.qi) for c in mine}) >= 2, name
    assert {tuple(c.qi) for c in cases if c.name == "420"} == {tuple(q) for q in B.QI}
    assert [c.name for c in B.STAGED_CASES] == ["411", "420-cosited"] and len(B.STAGED_PLACEMENTS) == 3
    for c in cases + B.STAGED_CASES:
        q = B.tables(c)
        assert q.shape == (3 if c.per_image else 1, 3, 64) and q.min() >= 1
        assert all(not (q[i, a] == q[i, b]).all() for i in range(len(q)) for a, b in ((0, 1), (0, 2), (1, 2)))
        if c.per_image:
            assert not (q[0] == q[1]).all() and not (q[1] == q[2]).all()
        assert all(B.coef_gap_blocks(p) >= 1 for p in range(len(c.factors)))


@pytest.mark.parametrize("placement", B.PLACEMENTS, ids=B.placement_id)
def test_guard_helpers_see_a_stray_byte(placement):
    w, h = 24, 9
    p = B.place(3 * w * h, *placement)
    images = [np.full(3 * w * h, 10 + i, np.uint8) for i in range(3)]
    clean = B.placed_pixels(images, p, SENTINEL)
    assert clean.size == p.nbytes and B.guard_report(clean, p) == ""
    B.assert_guarded(clean, p)
    spots = [("gap", p.spans[0][0] + p.spans[0][1]), ("gap", p.spans[1][0] - 1), ("gap", p.spans[1][0] + p.spans[1][1] + 15),
             ("gap and tail", p.spans[2][0] + p.spans[2][1]), ("gap and tail", p.nbytes - 1)]
    if p.lead:
        spots += [("lead", 0), ("lead", p.lead - 1)]
    for where, at in spots:
        dirty = clean.copy()
        dirty[at] ^= 1
        assert where in B.guard_report(dirty, p), (where, at)
        with pytest.raises(AssertionError):
            B.assert_guarded(dirty, p)
        with pytest.raises(AssertionError):
            assert_only_spans_written(dirty, p.spans)
    inside = clean.copy()                                   # a byte of an image is not the guard's business
    inside[p.spans[1][0]] ^= 1
    B.assert_guarded(inside, p)
    for fill in (0x00, 0xFF):                               # the encoder's inputs: images intact, everything else the filler
        buf = B.placed_pixels(images, p, fill)
        assert all((buf[a:a + m] == 10 + i).all() for i, (a, m) in enumerate(p.spans))
        assert int((buf == fill).sum()) == p.nbytes - 3 * 3 * w * h


def test_difference_reports_name_row_column_channel_and_chunk():
    w, h = 24, 9
    want = np.arange(3 * w * h, dtype=np.uint32).astype(np.uint8)
    assert B.first_difference(want, want, (w, h)) == ""
    got = want.copy()
    got[3 * w * 5 + 3 * 7 + 2] ^= 1
    assert "(row 5, column 7, channel 2) [byte 23 of its row, chunk 1]" in B.first_difference(got, want, (w, h))
    a = [np.zeros((2, 3, 64), np.int16)]
    b = [a[0].copy()]
    b[0][1, 2, 5] = 4
    assert B.first_coefficient(a, a) == "" and "(block x 2, block y 1, zigzag 5)" in B.first_coefficient(a, b)
