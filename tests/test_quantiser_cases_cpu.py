"""The data of tests/test_gpu_quantiser.py, judged on the reference alone (no GPU): the restatement of _quantiser_ref equals
the oracle, every constructed block is an exact tie at its position, both signs occur for every table value, no quotient
leaves Int16, and every wrong quantiser a build could fall back to -- ties to even, ties toward zero, floor(x + 1/2), a half
without its sign, the reciprocal without Markstein's correction step -- differs from the oracle somewhere on that data.

Measured here (the assertion messages print them): over the 12 434 DC ties of Q = 1 .. 255 at 8 bits the uncorrected
reciprocal misses 226 blocks under 38 table values, the smallest 41; at 16 bits it misses all 8 ties of Q = 65521."""
import numpy as np
import pytest

import _quantiser_ref as QR
import _reduce_ref as R
import _scaled_ref as S
from oracle import oracle as O


def _sets(precision):
    """(Q, every_m) of the GPU tests at this precision."""
    if precision == 8:
        return [(q, True) for q in QR.Q8]
    return [(q, False) for q in QR.Q8] + [(q, False) for q, _ in QR.pairs16(precision)]


class Stats:
    def __init__(self):
        self.blocks = 0
        self.restatement_differs = 0
        self.not_a_tie = 0
        self.one_sided = []                       # (Q, position) without both signs
        self.peak = 0                             # the largest |coefficient|
        self.wrong = {name: {"8": 0, "16": 0} for name in QR.WRONG_QUANTISERS}     # coefficients that differ, by table width
        self.dc_missed = {}                       # Q -> DC tie blocks the uncorrected reciprocal gets wrong
        self.model_differs = 0                    # the kernels' form (exact FMAs) against the oracle, at the tie positions
        self.model_checked = 0


def _walk(precision):
    st = Stats()
    for Q, every_m in _sets(precision):
        blocks, where, ms = QR.cases(Q, precision, every_m)
        width = "8" if Q < 256 else "16"
        for seed in (0, 1):                       # the luma and the chroma table of that value
            tab = QR.table_for(Q, precision, seed)
            want = O.fdct_plane(QR.plane_of(blocks[None]), tab, precision)[0].astype(np.int64)       # [n, 64]
            v, H, q = QR.quotient(blocks, tab, precision)
            got = QR.round_half_away(v)
            st.restatement_differs += int((QR.to_zigzag(got) != want).sum())
            st.peak = max(st.peak, int(np.abs(got).max()))
            if seed:
                continue
            st.blocks += len(blocks)
            k = np.array([p[0] for p in QR.POSITIONS])[where]
            h = np.array([p[1] for p in QR.POSITIONS])[where]
            at = v[np.arange(len(blocks)), h, k].astype(np.float64)
            st.not_a_tie += int((at != ms / 2.0).sum())
            for i in range(4):
                signs = set(np.sign(ms[where == i]).tolist())
                if signs != {-1, 1}:
                    st.one_sided.append((Q, QR.POSITIONS[i]))
            for name, fn in QR.WRONG_QUANTISERS.items():
                bad = QR.to_zigzag(fn(H, np.broadcast_to(q, H.shape))) != want
                st.wrong[name][width] += int(bad.sum())
                if name == "reciprocal without the correction step" and precision == 8:
                    miss = int(bad[where == 0, 0].sum())
                    if miss:
                        st.dc_missed[Q] = miss
            # the kernels' own form with exact fused multiply-adds, at the tie positions (DC at 8 bits, where every m is there)
            pick = np.flatnonzero(where == 0) if every_m else np.arange(len(blocks))
            Hs, qs = H[pick, h[pick], k[pick]], np.full(len(pick), q[0, 0])
            st.model_differs += int((QR.kernel_quantiser(Hs, qs) != want[pick, [QR.TIE_ZIGZAG[i] for i in where[pick]]]).sum())
            st.model_checked += len(pick)
    return st


@pytest.fixture(scope="module", params=[8, 12, 16])
def walked(request):
    return request.param, _walk(request.param)


def test_every_position_has_12434_ties_at_8_bits():
    assert sum(len(QR.tie_multipliers(Q, 8)) for Q in QR.Q8) == 12434
    for i, pos in enumerate(QR.POSITIONS):
        assert sum(len(QR.tie_blocks(pos, Q, 8)[0]) for Q in QR.Q8) == 12434, pos
        assert sum(int((QR.cases(Q, 8)[1] == i).sum()) for Q in QR.Q8) == 12434, pos          # ... and in what the batches take
    assert len(QR.tie_multipliers(65521, 16)) == 8 and len(QR.tie_multipliers(1, 16)) == 65534 and len(QR.tie_multipliers(32753, 12)) == 0


@pytest.mark.parametrize("precision", [8, 12, 16])
def test_restatement_equals_the_oracle_on_random_blocks(precision):
    rng = np.random.default_rng(precision)
    blocks = rng.integers(0, 1 << precision if precision < 12 else 65536, (8, 512, 8, 8)).astype(np.uint16)   # 12 bits: above the limit too
    tab = rng.integers(16 if precision > 8 else 1, 256, 64).astype(np.uint16)
    want = O.fdct_plane(QR.plane_of(blocks), tab, precision)
    assert int(np.abs(want.astype(np.int64)).max()) < 32767
    assert (QR.coefficients(blocks, tab, precision) == want).all()
    if precision == 12:
        assert (blocks > 4095).any() and (QR.coefficients(np.minimum(blocks, 4095), tab, precision) == want).all()


def test_restatement_equals_the_oracle_on_every_constructed_block(walked):
    precision, st = walked
    assert st.blocks == 4 * 12434 if precision == 8 else st.blocks >= 255 * 4 * 2
    assert st.restatement_differs == 0, f"P = {precision}: {st.restatement_differs} coefficients of {st.blocks} blocks"


def test_every_constructed_block_is_an_exact_tie_at_its_position(walked):
    precision, st = walked
    assert st.not_a_tie == 0, f"P = {precision}: {st.not_a_tie} of {st.blocks} blocks"


def test_both_signs_for_every_table_value_at_each_position(walked):
    precision, st = walked
    assert st.one_sided == [], f"P = {precision}: {st.one_sided[:8]}"


def test_no_quotient_leaves_int16(walked):
    precision, st = walked
    assert st.peak <= 32767, f"P = {precision}: a coefficient of magnitude {st.peak}"
    if precision == 16:
        assert st.peak == 32767          # ... and the largest one is reached: m = +-65533 under Q = 1


def test_every_wrong_quantiser_differs_from_the_oracle_on_this_data(walked):
    precision, st = walked
    report = f"P = {precision}, {st.blocks} blocks; coefficients that differ under 8-bit / 16-bit tables: " + \
        "; ".join(f"{name}: {c['8']} / {c['16']}" for name, c in st.wrong.items())
    print(report)
    for name, c in st.wrong.items():
        if name == "reciprocal without the correction step" and precision == 12:
            continue                      # (its misses need the larger quotients: asserted at 8 and at 16 bits)
        assert c["8"] > 0, report
        if precision == 16:
            assert c["16"] > 0, report
    if precision == 8:
        missed = st.dc_missed
        detail = f"uncorrected reciprocal: {sum(missed.values())} of 12434 DC ties missed under {len(missed)} table values, smallest {min(missed, default=None)}"
        print(detail)
        assert sum(missed.values()) > 0, detail


def test_the_kernels_form_with_exact_fused_operations_matches_on_the_ties(walked):
    precision, st = walked
    assert st.model_checked >= (12434 if precision == 8 else 255 * 4 * 2)
    assert st.model_differs == 0, f"P = {precision}: {st.model_differs} of {st.model_checked} ties"


def test_sixteen_bit_ties_under_65521_all_miss_without_the_correction_step():
    blocks, where, ms = QR.cases(65521, 16, False)
    dc = where == 0
    assert dc.sum() == 8
    tab = QR.table_for(65521, 16)
    want = O.fdct_plane(QR.plane_of(blocks[None]), tab, 16)[0][dc, 0]
    _, H, q = QR.quotient(blocks[dc], tab, 16)
    got = QR.uncorrected_reciprocal(H[:, 0, 0], q[0, 0])
    assert (got != want).sum() == 8, (got, want)
    assert (QR.kernel_quantiser(H[:, 0, 0], np.full(8, q[0, 0])) == want).all()


# ---- the batches as the GPU tests build them ------------------------------------------------------------------------------

@pytest.mark.parametrize("name,crop", [("grey", (0, 0)), ("420", (0, 0)), ("422", (3, 5)), ("444", (3, 5))])
def test_batch_holds_every_tie_and_its_reference_is_the_restatement(name, crop):
    b = QR.batch(name, 8, QR.pairs8(), crop=crop)
    assert b.n >= 255 and sorted({v[0] for v in b.values}) == list(QR.Q8)
    for Q in (1, 16, 255):                        # every tie of the value sits in the images of that value, luma and chroma
        want = {blk.tobytes() for blk in QR.cases(Q, 8)[0]}
        planes = [0] if name == "grey" else [0, 1]
        for p in planes:
            idx = [i for i, v in enumerate(b.values) if v[min(p, 1)] == Q]
            have = {blk.tobytes() for i in idx for pl in ([0] if p == 0 else [1, 2]) for blk in b.blocks[pl][i].reshape(-1, 8, 8)}
            assert want <= have, (Q, p)
    for i in (0, b.n // 2, b.n - 1):
        for plane, tab, ref in zip(b.planar(i), b.plane_tables(i), b.reference(i)):
            assert (QR.coefficients(QR.blocks_of(plane), tab, 8) == ref).all()
        if crop == (0, 0):                        # chroma replicated over its cell: the box mean gives the chroma block back
            for p, plane in enumerate(b.planar(i)):
                assert (QR.blocks_of(plane) == b.blocks[p][i]).all()


def test_every_luma_tie_survives_the_rgb_conversion():
    """The RGB instantiations get luma ties through a map Y -> near-grey RGB whose Y the reference's conversion restores
    (plain greys do not all map to themselves): with the map exact for all 256 values every luma tie survives."""
    grey = np.repeat(np.arange(256, dtype=np.uint8)[:, None], 3, axis=1)
    assert O.pack_rgb8(grey, 3)[37, 0] == 36
    m = QR.grey_rgb_map()
    assert (O.pack_rgb8(m, 3)[:, 0] == np.arange(256)).all()
    assert np.abs(m.astype(int) - np.arange(256)[:, None]).max() <= 3
    b = QR.batch("420", 8, QR.pairs8()[:3])
    rgb = m[b.samples[..., 0]]
    back = O.pack_rgb8(rgb.reshape(-1, 3), 3)[:, 0].reshape(rgb.shape[:3])
    survived = int((QR.blocks_of(back[0]) == b.blocks[0][0]).all(axis=(2, 3)).sum())
    assert survived == b.blocks[0][0].shape[0] * b.blocks[0][0].shape[1], survived


@pytest.mark.parametrize("denom", [8, 4])
def test_reduce_inputs_decode_to_the_ties(denom):
    """DC-only inputs under an all-ones table: _reduce_ref's samples ARE the constructed blocks, and every one of them is an
    exact tie under its image's output table, with both signs."""
    coef, size, samples, tables = QR.reduce_batch(denom)
    n, uy, ux, _ = coef.shape
    got = S.idct_plane_scaled(coef.reshape(n * uy, ux, 64), np.ones(64, np.uint16), 8 // denom).reshape(samples.shape)
    assert (got == samples).all()
    units = (samples.shape[2] // 8, samples.shape[1] // 8)
    assert (R.reduced_samples(coef[100], np.ones(64, np.uint16), denom, units) == samples[100]).all()
    kk, hh = [p[0] for p in QR.POSITIONS], [p[1] for p in QR.POSITIONS]
    for i in range(n):
        v = QR.quotient(QR.blocks_of(samples[i]), tables[i, 0], 8)[0][..., hh, kk].astype(np.float64)      # [gy, gx, 4]
        half = (v * 2 == np.round(v * 2)) & ((v * 2) % 2 == 1)
        assert half.any(axis=-1).all(), i
        assert (v[half] > 0).any() and (v[half] < 0).any(), i
        assert (R.reduce_plane(coef[i], np.ones(64, np.uint16), denom, units, tables[i, 0]) ==
                QR.coefficients(QR.blocks_of(samples[i]), tables[i, 0], 8)).all()
