"""The two decks of tests/attn16cases.py proven without a GPU.  The selector deck: the margin condition on the float64 scores of every case, the
stated coverage recomputed from the cases, distinct V rows, and both oracle twins returning the selected rows exactly.  The bar deck: every score
profile is what its name says (on the float64 scores of the ROUNDED operands of both flavours), the effective support stays small, both twins
stay within the derived bar, and six mutants of the float64 reference each leave 2 bar somewhere in every case (or in its named sibling).
tests/test_attn16_dispatch_gpu.py then runs the same decks through varhip_attn_cached_f16 / _bf16."""
import numpy as np
import pytest

from tests import attn16cases as ac
from tests import util


@pytest.fixture(scope='module')
def L():
    util.ensure_oracle_built()
    from oracle import var_oracle
    return var_oracle.lib()


_BAR = {}


def bar_built(c, flav):
    """(operands, ref, bar) of a bar case, computed once per module run"""
    key = (c['name'], flav)
    if key not in _BAR:
        b = ac.build_bar(c, flav)
        _BAR[key] = (b,) + ac.reference(b)
    return _BAR[key]


def test_hadamard_rows_and_rounding():
    assert np.array_equal(ac.HD @ ac.HD.T, np.eye(64)) and set(np.unique(ac.HD)) == {-0.125, 0.125}
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, -(1.0 + 2.0 ** -9 + 2.0 ** -30), 3.3, 1e-3, 200.5, 0.0])
    from oracle.var_oracle import r16
    for flav in ac.FLAVOURS:
        got = ac.round16(x, flav)
        assert np.array_equal(got, r16(got, flav)), 'round16 left the type'
        assert np.array_equal(got, r16(x.astype(np.float32), flav))            # (every x above is an fp32 value or far from a tie: one rounding = two)
    assert ac.round16(1.0 + 2.0 ** -8, 'bf16') == 1.0 and ac.round16(1.0 + 3 * 2.0 ** -8, 'bf16') == np.float32(1.0 + 2.0 ** -6)      # ties to even


def test_wave_heuristic_restated():
    """the largest NW of 4, 3, 2, 1 that divides ceil(l / 32): no launch has a wave with t0 >= l"""
    for l in range(1, 4097):
        nq = (l + 31) // 32
        assert ac.waves(l) == max(nw for nw in (1, 2, 3, 4) if nq % nw == 0) and ac.idle_waves(l) == 0 and ac.grid_x(l) * ac.waves(l) == nq
    assert [ac.waves(l) for l in (1, 31, 33, 64, 65, 96, 97, 128, 161)] == [1, 1, 2, 2, 3, 3, 4, 4, 3]


# ---- the selector deck ------------------------------------------------------------------------------------------------------------------------
def test_selector_coverage_is_what_the_deck_states():
    got = ac.sel_coverage()
    assert got == ac.SEL_COVERAGE, {k: (got[k], ac.SEL_COVERAGE.get(k)) for k in got if got[k] != ac.SEL_COVERAGE.get(k)}
    # and the stated coverage is what is asked for
    cov = ac.SEL_COVERAGE
    assert cov['stage_pos'] == 64 and set(cov['ragged_complete']) >= {1, 5, 17, 31} and cov['exact_multiple'] and cov['single_tile']
    assert cov['ntile_parity'] == [0, 1] and cov['lane_half'] == 64
    assert all(cov['nw'][nw] for nw in (1, 2, 3, 4)) and cov['nw_grid_gt1'] == [1, 2, 3, 4] and cov['nw_partial_last_wave'] == [1, 2, 3, 4]
    assert {1, 31, 33, 64, 65, 96, 97, 128, 161} <= {l for ls in cov['nw'].values() for l in ls}
    assert (2, 3) in cov['b2_h'] and 2 * cov['lmax_pad33'] >= cov['cases']
    for c in ac.sel_cases():
        assert c['B2'] <= 2 and c['H'] <= 3 and c['l'] <= c['curL'] <= 330 and c['nw'] == ac.waves(c['l'])
        wins = ac.sel_windows(c)
        assert len({w for w, n, a, c0 in wins}) == len(wins), f"{c['name']}: two slices share a window"
        for w, n, a, c0 in wins:
            assert 1 <= n <= 63 and 0 <= w and w + n <= c['curL'] and np.gcd(a, n) == 1, (c['name'], w, n, a)


@pytest.mark.parametrize('case', ac.sel_cases(), ids=lambda c: c['name'])
def test_selector_margin_rows_and_twins(L, case):
    b = ac.build_selector(case)
    B2, H, l, curL = case['B2'], case['H'], case['l'], case['curL']
    assert np.isnan(b.k[:, :, curL:]).all() and np.isnan(b.v[:, :, curL:]).all() and np.isfinite(b.k[:, :, :curL]).all()
    for flav in ac.FLAVOURS:                                                      # every operand is a value of both types
        assert all(np.array_equal(ac.round16(a[np.isfinite(a)], flav), a[np.isfinite(a)]) for a in (b.q, b.k, b.v))
    q = b.q.reshape(B2, l, H, 64)
    for bb in range(B2):
        for h in range(H):
            s = q[bb, :, h].astype(np.float64) @ b.k[bb, h, :curL].astype(np.float64).T
            rows = np.arange(l)
            assert np.array_equal(s.argmax(1), b.sel[bb, h]) and (s[rows, b.sel[bb, h]] == 128.0).all()
            rest = np.delete(s, b.sel[bb, h] + rows * curL).reshape(l, curL - 1)
            assert (rest == 0.0).all() and ((128.0 - rest) * ac.LOG2E >= 160.0).all(), f"{case['name']}: the margin condition"
            v = b.v[bb, h, :curL]
            assert len(np.unique(v, axis=0)) == curL, f"{case['name']}: two keys of a slice hold the same V row"
            for b2 in range(B2):
                for h2 in range(H):
                    if (b2, h2) != (bb, h):
                        assert (b.v[b2, h2, b.sel[bb, h]] != v[b.sel[bb, h]]).any(1).all(), f"{case['name']}: another slice holds the same row at the same key"
    assert len(np.unique(b.sel.reshape(B2 * H, l), axis=0)) == B2 * H or l == 1 and len(set(b.sel.reshape(-1))) == B2 * H or B2 * H == 1
    for flav in ac.FLAVOURS:
        got = ac.twin(L, flav, b)
        bad = np.argwhere(got != b.expected)
        assert bad.size == 0, f"{case['name']} {flav} twin: first mismatch at {tuple(bad[0])}"


# ---- the bar deck -----------------------------------------------------------------------------------------------------------------------------
def test_bar_deck_shape():
    cases = ac.bar_cases()
    assert {c['kind'] for c in cases} == {'asc', 'desc', 'late', 'split', 'split1', 'wide'} and 8 <= len(cases) <= 10
    assert {c['nw'] for c in cases} == {1, 2, 3, 4}
    names = {c['name'] for c in cases}
    for c in cases:
        assert c['B2'] <= 2 and c['H'] <= 3 and c['l'] <= c['curL'] <= 330 and (c['sibling'] is None or c['sibling'] in names)
    assert 2 * sum(c['Lmax'] >= c['curL'] + 33 for c in cases) >= len(cases)


@pytest.mark.parametrize('flav', ac.FLAVOURS)
@pytest.mark.parametrize('case', ac.bar_cases(), ids=lambda c: c['name'])
def test_bar_profiles_are_built_as_named(case, flav):
    """on the float64 scores of the rounded operands: where the running maximum moves, per query"""
    b, ref, bar = bar_built(case, flav)
    curL, kind = case['curL'], case['kind']
    ntile, l = (curL + 31) // 32, case['l']
    assert np.isnan(b.k[:, :, curL:]).all() and np.isnan(b.v[:, :, curL:]).all()
    assert b.support <= 16.0, f'effective support {b.support:.1f} keys'
    tm = np.arange(l) % 32
    for bb, h, q, k, v in ac.slices(b):
        s = q @ k.T
        run, kstar, peak = ac.tile_walk(s)
        step = run[:, 1:] - run[:, :-1]
        if kind == 'asc':
            assert (np.abs(step - 3.0) <= 0.5).all() and (kstar == ntile - 1).all() and curL % 32
        elif kind == 'desc':
            assert (kstar == 0).all() and (peak == 0).all()
        elif kind == 'late':
            assert curL % 32 and (s.argmax(1) == curL - 1).all() and (kstar == ntile - 1).all()
            assert (step[:, -1] >= 4.0).all() and (np.ptp(s[:, :curL - 1], axis=1) <= 2.0).all()
        elif kind == 'split':
            X = case['X']
            assert X & 1 and 0 < X < ntile - 1
            assert (kstar[tm >= 16] == X).all() and (kstar[tm < 16] == 0).all() and (step[tm >= 16, X - 1] >= 3.0).all()
        elif kind == 'split1':
            assert curL % 32 and (kstar[tm == 7] == ntile - 1).all() and (kstar[tm != 7] == 0).all() and (tm == 7).sum() >= 2
        else:
            assert np.ptp(s, axis=1).min() >= 100.0 and s.max() >= 55.0 and s.min() <= -55.0
            assert len(np.unique(kstar)) >= min(ntile, 3) and len(np.unique(peak)) >= min(ntile, 3)                    # the maximum moves last in, and peaks in, different tiles
            assert (np.abs(q) @ np.abs(k).T).max() >= 100.0                                    # the score term of the bar is in play


@pytest.mark.parametrize('flav', ac.FLAVOURS)
@pytest.mark.parametrize('case', ac.bar_cases(), ids=lambda c: c['name'])
def test_bar_twins_within_the_bar(L, case, flav):
    b, ref, bar = bar_built(case, flav)
    ratio = ac.within(f"{case['name']} {flav} twin", ac.twin(L, flav, b), ref, bar)
    assert ratio >= 0.05, f'a bar the twin meets at {ratio:.4f} is vacuous'


MUTANT_RATIOS = {}


@pytest.mark.parametrize('flav', ac.FLAVOURS)
@pytest.mark.parametrize('case', ac.bar_cases(), ids=lambda c: c['name'])
def test_bar_deck_has_teeth(case, flav):
    """every mutant of the float64 reference is more than 2 bar away somewhere in the case (the two rescale mutants: in the named sibling, for a
    profile whose maximum never moves after tile 0); the unmutated reference restated by the mutant code is the reference"""
    b, ref, bar = bar_built(case, flav)
    by_name = {c['name']: c for c in ac.bar_cases()}
    for what in ac.MUTANTS:
        bm, refm, barm = b, ref, bar
        if what in ac.NEED_MOVE and case['sibling'] is not None:
            assert np.array_equal(ac.mutant(b, what), ac.mutant(b, 'swap j^0')), 'a case with a sibling has a moving maximum after all'
            bm, refm, barm = bar_built(by_name[case['sibling']], flav)
        ratio = float((np.abs(ac.mutant(bm, what) - refm) / barm).max())
        print(f"{case['name']} {flav} {what}: max |mutant - ref| / bar = {ratio:.1f}")
        MUTANT_RATIOS[(case['name'], flav, what)] = ratio
        assert ratio > 2.0, f"{case['name']} {flav}: the mutant '{what}' stays within 2 bar (largest ratio {ratio:.2f})"
    assert np.abs(ac.mutant(b, 'swap j^0') - ref).max() <= 1e-12 * np.abs(ref).max()


def test_smallest_mutant_ratio():
    if len(MUTANT_RATIOS) != len(ac.bar_cases()) * len(ac.FLAVOURS) * len(ac.MUTANTS):
        pytest.skip('the teeth tests of this module did not all run before this one')
    key = min(MUTANT_RATIOS, key=MUTANT_RATIOS.get)
    print(f'smallest mutant / bar over the deck: {MUTANT_RATIOS[key]:.2f} at {key}')
    assert MUTANT_RATIOS[key] > 2.0


def test_within_can_fail():
    c = ac.bar_cases()[1]
    b, ref, bar = bar_built(c, 'f16')
    with pytest.raises(AssertionError, match='outside the float64 bar'):
        nudged = ref.copy(); nudged[5, 7] += 1.01 * bar[5, 7]
        ac.within('planted', nudged, ref, bar)
    with pytest.raises(AssertionError, match='non-finite'):
        poisoned = ref.copy(); poisoned[0, 0] = np.nan
        ac.within('planted', poisoned, ref, bar)
