"""The decks of tests/attncases.py proven without a GPU.  The selector deck: the fp32 scores are exactly 128 / 0 in two summation orders, the
stated coverage recomputed from the cases, distinct non-zero V rows, and the oracle's twin returning the selected rows exactly (the CPU proof of
the exactness argument in the deck's docstring, eps = vm_exp_le0(-87) and all).  The bar deck: every score profile is what its name says, the
effective support stays small, the twin stays within the derived bar, vm_exp_le0 keeps the error bound the bar charges for it, and six mutants of
the float64 reference each leave 2 bar somewhere in every case (or in its named sibling).  The dispatch restated, and the forced-NW deck's table
of idle waves.  tests/test_attn_dispatch_gpu.py then runs the same decks through varhip_attn_cached_f32."""
import numpy as np
import pytest

from tests import attncases as ac
from tests import util


@pytest.fixture(scope='module')
def L():
    util.ensure_oracle_built()
    from oracle import var_oracle
    return var_oracle.lib()


def test_wave_heuristic_restated():
    """attn_waves (attn.hip) starts from NW = 4 and takes a smaller NW only for strictly fewer idle waves; NW = 1 leaves none, so the choice is the
    largest NW of 4, 3, 2, 1 that divides ceil(l / 32), and no launch of the dispatch has a wave with t0 >= l"""
    for l in range(1, 4097):
        nq = (l + 31) // 32
        assert ac.waves(l) == max(nw for nw in (1, 2, 3, 4) if nq % nw == 0) and ac.idle_waves(l) == 0 and ac.grid_x(l) * ac.waves(l) == nq
        assert ac.forced_idle(l, ac.waves(l)) == 0
    assert [ac.waves(l) for l in (1, 31, 33, 64, 65, 96, 97, 128, 161)] == [1, 1, 2, 2, 3, 3, 4, 4, 3]


def test_forced_deck_reaches_the_idle_waves():
    cases = ac.forced_cases()
    assert [c['l'] for c in cases] == [1, 33, 65, 97, 130]
    assert {c['l']: [ac.forced_idle(c['l'], nw) for nw in (1, 2, 3, 4)] for c in cases} == ac.FORCED_IDLE
    for c in cases:
        assert c['curL'] % 32 and c['Lmax'] > c['curL'] and (c['B2'], c['H']) == (2, 2) and c['l'] <= c['curL']
    idle = {(nw, n) for ls in ac.FORCED_IDLE.values() for nw, n in zip((1, 2, 3, 4), ls)}
    assert {n for _, n in idle} == {0, 1, 2, 3} and all(any(n for w, n in idle if w == nw) for nw in (2, 3, 4))
    assert all(any(nw != ac.waves(c['l']) and ac.forced_idle(c['l'], nw) == 0 for nw in (1, 2, 3, 4)) for c in cases if 32 < c['l'] <= 128)      # another NW than the dispatch's, no idle wave


# ---- the selector deck ------------------------------------------------------------------------------------------------------------------------
def test_selector_coverage_is_what_the_deck_states():
    got = ac.sel_coverage()
    assert got == ac.SEL_COVERAGE, {k: (got[k], ac.SEL_COVERAGE.get(k)) for k in got if got[k] != ac.SEL_COVERAGE.get(k)}
    cov = ac.SEL_COVERAGE
    assert cov['stage_pos'] == 64, 'every position of a tile in both K stages'
    assert set(cov['ragged_complete']) >= {1, 5, 17, 31} and set(cov['last_key_selected']) >= {1, 5, 17, 31} and cov['exact_multiple'] and cov['single_tile']
    assert cov['ntile_parity'] == [0, 1] and cov['lane_half'] == 64
    assert all(cov['nw'][nw] for nw in (1, 2, 3, 4)) and cov['nw_grid_gt1'] == [1, 2, 3, 4] and cov['nw_partial_last_wave'] == [1, 2, 3, 4]
    cases = ac.sel_cases()
    assert (cases[0]['l'], cases[0]['curL']) == (1, 1) and (cases[-1]['l'], cases[-1]['curL']) == (300, 319)
    assert any(c['Lmax'] == c['curL'] for c in cases) and max(c['B2'] * c['H'] * c['l'] * c['curL'] for c in cases) <= 2 * 3 * 300 * 319


def _chain(q, k, order):
    """the fp32 dot products q[t] . k[j] as one chain of additions in `order` -> (result [l][curL], every partial sum an integer)"""
    prod = (q[:, None, order] * k[None, :, order]).astype(np.float32)
    part = np.cumsum(prod, axis=2, dtype=np.float32)
    return part[:, :, -1], bool((part == np.rint(part)).all() and (np.abs(part) <= 128).all())


IL4 = np.array([(i & ~7) + ((i & 1) << 2) + ((i & 7) >> 1) for i in range(64)])          # the kernel's 4-interleaved order


@pytest.mark.parametrize('case', ac.sel_cases(), ids=lambda c: c['name'])
def test_selector_scores_rows_and_twin(L, case):
    b = ac.build_selector(case)
    B2, H, l, curL = case['B2'], case['H'], case['l'], case['curL']
    assert np.isnan(b.k[:, :, curL:]).all() and np.isnan(b.v[:, :, curL:]).all() and np.isfinite(b.k[:, :, :curL]).all()
    v_all = b.v[:, :, :curL]
    assert (v_all != 0).all() and (v_all == np.rint(v_all)).all() and np.abs(v_all).max() <= 128, 'V: non-zero integers of [-128, 128]'
    assert sorted(IL4.tolist()) == list(range(64))
    q = b.q.reshape(B2, l, H, 64)
    rows = np.arange(l)
    for bb in range(B2):
        for h in range(H):
            want = np.zeros((l, curL), np.float32)
            want[rows, b.sel[bb, h]] = 128.0
            for order in (np.arange(64), IL4):
                s, integral = _chain(q[bb, :, h], b.k[bb, h, :curL], order)
                assert integral and np.array_equal(s, want), f"{case['name']}: the fp32 scores are not exactly 128 / 0"
            v = b.v[bb, h, :curL]
            assert len(np.unique(v, axis=0)) == curL, f"{case['name']}: two keys of a slice hold the same V row"
            for b2 in range(B2):
                for h2 in range(H):
                    if (b2, h2) != (bb, h):
                        assert (b.v[b2, h2, b.sel[bb, h]] != v[b.sel[bb, h]]).any(1).all(), f"{case['name']}: another slice holds the same row at the same key"
    assert curL * 128 * 2.0 ** -125 < 2.0 ** -100, 'the stray mass'
    got = ac.twin(L, b)
    bad = np.argwhere(got != b.expected)
    assert bad.size == 0, f"{case['name']} twin: first mismatch at {tuple(bad[0])}: {got[tuple(bad[0])]!r} != {b.expected[tuple(bad[0])]!r}"


def test_a_zero_in_v_would_break_the_selector_argument(L):
    """why V holds no zero: channel 5 zeroed from key 32 on (l = 33, curL = 81, H = 1).  A query that selects one of those keys gets what tile 0
    left in the accumulator times eps, about 1e-36, where the one-hot softmax gives 0"""
    case = next(c for c in ac.sel_cases() if c['l'] == 33)
    assert case['H'] == 1
    b = ac.build_selector(case)
    b.v[:, :, 32:case['curL'], 5] = 0.0
    got = ac.twin(L, b)[:, 5][b.sel.reshape(-1) >= 32]
    assert got.size >= 33 and (np.abs(got) < 1e-30).all() and (got != 0).any()


# ---- the exponential --------------------------------------------------------------------------------------------------------------------------
def test_vm_exp_le0_keeps_the_bound_the_bar_charges(L):
    """vm_exp_le0 on [-87, 0] through the twin: one query per x, two keys with scores 0 and x exactly (k0 = 0, k1 = e0, q = x e0), v0 = e0, v1 = e1:
    out = (1, p) / (1 + p), so out[1] / out[0] is p within three roundings (1 + p, and the two products with inv)"""
    x = np.concatenate([-np.linspace(0.0, 87.0, 8192), -np.geomspace(1e-6, 87.0, 2048), [-87.0, -86.99999, -0.6931472, -0.34657359]]).astype(np.float32)
    b = ac.Built()
    b.case = dict(B2=1, H=1, l=x.size, curL=2, Lmax=3)
    b.q = np.zeros((x.size, 64), np.float32); b.q[:, 0] = x
    b.k = np.full((1, 1, 3, 64), np.nan, np.float32); b.k[0, 0, :2] = 0.0; b.k[0, 0, 1, 0] = 1.0
    b.v = np.full((1, 1, 3, 64), np.nan, np.float32); b.v[0, 0, :2] = 0.0; b.v[0, 0, 0, 0] = 1.0; b.v[0, 0, 1, 1] = 1.0
    out = ac.twin(L, b).astype(np.float64)
    p = out[:, 1] / out[:, 0]
    rel = np.abs(p / np.exp(x.astype(np.float64)) - 1.0)
    print(f'vm_exp_le0 on [-87, 0]: max relative error {rel.max():.3e} (three roundings of the quotient included)')
    assert rel.max() <= ac.E_EXP + 3 * 2.0 ** -24


# ---- the bar deck -----------------------------------------------------------------------------------------------------------------------------
def test_bar_deck_shape():
    cases = ac.bar_cases()
    assert {c['kind'] for c in cases} == {'asc', 'desc', 'late', 'split', 'split1', 'wide'} and {c['nw'] for c in cases} == {1, 2, 3, 4}
    names = {c['name'] for c in cases}
    for c in cases:
        assert c['B2'] <= 2 and c['H'] <= 3 and c['l'] <= c['curL'] <= 330 and (c['sibling'] is None or c['sibling'] in names)
    assert ac.C_ROUND == 64 + 1 + 1 and ac.E_EXP == 4e-7


@pytest.mark.parametrize('case', ac.bar_cases() + ac.forced_cases(), ids=lambda c: c['name'])
def test_bar_profiles_are_built_as_named(case):
    """on the float64 scores of the rounded operands: where the running maximum moves, per query"""
    b, ref, bar = ac.bar_built(case)
    curL, kind = case['curL'], case['kind']
    ntile, l = (curL + 31) // 32, case['l']
    assert np.isnan(b.k[:, :, curL:]).all() and np.isnan(b.v[:, :, curL:]).all() and np.isfinite(ref).all() and (bar > 0).all()
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
            assert len(np.unique(kstar)) >= min(ntile, 3) and len(np.unique(peak)) >= min(ntile, 3)
            assert (np.abs(q) @ np.abs(k).T).max() >= 100.0                                    # the score term of the bar is in play


@pytest.mark.parametrize('case', ac.bar_cases() + ac.forced_cases(), ids=lambda c: c['name'])
def test_twin_within_the_bar(L, case):
    b, ref, bar = ac.bar_built(case)
    ac.within(f"{case['name']} twin", ac.twin(L, b), ref, bar)


MUTANT_RATIOS = {}


@pytest.mark.parametrize('case', ac.bar_cases(), ids=lambda c: c['name'])
def test_bar_deck_has_teeth(case):
    """every mutant of the float64 reference is more than 2 bar away somewhere in the case (the two rescale mutants: in the named sibling, for a
    profile whose maximum never moves after tile 0); the unmutated reference restated by the mutant code is the reference"""
    b, ref, bar = ac.bar_built(case)
    by_name = {c['name']: c for c in ac.bar_cases()}
    for what in ac.MUTANTS:
        bm, refm, barm = b, ref, bar
        if what in ac.NEED_MOVE and case['sibling'] is not None:
            assert np.array_equal(ac.mutant(b, what), ac.mutant(b, 'swap j^0')), 'a case with a sibling has a moving maximum after all'
            bm, refm, barm = ac.bar_built(by_name[case['sibling']])
        ratio = float((np.abs(ac.mutant(bm, what) - refm) / barm).max())
        print(f"{case['name']} {what}: max |mutant - ref| / bar = {ratio:.1f}")
        MUTANT_RATIOS[(case['name'], what)] = ratio
        assert ratio > 2.0, f"{case['name']}: the mutant '{what}' stays within 2 bar (largest ratio {ratio:.2f})"
    assert np.abs(ac.mutant(b, 'swap j^0') - ref).max() <= 1e-12 * np.abs(ref).max()


def test_within_can_fail():
    b, ref, bar = ac.bar_built(ac.bar_cases()[1])
    with pytest.raises(AssertionError, match='outside the float64 bar'):
        nudged = ref.copy(); nudged[5, 7] += 1.01 * bar[5, 7]
        ac.within('planted', nudged, ref, bar)
    with pytest.raises(AssertionError, match='non-finite'):
        poisoned = ref.copy(); poisoned[0, 0] = np.nan
        ac.within('planted', poisoned, ref, bar)
