"""The case table, the operand builder and the float64 bound of tests/gemmcases.py, validated without a GPU: varref_gemm_nt_f32 and
varref_gemm_qkv_f32 run over the whole table on guarded host arenas.  Every case must leave the padding of `out` at the sentinel, write
every element inside [M][N] with a finite value (all padding of the inputs is NaN) and stay within the float64 bound; the twin is
bit-stable from call to call.  tests/test_gemm_dispatch_gpu.py then runs the same table through every dispatch path of the HIP library."""
import numpy as np
import pytest

from tests import gemmcases as gc
from tests import util


@pytest.fixture(scope='module')
def L():
    util.ensure_oracle_built()
    from oracle import var_oracle
    return var_oracle.lib()


def test_table_covers_what_it_claims():
    rag = gc.ragged_cases()
    for tile in range(4):
        mine = [c for c in rag if c['tile'] == tile and c['pick'] != gc.PICK_ANY]
        assert len(mine) >= 36 and {c['epi'] for c in mine} == {0, 1, 2}
        for key, vals in (('M', gc.M_VALUES), ('N', gc.N_VALUES), ('K', gc.K_VALUES)):
            assert {c[key] for c in mine} == set(vals)
        assert any(not c['bias'] for c in mine) and any(c['epi'] == 2 and not c['gamma'] for c in mine) and any(c['epi'] == 2 and c['gamma'] for c in mine)
        assert all(c['M'] % c['rpg'] for c in mine)
        assert [c for c in rag if c['tile'] == tile and c['pick'] == gc.PICK_ANY and c['K'] == 40]
    # the vec / evec predicates of the dispatch, restated on the case's geometry: every "broken" case breaks exactly one term
    def vec_terms(c):
        return [c['K'] % 32 != 0, c['lda'] % 4 != 0, c['ldw'] % 4 != 0, c['sA'] % 4 != 0, c['sW'] % 4 != 0, c['offA'] % 4 != 0, c['offW'] % 4 != 0]
    def evec_terms(c):
        res = c['epi'] == 2
        gam = res and c['gamma']
        return [c['N'] % 4 != 0, c['ldo'] % 4 != 0, c['sO'] % 4 != 0, c['offO'] % 4 != 0, bool(c['bias'] and not c['bpr'] and c['offB'] % 4),
                bool(res and c['ldr'] % 4), bool(res and c['offR'] % 4), bool(gam and c['ldg'] % 4), bool(gam and c['offG'] % 4)]
    seen = set()
    for c in gc.vec_cases():
        n = sum(vec_terms(c))
        assert n == (1 if c['pick'] == gc.PICK_ANY else 0), c['name']
        assert sum(evec_terms(c)) == 0, c['name']
        if n:
            seen.add(vec_terms(c).index(True))
    assert seen == set(range(7))
    seen = set()
    for c in gc.evec_cases():
        assert sum(vec_terms(c)) == 0 and c['pick'] == gc.PICK_OF_TILE[c['tile']], c['name']
        n = sum(evec_terms(c))
        assert n == (0 if ' ctl ' in c['name'] else 1) and c['evec'] == 1 - n, c['name']
        if n:
            seen.add((c['tile'], evec_terms(c).index(True)))
    assert seen == {(t, i) for t in range(4) for i in range(9)}
    # every case that asserts varhip_gemm_last_evec expects what the predicate gives on its geometry (-1 on the fallback)
    for group in ('ragged', 'vec', 'evec', 'fallback', 'batched'):
        for c in gc.GROUPS[group]():
            assert c['evec'] == (-1 if c['pick'] == gc.PICK_ANY else int(not any(evec_terms(c)))), c['name']
            assert (c['pick'] == gc.PICK_ANY) == any(vec_terms(c)), c['name']
    # the three epilogues of k_dma_gemm meet padded ldo, ldr and ldg on every tile: the lean one needs evec, a column bias and a full BM x BN
    # tile inside M x N, the general loop with 16-byte accesses takes the partial tiles of the same call, the element-wise one the broken cases
    for tile, (BM, BN) in gc.TILE_DIMS.items():
        mine = [c for c in gc.evec_cases() if c['tile'] == tile]
        lean = [c for c in mine if c['evec'] == 1 and c['bias'] and not c['bpr'] and c['M'] >= BM and c['N'] >= BN and (c['M'] % BM or c['N'] % BN)]
        for epi in (0, 1, 2):
            assert any(c['epi'] == epi and c['ldo'] > c['N'] for c in lean), (tile, epi)
        assert any(c['epi'] == 2 and c['ldr'] > c['N'] for c in lean) and any(c['epi'] == 2 and c['gamma'] and c['ldg'] > c['N'] and c['offG'] for c in lean)
        assert any(c['ldo'] > c['N'] and c['ldr'] > c['N'] and c['ldg'] > c['N'] and c['epi'] == 2 for c in lean)
        slow = [c for c in mine if c['evec'] == 0 and c['M'] >= BM and c['N'] >= BN]
        assert any(c['ldo'] > c['N'] for c in slow) and any(c['epi'] == 2 and c['ldr'] > c['N'] for c in slow) and any(c['epi'] == 2 and c['ldg'] > c['N'] for c in slow)
    # k_gemm_any's epilogue meets each leading dimension padded by a multiple of 4 and by an odd amount, and gamma behind an interior pointer
    fb = gc.fallback_cases()
    assert all(c['K'] % 32 for c in fb)
    for key, epi in (('ldo', 0), ('ldo', 1), ('ldo', 2), ('ldr', 2), ('ldg', 2)):
        pads = {(c[key] - c['N']) % 4 == 0 for c in fb if c['epi'] == epi and c[key] > c['N'] and (key != 'ldg' or c['gamma'])}
        assert pads == {True, False}, (key, epi)
    assert any(c['offG'] >= c['N'] for c in fb) and any(c['batch'] > 1 and c['sO'] > c['M'] * c['ldo'] for c in fb)
    bat = gc.batched_cases()
    for tile in (0, 1, 2, 3, None):
        mine = [c for c in bat if (c['pick'] == gc.PICK_ANY) == (tile is None) and (tile is None or c['tile'] == tile)]
        assert {(c['batch'], bool(c['sA']), bool(c['sW']), c['bpr'], c['epi']) for c in mine} == {(b, a, w, r, e) for b in (2, 3) for a in (False, True)
                                                                                                  for w in (False, True) for r in (0, 1) for e in (0, 1)}
        assert {(c['M'], c['N']) for c in mine} == {(33, 68), (130, 36)} and all(c['sO'] > c['M'] * c['ldo'] for c in mine)


@pytest.mark.parametrize('group', sorted(gc.GROUPS))
def test_twin_on_the_case_table(L, group):
    call = gc.host_call(L)
    for c in gc.GROUPS[group]():
        _, res = gc.run_case(c, call)
        _, again = gc.run_case(c, call)
        for a, b in zip(res, again):
            assert np.array_equal(gc.bits(a), gc.bits(b)), f"{c['name']}: the twin is not bit-stable"


def test_twin_refuses_batched_resid_and_gamma(L):
    for c in gc.einval_cases():
        gc.run_case(c, gc.host_call(L))


@pytest.mark.parametrize('HW', [36, 100])
def test_twin_on_the_attnblock_geometry(L, HW):
    gc.attn_chain(gc.host_call(L), Cc=32, HW=HW)


def test_the_checks_can_fail(L):
    """planted faults: ldo read as N, one row of A read one element late, and a result off by four bounds"""
    c = gc.nt('planted', 33, 36, 64, 0, ldo=40)
    call = gc.host_call(L)

    def wrong_ldo(c_, name, args, outs):
        args = list(args); args[6] = c['N']
        return call(c_, name, args, outs)
    with pytest.raises(AssertionError, match='padding elements of out were written'):
        gc.run_case(c, wrong_ldo)

    def late_a(c_, name, args, outs):
        args = list(args); args[0] = (args[0], 1)
        return call(c_, name, args, outs)
    with pytest.raises(AssertionError, match='non-finite'):
        gc.run_case(gc.nt('planted', 33, 36, 64, 0, lda=68), late_a)

    def nudged(c_, name, args, outs):
        (out,) = call(c_, name, args, outs)
        b = gc.build_nt(c)
        _, bound = gc.reference_nt(b.A64, b.W64, b.bias64, 0)
        out[:c['N']] += (4 * bound[0, 0]).astype(np.float32)
        return [out]
    with pytest.raises(AssertionError, match='outside the float64 bound'):
        gc.run_case(c, nudged)
