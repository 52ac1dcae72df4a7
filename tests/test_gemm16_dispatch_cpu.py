"""tests/gemm16cases.py without a GPU: the dispatch of var_amd/csrc/gemm16.hip (pick_tile16, split_rows16, small_pick, the thresholds of the deep
kernels, the persistence condition) restated in Python and compared with every hook code the table expects; the table's reach (every
instantiation, epilogue, store, pipeline-fill class and split variant, in both flavours); the conditions under which the reference is exact
and needs a real rounding; and planted faults, each of which must change the expectation of every case it applies to."""
import pytest

from tests import gemm16cases as gc

torch = pytest.importorskip('torch')


# ---------------------------------------------------------------------------------------------------------------------
# the dispatch, restated (var_amd/csrc/gemm16.hip: pick_tile16, split_rows16, run_gemm16 and the two small_launch lambdas)
def cdiv(a, b):
    return (a + b - 1) // b


def pick_tile16(M, N, batch, resid32, tile):
    if tile >= 0:
        return tile
    nb256, nb192, nb128 = cdiv(M, 256) * cdiv(N, 256) * batch, cdiv(M, 192) * cdiv(N, 256) * batch, cdiv(M, 128) * cdiv(N, 128) * batch
    if nb128 < 256:
        return 1
    t256 = float(cdiv(nb256, 256)) * (0.95 if resid32 else 1.0)
    t192 = float(cdiv(nb192, 256)) * 0.8625 if (batch == 1 and nb192 >= 256) else 1e30
    t128 = float(cdiv(nb128, 512)) * 0.62
    if t256 <= t128 and t256 <= t192:
        return 2
    return 3 if t192 < t128 * 0.95 else 0


def split_rows16(M, N, batch, tile):
    if tile >= 0 or batch != 1:
        return 0
    tilesN, tilesM = cdiv(N, 256), cdiv(M, 256)
    T = tilesM * tilesN
    rounds = T // 256
    frac = T / 256.0 - rounds
    if rounds < 3 or frac == 0.0 or frac >= 0.7:
        return 0
    mA = (rounds * 256) // tilesN
    return 0 if (mA < 1 or mA >= tilesM) else mA * 256


def small_code(entry, rows, N, batch, pick, deep):
    if pick == 0:
        return gc.K128
    if entry == 'nt':
        return (gc.K32D if cdiv(rows, 64) * cdiv(N, 64) * batch < 256 else gc.K64D) if deep else gc.K64
    return (gc.Q32D if cdiv(rows, 64) * cdiv(N, 128) < 256 else gc.Q64D) if deep else gc.Q64


def dispatch(c):
    """-> ((code of launch 0, code of launch 1 or 0), first row of the second launch or 0)"""
    M, N, batch = c['M'], c['N'], c['batch']
    resid32 = c['entry'] == 'nt' and c['epi'] == 'resid' and c['resid'] == 32
    persist_ok = bool(c['persist']) and N % 256 == 0
    mA = split_rows16(M, N, batch, c['tile'])
    if mA:
        rest = M - mA
        segs = [(mA, 2), (rest, 0 if cdiv(rest, 128) * cdiv(N, 128) >= 384 else 1)]
    else:
        segs = [(M, pick_tile16(M, N, batch, resid32, c['tile']))]
    codes = []
    for rows, pick in segs:
        if pick == 3:
            codes.append(gc.K192)
        elif pick == 2:
            codes.append(gc.KP if (persist_ok and rows % 256 == 0) else gc.K256)
        else:
            codes.append(small_code(c['entry'], rows, N, batch, pick, c['deep']))
    return tuple(codes + [0] * (2 - len(codes))), mA


ALL = gc.cases()
EXACT = [c for c in ALL if c['exact']]


def test_every_expected_hook_code_follows_from_the_dispatch():
    for c in ALL:
        got, _ = dispatch(c)
        assert got == c['expect'], f'{gc.name(c)}: the restated dispatch gives {got}'
    for base, variants in gc.equal_groups():
        for tile, persist, deep, code in variants:
            got, cut = dispatch(dict(base, tile=tile, persist=persist, deep=deep))
            assert got == (code, 0) and cut == 0, f'{gc.name(base)} tile {tile} persist {persist} deep {deep}: the restated dispatch gives {got}'


def test_the_abi_accepts_every_case():
    """the argument checks of varhip_gemm_nt_* / varhip_gemm_qkv_*, restated: K % 64, N % 4, lda / ldw / sA / sW % 8, ldo / ldr / ldg / sO % 4, no
    residual or gamma in a batched call, operands addressable through 32-bit byte offsets; the issue's K range"""
    for c in ALL + [b for b, _ in gc.equal_groups()]:
        g = gc.geometry(c)
        assert 64 <= c['K'] <= 320 and c['K'] % 64 == 0 and c['N'] % 4 == 0, gc.name(c)
        assert all(g[k] % 8 == 0 for k in ('lda', 'ldw', 'sA', 'sW')) and all(g[k] % 4 == 0 for k in ('ldo', 'ldr', 'ldg', 'sO')), gc.name(c)
        assert c['batch'] == 1 or (c['resid'] is None and not c['gamma']), gc.name(c)
        assert ((c['M'] - 1) * g['lda'] + c['K']) * 2 < 2 ** 32 and ((c['N'] - 1) * g['ldw'] + c['K']) * 2 < 2 ** 32, gc.name(c)
        assert g['sA'] > c['M'] * g['lda'] - 1 and (c['batch'] == 1 or (c['slack'] > 0 and g['sO'] > c['M'] * g['ldo'])), gc.name(c)
        if c['entry'] == 'qkv':
            assert c['pos0'] > 0 and c['Lmax'] > c['pos0'] + c['l'] and c['M'] == c['B2'] * c['l'], gc.name(c)


def _reached(flav, entry):
    return [c for c in ALL if c['flav'] == flav and c['entry'] == entry]


@pytest.mark.parametrize('flav', gc.FLAVOURS)
def test_the_table_reaches_every_instantiation_epilogue_store_and_fill_class(flav):
    ntc, qc = _reached(flav, 'nt'), _reached(flav, 'qkv')
    for code, inst in gc.NT_INST.items():
        mine = [c for c in ntc if c['expect'] == (code, 0) and c['tile'] >= 0 and c['batch'] == 1]
        bm, bn = inst['bm'], inst['bn']
        assert {c['mode'] for c in mine} >= set(gc.MODES), f'{code}: modes {sorted({c["mode"] for c in mine})}'
        assert {gc.fill_class(c['K'], inst['nst']) for c in mine if c['exact']} == {'below', 'equal', 'above'}, code
        assert {c['K'] for c in mine} >= set(gc.FILL_K[inst['nst']]), code
        assert any(c['M'] % bm == 0 and c['N'] % bn == 0 for c in mine), f'{code}: no exact fit'
        assert any(any(c['pad'][k] for k in c['pad']) and all(c['pad'].values()) for c in mine), f'{code}: no padded case'
        if code != gc.KP:
            assert any(c['M'] == 1 for c in mine) and any(c['M'] > bm and c['M'] % bm for c in mine), f'{code}: one row / ragged M'
            assert any(c['N'] % bn == 4 for c in mine), f'{code}: N four past the tile'
        for batch in (2, 40):
            assert any(c['expect'] == (code, 0) and c['batch'] == batch and c['slack'] > 0 for c in ntc), f'{code}: batch {batch}'
    for code, inst in gc.QKV_INST.items():
        mine = [c for c in qc if c['expect'] == (code, 0) and c['tile'] >= 0]
        assert {c['l2'] for c in mine} == {0, 1}, code
        assert {gc.fill_class(c['K'], inst['nst']) for c in mine if c['exact']} == {'below', 'equal', 'above'}, code
        assert any(any(c['pad'].values()) for c in mine), code
        if code != gc.KP:
            assert any(c['M'] == 1 for c in mine) and {1, 3} <= {c['H'] for c in mine}, f'{code}: M = 1, H 1 and 3'
    # the persistent kernel: 1 tile, 9 tiles, more than one round; what must fall through to k_gemm16<8,4,2,4>
    tiles = {cdiv(c['M'], 256) * cdiv(c['N'], 256) for c in ntc if c['expect'] == (gc.KP, 0) and c['batch'] == 1}
    assert {1, 9} <= tiles and max(tiles) > 256, tiles
    fall = [c for c in ntc + qc if c['group'] == 'fallthrough']
    assert all(c['tile'] == 2 and c['persist'] == 1 and c['expect'] == (gc.K256, 0) for c in fall)
    assert any(c['N'] % 256 and c['M'] % 256 == 0 for c in fall) and any(c['N'] % 256 == 0 and c['M'] % 256 for c in fall)
    # the row split: first segment persistent / k_gemm16<8,4,2,4> (N = 320), second 128x128 / 64-row kernel either side of 384, both entries
    split = {(c['entry'], c['expect']) for c in ntc + qc if c['group'] == 'split'}
    assert split >= {('nt', (gc.KP, gc.K64D)), ('nt', (gc.K256, gc.K64D)), ('nt', (gc.KP, gc.K128)), ('nt', (gc.K256, gc.K128)), ('nt', (gc.K256, gc.K64)),
                     ('qkv', (gc.KP, gc.Q64D)), ('qkv', (gc.K256, gc.Q64D)), ('qkv', (gc.K256, gc.Q64))}, split
    for c in ntc + qc:
        if c['group'] == 'split':
            cut = dispatch(c)[1]
            assert cut and (cut % c['l'] if c['entry'] == 'qkv' else (not c['gamma'] or cut % c['rpg'])), f'{gc.name(c)}: nothing straddles the cut'
    assert any(c['N'] == 320 and c['expect'][0] == gc.K256 for c in ntc if c['group'] == 'split')
    # the automatic picker reaches every pick and every small kernel
    auto = {c['expect'] for c in ntc + qc if c['group'] == 'picker'}
    assert auto >= {(k, 0) for k in (gc.K128, gc.K192, gc.KP, gc.K32D, gc.K64D, gc.Q32D, gc.Q64D)}, auto


def test_the_picker_cases_sit_one_step_either_side_of_each_decision():
    P = lambda M, N, b=1, r=False: pick_tile16(M, N, b, r, -1)
    assert P(3968, 1024) == 1 and P(4096, 1024) == 0                              # nb128 = 248 / 256
    assert (P(21632, 1024), P(4608, 3072), P(8192, 1024)) == (3, 2, 0)              # the comment's three shapes
    by = {(c['M'], c['N'], c['batch'], c['resid'] == 32): c['expect'][0] for c in gc.picker_cases() if c['entry'] == 'nt'}
    picks = {k: P(*k) for k in by}
    # each pick of the cost model appears, and neighbours (same N, the next M in the table) disagree at least once per decision
    assert {0, 2, 3} <= set(picks.values())
    pair = [c for c in gc.picker_cases() if c['entry'] == 'nt' and c['M'] == gc.RESID32_PAIR[0]['M']]
    assert len(pair) == 2 and {c['resid'] for c in pair} == {32, 16} and pair[0]['expect'] != pair[1]['expect'], 'the resid32 factor decides nothing'
    assert P(10816, 1024, 2) == 0 and P(21632, 1024, 1) == 3                        # batch > 1 excludes 192x256 at the same tile counts


def _exact_both_flavours():
    """every exact case in both flavours, the two of a case in a row (they share the operands, which are cached)"""
    for c in EXACT:
        if c['flav'] == gc.FLAVOURS[0]:
            for flav in gc.FLAVOURS:
                yield dict(c, flav=flav), flav


def test_every_exact_case_is_exact_and_needs_a_real_rounding():
    """per case: the budget (any order of partial sums stays below 2^24 units of the finest grid); 16-bit stores: at least a quarter of the exact
    results do not fit the output type; fp32 RESID stores: at least a quarter of gamma (acc + bias) does not fit the flavour's 16 bits"""
    for c, flav in _exact_both_flavours():
        o = gc.operands(c)
        rows = gc.probe_rows(c, dispatch(c)[1])
        assert gc.exactness_budget(c, o, rows) < 2.0 ** 24, gc.name(c)
        if c['entry'] == 'qkv':
            v = gc.acc64(o, rows) + o.bias
            assert gc.needs_rounding(v, flav) >= 0.25, gc.name(c)
        elif c['out16']:
            v = gc.before_resid(c, o, rows) + (o.resid[rows].double() if o.resid is not None else 0.0)
            assert gc.needs_rounding(v, flav) >= 0.25, f'{gc.name(c)}: {gc.needs_rounding(v, flav):.2f}'
            assert gc.needs_rounding(gc.acc64(o, rows), flav) >= 0.25, f'{gc.name(c)}: the sum before the bias fits'
        elif c['epi'] == 'resid':
            assert gc.needs_rounding(gc.before_resid(c, o, rows), flav) >= 0.25, gc.name(c)


def _differs(a, b):
    return any(not torch.equal(a[k][0], b[k][0]) or not torch.equal(gc.bits(a[k][1]), gc.bits(b[k][1])) for k in a)


def test_planted_faults_change_every_expectation_they_apply_to():
    hit = {f: 0 for f in gc.FAULTS}
    for c, flav in _exact_both_flavours():
        cut = dispatch(c)[1]
        faults = [f for f in gc.FAULTS if gc.applies(f, c, cut)]
        o = gc.operands(c)
        rows = gc.probe_rows(c, cut)
        good = gc.parts(c, flav, o, rows)
        for f in faults:
            assert _differs(good, gc.parts(c, flav, o, rows, fault=f, cut=cut)), f'{gc.name(c)}: the fault {f} leaves the expectation unchanged'
            hit[f] += 1
    assert all(n >= 2 for n in hit.values()), f'faults no case applies to: {[f for f, n in hit.items() if not n]}'


def test_scatter_places_every_part_and_leaves_the_fill():
    """expected(): values at their offsets, NaN everywhere else (padding of out, cache rows outside [pos0, pos0 + l)), on a padded batched case and a
    q/k/v case"""
    c = next(c for c in ALL if c['group'] == 'batched' and c['batch'] == 2 and c['exact'] and c['pad']['ldo'])
    want = gc.expected(c)['out']
    g = gc.geometry(c)
    inside = torch.zeros(want.numel(), dtype=torch.bool)
    inside.as_strided((2, c['M'], c['N']), (g['sO'], g['ldo'], 1)).fill_(True)
    assert bool(torch.isnan(want[~inside]).all()) and not bool(torch.isnan(want[inside]).any()) and int((~inside).sum()) > 0
    c = next(c for c in ALL if c['entry'] == 'qkv' and c['exact'] and c['B2'] > 1 and c['H'] > 1)
    e = gc.expected(c)
    kc = e['kc'].view(c['B2'], c['H'], c['Lmax'], 64)
    assert not bool(torch.isnan(e['q']).any()) and not bool(torch.isnan(kc[:, :, c['pos0']:c['pos0'] + c['l']]).any())
    assert bool(torch.isnan(kc[:, :, :c['pos0']]).all()) and bool(torch.isnan(kc[:, :, c['pos0'] + c['l']:]).all())
    o = gc.operands(c)
    ref = (o.A[0].double() @ o.W[0].double().T + o.bias).view(c['B2'], c['l'], 3, c['H'], 64)
    assert torch.equal(kc[:, :, c['pos0']:c['pos0'] + c['l']].double(), gc.round16(ref[:, :, 1], c['flav']).double().permute(0, 2, 1, 3))
