"""tests/rowcases.py proven without a GPU: the float64 references against torch's own group_norm / silu / softmax / casts, every seam of every
deck reached (the table is recomputed from the deck and has no empty row), every bar satisfied by a numpy emulation of the kernel's stated order in
the kernel's precision on every case, and every bar violated by the planted slips (a group index off by one channel, a dropped last pixel, rstd
without eps on the constant group): the bars can pass and can fail.  The null-pointer refusals of the GroupNorm entry points are checked here too:
a refused call returns before any launch, so it needs no device (and must never be tried with one)."""
import numpy as np
import pytest

from tests import rowcases as rc

torch = pytest.importorskip('torch')
F = torch.nn.functional
FLAVS = ('f32', 'f16', 'bf16')


# ---------------------------------------------------------------------------------------------------------------------
# the references are not self-made
@pytest.mark.parametrize('B,HW,C,G', [(2, 7, 12, 4), (1, 33, 96, 32), (3, 5, 8, 8), (2, 9, 16, 1)])
def test_references_against_torch(B, HW, C, G):
    rng = np.random.default_rng(HW + C)
    x = rng.standard_normal((B, HW, C)) * 1.7 + 0.3
    gamma, beta = 1 + 0.2 * rng.standard_normal(C), 0.2 * rng.standard_normal(C)
    mean, rstd = rc.gn_stats64(x, G)
    want = F.group_norm(torch.from_numpy(x).permute(0, 2, 1), G, torch.from_numpy(gamma), torch.from_numpy(beta), eps=rc.EPS).permute(0, 2, 1)
    assert np.allclose(rc.gn_apply64(x, mean, rstd, gamma, beta, 0), want.numpy(), rtol=1e-12, atol=1e-12)
    assert np.allclose(rc.gn_apply64(x, mean, rstd, gamma, beta, 1), F.silu(want).numpy(), rtol=1e-12, atol=1e-12)
    xt = torch.from_numpy(x).view(B, HW, G, C // G)
    assert np.allclose(mean, xt.mean(dim=(1, 3)).numpy(), rtol=1e-13, atol=1e-13)
    assert np.allclose(rstd, (xt.var(dim=(1, 3), unbiased=False) + rc.EPS).rsqrt().numpy(), rtol=1e-12)
    # partials of the same map, split unevenly
    part = np.zeros((B, 3, C, 2))
    for k, idx in enumerate(np.array_split(np.arange(HW), 3)):
        part[:, k, :, 0], part[:, k, :, 1] = x[:, idx].sum(1), (x[:, idx] ** 2).sum(1)
    pm, pr = rc.gn_part_stats64(part, HW, G)
    assert np.allclose(pm, mean, rtol=1e-12, atol=1e-13) and np.allclose(pr, rstd, rtol=1e-10)
    s = rng.standard_normal((B * 3, HW)) * 5
    assert np.allclose(rc.softmax_rows64(s, 0.25), F.softmax(torch.from_numpy(s) * 0.25, dim=-1).numpy(), rtol=1e-12, atol=1e-300)
    a = rng.standard_normal((B, C, HW))
    t = torch.from_numpy(a)
    assert np.array_equal(rc.nchw_to_nhwc(a), t.permute(0, 2, 1).contiguous().numpy())
    assert np.array_equal(rc.nhwc_to_nchw(rc.nchw_to_nhwc(a)), a)
    assert np.array_equal(rc.nchw_to_nhwc_pad(a, C + 3), F.pad(t.permute(0, 2, 1), (0, 3)).numpy())


@pytest.mark.parametrize('flav', ['f16', 'bf16'])
def test_cast_specials_are_the_edges_they_claim(flav):
    """torch's CPU cast on the special values: ties go to even on both sides, the overflow tie and everything above it is inf, the value just below
    it is the largest finite, half the smallest subnormal is 0 and anything above it the smallest subnormal; the round trip of every 16-bit pattern
    is the identity (so the 16 -> 32 reference is exact)"""
    p, emin, emax = (10, -14, 15) if flav == 'f16' else (7, -126, 127)
    sub, one = 2.0 ** (emin - p), 2.0 ** -p
    sp = rc.cast_specials(flav)
    got = dict(zip(sp.astype(np.float64).tolist(), rc.cast_from16(flav, rc.cast_to16(flav, sp)).astype(np.float64).tolist()))
    maxfin, tie = (2 - one) * 2.0 ** emax, (2 - one / 2) * 2.0 ** emax
    assert got[1 + one / 2] == 1.0 and got[1 + 3 * one / 2] == 1 + 2 * one and got[-(1 + one / 2)] == -1.0 and got[-(1 + 3 * one / 2)] == -(1 + 2 * one)
    assert got[sub / 2] == 0.0 and got[1.5 * sub] == 2 * sub and got[2.5 * sub] == 2 * sub and got[2.0 ** emin - sub / 2] == 2.0 ** emin
    assert got[float(np.nextafter(np.float32(sub / 2), np.float32(1)))] == sub and got[float(np.nextafter(np.float32(sub / 2), np.float32(0)))] == 0.0
    assert got[tie] == np.inf and got[-tie] == -np.inf and got[float(np.nextafter(np.float32(tie), np.float32(0)))] == maxfin and got[maxfin] == maxfin
    assert got[float(np.nextafter(np.float32(tie), np.float32(np.inf)))] == np.inf
    bits = rc.cast_to16(flav, sp)
    assert bits[0] == 0 and bits[1] == 0x8000 and np.isnan(rc.cast_from16(flav, bits)[np.isnan(sp)]).all()
    allbits = np.arange(1 << 16, dtype=np.uint16)
    back = rc.cast_to16(flav, rc.cast_from16(flav, allbits))
    nan = np.isnan(rc.cast_from16(flav, allbits))
    assert np.array_equal(back[~nan], allbits[~nan])
    for n in rc.CAST_NS:
        assert rc.build_cast_to16(flav, n).shape == (n,) and rc.build_cast_from16(flav, n).shape == (n,)


# ---------------------------------------------------------------------------------------------------------------------
# coverage
def _table(required, seams_by_id):
    table = {s: [i for i, have in seams_by_id.items() if s in have] for s in required}
    empty = [s for s, ids in table.items() if not ids]
    assert not empty, f'no case reaches: {empty}'
    return table


@pytest.mark.parametrize('flav', FLAVS)
def test_groupnorm_deck_reaches_every_seam(flav):
    geos = rc.gn_geometries(flav)
    table = _table(rc.GN_SEAMS[flav], {g: rc.seams_of(flav, g) for g in geos})
    vec = rc.FLAVOURS[flav]['vec']
    # the seams recomputed here from the kernels' index arithmetic, independently of seams_of
    assert any(256 % (C // vec) for _, _, C, _ in geos) and any(256 % (C // vec) == 0 for _, _, C, _ in geos)
    assert any((C // G) % vec and C // G > 1 for _, _, C, G in geos), 'no thread whose vector holds channels of two groups'
    for B, HW, C, G in geos:
        cv = C // vec
        rpp = 256 // cv
        assert rpp >= 1 and rpp * cv <= 256 and rpp * C * 16 <= 64 * 1024           # the statistics kernel's LDS: rpp C 2 doubles
    if flav == 'f32':
        at, past = table['unrolled loop: at the bound, not entered'], table['unrolled loop: one past the bound, entered']
        assert {g[2] for g in at} == {g[2] for g in past}                               # both sides for the same C
        for (B, HW, C, G), entered in [(g, False) for g in at] + [(g, True) for g in past]:
            rpp = 256 // (C // 4)
            assert HW <= 256 and any(prow + 3 * rpp < HW for prow in range(rpp)) == entered
    assert {r for _, _, r in rc.gn_cases(flav)} == {'randn', 'const', 'mean300', 'outlier', 'silu_neg'} | ({'mean1e4'} if flav == 'f32' else set())
    for g in rc.REGIME_GEOMETRIES:
        assert g[2] % g[3] == 0 and g[2] % 8 == 0 and g[3] > 1 and g[1] > 1         # the slips below need a second group and a second pixel


def test_other_decks_reach_their_seams():
    _table(rc.PART_SEAMS, {c: rc.part_seams_of(c) for _, c in rc.PART_CASES})
    _table(rc.SOFTMAX_SEAMS, {c: rc.softmax_seams_of(c) for c in rc.SOFTMAX_CASES})
    assert max(r * n for r, n, _, _ in rc.SOFTMAX_CASES) * 4 == 4099 * 1024 * 4 and rc.SOFTMAX_REFUSED == [0, 1025]
    assert {c[1] for c in rc.LAYOUT_CASES} == {1, 3, 32, 33} and {c[2] for c in rc.LAYOUT_CASES} == {1, 255, 4097} and {c[0] for c in rc.LAYOUT_CASES} == {1, 2}
    assert all(rc.layout_pads(C)[0] == C and C + 1 in rc.layout_pads(C) and (32 in rc.layout_pads(C)) == (C <= 32) for C in (1, 3, 32, 33))


# ---------------------------------------------------------------------------------------------------------------------
# the bars pass a correct kernel and fail the slips
def _regime_values_are_what_they_claim(b, mean, var):
    B, HW, C, G = b.geometry
    if b.regime == 'const':
        assert (var[:, 0] == 0).all() and (mean[:, 0] == 0.75).all() and (var[:, 1:] > 0).all()
    if b.regime in ('mean300', 'mean1e4'):
        ratio = np.abs(mean) / np.sqrt(var)
        want = 300 if b.regime == 'mean300' else 1e4
        assert (ratio > want / 2).all() and (ratio < want * 2).all()
    if b.regime == 'outlier':
        assert (np.abs(b.x).reshape(B, HW, G, C // G).max(axis=(1, 3)) == rc.FLAVOURS[b.flav]['fmax'] / 4).all()
    if b.regime == 'silu_neg':
        y = rc.gn_apply64(b.x, mean, 1 / np.sqrt(var + rc.EPS), b.gamma, b.beta, 0)
        assert -122 < y.min() < -115 and -65 < y.max() < -58 and (y < -88.8).any() and (y > -87).any()


@pytest.mark.parametrize('flav', FLAVS)
def test_groupnorm_bars_hold_the_emulation_and_reject_the_slips(flav):
    for cid, geo, regime in rc.gn_cases(flav):
        b = rc.build_gn(flav, geo, regime)
        B, HW, C, G = geo
        n = HW * (C // G)
        mean, var = rc.gn_moments64(b.x, G)
        _regime_values_are_what_they_claim(b, mean, var)
        rstd = 1 / np.sqrt(var + rc.EPS)
        bm, br = rc.bar_stats(mean, var, n)
        st = rc.emu_stats(b.x, G)
        assert rc.within(st[..., 0], mean, bm) and rc.within(st[..., 1], rstd, br), f'{flav} {cid}: the emulated statistics miss their bar'
        slips = ['group', 'pixel'] + (['eps'] if regime == 'const' else [])
        for slip in slips:
            bad = rc.emu_stats(b.x, G, slip=slip)
            if slip == 'group' and G == 1:
                assert np.array_equal(bad, st), 'with one group there is no other index: the slipped program is the program'
                continue
            assert not (rc.within(bad[..., 0], mean, bm) and rc.within(bad[..., 1], rstd, br)), f'{flav} {cid}: statistics bar lets slip {slip!r} through'
        # apply: on the emulated fp32 statistics, as the GPU test runs it on the kernel's
        m32, r32 = st[..., 0].astype(np.float64), st[..., 1].astype(np.float64)
        caught = {s: False for s in ('group', 'pixel')}
        for silu in (0, 1):
            ref = rc.gn_apply64(b.x, m32, r32, b.gamma, b.beta, silu)
            bar = rc.bar_apply(flav, b.x, m32, r32, b.gamma, b.beta, silu)
            assert rc.within(rc.emu_apply(flav, b.x, st, b.gamma, b.beta, silu), ref, bar), \
                f'{flav} {cid} silu={silu}: the emulated apply misses its bar ({rc.margin(rc.emu_apply(flav, b.x, st, b.gamma, b.beta, silu), ref, bar):.3g})'
            for slip in caught:
                caught[slip] |= not rc.within(rc.emu_apply(flav, b.x, st, b.gamma, b.beta, silu, slip=slip), ref, bar)
        if G == 1:
            assert np.array_equal(rc.group_of(C, G, 'group'), rc.group_of(C, G))
            caught['group'] = True
        assert all(caught.values()), f'{flav} {cid}: apply bar lets through {[s for s, c in caught.items() if not c]}'


def test_part_stats_bars_hold_the_emulation_and_reject_the_slips():
    for cid, case in rc.PART_CASES:
        B, nblk, HW, C, G = case
        x, part = rc.build_part(case)
        mean, var = rc.gn_moments64(x, G)
        rstd = 1 / np.sqrt(var + rc.EPS)
        pm, pr = rc.gn_part_stats64(part, HW, G)
        bm, br = rc.bar_stats(mean, var, HW * (C // G))
        assert rc.within(pm, mean, bm) and rc.within(pr, rstd, br), cid
        st = rc.emu_part_stats(part, HW, G)
        assert rc.within(st[..., 0], mean, bm) and rc.within(st[..., 1], rstd, br), cid
        for slip in ('group', 'pixel'):
            bad = rc.emu_part_stats(part, HW, G, slip=slip)
            if slip == 'group' and G == 1:
                assert np.array_equal(bad, st)
                continue
            assert not (rc.within(bad[..., 0], mean, bm) and rc.within(bad[..., 1], rstd, br)), f'{cid}: lets slip {slip!r} through'
    # rstd without eps: a map that is constant per channel group
    x = np.full((1, 64, 8), 0.75)
    part = np.stack([x.reshape(1, 4, 16, 8).sum(2), (x ** 2).reshape(1, 4, 16, 8).sum(2)], axis=-1)
    mean, var = rc.gn_moments64(x, 2)
    bm, br = rc.bar_stats(mean, var, 64 * 4)
    st, bad = rc.emu_part_stats(part, 64, 2), rc.emu_part_stats(part, 64, 2, slip='eps')
    assert (var == 0).all() and rc.within(st[..., 1], 1 / np.sqrt(var + rc.EPS), br) and not rc.within(bad[..., 1], 1 / np.sqrt(var + rc.EPS), br)


def test_scale_shift_bar_holds_the_emulation_and_rejects_the_slip():
    for case in rc.SCALE_SHIFT_CASES:
        B, C, G = case
        stats, gamma, beta = rc.build_scale_shift(case)
        t = rc.emu_scale_shift(stats, gamma, beta)
        m, r = stats[..., 0].astype(np.float64), stats[..., 1].astype(np.float64)
        bsc, bsh = rc.bar_scale_shift(m, r, gamma, beta, C)
        sc64 = rc.per_channel(r, C)[:, 0] * gamma.astype(np.float64)
        sh64 = beta.astype(np.float64) - rc.per_channel(m, C)[:, 0] * t[:, 0].astype(np.float64)
        assert rc.within(t[:, 0], sc64, bsc[:, 0]) and rc.within(t[:, 1], sh64, bsh[:, 0]), case
        fused = (beta.astype(np.float64) - rc.per_channel(m, C)[:, 0] * t[:, 0].astype(np.float64)).astype(np.float32)       # what one fma would give
        if C >= 96:
            assert not np.array_equal(fused, t[:, 1]), 'the deck cannot tell the separately rounded shift from the fused one'
        if G > 1:
            bad = rc.emu_scale_shift(stats, gamma, beta, slip='group')
            assert not (rc.within(bad[:, 0], sc64, bsc[:, 0]) and rc.within(bad[:, 1], sh64, bsh[:, 0])), case


def test_softmax_bar_holds_the_emulation_and_rejects_a_dropped_entry():
    for c in rc.SOFTMAX_CASES:
        rows, n, kind, scale = c
        x = rc.build_softmax(c)[:64]                         # (the emulation of 64 rows says what 4099 would)
        ref, bar = rc.softmax_rows64(x, scale), rc.bar_softmax(x, scale)
        got = rc.emu_softmax(x, scale)
        assert rc.within(got, ref, bar), f'{rc.softmax_id(c)}: {rc.margin(got, ref, bar):.3g}'
        if kind == 'peak':
            peak = ref.argmax(axis=1)
            assert (got[np.arange(len(x)), peak] == 1.0).all() and got.sum() == len(x), 'every other term must underflow to exactly 0'
        if kind == 'equal':
            assert np.array_equal(got, np.full_like(got, np.float32(1.0) / np.float32(n)))
        if kind in ('plain', 'equal') and n > 1:
            assert not rc.within(rc.emu_softmax(x, scale, slip='last'), ref, bar), f'{rc.softmax_id(c)}: lets a dropped entry through'


# ---------------------------------------------------------------------------------------------------------------------
def test_groupnorm_entry_points_refuse_null_pointers():
    """stats, gamma, beta, x and out are dereferenced by the kernels: a null one is VARHIP_EINVAL before any launch (the argument checks come first, so
    this runs without a device)"""
    from var_amd import abi, hip
    fn = hip.lib().fn
    buf = np.zeros(4096, np.float64)
    p = buf.ctypes.data
    for flav in FLAVS:
        C = 8
        for null in range(3):                      # x, stats, scratch
            a = [p, p, p]; a[null] = None
            assert fn['gn_stats_' + flav](*a, 1, 4, C, 2, 1e-6, None) == abi.EINVAL, (flav, 'stats', null)
        for null in range(5):                      # x, stats, gamma, beta, out
            a = [p] * 5; a[null] = None
            assert fn['gn_apply_' + flav](*a, 1, 4, C, 2, 0, None) == abi.EINVAL, (flav, 'apply', null)
    for null in range(2):
        a = [p, p]; a[null] = None
        assert fn['gn_stats_part_f32'](*a, 1, 1, 4, 8, 2, 1e-6, None) == abi.EINVAL
    for null in range(4):
        a = [p] * 4; a[null] = None
        assert fn['gn_scale_shift_f32'](*a, 1, 8, 2, None) == abi.EINVAL
    assert not buf.any()
