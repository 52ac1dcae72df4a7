"""varhip_ctl_sample_rows_f32 on the MI355X, with varhip_cfg_sample_rows_f32 — pinned elsewhere — as the reference for everything
but the three new stages, and tests/ctlref.py's numpy float32 restatement for those:
  null controls      bit-identical to the rows entry on the same operands
  bias, temperature  the rows entry on (x' | zero rows) with t = 0, x' = the combine, the add and the division formed in numpy: 1 * x' - 0 * 0 is x'
  min-p              the rows entry with top_p = 0, its filtered rows cut in numpy, the rows entry again with top_k = 0 and the case's top_p
  independence       every image of a mixed launch equals the B = 1 launch on its rows
All under both settings of varhip_sampler_force_walk, outputs pre-filled with sentinels, operands between guard bands."""
import numpy as np
import pytest

from tests import ctlref, util

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SHAPES = [(B, l, V) for V in (256, 4096, 8192) for l in (1, 5) for B in (1, 3)]
IDX_SENTINEL = -7
F = np.float32
TS = [0.0, 1.5 * (1 / 9), 4.0 * (7 / 9)]


def _hip():
    from var_amd import hip
    return hip


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _outputs(B, l, V):
    idx = torch.full((B * l,), IDX_SENTINEL, dtype=torch.int64, device='cuda')
    masked = torch.empty(B * l, V, device='cuda'); _bits(masked).fill_(-1)               # 0xFF bytes: a NaN the kernels never produce
    return idx, masked


def _case(B, l, V, seed):
    """logits (2, B, l, V) = 3 * randn and Exp(1) noise.  The last row of image 0 takes three values in both halves (a tie crowd larger than any
    sort buffer below V at the k-th value); element 0 of image 0's first row is a negative zero after the combine with t = 0."""
    rng = np.random.default_rng(seed)
    logits = (3.0 * rng.standard_normal((2, B, l, V))).astype(F)
    logits[:, 0, l - 1] = rng.integers(0, 3, size=V).astype(F)
    if l > 1:                                                          # ... and the row's maximum, so that no filter removes it
        logits[0, 0, 0] = -np.abs(logits[0, 0, 0]) - F(1.0)
        logits[0, 0, 0, 0], logits[1, 0, 0, 0] = -0.0, 1.0
    noise = rng.exponential(1.0, size=(B * l, V)).astype(F)
    return logits, noise


def _bias_table(V, ld, seed):
    """two rows with leading dimension ld: a smooth push with a banned stretch, and mostly zeros with bans and one large push"""
    rng = np.random.default_rng(seed)
    tab = np.full((2, ld), np.nan, F)                                  # (the padding is never read)
    tab[0, :V] = rng.standard_normal(V).astype(F); tab[0, 10:40] = -np.inf
    tab[1, :V] = 0.0; tab[1, ::3] = -np.inf; tab[1, 7] = 2.5
    return tab


def _rows(logits2, noise, B, l, V, ts, ks, ps, cap):
    idx, masked = _outputs(B, l, V)
    util.guarded_call('cfg_sample_rows_f32', logits2, noise, idx, masked, B, l, V, _dev(np.asarray(ts, np.float64)), _dev(np.asarray(ks, np.int32)),
                      _dev(np.asarray(ps, np.float64)), cap)
    return idx, masked


def _ctl(logits2, noise, B, l, V, ts, ks, ps, taus, mps, bias, brow, R, ld, cap):
    idx, masked = _outputs(B, l, V)
    util.guarded_call('ctl_sample_rows_f32', logits2, noise, idx, masked, B, l, V, _dev(np.asarray(ts, np.float64)), _dev(np.asarray(ks, np.int32)),
                      _dev(np.asarray(ps, np.float64)), _dev(np.asarray(taus, F)), _dev(np.asarray(mps, F)), bias,
                      None if brow is None else _dev(np.asarray(brow, np.int32)), R, ld, cap)
    return idx, masked


def _cap(ks, V):
    return V if 0 in ks else max(ks)


def _both_walks(fn):
    hip = _hip()
    try:
        for walk in (0, 1):
            hip.lib().so.varhip_sampler_force_walk(walk)
            fn(walk)
    finally:
        hip.lib().so.varhip_sampler_force_walk(0)


def _same(got, want, what):
    assert torch.equal(got[0], want[0]), (what, got[0], want[0])
    assert torch.equal(_bits(got[1]), _bits(want[1])), what


@pytest.mark.parametrize('B, l, V', SHAPES)
def test_null_controls_are_the_rows_entry_bit_for_bit(B, l, V):
    logits, noise = _case(B, l, V, seed=V + 10 * l + B)
    deck = [(min(900, V // 2), 0.96), (0, 0.5), (V // 4, 0.0)]
    ts, ks, ps = TS[:B], [d[0] for d in deck[:B]], [d[1] for d in deck[:B]]
    lg, nz = _dev(logits.reshape(2 * B * l, V)), _dev(noise)
    bias = _dev(_bias_table(V, V, 1))

    def check(walk):
        want = _rows(lg, nz, B, l, V, ts, ks, ps, _cap(ks, V))
        assert int(want[0].min()) >= 0
        _same(_ctl(lg, nz, B, l, V, ts, ks, ps, [1.0] * B, [0.0] * B, bias, [-1] * B, 2, V, _cap(ks, V)), want, (walk, 'bias_row = -1'))
        _same(_ctl(lg, nz, B, l, V, ts, ks, ps, [1.0] * B, [0.0] * B, None, None, 0, 0, _cap(ks, V)), want, (walk, 'no bias table'))
        if l > 1:                                                      # the planted negative zero is still one: no stage touched it
            assert int(_bits(want[1])[0, 0]) == -(1 << 31)
    _both_walks(check)


@pytest.mark.parametrize('B, l, V', SHAPES)
def test_bias_and_temperature_equal_the_rows_entry_on_rows_prepared_in_numpy(B, l, V):
    logits, noise = _case(B, l, V, seed=2 * V + 10 * l + B)
    ld = V + 4 if l == 5 else V
    tab = _bias_table(V, ld, 2)
    deck = [(1, 0.7, min(900, V // 2), 0.96), (-1, 1.0, 0, 0.5), (0, 2.5, V // 4, 0.0)]           # bias row, tau, top_k, top_p; image 1: neither
    ts, brow, taus, ks, ps = TS[:B], *[[d[i] for d in deck[:B]] for i in range(4)]
    x = ctlref.guided(logits[0], logits[1], ts)
    xp = np.stack([ctlref.bias_temper(x[b], None if brow[b] < 0 else tab[brow[b], :V], taus[b]) for b in range(B)])
    assert B == 1 or np.array_equal(xp[1].view(np.uint32), x[1].view(np.uint32))
    lg, nz = _dev(logits.reshape(2 * B * l, V)), _dev(noise)
    pair = _dev(np.concatenate((xp.reshape(B * l, V), np.zeros((B * l, V), F))))
    bias = _dev(tab)

    def check(walk):
        want = _rows(pair, nz, B, l, V, [0.0] * B, ks, ps, _cap(ks, V))
        got = _ctl(lg, nz, B, l, V, ts, ks, ps, taus, [0.0] * B, bias, brow, 2, ld, _cap(ks, V))
        assert int(got[0].min()) >= 0 and int(got[0].max()) < V
        _same(got, want, walk)
        m = got[1].view(B, l, V)
        assert bool((m[0, :, ::3] == float('-inf')).all())              # image 0 uses bias row 1: its bans hold
    _both_walks(check)


@pytest.mark.parametrize('B, l, V', SHAPES)
def test_min_p_equals_the_rows_entry_chained_through_the_numpy_cut(B, l, V):
    logits, noise = _case(B, l, V, seed=3 * V + 10 * l + B)
    deck = [(min(900, V // 2), 0.96, 0.2), (0, 0.5, 1.0), (V // 4, 0.0, 0.05)]                   # top_k, top_p, min_p
    ts, ks, ps, mps = TS[:B], *[[d[i] for d in deck[:B]] for i in range(3)]
    lg, nz = _dev(logits.reshape(2 * B * l, V)), _dev(noise)
    cap = _cap(ks, V)

    def check(walk):
        _, after_k = _rows(lg, nz, B, l, V, ts, ks, [0.0] * B, cap)
        a = after_k.cpu().numpy().reshape(B, l, V)
        cut = np.stack([ctlref.min_p_cut(a[b], mps[b]) for b in range(B)])
        pair = _dev(np.concatenate((cut.reshape(B * l, V), np.zeros((B * l, V), F))))
        want = _rows(pair, nz, B, l, V, [0.0] * B, [0] * B, ps, V)
        got = _ctl(lg, nz, B, l, V, ts, ks, ps, [1.0] * B, mps, None, None, 0, 0, cap)
        assert int(got[0].min()) >= 0 and int(got[0].max()) < V
        _same(got, want, walk)
        kept = (got[1] != float('-inf')).sum(-1).view(B, l)
        ties = int((a[0, l - 1] > -np.inf).sum())
        assert ties > max(cap, 2) or cap == V, (ties, cap)                # image 0's last row: the tie crowd at the k-th value exceeds the sort buffer
        if B > 1:
            assert bool((kept[1] == 1).all())                            # min_p = 1: the maximum alone
    _both_walks(check)


@pytest.mark.parametrize('l, V', [(l, V) for V in (256, 4096, 8192) for l in (1, 5)])
def test_every_image_equals_the_launch_on_its_rows_alone(l, V):
    B = 3
    logits, noise = _case(B, l, V, seed=4 * V + l)
    tab = _bias_table(V, V, 3)
    deck = [(1, 0.7, min(900, V // 2), 0.96, 0.2), (-1, 1.0, 0, 0.5, 0.0), (0, 2.5, V // 4, 0.0, 0.05)]
    brow, taus, ks, ps, mps = [[d[i] for d in deck] for i in range(5)]
    lg, nz, bias = _dev(logits.reshape(2 * B * l, V)), _dev(noise), _dev(tab)

    def check(walk):
        idx, masked = _ctl(lg, nz, B, l, V, TS, ks, ps, taus, mps, bias, brow, 2, V, _cap(ks, V))
        assert int(idx.min()) >= 0
        for b in range(B):
            one = _dev(logits[:, b].reshape(2 * l, V))
            i1, m1 = _ctl(one, _dev(noise[b * l:(b + 1) * l]), 1, l, V, TS[b:b + 1], ks[b:b + 1], ps[b:b + 1], taus[b:b + 1], mps[b:b + 1], bias,
                          brow[b:b + 1], 2, V, _cap(ks[b:b + 1], V))
            _same((i1, m1), (idx[b * l:(b + 1) * l], masked[b * l:(b + 1) * l]), (walk, b))
    _both_walks(check)


def test_a_refused_image_gets_minus_one_and_nothing_else():
    B, l, V = 3, 2, 1024
    logits, noise = _case(B, l, V, seed=5)
    lg, nz, bias = _dev(logits.reshape(-1, V)), _dev(noise), _dev(_bias_table(V, V, 4))
    good = dict(taus=[0.7, 1.0, 1.3], mps=[0.0, 0.1, 1.0], brow=[0, 1, -1], ks=[8, 8, 8])
    bad = [('taus', 0.0), ('taus', -1.0), ('taus', float('inf')), ('taus', float('nan')), ('mps', -0.1), ('mps', 1.5), ('mps', float('nan')),
           ('brow', 2), ('brow', 7), ('ks', 900), ('ks', -1)]
    for key, val in bad:
        a = {k: list(v) for k, v in good.items()}
        a[key][1] = val
        idx, masked = _ctl(lg, nz, B, l, V, TS, a['ks'], [0.0] * B, a['taus'], a['mps'], bias, a['brow'], 2, V, 8)
        i2 = idx.view(B, l)
        assert bool((i2[1] == -1).all()) and int(i2[[0, 2]].min()) >= 0, (key, val, idx)
        assert bool((_bits(masked).view(B, l, V)[1] == -1).all()), (key, val)
        assert bool(((masked.view(B, l, V)[[0, 2]] != float('-inf')).sum(-1) >= 1).all())
    idx, _ = _ctl(lg, nz, B, l, V, TS, good['ks'], [0.0] * B, good['taus'], good['mps'], bias, good['brow'], 2, V, 8)
    assert int(idx.min()) >= 0


def test_refused_calls_write_nothing():
    hip = _hip()
    from var_amd import abi
    B, l, V = 2, 3, 256
    lg = torch.zeros(2 * B * l * V + 4, device='cuda')
    nz = torch.ones(B * l, V, device='cuda')
    tk = torch.zeros(B, dtype=torch.int32, device='cuda')
    z64 = torch.zeros(B, dtype=torch.float64, device='cuda')
    tau, mp = torch.ones(B, device='cuda'), torch.zeros(B, device='cuda')
    bias = torch.zeros(2 * (V + 4) + 4, device='cuda')
    brow = torch.zeros(B, dtype=torch.int32, device='cuda')
    idx, masked = _outputs(B, l, V)
    fn, st = hip.lib().fn['ctl_sample_rows_f32'], hip.current_stream()
    invoke = lambda *a: fn(*a, st)
    #       0                    1   2    3       4  5  6  7    8   9    10   11  12                   13    14 15     16
    good = [lg[:2 * B * l * V], nz, idx, masked, B, l, V, z64, tk, z64, tau, mp, bias[:2 * (V + 4)], brow, 2, V + 4, V]
    bad = [(10, None), (11, None), (12, None), (12, bias[1:2 * (V + 4) + 1]), (14, -1), (15, V - 4), (15, V + 2), (0, None), (1, None), (2, None),
           (7, None), (8, None), (9, None), (0, lg[1:2 * B * l * V + 1]), (4, 0), (5, 0), (6, 0), (6, 255), (6, 260), (6, 8448), (16, 0), (16, V + 1)]
    for pos, val in bad:
        a = list(good); a[pos] = val
        rc = util.guarded_invoke('varhip_ctl_sample_rows_f32', a, invoke, torch.cuda.synchronize)
        assert rc == abi.EINVAL, (pos, val, rc)
        assert bool((idx == IDX_SENTINEL).all()) and bool((_bits(masked) == -1).all()), (pos, val)
    with pytest.raises(hip.VarHipError, match='EINVAL'):
        hip.call('ctl_sample_rows_f32', *[good[i] if i != 10 else None for i in range(len(good))])
    assert util.guarded_invoke('varhip_ctl_sample_rows_f32', good, invoke, torch.cuda.synchronize) == 0          # the same operands, accepted
    assert int(idx.min()) >= 0 and not bool((_bits(masked) == -1).any())
