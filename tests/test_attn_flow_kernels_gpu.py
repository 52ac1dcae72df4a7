"""varhip_attn_rowstats_f32 and varhip_attn_flow_f32 on the GPU: bit for bit against their host twins, within the derived bars of the dense float64
restatement (tests/attnflowref.py), the exact properties of the contract, the tie to varhip_attn_cached_f32, refusals and NaN queries.
B = 2, H = 3 (one idle wave in the head round), Lmax = Lq + 7 with a NaN-filled cache tail, outputs sentinel-filled."""
import numpy as np
import pytest
import torch

from tests import attnflowref as R
from tests import util
from var_amd import hip

pytestmark = pytest.mark.gpu

ALPHA = 0.37
_CASES = {}


def case_of(ends):
    if ends not in _CASES:
        _CASES[ends] = R.make_case(ends)
    return _CASES[ends]


def _targets(T, Lq):
    return (np.arange(T) * 7 + Lq - 1) % Lq


def _l1(got, want):
    return np.abs(got.astype(np.float64) - want).sum(-1)


@pytest.mark.parametrize('ends', R.ENDS)
@pytest.mark.parametrize('T', [1, 5, 32])
def test_kernels_equal_their_twins_and_meet_the_bars(ends, T):
    case = case_of(ends)
    Lq = case['Lq']
    tg = _targets(T, Lq)
    lim = R.limits(ends, Lq)
    hot, dense = R.make_r(case, T, onehot=tg), R.make_r(case, T, seed=3)
    for r, ph, alpha in ((hot, True, 0.0), (dense, True, 0.0), (dense, False, ALPHA), (hot, False, 1.0), (dense, False, 0.0)):
        host = R.run(case, r, ph, alpha)
        dev = R.run(case, r, ph, alpha, device=True, out_fill=-7.0)                            # (the sentinel: every entry must be written)
        for k in ('m', 'rinv', 'out'):
            assert R.same_bits(dev[k], host[k]), f'{k}: {int((dev[k].view(np.uint32) != host[k].view(np.uint32)).sum())} of {dev[k].size} entries differ'
        assert not dev['nan'].any() and np.array_equal(dev['nan'], host['nan'])
        want, bar = R.reference(case, r, ph, alpha)
        err = _l1(dev['out'], want)
        print(f'ends={ends} T={T} per_head={ph} alpha={alpha}: worst L1 error / bar = {float((err / bar).max()):.3f} (bar up to {bar.max():.3e})')
        assert (err <= bar).all()
        total = dev['out'].astype(np.float64).sum(-1)
        assert (np.abs(total - 1) <= bar + 64 * R.U).all() and (dev['out'] >= 0).all()        # rows and rollouts sum to 1 (r does, up to its own rounding)
        if r is hot and ph:
            for s, t in enumerate(tg):                                                         # +0 at every key the target does not see
                assert not dev['out'][:, :, s, lim[t]:].view(np.uint32).any()
        if alpha == 0.0 and not ph:
            assert R.same_bits(dev['out'], r)                                                  # alpha = 0 returns r bit for bit


@pytest.mark.parametrize('ends', R.ENDS[1:])
def test_a_target_does_not_depend_on_the_others(ends):
    case = case_of(ends)
    Lq = case['Lq']
    tg = np.asarray([0, 3, 17, Lq - 37, Lq - 1])
    five = R.run(case, R.make_r(case, 5, onehot=tg), True, device=True)['out']
    assert (five[:, :, 0, 0] == 1.0).all() and not five[:, :, 0, 1:].view(np.uint32).any()     # token 0: exactly 1.0 at key 0
    big = R.run(case, R.make_r(case, 32, onehot=np.concatenate([np.arange(27), tg])), True, device=True)['out']
    assert R.same_bits(big[:, :, 27:], five)
    one = R.run(case, R.make_r(case, 1, onehot=tg[3:4]), True, device=True)['out']
    assert R.same_bits(one[:, :, 0], five[:, :, 3])
    r = R.make_r(case, 5, seed=1)
    roll5 = R.run(case, r, False, ALPHA, device=True)['out']
    roll1 = R.run(case, r[:, 2:3].copy(), False, ALPHA, device=True)['out']
    assert R.same_bits(roll1[:, 0], roll5[:, 2])


@pytest.mark.parametrize('ends', R.ENDS)
def test_rows_reproduce_the_attention_kernel(ends):
    """the one-hot rows of the last scale's first (up to) 32 queries, multiplied by V in float64, against varhip_attn_cached_f32's output for those
    queries (the last scale's queries over all Lq keys: exactly what the sampler launches); the bar is attnflowref's (e)"""
    case = case_of(ends)
    B, H, Lq, Lmax = case['B'], case['H'], case['Lq'], case['Lmax']
    own0 = int(ends[-2])
    l = Lq - own0
    T = min(32, l)
    tg = own0 + np.arange(T)
    rows = R.run(case, R.make_r(case, T, onehot=tg), True, device=True)['out'].astype(np.float64)      # (B, H, T, Lq)
    rng = np.random.default_rng(5)
    v = np.full((B, H, Lmax, 64), np.nan, np.float32)
    v[:, :, :Lq] = rng.standard_normal((B, H, Lq, 64)).astype(np.float32)
    q = torch.from_numpy(np.ascontiguousarray(case['q'][:, own0:])).cuda()
    out = torch.empty(B, l, H * 64, dtype=torch.float32, device='cuda')
    util.guarded_call('attn_cached_f32', q, torch.from_numpy(case['kc']).cuda(), torch.from_numpy(v).cuda(), out, B, l, H, Lq, Lmax)
    got = out.view(B, l, H, 64)[:, :T].permute(0, 2, 1, 3).double().cpu().numpy()               # (B, H, T, 64)
    want = np.einsum('bhsj,bhjc->bhsc', rows, v[:, :, :Lq].astype(np.float64))
    eps = R.dense(case)[1][:, :, tg]                                                            # (B, H, T)
    tol = (2 * eps + R.gamma(2 * Lq + 4))[..., None] * np.abs(v[:, :, :Lq]).max(2)[:, :, None, :]
    err = np.abs(got - want)
    print(f'ends={ends}: rows . V against attn_cached: worst error / bar = {float((err / tol).max()):.3f}')
    assert (err <= tol).all()


def _dev_args(case, T, per_head=1):
    B, H, Lq = case['B'], case['H'], case['Lq']
    f = lambda *s: torch.full(s, -7.0, dtype=torch.float32, device='cuda')
    a = dict(q=torch.from_numpy(case['q']).cuda(), kc=torch.from_numpy(case['kc']).cuda(), m=f(B, H, Lq), rinv=f(B, H, Lq),
             nan=torch.full((B, H), -7, dtype=torch.int32, device='cuda'), r=torch.zeros(B, T, Lq, device='cuda'),
             out=f(B, H, T, Lq), ends=torch.from_numpy(case['ends'].copy()))
    return a


def _call(a, case, T=5, **kw):
    """both entry points with the overrides kw -> the names that were refused"""
    p = dict(B=case['B'], Lq=case['Lq'], H=case['H'], Lmax=case['Lmax'], S1=len(case['ends']), T=T)
    p.update({k: v for k, v in kw.items() if k in p})
    t = dict(a)
    t.update({k: v for k, v in kw.items() if k not in p})
    refused = []
    for name, args in (('attn_rowstats_f32', (t['q'], t['kc'], p['B'], p['Lq'], p['H'], p['Lmax'], t['ends'], p['S1'], t['m'], t['rinv'], t['nan'])),
                       ('attn_flow_f32', (t['q'], t['kc'], t['m'], t['rinv'], t['r'], t['out'], p['B'], p['Lq'], p['H'], p['Lmax'], t['ends'], p['S1'],
                                          p['T'], 1, 0.5))):
        try:
            util.guarded_call(name, *args)
        except hip.VarHipError as e:
            assert 'EINVAL' in str(e)
            refused.append(name)
    return refused


def test_every_refusal_leaves_the_outputs_untouched():
    case = case_of(R.ENDS[0])
    a = _dev_args(case, 5)
    both = ['attn_rowstats_f32', 'attn_flow_f32']
    e = lambda *v: torch.tensor(v, dtype=torch.int32)
    mis = torch.zeros(case['q'].size + 4, dtype=torch.float32, device='cuda')[1:1 + case['q'].size].view(case['q'].shape)
    assert mis.data_ptr() % 16 == 4
    for kw in (dict(B=0), dict(Lq=0), dict(H=0), dict(Lmax=0), dict(Lmax=13), dict(S1=0), dict(S1=17), dict(B=65536), dict(H=65536), dict(q=None),
               dict(kc=None), dict(ends=None), dict(ends=e(1, 1, 14)), dict(ends=e(5, 1, 14)), dict(ends=e(1, 5, 13)), dict(ends=e(0, 5, 14)),
               dict(Lq=4097, Lmax=5000), dict(q=mis), dict(m=None), dict(rinv=None)):
        assert _call(a, case, **kw) == both, kw
    for kw in (dict(T=0), dict(T=33), dict(r=None), dict(out=None)):
        a['m'].fill_(0); a['rinv'].fill_(1); a['nan'].fill_(-7)
        assert _call(a, case, **kw) == both[1:], kw
        a['m'].fill_(-7); a['rinv'].fill_(-7)
    torch.cuda.synchronize()
    assert bool((a['out'] == -7).all()) and bool((a['nan'] == -7).all())
    assert _call(a, case, nan=None) == both[:1]                                                # (the flow launch of this pair is a good one)
    torch.cuda.synchronize()
    assert bool((a['m'] == -7).all()) and bool((a['rinv'] == -7).all()) and bool((a['nan'] == -7).all())
    a = _dev_args(case, 5)
    assert _call(a, case, T=0) == both[1:] and bool((a['out'] == -7).all()) and not bool((a['m'] == -7).any())


def test_a_nan_query_poisons_what_it_feeds_and_is_counted():
    case = R.make_case(R.ENDS[1], seed=7)
    tg = np.asarray([3, 40, 60])
    hot = R.make_r(case, 3, onehot=tg)
    clean = R.run(case, hot, True, device=True)
    bad = dict(case, q=case['q'].copy())
    bad['q'][1, 40, 64 + 5] = np.nan                                                           # row 1, query 40 (sees 55 keys), head 1
    got, host = R.run(bad, hot, True, device=True), R.run(bad, hot, True)
    assert got['nan'][1, 1] == 1 and got['nan'].sum() == 1 and np.isnan(got['rinv'][1, 1, 40]) and np.isnan(got['rinv']).sum() == 1
    want = clean['out'].copy()
    want[1, 1, :, :55] = np.nan
    assert R.same_bits(got['out'], want) and R.same_bits(got['out'], host['out'])
    roll = R.run(bad, hot, False, ALPHA, device=True)['out']
    assert R.same_bits(roll, R.run(bad, hot, False, ALPHA)['out'])
    assert np.isnan(roll[1, :, :55]).all() and not np.isnan(roll[0]).any() and not np.isnan(roll[1, :, 55:]).any()
