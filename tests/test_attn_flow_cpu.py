"""VAR.attention_maps / VAR.attention_rollout without a GPU: the host twins of varhip_attn_rowstats_f32 and varhip_attn_flow_f32 against the dense
float64 restatement of tests/attnflowref.py within its derived bars, planted faults the bars must catch, the exact identities of the contract,
the argument checks, and the PyTorch twins, the result classes and the target parsing on a tiny CPU model."""
import contextlib
import copy
import ctypes
import io

import numpy as np
import pytest
import torch

from tests import attnflowref as R
from tests import util
from var_amd import abi, hip

ALPHA = 0.37


def _l1(got, want):
    return np.abs(got.astype(np.float64) - want).sum(-1)


@pytest.mark.parametrize('ends', R.ENDS)
@pytest.mark.parametrize('T', [1, 5, 32])
def test_host_twins_within_the_derived_bars(ends, T):
    case = R.make_case(ends)
    Lq = case['Lq']
    tg = (np.arange(T) * 7 + Lq - 1) % Lq
    hot = R.make_r(case, T, onehot=tg)
    got = R.run(case, hot, True)
    want, bar = R.reference(case, hot, True)
    err = _l1(got['out'], want)
    print(f'ends={ends} T={T}: rows, worst L1 error / bar = {float((err / bar).max()):.3f} (bar up to {bar.max():.3e})')
    assert (err <= bar).all() and not got['nan'].any()
    assert (np.abs(got['out'].astype(np.float64).sum(-1) - 1) <= bar).all()                    # each per-head row sums to 1
    lim = R.limits(ends, Lq)
    for s, t in enumerate(tg):                                                                 # +0 at every key the target does not see
        assert not got['out'][:, :, s, lim[t]:].view(np.uint32).any()
    dense = R.make_r(case, T, seed=3)
    for ph, alpha in ((True, 0.0), (False, ALPHA), (False, 1.0)):
        got = R.run(case, dense, ph, alpha)
        want, bar = R.reference(case, dense, ph, alpha)
        err = _l1(got['out'], want)
        print(f'ends={ends} T={T} per_head={ph} alpha={alpha}: worst L1 error / bar = {float((err / bar).max()):.3f}')
        assert (err <= bar).all()
        if not ph:
            assert (got['out'] >= 0).all() and (np.abs(got['out'].astype(np.float64).sum(-1) - 1) <= bar + 32 * R.U).all()


def test_exact_identities():
    case = R.make_case(R.ENDS[1])
    Lq = case['Lq']
    r = R.make_r(case, 5, seed=1)
    assert R.same_bits(R.run(case, r, False, 0.0)['out'], r)                                   # alpha = 0 returns r
    tg = np.asarray([0, 3, 17, 54, 90])
    five = R.run(case, R.make_r(case, 5, onehot=tg), True)['out']
    assert (five[:, :, 0, 0] == 1.0).all() and not five[:, :, 0, 1:].any()                     # token 0 sees key 0 only
    full = np.concatenate([np.arange(27), tg])                                                 # the same targets among others, T = 32
    big = R.run(case, R.make_r(case, 32, onehot=full), True)['out']
    assert R.same_bits(big[:, :, 27:], five)                                                   # ... do not depend on T or on the other targets
    one = R.run(case, R.make_r(case, 1, onehot=tg[3:4]), True)['out']
    assert R.same_bits(one[:, :, 0], five[:, :, 3])
    roll5 = R.run(case, r, False, ALPHA)['out']
    roll1 = R.run(case, r[:, 2:3].copy(), False, ALPHA)['out']
    assert R.same_bits(roll1[:, 0], roll5[:, 2])
    # a one-hot row is a row of P: the per-head mean of the rows is the rollout's one layer at alpha = 1, up to the rounding of the mean
    m1 = R.run(case, R.make_r(case, 5, onehot=tg), False, 1.0)['out']
    assert np.abs(m1 - five.astype(np.float64).mean(1)).max() <= 4 * R.U


def test_planted_faults_are_caught():
    case = R.make_case(R.ENDS[1], seed=2)
    H, Lq = case['H'], case['Lq']
    r = R.make_r(case, 5, seed=2)
    want, bar = R.reference(case, r, False, ALPHA)
    good = R.run(case, r, False, ALPHA)
    assert (_l1(good['out'], want) <= bar).all()
    wrong = dict(case, ends=np.asarray((1, 5, 14, 30, 56, 91), np.int32))                      # a visibility limit off by one key
    assert (_l1(R.run(wrong, r, False, ALPHA)['out'], want) > bar).any()
    ones = np.ones_like(good['rinv'])                                                          # a missing rinv
    assert (_l1(R.run(case, r, False, ALPHA, rowstats=(good['m'], ones))['out'], want) > bar).any()
    heads = R.run(case, r, True)['out'].astype(np.float64)                                     # a head left out of the mean
    assert (_l1((1 - ALPHA) * r + ALPHA * heads[:, :H - 1].sum(1) / H, want) > bar).any()
    assert (_l1(R.run(case, r, False, 1 - ALPHA)['out'], want) > bar).any()                    # a swapped alpha
    hot = R.make_r(case, 25, onehot=np.arange(30, 55))                                         # the queries whose limit `wrong` moves
    want, bar = R.reference(case, hot, True)
    assert (_l1(R.run(case, hot, True)['out'], want) <= bar).all()
    assert (_l1(R.run(wrong, hot, True)['out'], want) > bar).any()
    assert (_l1(R.run(case, hot, True, rowstats=(good['m'], ones))['out'], want) > bar).any()


def test_rollout_over_layers_within_the_bar():
    """three 'layers' (three cases of the same geometry), last to first, against the float64 product"""
    cases = [R.make_case(R.ENDS[2], seed=s) for s in (4, 5, 6)]
    tg = np.asarray([0, 31, 32, 33, 96])
    r = R.make_r(cases[0], 5, onehot=tg)
    r64 = r.astype(np.float64)
    for c in reversed(cases):
        r64 = R.reference(c, r64, False, ALPHA)[0]
        r = R.run(c, r, False, ALPHA)['out']
    eps_max = max(float(R.dense(c)[1].max()) for c in cases)                                   # E0 at ||r||_1 = 1 with every eps at its maximum; 128 = 32 ceil(97 / 32)
    bar = R.rollout_bar(3, ALPHA * (eps_max + R.gamma(128) * (1 + eps_max)) + R.gamma(cases[0]['H'] + 6) * (1 + eps_max))
    err = _l1(r, r64)
    print(f'three-layer rollout: worst L1 error {err.max():.3e} (bar {bar:.3e})')
    assert (err <= bar).all() and (r >= 0).all() and (np.abs(r.astype(np.float64).sum(-1) - 1) <= bar).all()
    assert not r[:, 0, 1:].any() and (r[:, 0, 0] == 1.0).all()                                 # token 0 stays on key 0 exactly


def test_nan_query_poisons_what_it_feeds_and_is_counted():
    case = R.make_case(R.ENDS[1], seed=7)
    H, Lq = case['H'], case['Lq']
    tg = np.asarray([3, 40, 60])
    hot = R.make_r(case, 3, onehot=tg)
    clean = R.run(case, hot, True)
    bad = dict(case, q=case['q'].copy())
    bad['q'][1, 40, 64 + 5] = np.nan                                                           # row 1, query 40 (scale 4: sees 55 keys), head 1
    got = R.run(bad, hot, True)
    assert got['nan'][1, 1] == 1 and got['nan'].sum() == 1 and np.isnan(got['rinv'][1, 1, 40]) and np.isnan(got['rinv']).sum() == 1
    want = clean['out'].copy()
    want[1, 1, :, :55] = np.nan                                                                # 0 * NaN: every target of (row 1, head 1), at the keys query 40 sees
    assert R.same_bits(got['out'], want)
    assert not got['out'][1, 1, :, 55:].view(np.uint32)[[0, 1]].any()                          # targets 3 and 40 keep +0 beyond
    roll = R.run(bad, hot, False, ALPHA)['out']
    assert np.isnan(roll[1, :, :55]).all() and not np.isnan(roll[0]).any() and not np.isnan(roll[1, :, 55:]).any()
    huge = dict(case, q=case['q'].copy())
    huge['q'][0, 0, :64] = np.float32(3e38)                                                    # a score that overflows: no finite maximum
    assert R.run(huge, hot, True)['nan'][0, 0] == 1


def _rc(name, c, **kw):
    B, H, Lq = c['B'], c['H'], c['Lq']
    T = kw.pop('Tbuf', 5)
    a = dict(q=c['q'], kc=c['kc'])
    if name == 'attn_flow_host_f32':
        a.update(m=np.zeros((B, H, Lq), np.float32), rinv=np.ones((B, H, Lq), np.float32), r=np.zeros((B, T, Lq), np.float32),
                 out=np.full((B, H, T, Lq), -7, np.float32))
    a.update(B=B, Lq=Lq, H=H, Lmax=c['Lmax'], ends=c['ends'], S1=len(c['ends']))
    if name == 'attn_flow_host_f32':
        a.update(T=T, per_head=1, alpha=0.5)
    else:
        a.update(m=np.full((B, H, Lq), -7, np.float32), rinv=np.full((B, H, Lq), -7, np.float32), nan=np.full((B, H), -7, np.int32))
    a.update(kw)
    args = [ctypes.c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else v for v in a.values()]
    return hip.lib().host[name](*args), a


@pytest.mark.parametrize('name', ['attn_rowstats_host_f32', 'attn_flow_host_f32'])
def test_argument_checks(name):
    c = R.make_case(R.ENDS[0])
    assert _rc(name, c)[0] == 0
    outs = ('out',) if 'flow' in name else ('m', 'rinv', 'nan')
    bad = [dict(B=0), dict(Lq=0), dict(H=0), dict(Lmax=0), dict(Lmax=13), dict(S1=0), dict(S1=17), dict(B=65536), dict(H=65536), dict(q=None), dict(kc=None),
           dict(ends=None), dict(ends=np.asarray([1, 1, 14], np.int32)), dict(ends=np.asarray([5, 1, 14], np.int32)),
           dict(ends=np.asarray([1, 5, 13], np.int32)), dict(ends=np.asarray([0, 5, 14], np.int32)), dict(Lq=4097, Lmax=5000)]
    bad += [dict(T=0), dict(T=33), dict(m=None), dict(rinv=None), dict(r=None), dict(out=None)] if 'flow' in name else [dict(m=None), dict(rinv=None), dict(nan=None)]
    for kw in bad:
        rc, a = _rc(name, c, **kw)
        assert rc == abi.EINVAL, kw
        assert all(a[o] is None or (a[o] == -7).all() for o in outs), kw
    mis = np.zeros(c['q'].size + 1, np.float32)[1:].reshape(c['q'].shape)                       # 4 bytes off a 16-byte boundary
    if mis.ctypes.data % 16:
        assert _rc(name, c, q=mis)[0] == abi.EINVAL


# ---- the PyTorch twins, the result classes and the target parsing on a tiny CPU model -----------------------------------------------------------
_M = {}


def _model(l2=True):
    if l2 not in _M:
        from models import build_vae_var
        _, meta = util.load_case('t_pn12345')
        meta = dict(meta, attn_l2_norm=l2)
        var_sd, vae_sd = util.make_weights(meta)
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'],
                                     shared_aln=meta['shared_aln'], attn_l2_norm=l2)
        var.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in var_sd.items()}, strict=False)
        vae.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vae_sd.items()}, strict=False)
        _M[l2] = (vae.eval(), var.eval())
    return _M[l2]


def _inputs(var, n=3):
    g = torch.Generator().manual_seed(0)
    return torch.randint(0, var.V, (n, var.L), generator=g), torch.tensor([1, 2, var.num_classes][:n])


TARGETS = (0, 3, (2, 1, 1), 29, (4, 4, 4))


@pytest.mark.parametrize('l2', [True, False])
def test_torch_twins_against_the_dense_product(l2):
    """every row of P from attention_maps (all L tokens as targets, two calls), the rollout as the explicit float64 product of the D matrices
    (1 - alpha) I + alpha Pbar, and the per-scale sums of the rows against attention_profile's integer shares"""
    from var_amd.models.var import AttentionMaps, AttentionRollout
    vae, var = _model(l2)
    gt, lab = _inputs(var)
    L, S, H, D = var.L, len(var.patch_nums), var.num_heads, var.depth
    a = var.attention_maps(gt, lab, tuple(range(32)))
    b = var.attention_maps(gt, lab, tuple(range(32, L)))
    assert isinstance(a, AttentionMaps) and 'AttentionMaps(' in repr(a) and a.rows.shape == (3, D, H, 32, L) and a.rows.dtype == torch.float32
    assert a.nan_queries.shape == (3, D, H) and a.nan_queries.dtype == torch.int32 and not a.nan_queries.any()
    P = torch.cat((a.rows, b.rows), 3).double()                                                # (3, D, H, L, L)
    assert float((P.sum(-1) - 1).abs().max()) <= L * 2.0 ** -23
    lim = torch.tensor([e for (_, e), pn in zip(var.begin_ends, var.patch_nums) for _ in range(pn * pn)])
    assert not P[..., torch.arange(L)[None, :] >= lim[:, None]].any()                          # block-causal: exactly 0
    prof = var.attention_profile(gt, lab, return_tokens=True)
    mass = torch.cat((a.scale_mass(), b.scale_mass()), 3)                                      # (3, D, H, L, S)
    assert mass.shape == (3, D, H, L, S) and mass.dtype == torch.float64
    assert float((mass - prof.tokens[..., :S].double() / 2 ** 21).abs().max()) <= 2.0 ** -21 + L * 2.0 ** -30 + L * 2.0 ** -23
    r = var.attention_rollout(gt, lab, TARGETS, alpha=0.3)
    assert isinstance(r, AttentionRollout) and 'AttentionRollout(' in repr(r) and r.flow.shape == (3, 5, L) and r.alpha == 0.3
    assert r.targets == (0, 3, 9, 29, 54) and r.layers == tuple(range(D)) and r.patch_nums == tuple(var.patch_nums)
    M = torch.eye(L, dtype=torch.float64).expand(3, L, L)
    for d in reversed(range(D)):
        M = M @ (0.7 * torch.eye(L, dtype=torch.float64) + 0.3 * P[:, d].mean(1))
    want = M[:, list(r.targets)]
    err = float((r.flow.double() - want).abs().max())
    print(f'attn_l2_norm={l2}: rollout twin against the product of the float32 rows: {err:.3e}')
    assert err <= D * L * 2.0 ** -23                                                           # the rows went through float32 once: 2^-24 each, L per sum, D layers
    assert float((r.flow.double().sum(-1) - 1).abs().max()) <= L * 2.0 ** -23 and bool((r.flow >= 0).all())
    assert torch.equal(var.attention_rollout(gt, lab, TARGETS, alpha=0.0).flow, torch.nn.functional.one_hot(torch.tensor(r.targets), L).float().expand(3, -1, -1))


def test_result_classes_and_invariances():
    vae, var = _model()
    gt, lab = _inputs(var)
    L, S, H, D = var.L, len(var.patch_nums), var.num_heads, var.depth
    m = var.attention_maps(gt, lab, TARGETS)
    r = var.attention_rollout(gt, lab, TARGETS)
    assert m.targets == r.targets == (0, 3, 9, 29, 54) and r.alpha == 0.5
    for x, lead in ((m, (3, D, H)), (r, (3,))):
        sm = x.scale_mass()
        assert sm.shape == lead + (5, S) and float((sm.sum(-1) - 1).abs().max()) <= L * 2.0 ** -23
        scale_of = [0, 1, 2, 3, 4]                                                             # the targets' scales
        for s, sc in enumerate(scale_of):
            assert not sm[..., s, sc + 1:].any()
        field = getattr(x, x._FIELD)
        for si, pn in enumerate(var.patch_nums):
            v = x.scale_maps(si)
            assert v.shape == lead + (5, pn, pn) and v.data_ptr() == field[..., var.begin_ends[si][0]:].data_ptr()
        with pytest.raises(ValueError):
            x.scale_maps(S)
    one = var.attention_maps(gt[1:2], lab[1:2], TARGETS[2:4], layers=(1,))
    assert one.layers == (1,) and torch.equal(one.rows[0, 0], m.rows[1, 1][:, 2:4])
    assert torch.equal(var.attention_rollout(gt[1:2], lab[1:2], TARGETS[3:]).flow[0], r.flow[1, 3:])
    ev = r.evidence(scales=(0, 1, 2, 3, 4), size=32)
    from var_amd.models.var import EvidenceMaps
    assert isinstance(ev, EvidenceMaps) and ev.pred.shape == (3, 32, 32)


def test_target_parsing_and_refusals():
    from var_amd.models import args as A
    pns = (1, 2, 3, 4, 5)
    assert A.flow_targets([0, (1, 1, 1), (4, 0, 0), 54], pns) == (0, 4, 30, 54)
    assert A.flow_targets(torch.tensor([3, 7]), pns) == (3, 7) and A.flow_targets(np.asarray([[2, 0, 1]]), pns) == (6,) and A.flow_targets(5, pns) == (5,)
    assert len(A.flow_targets(list(range(32)), pns)) == 32
    for bad in ([], list(range(33)), [55], [-1], [(5, 0, 0)], [(1, 2, 0)], [(1, 0, -1)], [(1, 0)], [1.5], [True], 'ab', None, [(1, 0.0, 0)]):
        with pytest.raises(ValueError, match='targets must be'):
            A.flow_targets(bad, pns)
    assert A.rollout_alpha(0) == 0.0 and A.rollout_alpha(1.0) == 1.0
    for bad in (-0.1, 1.1, float('nan'), 'x', None, True):
        with pytest.raises(ValueError, match='alpha'):
            A.rollout_alpha(bad)
    vae, var = _model()
    gt, lab = _inputs(var)
    D = var.depth
    for kw in (dict(layers=(1, 0)), dict(layers=(D,)), dict(layers=()), dict(max_rows=0)):
        with pytest.raises(ValueError):
            var.attention_maps(gt, lab, TARGETS, **kw)
        with pytest.raises(ValueError):
            var.attention_rollout(gt, lab, TARGETS, **kw)
    with pytest.raises(ValueError):
        var.attention_rollout(gt, lab, TARGETS, alpha=2)
    with pytest.raises(ValueError):
        var.attention_maps(gt, lab[:2], TARGETS)
    with pytest.raises(ValueError):
        var.attention_maps(gt, lab, [var.L])


def test_torch_twins_f32_against_f64():
    """the figures attnflowref.TORCH_F32_VS_F64_ROWS / _FLOW record: float32 modules against float64 modules, PyTorch alone"""
    worst = [0.0, 0.0]
    for l2 in (True, False):
        vae, var = _model(l2)
        gt, lab = _inputs(var)
        v64 = copy.deepcopy(var).double()
        worst[0] = max(worst[0], float((var.attention_maps(gt, lab, TARGETS).rows - v64.attention_maps(gt, lab, TARGETS).rows).abs().max()))
        worst[1] = max(worst[1], float((var.attention_rollout(gt, lab, TARGETS).flow - v64.attention_rollout(gt, lab, TARGETS).flow).abs().max()))
    print(f'attention_maps_torch, f32 modules against f64 modules: rows {worst[0]:.3e}, flow {worst[1]:.3e}')
    assert worst[0] <= 4 * R.TORCH_F32_VS_F64_ROWS and worst[1] <= 4 * R.TORCH_F32_VS_F64_FLOW
