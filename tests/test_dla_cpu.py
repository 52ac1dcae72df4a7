"""VAR.logit_attribution without a GPU: the host twins of varhip_dla_target_f32, varhip_dla_direction_f32 and varhip_rowdot_seg_f64 against the
numpy restatement tests/dlaref.py, bit for bit and inside guard bands, on padded leading dimensions with NaN padding; their refusals; the
argument checks; LogitAttribution's methods; and logit_attribution_torch in float64 on a tiny CPU model: completeness, margin against an
explicit rival, and layer subsets."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

from tests import dlaref as DR
from tests import util
from var_amd import abi, hip

_M = {}
SENT = np.float32(-7.5)


def host(name, *args):
    fn = hip.lib().host[name]
    return util.guarded_invoke('varhip_' + name, list(args), lambda *a: fn(*a))


def bits(a):
    return a.view(np.int64) if a.dtype == np.float64 else a.view(np.int32) if a.dtype == np.float32 else a


def same(a, b):
    """equal bits, any NaN equal to any NaN (the twins promise a NaN, not its payload)"""
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == 'f' else a == b))


# ---- the target ------------------------------------------------------------------------------------------------------------------------------
def target_case(R, l, V, seed):
    """logits with planted rows: 0 a tie at the rival, 1 gt is the arg-max, 2 gt is not, 3 (l > 3) an out-of-range gt, 4 a NaN row, 5 an
    out-of-range rival"""
    g = np.random.default_rng(seed)
    z = g.standard_normal((R, l, V)).astype(np.float32)
    gt = g.integers(0, V, (R, l))
    ag = g.integers(0, V, (R, l))
    zz, gg, aa = z.reshape(-1, V), gt.reshape(-1), ag.reshape(-1)
    n = R * l
    if V >= 5:
        gg[0] = 2; zz[0, 1] = zz[0, 4] = 9.0; zz[0, 2] = 9.0                                 # the greatest three times, gt among them: rival 1
        if n > 1: gg[1 % n] = 3; zz[1, 3] = 11.0
        if n > 2: gg[2] = 0; zz[2, V - 1] = 12.0
        if n > 3: gg[3] = V
        if n > 4: zz[4, V // 2] = np.nan
        if n > 5: aa[5] = -1
        if n > 6: aa[6] = V
    return z, gt, ag


@pytest.mark.parametrize('V', [5, 4096, 4100])
@pytest.mark.parametrize('R, l', [(1, 1), (3, 4), (1, 9), (3, 9)])
def test_target_twin_is_the_restatement(R, l, V):
    z, gt, ag = target_case(R, l, V, V + l)
    ld = l + 3
    pad = lambda a, fill, dt: np.concatenate([a.astype(dt), np.full((R, 3), fill, dt)], 1)
    gtp, agp = pad(gt, -1, np.int64), pad(ag, -1, np.int64)
    for mode in (0, 1, 2):
        rival, value = np.full((R, ld), -9, np.int64), np.full((R, ld), SENT, np.float32)
        assert host('dla_target_host_f32', z, gtp, agp if mode == 2 else None, ld, mode, R, l, V, rival, value, ld) == 0
        wr, wv = DR.target(z, gt, ag, mode)
        assert np.array_equal(rival[:, :l], wr) and same(value[:, :l], wv), mode
        assert (rival[:, l:] == -9).all() and (value[:, l:] == SENT).all()
        if V >= 5:
            assert (wr.reshape(-1)[0], wv.reshape(-1)[0]) == ((-1, 9.0) if mode == 0 else (1, 0.0) if mode == 1 else (int(ag.reshape(-1)[0]), wv.reshape(-1)[0]))
            if R * l > 6:
                f = lambda a: a.reshape(-1)
                assert f(wr)[3] == -1 and np.isnan(f(wv)[3]) and f(wr)[4] == -1 and np.isnan(f(wv)[4])
                assert mode != 1 or (f(wr)[1] != 3 and f(wv)[1] > 0 and f(wr)[2] == V - 1 and f(wv)[2] < 0)
                assert mode != 2 or (f(wr)[5] == -1 and np.isnan(f(wv)[5]) and f(wr)[6] == -1 and np.isnan(f(wv)[6]))


def test_target_refusals_write_nothing():
    R, l, V = 2, 3, 8
    z, gt, ag = target_case(R, l, V, 1)
    gt, ag = gt.astype(np.int64), ag.astype(np.int64)
    good = dict(ld_gt=l, mode=2, R=R, l=l, V=V, ld_out=l)
    for bad in (dict(R=0), dict(l=0), dict(V=0), dict(mode=3), dict(mode=-1), dict(ld_gt=l - 1), dict(ld_out=l - 1), *[dict(null=i) for i in range(5)]):
        a = dict(good, **{k: v for k, v in bad.items() if k != 'null'})
        rival, value = np.full((R, l), -9, np.int64), np.full((R, l), SENT, np.float32)
        ops = [z, gt, ag, rival, value]
        if 'null' in bad:
            ops[bad['null']] = None
        assert host('dla_target_host_f32', ops[0], ops[1], ops[2], a['ld_gt'], a['mode'], a['R'], a['l'], a['V'], ops[3], ops[4], a['ld_out']) == abi.EINVAL, bad
        assert (rival == -9).all() and (value == SENT).all(), bad
    rival, value = np.full((R, l), -9, np.int64), np.full((R, l), SENT, np.float32)
    assert host('dla_target_host_f32', z, gt, None, l, 1, R, l, V, rival, value, l) == 0              # against may be NULL outside mode 2


# ---- the direction ---------------------------------------------------------------------------------------------------------------------------
def direction_case(R, l, C, V, seed):
    g = np.random.default_rng(seed)
    x = (g.standard_normal((R * l, C)) * 3 + 0.5).astype(np.float32)
    hn = np.full((R, 2 * C + 4), np.nan, np.float32)                              # scale | shift | NaN padding
    hn[:, :2 * C] = g.standard_normal((R, 2 * C)).astype(np.float32) * 0.3
    W = (g.standard_normal((V, C)) * 0.02).astype(np.float32)
    b = g.standard_normal(V).astype(np.float32)
    a, r = g.integers(0, V, (R, l)), g.integers(0, V, (R, l))
    if R * l > 3:
        a.reshape(-1)[1] = V; r.reshape(-1)[2] = -1; r.reshape(-1)[3] = a.reshape(-1)[3]          # out of range twice; rival == target: g = 0
    return x, hn, W, b, a.astype(np.int64), r.astype(np.int64)


@pytest.mark.parametrize('C', [128, 1024])
@pytest.mark.parametrize('R, l, V', [(1, 1, 5), (3, 4, 4100), (1, 9, 4096), (3, 9, 5), (1, 256, 4096)])
def test_direction_twin_is_the_restatement(R, l, C, V):
    x, hn, W, b, a, r = direction_case(R, l, C, V, C + l)
    ld, ldo = l + 2, l + 1
    pad = lambda t: np.concatenate([t, np.full((R, 2), -1, np.int64)], 1)
    for rival in (None, r):
        ghat = np.full((R * l, C), SENT, np.float32)
        konst, gx = np.full((R, ldo), -3.0), np.full((R, ldo), -3.0)
        assert host('dla_direction_host_f32', x, hn, hn[:, C:], hn.shape[1], W, b, pad(a), None if rival is None else pad(rival), ld, R, l, C, V,
                    1e-6, ghat, konst, gx, ldo) == 0
        wg, wk, wx = DR.direction(x, hn[:, :C], hn[:, C:2 * C], W, b, a, rival, l, 1e-6)
        assert same(ghat, wg) and same(konst[:, :l], wk) and same(gx[:, :l], wx)
        assert (konst[:, l:] == -3.0).all() and (gx[:, l:] == -3.0).all()
        if R * l > 3:
            f = lambda t: t[:, :l].reshape(-1)
            assert np.isnan(f(konst)[1]) and np.isnan(ghat[1]).all() and np.isfinite(f(konst)[0]) and np.isfinite(ghat[0]).all()
            assert (rival is None) == bool(np.isfinite(f(gx)[2]))
            if rival is not None:
                assert not ghat[3].any() and f(konst)[3] == 0.0 and f(gx)[3] == 0.0
    # the identity the kernel exists for, in float64: r . (LN(x) (1 + s) + sh) + b_a - b_b = ghat . x + konst
    gh, kc = DR.ghat64(x, hn[:, :C], hn[:, C:2 * C], W, b, np.clip(a.reshape(-1), 0, V - 1), np.clip(r.reshape(-1), 0, V - 1), l, 1e-6)
    xd = x.astype(np.float64)
    ln = (xd - xd.mean(-1, keepdims=True)) / np.sqrt(xd.var(-1) + np.float64(np.float32(1e-6)))[:, None]
    row = np.arange(R * l) // l
    aa, rr = np.clip(a.reshape(-1), 0, V - 1), np.clip(r.reshape(-1), 0, V - 1)
    direct = ((W[aa].astype(np.float64) - W[rr]) * (ln * (1 + hn[row, :C].astype(np.float64)) + hn[row, C:2 * C])).sum(-1) + b[aa].astype(np.float64) - b[rr]
    assert np.abs(direct - ((gh * xd).sum(-1) + kc)).max() <= 1e-12


def test_direction_refusals_write_nothing():
    R, l, C, V = 2, 3, 128, 9
    x, hn, W, b, a, r = direction_case(R, l, C, V, 3)
    good = dict(ld_hn=hn.shape[1], ld_tok=l, R=R, l=l, C=C, V=V, eps=1e-6, ld_out=l)

    def odd(t):
        """a copy of t 4 bytes past where numpy put a buffer"""
        buf = np.zeros(t.size + 4, t.dtype)
        v = buf[1:1 + t.size].reshape(t.shape)
        v[...] = t
        return v
    for bad in (dict(R=0), dict(l=0), dict(C=0), dict(V=0), dict(C=126), dict(ld_hn=C - 4), dict(ld_hn=hn.shape[1] + 2), dict(ld_tok=l - 1), dict(ld_out=l - 1),
                dict(eps=-1.0), dict(eps=float('nan')), *[dict(null=i) for i in (0, 1, 2, 3, 4, 5, 7, 8, 9)], *[dict(odd=i) for i in (0, 1, 3, 7)]):
        k = dict(good, **{key: v for key, v in bad.items() if key not in ('null', 'odd')})
        ghat, konst, gx = np.full((R * l, C), SENT, np.float32), np.full((R, l), -3.0), np.full((R, l), -3.0)
        ops = [x, hn, hn[:, C:], W, b, a, r, ghat, konst, gx]
        if 'null' in bad:
            ops[bad['null']] = None
        if 'odd' in bad:
            ops[bad['odd']] = odd(ops[bad['odd']])
            if ops[bad['odd']].ctypes.data % 16 == 0:
                continue
        assert host('dla_direction_host_f32', *ops[:3], k['ld_hn'], *ops[3:7], k['ld_tok'], k['R'], k['l'], k['C'], k['V'], k['eps'], *ops[7:], k['ld_out']) == abi.EINVAL, bad
        assert (ghat == SENT).all() and (konst == -3.0).all() and (gx == -3.0).all(), bad


# ---- the row dots ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C, nseg', [(128, 1), (128, 2), (1024, 1), (1024, 16), (1024, 4), (24, 2), (12, 1), (4, 1)])
@pytest.mark.parametrize('M', [1, 9, 257])
def test_rowdot_twin_is_the_restatement(M, C, nseg):
    g = np.random.default_rng(M + C + nseg)
    lda, ldb = C + 4, C + 8
    a, b = np.full((M, lda), np.nan, np.float32), np.full((M, ldb), np.nan, np.float32)
    a[:, :C] = (g.standard_normal((M, C)) * 1e3).astype(np.float32)
    b[:, :C] = g.standard_normal((M, C)).astype(np.float32)
    out = np.full((M, nseg), -3.0)
    assert host('rowdot_seg_host_f64', a, lda, b, ldb, M, C, nseg, out) == 0
    want = DR.rowdot(a[:, :C], b[:, :C], nseg)
    assert same(out, want)
    exact = np.array([[sum(float(a[m, j]) * float(b[m, j]) for j in range(s * C // nseg, (s + 1) * C // nseg)) for s in range(nseg)] for m in range(min(M, 3))])
    assert np.abs(out[:3] - exact).max() <= 1e-9 * np.abs(exact).max() + 1e-12
    one = np.full((M, nseg), -3.0)                                              # ldb == 0: one vector for every row
    assert host('rowdot_seg_host_f64', a, lda, b[0, :C].copy(), 0, M, C, nseg, one) == 0
    assert same(one, DR.rowdot(a[:, :C], b[0, :C], nseg))


def test_the_order_is_the_stated_one():
    """a row whose float64 sum depends on the order: the twin gives the stated order's, which differs from the ascending sum"""
    C = 1024
    g = np.random.default_rng(0)
    a = (g.standard_normal((1, C)) * 10.0 ** g.integers(-6, 7, (1, C))).astype(np.float32)
    b = g.standard_normal((1, C)).astype(np.float32)
    out = np.zeros((1, 1))
    assert host('rowdot_seg_host_f64', a, C, b, C, 1, C, 1, out) == 0
    asc = 0.0
    for j in range(C):
        asc += float(a[0, j]) * float(b[0, j])
    assert out[0, 0] == DR.rowdot(a, b, 1)[0, 0] and out[0, 0] != asc


def test_rowdot_refusals_write_nothing():
    M, C = 3, 128
    a, b = np.ones((M, C), np.float32), np.ones((M, C), np.float32)
    good = dict(lda=C, ldb=C, M=M, C=C, nseg=2)
    shifted = np.ones(M * C + 4, np.float32)[1:1 + M * C].reshape(M, C)
    for bad in (dict(M=0), dict(C=0), dict(nseg=0), dict(nseg=3), dict(nseg=64), dict(C=126, nseg=1), dict(lda=C - 4), dict(ldb=C - 4), dict(lda=C + 2),
                dict(ldb=C + 2), dict(null=0), dict(null=1), dict(null=2), dict(odd=0), dict(odd=1)):
        k = dict(good, **{key: v for key, v in bad.items() if key not in ('null', 'odd')})
        out = np.full((M, 2), -3.0)
        ops = [a, b, out]
        if 'null' in bad:
            ops[bad['null']] = None
        if 'odd' in bad:
            if shifted.ctypes.data % 16 == 0:
                continue
            ops[bad['odd']] = shifted
        assert host('rowdot_seg_host_f64', ops[0], k['lda'], ops[1], k['ldb'], k['M'], k['C'], k['nseg'], ops[2]) == abi.EINVAL, bad
        assert (out == -3.0).all(), bad


def test_the_twins_have_the_launchers_signatures():
    for k in ('dla_target', 'dla_direction'):
        assert abi.SIGNATURES_HOST[k + '_host_f32'] == abi.SIGNATURES_HIP_ONLY[k + '_f32']
    assert abi.SIGNATURES_HOST['rowdot_seg_host_f64'] == abi.SIGNATURES_HIP_ONLY['rowdot_seg_f64']
    mk = open(util.ROOT + '/var_amd/csrc/Makefile').read()
    assert 'dla.hip' in mk.split('SRCS16')[0] and 'dla' in mk.split('CHECKED')[1].split('\n')[0].split()


# ---- the public call on a tiny CPU model: the PyTorch route, in float64 --------------------------------------------------------------------------
def _model():
    if 'm' not in _M:
        from models import build_vae_var
        _, meta = util.load_case('t_pn12345')
        var_sd, vae_sd = util.make_weights(meta)
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'], shared_aln=meta['shared_aln'])
        var.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in var_sd.items()}, strict=False)
        vae.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in vae_sd.items()}, strict=False)
        var.eval(); vae.eval()
        g = torch.Generator().manual_seed(0)
        gt, lab = torch.randint(0, var.V, (3, var.L), generator=g), torch.tensor([1, 2, var.num_classes])
        v64 = copy.deepcopy(var).double()
        v64.vae_proxy = (copy.deepcopy(vae).double(),)
        _M['m'] = (var, v64, gt, lab)
    return _M['m']


def _t64(**kw):
    from var_amd.models.var import logit_attribution_torch
    var, v64, gt, lab = _model()
    with torch.no_grad():
        return logit_attribution_torch(v64, gt, lab, **kw)


def test_float64_completeness_on_a_tiny_model():
    var, v64, gt, lab = _model()
    r = _t64()
    N, D, H, L = 3, var.depth, var.num_heads, var.L
    assert r['head'].shape == (N, D, H, L) and r['attn'].shape == (N, D, L) and r['value'].shape == (N, L) and r['head'].dtype == torch.float64
    assert bool((r['rival'] == -1).all())
    res = float(r['residual'].abs().max())
    gap = float((r['head'].sum(2) + r['attn_bias'] - r['attn']).abs().max())
    print(f'float64: max |residual| {res:.3e}, max |sum_h head + attn_bias - attn| {gap:.3e}, max |rest| {float(r["rest"].abs().max()):.3e}')
    assert res <= 1e-10 and gap <= 1e-10
    assert float(r['rest'].abs().max()) <= 1e-10                                 # every block selected: nothing is left over
    assert float(r['attn'].abs().max()) > 1e-3 and float(r['mlp'].abs().max()) > 1e-3 and float(r['embed'].abs().max()) > 1e-3
    x = v64.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, b:e] for b, e in v64.begin_ends])      # value is the real logit
    with torch.no_grad():
        z = var._forward_torch(lab, x.float())
    assert float((r['value'] - z.gather(-1, gt.unsqueeze(-1)).squeeze(-1).double()).abs().max()) <= 1e-4


def test_margin_is_gt_against_the_rival():
    var, v64, gt, lab = _model()
    m = _t64(target='margin')
    assert bool((m['rival'] != gt).all()) and bool((m['rival'] >= 0).all())
    a = _t64(against=m['rival'])
    for k in m:
        assert torch.equal(m[k], a[k]), k
    g = _t64()
    assert float((m['value'] - g['value']).abs().max()) > 0
    assert float(m['residual'].abs().max()) <= 1e-10
    bad = m['rival'].clone(); bad[0, 0] = var.V; bad[1, 2] = -1
    o = _t64(against=bad)
    assert o['rival'][0, 0] == -1 and o['rival'][1, 2] == -1 and bool(torch.isnan(o['head'][0, :, :, 0]).all()) and bool(torch.isnan(o['value'][1, 2]))
    keep = torch.ones_like(bad, dtype=torch.bool); keep[0, 0] = keep[1, 2] = False
    assert torch.equal(o['attn'].transpose(1, 2)[keep], a['attn'].transpose(1, 2)[keep])


def test_layer_subsets_and_rest():
    var, v64, gt, lab = _model()
    full = _t64()
    D = var.depth
    for pick in ((D - 1,), (0,)):
        sub = _t64(layers=pick)
        for k in ('attn', 'mlp', 'attn_bias', 'head'):
            assert sub[k].shape[1] == 1 and torch.equal(sub[k][:, 0], full[k][:, pick[0]]), k
        for k in ('value', 'konst', 'embed', 'residual', 'rival'):
            assert torch.equal(sub[k], full[k]), k
        left = sum(full['attn'][:, d] + full['mlp'][:, d] for d in range(D) if d not in pick)
        assert D >= 2 and float((sub['rest'] - left).abs().max()) <= 1e-10 and float(left.abs().max()) > 1e-3
        gx = full['value'] - full['residual'] - full['konst']
        assert float((sub['rest'] - (gx - sub['embed'] - sub['attn'][:, 0] - sub['mlp'][:, 0])).abs().max()) <= 1e-12


def test_public_call_and_refusals():
    from var_amd.models.var import LogitAttribution
    var, v64, gt, lab = _model()
    r = var.logit_attribution(gt, lab, target='margin', layers=(0, 1))           # a CPU model: the PyTorch route, fp32
    assert isinstance(r, LogitAttribution) and r.layers == (0, 1) and r.head.shape == (3, 2, var.num_heads, var.L) and r.head.dtype == torch.float32
    assert r.rival.dtype == torch.int64 and r.patch_nums == tuple(var.patch_nums)
    c = r.completeness()
    print(f'fp32 PyTorch route: {c}')
    assert c['residual'] <= 1e-3 and c['heads'] <= 1e-3
    for kw in (dict(target='logit'), dict(target=None), dict(against=gt[:, :-1]), dict(against=gt.float()), dict(against=gt[:2]), dict(layers=(var.depth,)),
               dict(layers=(1, 0)), dict(max_rows=0)):
        with pytest.raises(ValueError):
            var.logit_attribution(gt, lab, **kw)
    bad = gt.clone(); bad[0, 0] = var.V
    with pytest.raises(ValueError):
        var.logit_attribution(bad, lab)


def test_methods_on_a_hand_made_result():
    from var_amd.models.var import LogitAttribution
    N, D, H, L = 2, 2, 3, 5                                                     # patch_nums (1, 2)
    t = lambda *s: torch.arange(int(np.prod(s)), dtype=torch.float32).view(*s)
    head = t(N, D, H, L)
    r = LogitAttribution((0, 3), (1, 2), torch.full((N, L), -1), value=t(N, L), konst=t(N, L), embed=t(N, L), rest=t(N, L), residual=t(N, L) * 0 + 0.25,
                         attn=head.sum(2) + 1.5, mlp=t(N, D, L), attn_bias=torch.full((N, D, L), 1.0), head=head)
    assert r.head_matrix().shape == (D, H) and r.head_matrix().dtype == torch.float64
    assert r.head_matrix()[0, 0].item() == float(torch.cat((head[0, 0, 0], head[1, 0, 0])).double().mean())
    ps = r.per_scale()
    assert ps['value'].shape == (2,) and ps['attn'].shape == (D, 2) and ps['head'].shape == (D, H, 2)
    assert ps['value'].tolist() == [2.5, 5.0]
    c = r.centered()
    assert c.value[:, 0].tolist() == [0.0, 0.0] and c.value[0, 1:].tolist() == [-1.5, -0.5, 0.5, 1.5] and c.head.shape == head.shape
    assert float(c.head[..., 1:].double().sum(-1).abs().max()) == 0.0
    assert r.completeness() == dict(residual=0.25, heads=0.5)
