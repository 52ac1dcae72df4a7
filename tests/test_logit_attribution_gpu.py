"""VAR.logit_attribution on the MI355X (d16, three images): the value is the real logit and the rival torch's masked arg-max, every term is the
host twins' on tapped clones bit for bit, packings, image orders and layer subsets give the same bits, the 16-bit modes are refused, the peak
allocation is the call's own buffers, and the terms and both completeness quantities stay inside the bars tests/dlaref.py derives from the
fp32 GEMM bound, against its float64 decomposition of the tapped activations and against logit_attribution_torch on the device."""
import numpy as np
import pytest
import torch

from tests import dlaref as DR
from tests import evalref
from tests.test_dla_cpu import host
from tests.test_likelihood_gpu import d16, tokens

pytestmark = pytest.mark.gpu

TERMS = ('value', 'konst', 'embed', 'rest', 'residual', 'attn', 'mlp', 'attn_bias', 'head')
SUB = (0, 7, 8, 15)                    # two blocks in a row (a shared stream point), a gap, the first and the last block
_R = {}


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _inputs():
    vae, var = d16()
    return var, tokens(var, 3, 31), torch.tensor([4, 1000, 31], device='cuda')


def _same(a, b, what, ia=slice(None), ib=slice(None), da=slice(None), db=slice(None), skip=()):
    for k in [k for k in TERMS + ('rival',) if k not in skip]:
        x, y = getattr(a, k)[ia], getattr(b, k)[ib]
        if k in ('attn', 'mlp', 'attn_bias', 'head'):
            x, y = x[:, da], y[:, db]
        assert torch.equal(bits(x), bits(y)), f'{what}: {k}'


def _full():
    if 'full' not in _R:
        var, gt, lab = _inputs()
        _R['full'] = var.logit_attribution(gt, lab, target='margin')
        _R['gt'] = var.logit_attribution(gt, lab, layers=SUB)
    return _R['full']


def _tapped():
    """the margin call on SUB through the engine with every scale's operands tapped -> (result dict, {scale: taps})"""
    if 'tap' not in _R:
        var, gt, lab = _inputs()
        taps = {}

        def tap(d, at):
            s = taps.setdefault(at[0], dict(at=at, blocks={}))
            if d['block'] is None:
                s.update({k: v for k, v in d.items() if k != 'block'})
            else:
                s['blocks'][d['block']] = {k: v.cpu() for k, v in d.items() if k != 'block'}
        out = var.engine().logit_attribution(gt, lab, 'margin', None, SUB, 64, _tap=tap)
        _R['tap'] = ({k: v.cpu() for k, v in out.items()}, taps)
    return _R['tap']


def test_value_and_rival_are_read_from_the_real_logits():
    var, gt, lab = _inputs()
    full, g = _full(), _R['gt']
    out, taps = _tapped()
    V = var.V
    for si, s in taps.items():
        _, cur, l = s['at']
        z = s['lg'].view(3, l, V)
        tok = gt[:, cur:cur + l]
        za = z.gather(-1, tok.unsqueeze(-1)).squeeze(-1)
        assert torch.equal(bits(g.value[:, cur:cur + l]), bits(za)), f'scale {si}: value under gt is not the gt logit'
        rival = z.masked_fill(torch.nn.functional.one_hot(tok, V).bool(), float('-inf')).argmax(-1)
        zb = z.gather(-1, rival.unsqueeze(-1)).squeeze(-1)
        assert torch.equal(zb, z.gather(-1, full.rival[:, cur:cur + l].unsqueeze(-1)).squeeze(-1)), f'scale {si}: the rival is not a greatest other logit'
        assert torch.equal(full.rival[:, cur:cur + l], rival), f'scale {si}: rival'
        assert torch.equal(bits(full.value[:, cur:cur + l]), bits(za - zb))
    assert bool((g.rival == -1).all()) and bool((full.rival != gt).all())
    assert full.head.shape == (3, 16, 16, var.L) and full.layers == tuple(range(16)) and bool(torch.isfinite(full.head).all())


def test_every_term_is_the_host_twins_on_tapped_clones():
    var, gt, lab = _inputs()
    out, taps = _tapped()
    C, H, V, L, depth = var.C, var.num_heads, var.V, var.L, var.depth
    w = var.engine().w
    W, b = w['head_w'].cpu().numpy(), w['head_b'].cpu().numpy()
    gtc = gt.cpu().numpy()
    f64 = lambda n: np.zeros(n)
    for si, s in taps.items():
        _, cur, l = s['at']
        R, n = s['R'], s['R'] * l
        tok = np.ascontiguousarray(gtc[:, cur:cur + l])
        rival, value = np.zeros((R, l), np.int64), np.zeros((R, l), np.float32)
        assert host('dla_target_host_f32', s['lg'].cpu().numpy(), tok, None, l, 1, R, l, V, rival, value, l) == 0
        hn = s['hn'].cpu().numpy()
        ghat, konst, gx = np.zeros((n, C), np.float32), np.zeros((R, l)), np.zeros((R, l))
        assert host('dla_direction_host_f32', s['x'].cpu().numpy(), hn, hn[:, C:], 2 * C, W, b, tok, rival, l, R, l, C, V, float(var.norm_eps), ghat,
                    konst, gx, l) == 0
        assert np.array_equal(ghat.view(np.int32), s['ghat'].cpu().numpy().view(np.int32)), f'scale {si}: ghat'

        def dot(a, bb, ldb, nseg=1):
            o = f64(n * nseg)
            assert host('rowdot_seg_host_f64', a, C, bb, ldb, n, C, nseg, o) == 0
            return torch.from_numpy(o)
        xf = torch.from_numpy(gx.reshape(-1).copy())
        at = {k: dot(ghat, v.cpu().numpy(), C) for k, v in s['pts'].items()}
        at[depth] = xf
        want = dict(attn=[], mlp=[], attn_bias=[], head=[])
        rest = xf - at[0]
        for bi in SUB:
            t = s['blocks'][bi]
            gg = (torch.from_numpy(ghat).view(R, l, C) * t['g1'].view(R, 1, C)).view(n, C)
            assert torch.equal(bits(gg), bits(t['gg'])), f'scale {si}, block {bi}: ghat * gamma1'
            dmid = dot(ghat, t['mid'].numpy(), C)
            attn, mlp = dmid - at[bi], at[bi + 1] - dmid
            rest = rest - (attn + mlp)
            want['attn'].append(attn); want['mlp'].append(mlp)
            want['attn_bias'].append(dot(t['gg'].numpy(), w['blocks'][bi]['proj_b'].cpu().numpy(), 0))
            want['head'].append(dot(t['u'].numpy(), t['att'].numpy(), C, H).view(n, H))
        val = torch.from_numpy(value)
        want = dict(value=val, konst=torch.from_numpy(konst), embed=at[0].view(R, l), rest=rest.view(R, l),
                    residual=(val.double().view(-1) - (torch.from_numpy(konst).view(-1) + xf)).view(R, l),
                    attn=torch.stack(want['attn']).view(-1, R, l).transpose(0, 1), mlp=torch.stack(want['mlp']).view(-1, R, l).transpose(0, 1),
                    attn_bias=torch.stack(want['attn_bias']).view(-1, R, l).transpose(0, 1),
                    head=torch.stack(want['head']).view(-1, R, l, H).permute(1, 0, 3, 2))
        for k in TERMS:
            assert torch.equal(bits(out[k][..., cur:cur + l]), bits(want[k].to(torch.float32))), f'scale {si}: {k}'
        assert np.array_equal(out['rival'][:, cur:cur + l].numpy(), rival)


def test_packings_orders_and_subsets_give_the_same_bits():
    var, gt, lab = _inputs()
    full = _full()
    sub = var.logit_attribution(gt, lab, target='margin', layers=SUB)
    _same(sub, full, 'layers subset', db=list(SUB), skip=('rest',))             # (rest: what the subset leaves out, below)
    out, _ = _tapped()
    for k in TERMS:
        assert torch.equal(bits(getattr(sub, k)).cpu(), bits(out[k])), f'the tapped call: {k}'
    gap = sub.rest.double() - sum(full.attn[:, d].double() + full.mlp[:, d].double() for d in range(16) if d not in SUB)
    assert float(gap.abs().max()) <= 16 * 2.0 ** -22 * float(full.attn.abs().max() + full.mlp.abs().max()), 'rest does not absorb the blocks left out'
    for mr in (2, 1):
        _same(var.logit_attribution(gt, lab, target='margin', layers=SUB, max_rows=mr), sub, f'max_rows={mr}')
    perm = [2, 0, 1]
    p = var.logit_attribution(gt[perm], lab[perm], target='margin', layers=SUB)
    _same(p, sub, 'permuted images', ib=perm)
    ag = var.logit_attribution(gt, lab, against=sub.rival, layers=SUB)
    _same(ag, sub, 'against = the margin rival')
    bad = sub.rival.clone(); bad[1, 5] = var.V; bad[2, 0] = -1
    o = var.logit_attribution(gt, lab, against=bad, layers=SUB)
    assert o.rival[1, 5] == -1 and o.rival[2, 0] == -1 and bool(torch.isnan(o.head[1, :, :, 5]).all()) and bool(torch.isnan(o.value[2, 0]))
    keep = torch.ones_like(bad, dtype=torch.bool); keep[1, 5] = keep[2, 0] = False
    assert torch.equal(bits(o.value[keep]), bits(sub.value[keep])) and torch.equal(bits(o.embed[keep]), bits(sub.embed[keep]))


def test_refused_in_the_16_bit_modes():
    var, gt, lab = _inputs()
    for prec in ('f16', 'bf16'):
        var.set_hip_precision(prec)
        try:
            with pytest.raises(ValueError, match='logit_attribution runs in f32'):
                var.logit_attribution(gt, lab, layers=SUB)
        finally:
            var.set_hip_precision('f32')


def test_peak_allocation_is_the_calls_own_buffers():
    """d16, 3 images, all 16 blocks in one pass: after a warm-up call the peak allocation rises by the call's own buffers (the stash, the
    float64 dots, the transposed proj weights, the results, the teacher-forcing inputs, one scale's temporaries) plus 1 % at most"""
    var, gt, lab = _inputs()
    var.logit_attribution(gt, lab)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    r = var.logit_attribution(gt, lab)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    N, L, C, H, D, Cv = 3, var.L, var.C, var.num_heads, 16, var.Cvae
    M = N * var.patch_nums[-1] ** 2
    stash = (D + 2 * D + 3) * M * C * 4                                           # 16 stream points, mid and att per block, ghat, gg, u
    dots = (D + 1 + 2 * D + D * H + 1) * M * 8
    weights = D * C * C * 4
    results = N * L * (5 * 4 + 8) + N * D * L * 4 * 3 + N * D * H * L * 4
    inputs = N * L * (Cv * 4 * 4 + 8 * 2)
    scale = 8 * M * 8 + 2 * M * H * 4 + 4 * M * 4                                 # the float64 differences of a block and the fp32 copies on their way out
    own = stash + dots + weights + results + inputs + scale
    print(f'peak rise {rise / 1e6:.1f} MB; own buffers {own / 1e6:.1f} MB')
    assert r.head.shape == (N, D, H, L)
    assert rise <= own * 1.01, f'peak allocation rose by {rise / 1e6:.1f} MB, the call\'s own buffers are {own / 1e6:.1f} MB'


def _float64_reference():
    """tests/dlaref.py's decomposition of the tapped activations, per scale, with the bars' ingredients -> {term: (ref, bar)} over (3, ..., L)"""
    if 'ref' in _R:
        return _R['ref']
    var, gt, lab = _inputs()
    out, taps = _tapped()
    C, H, V, L, depth = var.C, var.num_heads, var.V, var.L, var.depth
    w = var.engine().w
    W, b = w['head_w'].cpu().numpy(), w['head_b'].cpu().numpy()
    shp = dict(value=(3, L), konst=(3, L), embed=(3, L), rest=(3, L), residual=(3, L), attn=(3, 4, L), mlp=(3, 4, L), attn_bias=(3, 4, L), head=(3, 4, H, L))
    ref = {k: np.zeros(s) for k, s in shp.items()}
    bar = {k: np.zeros(s) for k, s in shp.items()}
    bar['heads_sum'], bar['abs_residual'] = np.zeros((3, 4, L)), np.zeros((3, L))
    eps = float(var.norm_eps)
    for si, s in taps.items():
        _, cur, l = s['at']
        R, n = 3, 3 * l
        sl = slice(cur, cur + l)
        a = gt[:, sl].reshape(-1).cpu().numpy()
        rv = out['rival'][:, sl].reshape(-1).numpy()
        x, hn = s['x'].cpu().numpy(), s['hn'].cpu().numpy()
        gh, konst = DR.ghat64(x, hn[:, :C], hn[:, C:], W, b, a, rv, l, eps)
        xd = x.astype(np.float64)
        pts = {k: v.cpu().numpy().astype(np.float64) for k, v in s['pts'].items()}
        pts[depth] = xd
        gx = (gh * xd).sum(-1)
        mag = lambda v: (np.abs(gh) * np.abs(v)).sum(-1)
        z = s['lg'].cpu().numpy().astype(np.float64).reshape(n, V)
        value = z[np.arange(n), a].astype(np.float32).astype(np.float64) - z[np.arange(n), rv]
        value = value.astype(np.float32).astype(np.float64)
        row = np.arange(n) // l
        ln = (xd - xd.mean(-1, keepdims=True)) / np.sqrt(xd.var(-1) + np.float64(np.float32(eps)))[:, None]
        xn = np.abs(ln * (1 + hn[row, :C].astype(np.float64)) + hn[row, C:])
        xnw = (xn * (np.abs(W[a]) + np.abs(W[rv]))).sum(-1)
        put = lambda name, v, idx=(): ref[name].__setitem__((slice(None),) + idx + (sl,), v.reshape(R, l))
        putb = lambda name, v, idx=(): bar[name].__setitem__((slice(None),) + idx + (sl,), v.reshape(R, l))
        embed = (gh * pts[0]).sum(-1)
        rest, rest_mag = gx - embed, mag(xd) + mag(pts[0])
        put('value', value); putb('value', np.zeros(n))
        r_abs = np.abs(W[a].astype(np.float64) - W[rv])                            # konst is a dot too: its magnitude is sum |r| |sh| + |b_a| + |b_b'|
        kmag = (r_abs * np.abs(hn[row, C:].astype(np.float64))).sum(-1) + np.abs(b[a]) + np.abs(b[rv])
        put('konst', konst); putb('konst', DR.bar_dot(kmag, konst))
        put('embed', embed); putb('embed', DR.bar_dot(mag(pts[0]), embed))
        res = value - (konst + gx)
        put('residual', res); putb('residual', DR.bar_dot(mag(xd) + kmag, res))
        putb('abs_residual', DR.bar_residual(xnw, mag(xd), C))
        for d, bi in enumerate(SUB):
            t = s['blocks'][bi]
            o = DR.decompose(gh, pts[0], pts[bi], t['mid'].numpy(), pts[bi + 1], t['att'].numpy(), t['g1'].numpy(), var.blocks[bi].attn.proj.weight.detach().cpu().numpy(),
                             var.blocks[bi].attn.proj.bias.detach().cpu().numpy(), l, H)
            rest = rest - (o['attn'] + o['mlp'])
            rest_mag = rest_mag + o['mag_attn'] + o['mag_mlp']
            for k, m in (('attn', 'mag_attn'), ('mlp', 'mag_mlp'), ('attn_bias', 'mag_bias')):
                put(k, o[k], (d,)); putb(k, DR.bar_dot(o[m], o[k]), (d,))
            putb('heads_sum', DR.bar_heads_sum(o['Q'], o['mag_attn'], C), (d,))
            for h in range(H):
                put('head', o['head'][:, h], (d, h)); putb('head', DR.bar_head(o['Q'][:, h], o['head'][:, h], C), (d, h))
        put('rest', rest); putb('rest', DR.bar_dot(rest_mag, rest))
    _R['ref'] = (ref, bar)
    return _R['ref']


def test_terms_against_the_float64_decomposition():
    """every term within its derived bar of tests/dlaref.py's float64 decomposition of the tapped activations, and both completeness
    quantities within theirs.  The measured maxima and the largest bars are printed (DESIGN.md section 40 records them)."""
    out, _ = _tapped()
    ref, bar = _float64_reference()
    worst = {}
    for k in TERMS:
        d = np.abs(out[k].numpy().astype(np.float64) - ref[k])
        worst[k] = (float(d.max()), float(bar[k].max()), float((d / np.maximum(bar[k], 1e-300)).max()) if k != 'value' else 0.0)
        print(f'{k}: max |HIP - float64| {worst[k][0]:.3e}, largest bar {worst[k][1]:.3e}, worst share of its bar {worst[k][2]:.3f}, max |term| {float(np.abs(ref[k]).max()):.3e}')
    gap = np.abs(out['head'].numpy().astype(np.float64).sum(2) + out['attn_bias'].numpy() - out['attn'].numpy())
    res = np.abs(out['residual'].numpy().astype(np.float64))
    print(f'completeness: max |sum_h head + attn_bias - attn| {gap.max():.3e} (largest bar {bar["heads_sum"].max():.3e}), '
          f'max |residual| {res.max():.3e} (largest bar {bar["abs_residual"].max():.3e}; evalref.BAR {evalref.BAR})')
    assert np.array_equal(out['value'].numpy().astype(np.float64), ref['value'])
    for k in TERMS:
        assert (np.abs(out[k].numpy().astype(np.float64) - ref[k]) <= bar[k]).all(), (k, worst[k])
    assert (gap <= bar['heads_sum']).all() and (res <= bar['abs_residual']).all()


def test_pytorch_route_agrees():
    """logit_attribution_torch on the device (fp32, the module stack) against the HIP route: the same per-token bars"""
    from var_amd.models.var import logit_attribution_torch
    var, gt, lab = _inputs()
    out, _ = _tapped()
    ref, bar = _float64_reference()
    with torch.no_grad():
        t = logit_attribution_torch(var, gt, lab, 'margin', out['rival'].cuda(), SUB)
    bad = []
    for k in TERMS:
        d = np.abs(out[k].numpy().astype(np.float64) - t[k].double().cpu().numpy())
        kb = bar[k] if k != 'value' else bar['abs_residual']
        share = float((d / np.maximum(kb, 1e-300)).max())
        print(f'{k}: max |HIP - PyTorch| {float(d.max()):.3e}, worst share of its bar {share:.3f}')
        if not (d <= kb).all():
            bad.append((k, float(d.max()), share))
    assert not bad, bad
