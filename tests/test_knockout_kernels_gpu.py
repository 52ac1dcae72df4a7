"""varhip_attn_keysel_f32 on the MI355X, on the deck of tests/knockoutcases.py under every forced NW, every call inside guard bands: bit for bit
varhip_attn_cached_f32 on the gathered cache of every (row, head); a full mask is the plain kernel; n = 0 writes +0; the float64 bar; refused
calls leave the sentinel; and varhip_adaln_block_keysel_f32 with full masks is varhip_adaln_block_f32."""
import numpy as np
import pytest
import torch

from tests import knockoutcases as KC
from tests import util
from var_amd import hip

pytestmark = pytest.mark.gpu

CASES = KC.cases()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _keysel(b, masks=None, nw=0):
    """the kernel on the case's operands -> out [B2 l][H 64] (from the sentinel), with NW forced for this launch only"""
    c = b.case
    out = torch.full((c['B2'] * c['l'], c['H'] * 64), float(KC.SENTINEL), device='cuda')
    so = hip.lib().so
    so.varhip_attn_force_waves(nw)
    try:
        util.guarded_call('attn_keysel_f32', _dev(b.q), _dev(b.k), _dev(b.v), out, c['B2'], c['l'], c['H'], c['curL'], c['Lmax'],
                          torch.from_numpy(b.ends), c['S1'], _dev(b.masks if masks is None else masks))
        assert nw == 0 or so.varhip_attn_last_waves() == nw
    finally:
        so.varhip_attn_force_waves(0)
    torch.cuda.synchronize()
    return out


def _plain(q, k, v, B2, l, H, curL, Lmax, nw=0):
    out = torch.full((B2 * l, H * 64), float(KC.SENTINEL), device='cuda')
    so = hip.lib().so
    so.varhip_attn_force_waves(nw)
    try:
        util.guarded_call('attn_cached_f32', _dev(q), _dev(k), _dev(v), out, B2, l, H, curL, Lmax)
    finally:
        so.varhip_attn_force_waves(0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('nw', [1, 2, 3, 4])
@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_keysel_is_the_plain_kernel_on_the_gathered_cache(c, nw):
    b = KC.build(c)
    l, H = c['l'], c['H']
    got = _keysel(b, nw=nw).cpu()
    assert torch.equal(bits(got), bits(_keysel(b).cpu())), 'the forced NW changes bits'
    worst = 0.0
    for bb in range(c['B2']):
        for h in range(H):
            mine = got[bb * l:(bb + 1) * l, h * 64:(h + 1) * 64]
            mask = c['masks'][bb][h]
            kc, vc, n = KC.gather(mask, c['ends'], b.k[bb, h], b.v[bb, h])
            if n == 0:
                assert torch.equal(bits(mine.contiguous()), torch.zeros(l, 64, dtype=torch.int32)), (bb, h, 'n = 0 must write +0')
                continue
            want = _plain(KC.q_of(b, bb, h), kc[None, None], vc[None, None], 1, l, 1, n, n, nw=nw).cpu()
            assert torch.equal(bits(mine.contiguous()), bits(want)), f'row {bb}, head {h} (n = {n}): not the plain kernel on the gathered cache'
            ref, bar = KC.masked_reference(KC.q_of(b, bb, h), b.k[bb, h], b.v[bb, h], KC.visible(c['ends'], mask))
            ratio = float((np.abs(mine.numpy().astype(np.float64) - ref) / bar).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (bb, h, ratio)
    print(f"{c['name']} NW={nw}: max |kernel - masked float64| / bar = {worst:.3f}")


@pytest.mark.parametrize('nw', [1, 2, 3, 4])
@pytest.mark.parametrize('c', [CASES[1], CASES[3], CASES[6]], ids=lambda c: c['name'])
def test_a_full_mask_is_the_plain_kernel(c, nw):
    """finite operands everywhere below curL, every mask full (some with bits at or above S1 beside it): varhip_attn_cached_f32's bits"""
    b = KC.build(c)
    rng = np.random.default_rng(c['l'])
    k, v = b.k.copy(), b.v.copy()
    k[:, :, :c['curL']] = (0.45 * rng.standard_normal(k[:, :, :c['curL']].shape)).astype(np.float32)
    v[:, :, :c['curL']] = rng.standard_normal(v[:, :, :c['curL']].shape).astype(np.float32)
    full = (1 << c['S1']) - 1
    masks = np.array([full | (KC.HI if i % 2 else 0) | ((1 << c['S1']) if i % 3 == 0 else 0) for i in range(c['B2'] * c['H'])], dtype=np.int64).astype(np.int32)
    fb = KC.Built()
    fb.case, fb.q, fb.k, fb.v, fb.ends, fb.masks = c, b.q, k, v, b.ends, masks
    got = _keysel(fb, nw=nw)
    want = _plain(b.q, k, v, c['B2'], c['l'], c['H'], c['curL'], c['Lmax'], nw=nw)
    assert torch.equal(bits(got), bits(want)) and bool(torch.isfinite(got).all())


def test_refused_calls_leave_the_sentinel():
    c = CASES[2]
    b = KC.build(c)
    good = dict(B2=c['B2'], l=c['l'], H=c['H'], curL=c['curL'], Lmax=c['Lmax'], S1=c['S1'], ends=list(c['ends']))
    q, k, v, m = _dev(b.q), _dev(b.k), _dev(b.v), _dev(b.masks)
    last = hip.lib().so.varhip_attn_last_waves()
    bads = [dict(B2=0), dict(l=0), dict(H=0), dict(curL=0), dict(Lmax=0), dict(B2=-1), dict(Lmax=c['curL'] - 1), dict(l=c['curL'] + 1), dict(S1=0), dict(S1=17),
            dict(S1=2), dict(ends=[1, 5, 13]), dict(ends=[1, 1, 14]), dict(ends=[0, 5, 14]), dict(ends=[5, 1, 14]), dict(ends=[1, 5, 15]), dict(B2=65536), dict(H=65536),
            dict(null='q'), dict(null='k'), dict(null='v'), dict(null='out'), dict(null='ends'), dict(null='mask'), dict(odd='q'), dict(odd='k'), dict(odd='v')]
    for bad in bads:
        a = dict(good, **{key: val for key, val in bad.items() if key not in ('null', 'odd')})
        out = torch.full((c['B2'] * c['l'], c['H'] * 64), float(KC.SENTINEL), device='cuda')
        ops = dict(q=q, k=k, v=v, out=out, ends=torch.tensor(a['ends'], dtype=torch.int32), mask=m)
        if 'null' in bad:
            ops[bad['null']] = None
        if 'odd' in bad:                                        # 4 bytes past a 16-byte boundary
            t = ops[bad['odd']]
            ops[bad['odd']] = torch.cat((torch.zeros(1, device='cuda'), t.reshape(-1)))[1:].view(t.shape)
            assert ops[bad['odd']].data_ptr() % 16 == 4
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('attn_keysel_f32', ops['q'], ops['k'], ops['v'], ops['out'], a['B2'], a['l'], a['H'], a['curL'], a['Lmax'], ops['ends'], a['S1'], ops['mask'])
        torch.cuda.synchronize()
        assert bool((out == float(KC.SENTINEL)).all()), bad
        assert hip.lib().so.varhip_attn_last_waves() == last, 'a refused call moved varhip_attn_last_waves'


@pytest.mark.parametrize('l', [1, 16])
def test_keysel_block_with_full_masks_is_the_block(l):
    """one block at B2 = 3 rows on top of 5 cached tokens (two key scales: the 5 cached tokens, the l new ones), C = 128, two heads, hidden 512:
    every buffer the block writes, bit for bit; and a cut changes its own row only"""
    B2, C, H, hidden, pos0, Lmax = 3, 128, 2, 512, 5, 24
    g = torch.Generator().manual_seed(l)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).cuda()
    M = B2 * l
    w = dict(ada=rnd(B2, 6 * C, sc=0.3), qkv_w=rnd(3 * C, C, sc=0.09), qkv_b=rnd(3 * C, sc=0.1), smul=rnd(H, sc=0.2) + 1.4, proj_w=rnd(C, C, sc=0.09),
             proj_b=rnd(C, sc=0.1), fc1_w=rnd(hidden, C, sc=0.09), fc1_b=rnd(hidden, sc=0.1), fc2_w=rnd(C, hidden, sc=0.05), fc2_b=rnd(C, sc=0.1))
    x0, kc0, vc0 = rnd(M, C), rnd(B2, H, Lmax, 64), rnd(B2, H, Lmax, 64)
    ends = torch.tensor([pos0, pos0 + l], dtype=torch.int32)

    def run(tail):
        buf = dict(x=x0.clone(), x2=torch.zeros(M, C, device='cuda'), xn=torch.zeros(M, C, device='cuda'), q=torch.zeros(M, C, device='cuda'),
                   att=torch.zeros(M, C, device='cuda'), hid=torch.zeros(M, hidden, device='cuda'), kc=kc0.clone(), vc=vc0.clone())
        args = (buf['x'], buf['x2'], buf['xn'], buf['q'], buf['att'], buf['hid'], w['ada'], 6 * C, w['qkv_w'], w['qkv_b'], w['smul'], 1.0, 1,
                w['proj_w'], w['proj_b'], w['fc1_w'], w['fc1_b'], w['fc2_w'], w['fc2_b'], buf['kc'], buf['vc'], B2, l, C, H, hidden, pos0, Lmax, 1e-6)
        if tail is None:
            util.guarded_call('adaln_block_f32', *args)
        else:
            util.guarded_call('adaln_block_keysel_f32', *args, *tail)
        torch.cuda.synchronize()
        return buf
    plain = run(None)
    full = run((ends, 2, torch.full((B2 * H,), 3, dtype=torch.int32, device='cuda')))
    for k in plain:
        assert torch.equal(bits(full[k]), bits(plain[k])), f'{k}: the key-selecting block with full masks differs from the block'
    assert bool(torch.isfinite(plain['x']).all()) and not torch.equal(plain['x'], x0)
    cut = run((ends, 2, torch.tensor([3, 3, 3, 2, 3, 3], dtype=torch.int32, device='cuda')))          # row 1, head 1 does not see the cached tokens
    assert torch.equal(bits(cut['x'][:l]), bits(plain['x'][:l])) and torch.equal(bits(cut['x'][2 * l:]), bits(plain['x'][2 * l:]))
    assert not torch.equal(cut['att'][l:2 * l, 64:], plain['att'][l:2 * l, 64:]) and torch.equal(bits(cut['att'][:, :64]), bits(plain['att'][:, :64]))
    assert torch.equal(bits(cut['kc']), bits(plain['kc'])) and torch.equal(bits(cut['vc']), bits(plain['vc']))
    for bad in ((None, 2, torch.zeros(B2 * H, dtype=torch.int32, device='cuda')), (ends, 2, None), (ends, 1, torch.zeros(B2 * H, dtype=torch.int32, device='cuda')),
                (torch.tensor([pos0, pos0 + l + 1], dtype=torch.int32), 2, torch.zeros(B2 * H, dtype=torch.int32, device='cuda'))):
        before = x0.clone()
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            run(bad)
        assert torch.equal(x0, before)
