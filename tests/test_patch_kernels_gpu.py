"""varhip_act_patch_f32 on the MI355X: bit for bit its host twin on the deck of tests/patchref.py, every call inside guard bands; its refusals;
and varhip_adaln_block_patched_f32 with empty tables against varhip_adaln_block_f32, bit for bit."""
import numpy as np
import pytest
import torch

from tests import patchref as PR
from tests import util
from var_amd import hip

pytestmark = pytest.mark.gpu

DECK = PR.deck()


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


@pytest.mark.parametrize('case', DECK, ids=[c[0] for c in DECK])
def test_kernel_is_its_host_twin(case):
    name, rows, l, width, ld, dirs = case
    act = PR.matrix(rows, l, width, ld, len(name) + l)
    want = act.copy()
    hip.call_host('act_patch_host_f32', want, ld, rows, l, width, dirs, len(dirs))
    assert np.array_equal(want.view(np.int32), PR.apply(act, rows, l, width, dirs).view(np.int32))
    got, d = torch.from_numpy(act).cuda(), torch.from_numpy(dirs).cuda()
    util.guarded_call('act_patch_f32', got, ld, rows, l, width, d, len(dirs))
    torch.cuda.synchronize()
    assert torch.equal(bits(got).cpu(), torch.from_numpy(want.view(np.int32))), f'{name}: the kernel differs from its host twin'
    assert torch.equal(d.cpu(), torch.from_numpy(dirs))


def test_refusals_and_the_empty_table_leave_the_matrix_untouched():
    rows, l, width, ld = 2, 4, 128, 132
    act = PR.matrix(rows, l, width, ld, 6)
    dirs = torch.tensor([[0, 0, 64, PR.ZERO], [1, 64, 128, PR.MEAN]], dtype=torch.int32).cuda()
    good = dict(ld=ld, rows=rows, l=l, width=width, n=2)
    for bad in (dict(rows=0), dict(l=0), dict(width=0), dict(rows=-1), dict(n=-1), dict(ld=width - 4), dict(ld=ld + 2), dict(null='act'), dict(null='dir'),
                dict(odd=True)):
        a = dict(good, **{k: v for k, v in bad.items() if k not in ('null', 'odd')})
        m = torch.from_numpy(act).cuda()
        if bad.get('odd'):
            m = torch.cat((torch.zeros(1, device='cuda'), m.view(-1)))[1:].view(rows * l, ld)         # 4 bytes past a 16-byte boundary
            assert m.data_ptr() % 16 == 4
        before = m.clone()
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            util.guarded_call('act_patch_f32', None if bad.get('null') == 'act' else m, a['ld'], a['rows'], a['l'], a['width'],
                              None if bad.get('null') == 'dir' else dirs, a['n'])
        torch.cuda.synchronize()
        assert torch.equal(bits(m), bits(before)), bad
    m = torch.from_numpy(act).cuda()
    util.guarded_call('act_patch_f32', m, ld, rows, l, width, None, 0)               # n_dir == 0: success without a launch
    torch.cuda.synchronize()
    assert torch.equal(bits(m).cpu(), torch.from_numpy(act.view(np.int32)))


@pytest.mark.parametrize('l', [1, 16])
def test_patched_block_with_empty_tables_is_the_block(l):
    """one block at B2 = 3 rows on top of 5 cached tokens, C = 128, two heads, hidden 512: every buffer the block writes, bit for bit"""
    B2, C, H, hidden, pos0, Lmax = 3, 128, 2, 512, 5, 24
    g = torch.Generator().manual_seed(l)
    rnd = lambda *s, sc=1.0: (torch.randn(*s, generator=g) * sc).cuda()
    M = B2 * l
    w = dict(ada=rnd(B2, 6 * C, sc=0.3), qkv_w=rnd(3 * C, C, sc=0.09), qkv_b=rnd(3 * C, sc=0.1), smul=rnd(H, sc=0.2) + 1.4, proj_w=rnd(C, C, sc=0.09),
             proj_b=rnd(C, sc=0.1), fc1_w=rnd(hidden, C, sc=0.09), fc1_b=rnd(hidden, sc=0.1), fc2_w=rnd(C, hidden, sc=0.05), fc2_b=rnd(C, sc=0.1))
    x0, kc0, vc0 = rnd(M, C), rnd(B2, H, Lmax, 64), rnd(B2, H, Lmax, 64)

    def run(tail):
        buf = dict(x=x0.clone(), x2=torch.zeros(M, C, device='cuda'), xn=torch.zeros(M, C, device='cuda'), q=torch.zeros(M, C, device='cuda'),
                   att=torch.zeros(M, C, device='cuda'), hid=torch.zeros(M, hidden, device='cuda'), kc=kc0.clone(), vc=vc0.clone())
        args = (buf['x'], buf['x2'], buf['xn'], buf['q'], buf['att'], buf['hid'], w['ada'], 6 * C, w['qkv_w'], w['qkv_b'], w['smul'], 1.0, 1,
                w['proj_w'], w['proj_b'], w['fc1_w'], w['fc1_b'], w['fc2_w'], w['fc2_b'], buf['kc'], buf['vc'], B2, l, C, H, hidden, pos0, Lmax, 1e-6)
        if tail is None:
            util.guarded_call('adaln_block_f32', *args)
        else:
            util.guarded_call('adaln_block_patched_f32', *args, *tail)
        torch.cuda.synchronize()
        return buf
    plain = run(None)
    empty = run((None, 0, None, 0))
    for k in plain:
        assert torch.equal(bits(empty[k]), bits(plain[k])), f'{k}: the patched block with empty tables differs from the block'
    assert bool(torch.isfinite(plain['x']).all()) and not torch.equal(plain['x'], x0)
    # ... and a table does what the kernel alone does between the launches: zero the last head, and the result is the block's on proj columns cut
    dirs = torch.tensor([[1, 64, 128, PR.ZERO]], dtype=torch.int32).cuda()
    cut = run((dirs, 1, None, 0))
    assert torch.equal(bits(cut['x'][:l]), bits(plain['x'][:l])) and torch.equal(bits(cut['x'][2 * l:]), bits(plain['x'][2 * l:]))
    assert not torch.equal(cut['x'][l:2 * l], plain['x'][l:2 * l]) and not bool(cut['att'][l:2 * l, 64:].any()) and torch.equal(cut['att'][:, :64], plain['att'][:, :64])
    for bad in ((None, 1, None, 0), (dirs, -1, None, 0), (None, 0, None, 2), (None, 0, dirs, -1)):
        with pytest.raises(hip.VarHipError, match='VARHIP_EINVAL'):
            run(bad)
