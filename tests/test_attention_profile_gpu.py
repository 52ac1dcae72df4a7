"""VAR.attention_profile on the GPU: varhip_attn_profile_f32 bit for bit against its host twin on every workgroup shape, against the attention
kernel that already exists (the mass its own arithmetic puts on every key scale), and the public call end to end on the tiny and the d16 model."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import attnprofref as R
from tests import util
from var_amd import abi, hip

pytestmark = pytest.mark.gpu

ONE = R.SHARE_ONE
SENT = -7


def _buffers(case, tokens, pad):
    """the outputs of one call with padded leading dimensions (pad > 0: a spare head row and spare columns, sentinel-filled)"""
    rows, H, l, S1 = case['rows'], case['H'], case['l'], len(case['ends'])
    Hp, W, Wt = H + (1 if pad else 0), S1 + 1 + pad, l * (S1 + 1) + pad
    share = np.full((rows, Hp, W), SENT, np.int64)
    share[:, :H, :S1 + 1] = 0
    nan = np.zeros((rows, H), np.int32)
    tok = np.full((rows, Hp, Wt), SENT, np.int32) if tokens else None
    return share, nan, tok, (Hp * W, W, Hp * Wt, Wt)


def _args(case, radius, q, kc, share, nan, tok, ld):
    return (q, kc, case['rows'], case['l'], case['H'], case['curL'], case['Lmax'], None, len(case['ends']), case['pn'], radius,
            share, ld[0], ld[1], nan, tok, ld[2], ld[3])


def both(case, radius, tokens=True, pad=0, calls=1):
    """the host twin on numpy arrays and the kernel (guarded) on device copies, `calls` times into the same outputs -> (host, device) triples"""
    share, nan, tok, ld = _buffers(case, tokens, pad)
    dev = [torch.from_numpy(a.copy()).cuda() if a is not None else None for a in (share, nan, tok)]
    q, kc = torch.from_numpy(case['q']).cuda(), torch.from_numpy(case['kc']).cuda()
    ends_t = torch.from_numpy(case['ends'].copy())
    for _ in range(calls):
        a = list(_args(case, radius, case['q'], case['kc'], share, nan, tok, ld)); a[7] = case['ends']
        hip.call_host('attn_profile_host_f32', *a)
        a = list(_args(case, radius, q, kc, *dev, ld)); a[7] = ends_t
        util.guarded_call('attn_profile_f32', *a)
    torch.cuda.synchronize()
    return (share, nan, tok), tuple(None if d is None else d.cpu().numpy() for d in dev)


def _equal(host, dev):
    for name, h, d in zip(('share_sum', 'nan_count', 'tokens'), host, dev):
        assert (h is None) == (d is None)
        if h is not None:
            assert np.array_equal(h, d), f'{name}: {int((h != d).sum())} of {h.size} entries differ, first at {np.argwhere(h != d)[0]}'


# (l, curL): one key; one ragged tile; (36, 91): two waves with a ragged query group, three scale boundaries inside one 32-key tile; (100, 155): NW = 4
# with idle lanes; (169, 424): two workgroups of three waves
@pytest.mark.parametrize('l,curL', [(1, 1), (4, 5), (9, 14), (36, 91), (100, 155), (169, 424)])
def test_kernel_equals_host_twin(l, curL):
    case = R.make_case(l, curL)
    pn = case['pn']
    for radius in sorted({0, 1, 2, pn}):
        _equal(*both(case, radius, tokens=True, pad=3))
    host, dev = both(case, 1, tokens=False)
    _equal(host, dev)
    assert dev[0].any() and not dev[1].any()
    S1 = len(case['ends'])
    tot = both(case, 1)[1][2].reshape(case['rows'], case['H'], l, S1 + 1)[..., :S1].sum(-1)
    assert tot.min() >= ONE - S1 and tot.max() <= ONE


def test_kernel_equals_host_twin_d16_last_scale():
    _equal(*both(R.make_case(256, 680), 1, tokens=True))


def test_second_call_doubles_and_nan_query():
    case = R.make_case(36, 91, seed=5)
    once = both(case, 1, pad=2)
    twice = both(case, 1, pad=2, calls=2)
    _equal(*twice)
    H, S1 = case['H'], len(case['ends'])
    assert np.array_equal(twice[1][0][:, :H, :S1 + 1], 2 * once[1][0][:, :H, :S1 + 1]) and np.array_equal(twice[1][2], once[1][2])
    bad = dict(case)
    bad['q'] = case['q'].copy()
    bad['q'][2, 33, 5] = np.nan                                                # row 2, query 33 (the second wave's ragged group), head 0
    host, dev = both(bad, 1)
    _equal(host, dev)
    tok = dev[2].reshape(case['rows'], H, 36, S1 + 1)
    ref = once[1][2][:, :H, :36 * (S1 + 1)].reshape(case['rows'], H, 36, S1 + 1)
    want = ref.copy(); want[2, 0, 33] = -1
    assert np.array_equal(tok, want)
    assert dev[1][2, 0] == 1 and dev[1].sum() == 1


def test_misaligned_q_is_einval_and_writes_nothing():
    case = R.make_case(9, 14)
    share, nan, tok, ld = _buffers(case, True, 0)
    share[:] = SENT; nan[:] = SENT
    dev = [torch.from_numpy(a.copy()).cuda() for a in (share, nan, tok)]
    q = torch.zeros(case['q'].size + 4, dtype=torch.float32, device='cuda')[1:1 + case['q'].size].view(case['q'].shape)
    assert q.data_ptr() % 16 == 4
    a = list(_args(case, 1, q, torch.from_numpy(case['kc']).cuda(), *dev, ld)); a[7] = torch.from_numpy(case['ends'].copy())
    with pytest.raises(hip.VarHipError, match='EINVAL'):
        util.guarded_call('attn_profile_f32', *a)
    torch.cuda.synchronize()
    assert all(bool((d == SENT).all()) for d in dev)


@pytest.mark.parametrize('l,curL', [(36, 91), (169, 424)])
def test_against_the_attention_kernel(l, curL):
    """varhip_attn_cached_f32 with an indicator V cache: v[j][c] = 1 if key j belongs to scale c.  Its output channel c is then the attention mass
    on scale c in the sampler's own arithmetic: fp32 numerators e_j (the same bits as here), their fp32 row sum and the fp32 products p.v.
    Tolerance, per share: curL * 2^-23 (the fp32 row sum and the P.V chain: each adds at most curL roundings of 2^-24 relative to values <= 1)
    + curL * 2^-31 (this kernel's quantisation of the numerators, attnprofref (d)) + 2^-21 (the truncating division)."""
    case = R.make_case(l, curL, seed=6)
    rows, H, S1 = case['rows'], case['H'], len(case['ends'])
    vc = np.zeros((rows, H, case['Lmax'], 64), np.float32)
    lo = 0
    for c, e in enumerate(case['ends']):
        vc[:, :, lo:e, c] = 1.0
        lo = int(e)
    q, kc, vcd = torch.from_numpy(case['q']).cuda(), torch.from_numpy(case['kc']).cuda(), torch.from_numpy(vc).cuda()
    out = torch.empty(rows, l, H * 64, dtype=torch.float32, device='cuda')
    util.guarded_call('attn_cached_f32', q, kc, vcd, out, rows, l, H, curL, case['Lmax'])
    mass = out.view(rows, l, H, 64)[..., :S1].permute(0, 2, 1, 3).double().cpu().numpy()          # (rows, H, l, S1)
    tok = both(case, 1)[1][2].reshape(rows, H, l, S1 + 1)[..., :S1]
    tol = curL * 2.0 ** -23 + curL * 2.0 ** -31 + 2.0 ** -21
    err = np.abs(tok / ONE - mass).max()
    print(f'l={l} curL={curL}: attention_profile against attn_cached: {err:.3e} (allowed {tol:.3e})')
    assert err <= tol


# ---- the public call ----------------------------------------------------------------------------------------------------------------------
_M = {}


def tiny():
    if 'tiny' not in _M:
        from models import build_vae_var
        from var_amd.detinit import fill_module_, fill_module_device_
        _, meta = util.load_case('t_pn12345')
        kw = dict(patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'])
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cuda', **kw)
            cvae, cvar = build_vae_var(device='cpu', **kw)
        fill_module_device_(var, meta['depth'], 0, 'var.'); fill_module_device_(vae, meta['depth'], 0, 'vae.')
        fill_module_(cvar, meta['depth'], 0, 'var.'); fill_module_(cvae, meta['depth'], 0, 'vae.')
        var.eval(); vae.eval(); cvar.eval(); cvae.eval()
        g = torch.Generator().manual_seed(11)
        gt = torch.randint(0, var.V, (3, var.L), generator=g)
        _M['tiny'] = (var, cvar, gt, torch.tensor([3, 980, var.num_classes]))
    return _M['tiny']


def _same(a, b):
    return torch.equal(a.share_q, b.share_q) and torch.equal(a.nan_queries, b.nan_queries) and torch.equal(a.tokens, b.tokens)


def test_public_call_equals_host_twin_on_its_own_operands():
    """_tap hands over the q and K every launch read; the host twin on them, assembled in the public layout, is the call's result bit for bit"""
    var, _, gt, lab = tiny()
    S, H, D, L = len(var.patch_nums), var.num_heads, var.depth, var.L
    caps = []
    r = var.engine().attention_profile(gt.cuda(), lab.cuda(), 1, tuple(range(D)), 64, True, _tap=lambda q, k, w: caps.append((q.cpu().numpy(), k.cpu().numpy(), w)))
    assert len(caps) == D * S
    share = np.zeros((3, D, H, S, S + 1), np.int64)
    nanq = np.zeros((3, D, H, S), np.int32)
    toks = np.zeros((3, D, H, L, S + 1), np.int32)
    for q, k, (bi, si, cur, l) in caps:
        S1, pn = si + 1, var.patch_nums[si]
        assert q.shape == (3 * l, H * 64) and k.shape == (3, H, cur + l, 64)
        case = dict(q=q.reshape(3, l, H * 64), kc=np.ascontiguousarray(k), ends=np.asarray([e for _, e in var.begin_ends[:S1]], np.int32), pn=pn, l=l,
                    curL=cur + l, Lmax=cur + l, rows=3, H=H)
        sh, nn, tk = R.run_host(case, 1)
        share[:, bi, :, si, :S1] = sh[..., :S1]; share[:, bi, :, si, S] = sh[..., S1]
        nanq[:, bi, :, si] = nn
        toks[:, bi, :, cur:cur + l, :S1] = tk[..., :S1]; toks[:, bi, :, cur:cur + l, S] = tk[..., S1]
    assert np.array_equal(r['share_q'].cpu().numpy(), share)
    assert np.array_equal(r['nan_queries'].cpu().numpy(), nanq) and not nanq.any()
    assert np.array_equal(r['tokens'].cpu().numpy(), toks)


def test_public_call_invariances():
    var, _, gt, lab = tiny()
    gt, lab = gt.cuda(), lab.cuda()
    base = var.attention_profile(gt, lab, radius=1, return_tokens=True)
    for mr in (1, 2):
        assert _same(var.attention_profile(gt, lab, radius=1, max_rows=mr, return_tokens=True), base), mr
    one = var.attention_profile(gt[1:2], lab[1:2], radius=1, return_tokens=True)
    assert torch.equal(one.share_q[0], base.share_q[1]) and torch.equal(one.tokens[0], base.tokens[1])
    sub = var.attention_profile(gt, lab, radius=1, layers=(1,), return_tokens=True)
    assert torch.equal(sub.share_q[:, 0], base.share_q[:, 1])
    var.autoregressive_infer_cfg(2, torch.tensor([1, 2], device='cuda'), g_seed=0)
    var.token_log_likelihood(gt, [1, 2, 3], cfg=1.5)
    assert _same(var.attention_profile(gt, lab, radius=1, return_tokens=True), base)
    assert var.attention_profile(gt, 3).tokens is None


def test_public_call_against_the_torch_twin():
    """per-query shares of the HIP route against attention_profile_torch on a CPU copy of the model: within 8x the twin's own f32-against-f64
    deviation (attnprofref.TORCH_F32_VS_F64, measured on the CPU without the library): the HIP GEMMs sum in another order than PyTorch's"""
    var, cvar, gt, lab = tiny()
    a = var.attention_profile(gt.cuda(), lab.cuda(), radius=1, return_tokens=True)
    b = cvar.attention_profile(gt, lab, radius=1, return_tokens=True)
    err = float((a.tokens.cpu() - b.tokens).abs().max()) / ONE
    tol = R.HIP_VS_TORCH_FACTOR * R.TORCH_F32_VS_F64
    print(f'HIP route against attention_profile_torch: {err:.3e} (allowed {tol:.3e})')
    assert err <= tol
    # the twin also takes the model where it is (a CUDA model outside the HIP route's conditions): PyTorch's GPU GEMMs, same allowance
    from var_amd.models.var import attention_profile_torch
    _, _, tok = attention_profile_torch(var, gt.cuda(), lab.cuda(), 1, tuple(range(var.depth)), True)
    err = float((a.tokens - tok).abs().max()) / ONE
    print(f'HIP route against attention_profile_torch on the GPU: {err:.3e} (allowed {tol:.3e})')
    assert err <= tol


def test_d16_call():
    from tests.test_likelihood_gpu import d16, tokens
    vae, var = d16()
    gt = tokens(var, 2, 3)
    p = var.attention_profile(gt, torch.tensor([5, 1000], device='cuda'), layers=(0, 15))
    S, H = len(var.patch_nums), var.num_heads
    assert p.share_q.shape == (2, 2, H, S, S + 1) and p.nan_queries.shape == (2, 2, H, S) and p.tokens is None and p.layers == (0, 15)
    assert not p.nan_queries.any()
    sm = p.scale_matrix()
    assert float((sm.sum(-1) - 1).abs().max()) <= S / ONE
    assert not torch.triu(sm, 1).any() and (p.near() <= p.own_scale()).all() and float(p.near().min()) > 0


def test_16_bit_precision_is_refused():
    var, _, gt, lab = tiny()
    var.set_hip_precision('bf16')
    try:
        with pytest.raises(ValueError, match='attention_profile runs in f32'):
            var.attention_profile(gt.cuda(), lab.cuda())
        assert var.engine().policy == 'bf16'                                  # the refusal changes nothing
    finally:
        var.set_hip_precision('f32')
    assert var.attention_profile(gt.cuda(), lab.cuda()).share_q.any()
