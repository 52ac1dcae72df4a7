"""VAR.attention_profile without a GPU: the host twin of varhip_attn_profile_f32 against the float64 restatement of tests/attnprofref.py within
its derived bound, the exact identities of the fixed-point shares, the argument checks, and attention_profile_torch on tiny CPU models."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

from tests import attnprofref as R
from tests import util
from var_amd import abi, hip

SHAPES = [(1, 1), (4, 5), (9, 14), (16, 30), (36, 91)]
ONE = R.SHARE_ONE


@pytest.mark.parametrize('l,curL', SHAPES)
@pytest.mark.parametrize('radius', [0, 1])
def test_host_twin_within_the_derived_bound(l, curL, radius):
    c = R.make_case(l, curL)
    share, nan, tok = R.run_host(c, radius)
    ref, bound = R.reference(c, radius)
    err = np.abs(tok / ONE - ref).max(-1)
    print(f'l={l} curL={curL} radius={radius}: max error {err.max():.3e}, smallest bound {bound.min():.3e}')
    assert (err <= bound).all(), float((err - bound).max())
    assert not nan.any() and np.array_equal(tok.sum(2), share)                 # share_sum is the integer sum of the queries' shares


def test_exact_identities():
    c = R.make_case(1, 1)
    share, nan, tok = R.run_host(c, 0)
    assert (tok == ONE).all() and (share == ONE).all()                         # one key: all of it, in bin 0 and in the near bin
    for l, curL in SHAPES[1:]:
        c = R.make_case(l, curL, seed=1)
        S1, pn = len(c['ends']), c['pn']
        _, _, tok = R.run_host(c, 1)
        tot = tok[..., :S1].sum(-1)
        assert tot.min() >= ONE - S1 and tot.max() <= ONE
        assert (tok[..., S1] <= tok[..., S1 - 1]).all()                        # near <= own scale
        _, _, full = R.run_host(c, pn - 1)
        assert np.array_equal(full[..., S1], full[..., S1 - 1])                # radius >= pn - 1: the whole own scale
        _, _, big = R.run_host(c, 1000)
        assert np.array_equal(big, full)


def test_radius_zero_tracks_a_dominant_self_key():
    c = R.make_case(16, 30, seed=2)
    q = c['q'].reshape(c['rows'], 16, c['H'], 64)
    for t in range(16):                                                        # every query points at its own key, sharply
        q[:, t] = 60.0 * c['kc'][:, :, 14 + t].transpose(0, 1, 2)
    _, _, tok = R.run_host(c, 0)
    ref, bound = R.reference(c, 0)
    S1 = len(c['ends'])
    assert (tok[..., S1] > 0.99 * ONE).all()                                   # e^-60(1 - cos) leaves the other keys almost nothing
    assert (np.abs(tok[..., S1] / ONE - ref[..., S1]) <= bound).all()


def test_bins_above_the_query_scale_do_not_exist():
    """the call of query scale sq has S1 = sq + 1 bins; in the public layout (S + 1 bins) everything above sq stays 0: the torch twin's output"""
    vae, var = _model(True)
    gt, lab = _inputs(var)
    p = var.attention_profile(gt, lab, return_tokens=True)
    S = len(var.patch_nums)
    for sq in range(S):
        assert not p.share_q[..., sq, sq + 1:S].any()
        b, e = var.begin_ends[sq]
        assert not p.tokens[..., b:e, sq + 1:S].any()


def test_order_freedom_inside_an_earlier_scale():
    c = R.make_case(36, 91, seed=3)
    _, _, tok = R.run_host(c, 1)
    d = dict(c)
    d['kc'] = c['kc'].copy()
    perm = np.random.default_rng(0).permutation(25) + 30                       # the keys of scale 4 (30 .. 54)
    d['kc'][:, :, 30:55] = c['kc'][:, :, perm]
    _, _, tok2 = R.run_host(d, 1)
    assert np.array_equal(tok, tok2)


def test_nan_query_and_padding():
    c = R.make_case(9, 14, seed=4)
    share, nan, tok = R.run_host(c, 1)
    d = dict(c)
    d['q'] = c['q'].copy()
    d['q'][1, 4, 64 + 3] = np.nan                                              # row 1, query 4, head 1
    share2, nan2, tok2 = R.run_host(d, 1)
    want = tok.copy(); want[1, 1, 4] = -1
    assert np.array_equal(tok2, want)
    wn = np.zeros_like(nan); wn[1, 1] = 1
    assert np.array_equal(nan2, wn)
    assert np.array_equal(share2[1, 1], share[1, 1] - tok[1, 1, 4]) and np.array_equal(np.delete(share2.reshape(-1, 4), 3, 0), np.delete(share.reshape(-1, 4), 3, 0))
    # the cache rows >= curL: NaN in every case of make_case; any other filling gives the same bits
    e = dict(c)
    e['kc'] = c['kc'].copy(); e['kc'][:, :, c['curL']:] = 7.0
    assert np.array_equal(R.run_host(e, 1)[2], tok)
    # an infinite score: no finite maximum, a NaN query by the contract
    f = dict(c)
    f['q'] = c['q'].copy(); f['q'][0, 0, :64] = np.float32(3e38)
    assert (R.run_host(f, 1)[2][0, 0, 0] == -1).all()


def _rc(c, radius=1, **kw):
    rows, H, l, S1 = c['rows'], c['H'], c['l'], len(c['ends'])
    a = dict(q=c['q'], kc=c['kc'], B2=rows, l=l, H=H, curL=c['curL'], Lmax=c['Lmax'], ends=c['ends'], S1=S1, pn=c['pn'], radius=radius,
             share=np.zeros((rows, H, S1 + 1), np.int64), ld_row=H * (S1 + 1), ld_head=S1 + 1, nan=np.zeros((rows, H), np.int32), tok=None,
             ld_tr=H * l * (S1 + 1), ld_th=l * (S1 + 1))
    a.update(kw)
    args = [hip.call_host.__globals__['ctypes'].c_void_p(v.ctypes.data) if isinstance(v, np.ndarray) else v for v in a.values()]
    return hip.lib().host['attn_profile_host_f32'](*args), a


def test_argument_checks():
    c = R.make_case(9, 14)
    assert _rc(c)[0] == 0
    e = c['ends']
    bad = [dict(B2=0), dict(l=0), dict(H=0), dict(curL=0), dict(S1=0), dict(pn=0), dict(Lmax=c['curL'] - 1), dict(pn=2), dict(S1=17), dict(radius=-1),
           dict(ends=np.asarray([1, 1, 14], np.int32)), dict(ends=np.asarray([5, 1, 14], np.int32)), dict(ends=np.asarray([1, 5, 13], np.int32)),
           dict(ends=np.asarray([1, 4, 14], np.int32)), dict(B2=65536), dict(H=65536)]
    for kw in bad:
        rc, a = _rc(c, **kw)
        assert rc == abi.EINVAL, kw
        assert not a['share'].any() and not a['nan'].any()
    big = R.make_case(1, 1)
    big.update(curL=4097, Lmax=5000, l=1, ends=np.asarray([4096, 4097], np.int32))          # curL > 4096 (checked before anything is read)
    assert _rc(big)[0] == abi.EINVAL
    l_gt = dict(c); l_gt.update(l=16, pn=4, curL=14)                                            # l > curL
    assert _rc(l_gt)[0] == abi.EINVAL
    mis = np.zeros(c['q'].size + 1, np.float32)[1:].reshape(c['q'].shape)                       # 4 bytes off a 16-byte boundary
    if mis.ctypes.data % 16:
        assert _rc(c, q=mis)[0] == abi.EINVAL
    assert (e == c['ends']).all()


# ---- attention_profile_torch on tiny CPU models -------------------------------------------------------------------------------------------
_M = {}


def _model(l2):
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


@pytest.mark.parametrize('l2', [True, False])
def test_torch_twin_on_a_tiny_model(l2):
    from var_amd.models.var import AttentionProfile
    vae, var = _model(l2)
    gt, lab = _inputs(var)
    p = var.attention_profile(gt, lab, radius=1, return_tokens=True)
    S, H, D = len(var.patch_nums), var.num_heads, var.depth
    assert isinstance(p, AttentionProfile) and 'AttentionProfile(' in repr(p)
    assert p.share_q.shape == (3, D, H, S, S + 1) and p.share_q.dtype == torch.int64
    assert p.nan_queries.shape == (3, D, H, S) and p.nan_queries.dtype == torch.int32 and not p.nan_queries.any()
    assert p.tokens.shape == (3, D, H, var.L, S + 1) and p.tokens.dtype == torch.int32
    assert p.layers == tuple(range(D)) and p.radius == 1 and p.patch_nums == tuple(var.patch_nums)
    sm = p.scale_matrix()
    assert sm.shape == (3, D, H, S, S) and sm.dtype == torch.float64
    assert float((sm.sum(-1) - 1).abs().max()) <= S / ONE
    assert not torch.triu(sm, 1).any()                                         # block-causal
    assert torch.equal(p.own_scale(), torch.diagonal(sm, dim1=-2, dim2=-1)) and (p.near() <= p.own_scale()).all()
    assert set(p.per_layer()) == {'scale_matrix', 'near', 'own_scale'} and p.per_layer()['near'].shape == (3, D, S)
    one = var.attention_profile(gt[1:2], lab[1:2], radius=1, return_tokens=True)             # alone against a batch of 3: the same integers
    assert torch.equal(one.share_q[0], p.share_q[1]) and torch.equal(one.tokens[0], p.tokens[1])
    sub = var.attention_profile(gt, lab, radius=1, layers=(1,), return_tokens=True)
    assert sub.layers == (1,) and torch.equal(sub.share_q[:, 0], p.share_q[:, 1]) and torch.equal(sub.tokens[:, 0], p.tokens[:, 1])
    assert var.attention_profile(gt, 2).share_q.shape == p.share_q.shape and var.attention_profile(gt, 2).tokens is None
    for kw in (dict(radius=-1), dict(radius=1.5), dict(layers=(1, 0)), dict(layers=(0, 0)), dict(layers=(D,)), dict(layers=()), dict(max_rows=0)):
        with pytest.raises(ValueError):
            var.attention_profile(gt, lab, **kw)
    with pytest.raises(ValueError):
        var.attention_profile(gt, lab[:2])
    with pytest.raises(ValueError):
        var.attention_profile(gt, torch.tensor([1, 2, var.num_classes + 1]))


def test_torch_twin_f32_against_f64():
    """the figure attnprofref.TORCH_F32_VS_F64 records: float32 modules against float64 modules, per-query shares, PyTorch alone"""
    worst = 0.0
    for l2 in (True, False):
        vae, var = _model(l2)
        gt, lab = _inputs(var)
        a = var.attention_profile(gt, lab, return_tokens=True)
        b = copy.deepcopy(var).double().attention_profile(gt, lab, return_tokens=True)
        worst = max(worst, float((a.tokens - b.tokens).abs().max()) / ONE)
    print(f'attention_profile_torch, f32 modules against f64 modules: {worst:.3e}')
    assert worst <= 4 * R.TORCH_F32_VS_F64          # (the record is from one CPU; another's GEMM may round a share across one more unit)
