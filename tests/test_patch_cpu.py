"""VAR.patch_effects without a GPU: the host twin of varhip_act_patch_f32 against the numpy restatement tests/patchref.py, bit for bit and inside
guard bands; its refusals; and the public call on a tiny CPU model through patch_effects_torch: argument refusals, the identities between sites
and modes, PatchEffects' methods, and zero ablation against weight surgery in float64."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

from tests import patchref as PR
from tests import util
from var_amd import abi, hip

_M = {}
DECK = PR.deck()


def _host(act, ld, rows, l, width, dirs, n_dir):
    fn = hip.lib().host['act_patch_host_f32']
    return util.guarded_invoke('varhip_act_patch_host_f32', [act, ld, rows, l, width, dirs, n_dir], lambda *a: fn(*a))


@pytest.mark.parametrize('case', DECK, ids=[c[0] for c in DECK])
def test_host_twin_is_the_numpy_restatement(case):
    name, rows, l, width, ld, dirs = case
    act = PR.matrix(rows, l, width, ld, len(name) + l)
    want = PR.apply(act, rows, l, width, dirs)
    assert not np.array_equal(want.view(np.int32), act.view(np.int32)), 'the case changes nothing'
    got = act.copy()
    assert _host(got, ld, rows, l, width, dirs, len(dirs)) == 0
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    assert np.isnan(got[:, width:]).all() and np.array_equal(got[:, width:].view(np.int32), act[:, width:].view(np.int32))
    if l == 1:                                                 # the mean of one token: the bits stay
        mean_only = dirs[dirs[:, 3] == PR.MEAN]
        one = act.copy()
        assert _host(one, ld, rows, l, width, mean_only, len(mean_only)) == 0 and np.array_equal(one.view(np.int32), act.view(np.int32))


def test_the_mean_is_the_ascending_fp32_sum():
    """a column whose ascending fp32 sum differs from the float64 mean and from the descending sum: the twin gives the ascending one"""
    l = 9
    act = np.zeros((l, 4), dtype=np.float32)
    act[:, 0] = [1e8, 3.0, -1e8, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]           # ascending 6, descending 8, exactly 9
    s = np.float32(0)
    for t in range(l):
        s = np.float32(s + act[t, 0]) if t else act[0, 0]
    down = act[l - 1, 0]
    for t in range(l - 2, -1, -1):
        down = np.float32(down + act[t, 0])
    assert s != down and float(s) != float(act[:, 0].astype(np.float64).sum())
    got = act.copy()
    assert _host(got, 4, 1, l, 4, np.array([[0, 0, 4, PR.MEAN]], dtype=np.int32), 1) == 0
    assert (got[:, 0] == np.float32(s / np.float32(l))).all() and not got[:, 1:].any()


def test_skipped_directives_write_nothing():
    rows, l, width = 3, 4, 128
    act = PR.matrix(rows, l, width, width, 5)
    bad = np.array([(-1, 0, 64, -1), (3, 0, 64, -1), (0, 0, 64, 3), (0, 0, 64, -3), (0, -4, 64, -1), (0, 64, 132, -1), (0, 64, 64, -2), (0, 64, 0, -2),
                    (0, 2, 64, -1), (0, 0, 62, -1), (0, 1, 5, 1)], dtype=np.int32)
    got = act.copy()
    assert _host(got, width, rows, l, width, bad, len(bad)) == 0 and np.array_equal(got.view(np.int32), act.view(np.int32))
    for d in bad:                                              # each alone, too
        assert _host(got, width, rows, l, width, d.reshape(1, 4).copy(), 1) == 0 and np.array_equal(got.view(np.int32), act.view(np.int32)), d


def test_refusals_write_nothing():
    rows, l, width, ld = 2, 4, 128, 132
    act = PR.matrix(rows, l, width, ld, 6)
    dirs = np.array([[0, 0, 64, PR.ZERO], [1, 64, 128, PR.MEAN]], dtype=np.int32)
    fn = hip.lib().host['act_patch_host_f32']
    good = dict(ld=ld, rows=rows, l=l, width=width, n=2)
    odd = np.full(rows * l * ld + 4, np.nan, dtype=np.float32)[1:1 + rows * l * ld].reshape(rows * l, ld)          # 4 bytes past a 16-byte boundary
    odd[:] = act
    assert odd.ctypes.data % 16 == 4
    for bad in (dict(rows=0), dict(l=0), dict(width=0), dict(rows=-1), dict(n=-1), dict(ld=width - 4, width=width), dict(ld=ld + 2), dict(null='act'),
                dict(null='dir'), dict(odd=True)):
        a = dict(good, **{k: v for k, v in bad.items() if k not in ('null', 'odd')})
        m = odd if bad.get('odd') else act.copy()
        before = m.copy()
        ap = None if bad.get('null') == 'act' else m.ctypes.data
        dp = None if bad.get('null') == 'dir' else dirs.ctypes.data
        assert PR.refused(None if ap is None else m, a['ld'], a['rows'], a['l'], a['width'], None if dp is None else dirs, a['n']), bad
        assert fn(ap, a['ld'], a['rows'], a['l'], a['width'], dp, a['n']) == abi.EINVAL, bad
        assert np.array_equal(m.view(np.int32), before.view(np.int32)), bad
    m = act.copy()                                             # n_dir == 0: success, nothing read or written, whatever else is passed
    assert fn(m.ctypes.data, ld, rows, l, width, None, 0) == 0 and fn(None, 0, 0, 0, 0, None, 0) == 0
    assert np.array_equal(m.view(np.int32), act.view(np.int32))
    assert fn(m.ctypes.data, ld, rows, l, width, dirs.ctypes.data, 2) == 0                                      # the same operands, accepted
    assert np.array_equal(m.view(np.int32), PR.apply(act, rows, l, width, dirs).view(np.int32))


# ---- the public call on a tiny CPU model: the PyTorch route ------------------------------------------------------------------------------------
SITES = (('head', 0, 0), ('head', 1, 1), ('attn', 0), ('mlp', 1), (('head', 0, 0), ('head', 0, 1)), (('head', 1, 0), ('mlp', 0)))
FIELDS = ('nll', 'entropy', 'kl', 'pred', 'rank')


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
        gt, lab = torch.randint(0, var.V, (2, var.L), generator=g), torch.tensor([1, var.num_classes])
        _M['m'] = (var, gt, lab)
    return _M['m']


def _same(a, i, b, j, what):
    for k in FIELDS:
        assert torch.equal(getattr(a, k)[:, i], getattr(b, k)[:, j]), f'{what}: {k}'


def test_result_and_clean_row():
    from var_amd.models.var import PatchEffects
    var, gt, lab = _model()
    assert var.depth == 2 and var.num_heads == 2 and var.patch_nums[0] == 1
    r = var.patch_effects(gt, lab, SITES, mode='zero')
    N, P, L = 2, len(SITES), var.L
    assert isinstance(r, PatchEffects) and r.mode == 'zero' and r.scales == tuple(range(len(var.patch_nums))) and r.patch_nums == tuple(var.patch_nums)
    assert r.sites == ((('head', 0, 0),), (('head', 1, 1),), (('attn', 0),), (('mlp', 1),), (('head', 0, 0), ('head', 0, 1)), (('head', 1, 0), ('mlp', 0)))
    for k, dt in zip(FIELDS, (torch.float32, torch.float32, torch.float32, torch.int64, torch.int32)):
        assert getattr(r, k).shape == (N, P + 1, L) and getattr(r, k).dtype == dt
    with torch.no_grad():                                                                # (an image at a time: the twin's rows are passes of their own)
        z = torch.cat([var._forward_torch(lab[i:i + 1], var.vae_proxy[0].quantize.idxBl_to_var_input([gt[i:i + 1, b:e] for b, e in var.begin_ends]))
                       for i in range(N)])
    want = -torch.log_softmax(z.double(), -1).gather(-1, gt.unsqueeze(-1)).squeeze(-1)
    err = float((r.nll[:, 0].double() - want).abs().max())
    print(f'clean row nll vs -log_softmax(forward logits): max |diff| {err:.3e}')
    assert err <= 1e-5 and torch.equal(r.pred[:, 0], z.argmax(-1))
    assert torch.equal(r.kl[:, 0], torch.zeros(N, L)) and not bool(torch.signbit(r.kl[:, 0]).any())
    assert bool((r.kl[:, 1:] > 0).all()) and bool(torch.isfinite(r.nll).all()) and bool((r.entropy >= 0).all())
    assert torch.equal(r.effect(), r.nll[:, 1:] - r.nll[:, :1])
    ps = r.per_scale()
    assert ps['effect'].shape == (P, len(var.patch_nums)) and ps['effect'].dtype == torch.float64 and ps['kl'].shape == ps['effect'].shape
    b, e = var.begin_ends[2]
    assert abs(float(ps['effect'][3, 2]) - float(r.effect()[:, 3, b:e].double().mean())) <= 1e-12
    hm = r.head_matrix()
    assert hm.shape == (2, 2) and bool(torch.isnan(hm[0, 1])) and bool(torch.isnan(hm[1, 0]))
    assert abs(float(hm[0, 0]) - float(r.effect()[:, 0].double().mean())) <= 1e-12 and abs(float(hm[1, 1]) - float(r.effect()[:, 1].double().mean())) <= 1e-12
    full = var.patch_effects(gt[:1], 1, mode='zero')                                     # sites=None: every head, every attn, every mlp, in that order
    assert full.sites == tuple((('head', b, h),) for b in range(2) for h in range(2)) + ((('attn', 0),), (('attn', 1),), (('mlp', 0),), (('mlp', 1),))
    assert not bool(torch.isnan(full.head_matrix()).any())
    for j, i in ((-1, -1), (0, 0), (3, 1), (4, 2), (7, 3)):                             # (-1: the clean row)
        for k in FIELDS:
            assert torch.equal(getattr(full, k)[0, j + 1], getattr(r, k)[0, i + 1]), (j, k)


@pytest.mark.parametrize('mode', ['zero', 'mean', 'donor'])
def test_identities(mode):
    var, gt, lab = _model()
    kw = dict(mode=mode, donor_label=torch.tensor([7, 3])) if mode == 'donor' else dict(mode=mode)
    r = var.patch_effects(gt, lab, SITES, **kw)
    _same(r, 3, r, 5, "('attn', 0) against the tuple of its heads")
    assert torch.equal(r.kl[:, 0], torch.zeros(2, var.L))
    if mode == 'donor':                                        # the donor under the image's own label: every row is the clean row
        own = var.patch_effects(gt, lab, SITES, mode='donor', donor_label=lab)
        for j in range(len(SITES) + 1):
            _same(own, j, r, 0, f'donor_label == label, row {j}')
        assert bool((r.kl[:, 3, 0] > 0).all())                 # another label: the class reaches the first token through block 0's attention
        uncond = var.patch_effects(gt[:1], lab[:1], SITES[:1], mode='donor', donor_label=var.num_classes)
        assert bool((uncond.kl[:, 1] > 0).any())
    if mode == 'mean':                                         # scale 0 has one token: its mean is itself
        first = var.patch_effects(gt, lab, SITES, mode='mean', scales=(0,))
        for j in range(len(SITES) + 1):
            _same(first, j, r, 0, f'mean at scales=(0,), row {j}')
    some = var.patch_effects(gt, lab, SITES, scales=(2, 1), **kw)                        # scales apply from their first token on
    b1 = var.begin_ends[1][0]
    for k in FIELDS:
        assert torch.equal(getattr(some, k)[:, :, :b1], getattr(r, k)[:, :1, :b1].expand(-1, len(SITES) + 1, -1)), k
    assert some.scales == (1, 2) and not torch.equal(some.nll[:, 1:, b1:], r.nll[:, :1, b1:].expand(-1, len(SITES), -1))
    _same(var.patch_effects(gt, lab, SITES, max_rows=3, **kw), slice(None), r, slice(None), 'max_rows')


def _forward64(var, lab, x):
    """VAR._forward_torch in the model's own dtype (get_logits casts to fp32)"""
    cond = var.class_emb(lab)
    B = lab.shape[0]
    sos = cond.unsqueeze(1).expand(B, var.first_l, -1) + var.pos_start.expand(B, var.first_l, -1)
    h = torch.cat((sos, var.word_embed(x)), dim=1) + var.lvl_embed(var.lvl_1L[:, :var.L].expand(B, -1)) + var.pos_1LC[:, :var.L]
    mask = var.attn_bias_for_masking[:, :, :var.L, :var.L].to(h.dtype)
    cg = var.shared_ada_lin(cond)
    for blk in var.blocks:
        h = blk(x=h, cond_BD=cg, attn_bias=mask)
    return var.head(var.head_nm(h, cond))


def test_zero_ablation_is_weight_surgery_in_float64():
    from var_amd.models import args as A
    from var_amd.models.var import patch_effects_torch
    var, gt, lab = _model()
    v64 = copy.deepcopy(var).double()
    sites = A.patch_sites((('head', 0, 1), ('head', 1, 0), ('mlp', 0), ('mlp', 1), ('attn', 1)), 2, 2)
    cols = A.patch_columns(sites, var.C, v64.blocks[0].ffn.fc1.weight.shape[0])
    with torch.no_grad():
        nll = patch_effects_torch(v64, gt, lab, cols, 'zero', None, tuple(range(len(var.patch_nums))))[0]
        assert nll.dtype == torch.float64 and nll.shape == (2, len(sites) + 1, var.L)
        # (an image's fp32 input computed on its own, as the twin does: the quantizer's interpolation is not batch-invariant)
        x = torch.cat([v64.vae_proxy[0].quantize.idxBl_to_var_input([gt[n:n + 1, b:e] for b, e in var.begin_ends]) for n in range(2)]).double()
        for j, group in enumerate(((),) + sites):
            cut = copy.deepcopy(v64)
            for e in group:
                if e[0] == 'mlp':
                    cut.blocks[e[1]].ffn.fc2.weight.zero_()
                else:
                    c0, c1 = (64 * e[2], 64 * e[2] + 64) if e[0] == 'head' else (0, var.C)
                    cut.blocks[e[1]].attn.proj.weight[:, c0:c1] = 0
            z = _forward64(cut, lab, x)
            want = -torch.log_softmax(z, -1).gather(-1, gt.unsqueeze(-1)).squeeze(-1)
            err = float((nll[:, j] - want).abs().max())
            print(f'{group or "clean"}: max |nll - surgery| {err:.2e}')
            assert err <= 1e-10, (group, err)
            assert j == 0 or float((nll[:, j] - nll[:, 0]).abs().max()) > 1e-3          # ... and the ablation does something


def test_argument_refusals():
    var, gt, lab = _model()
    bad_sites = [(), 'head', (('head', 0),), (('head', 0, 2),), (('head', 2, 0),), (('attn', 0, 0),), (('mlp', -1),), (('mlp', 0.0),), (('proj', 0),), ((),),
                 ((('head', 0, 0), ('head', 0, 0)),), ((('head', 0, 0), ('attn', 0)),), ((('mlp', 1), ('mlp', 1)),), (('head', True, 0),), 3, ((3, 0),)]
    for s in bad_sites:
        with pytest.raises(ValueError, match='sites'):
            var.patch_effects(gt, lab, s)
    with pytest.raises(ValueError, match=r"\('head', 0, 2\)"):                         # the message names the offending site
        var.patch_effects(gt, lab, (('mlp', 0), ('head', 0, 2)))
    for kw in (dict(mode='noise'), dict(mode='donor'), dict(mode='zero', donor_label=3), dict(mode='donor', donor_label=var.num_classes + 1),
               dict(mode='donor', donor_label=torch.tensor([1, 2, 3])), dict(mode='donor', donor_label=-1), dict(mode='donor', donor_label=1.5),
               dict(scales=()), dict(scales=(len(var.patch_nums),)), dict(scales=(0, 0)), dict(scales=(-1,)), dict(scales=0.5), dict(max_rows=1),
               dict(max_rows=2.0), dict(mode='donor', donor_label=1, max_rows=2)):
        with pytest.raises(ValueError):
            var.patch_effects(gt, lab, SITES, **kw)
    for bad_gt, bad_lab in ((gt[:, :-1], lab), (gt.view(-1), lab), (gt, lab[:1]), (gt, torch.tensor([1, var.num_classes + 1])), (gt, torch.tensor([-1, 0]))):
        with pytest.raises(ValueError):
            var.patch_effects(bad_gt, bad_lab, SITES)
    bad = gt.clone(); bad[0, 0] = var.V
    with pytest.raises(ValueError):
        var.patch_effects(bad, lab, SITES)
    assert var.patch_effects(gt, lab, SITES[:1], mode='donor', donor_label=1, max_rows=3).nll.shape == (2, 2, var.L)
