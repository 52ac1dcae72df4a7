"""VAR.logit_lens without a GPU: the host twin of varhip_token_lens_f32 against the float64 definitions of tests/lensref.py within the derived
bars ("Logit lens"), its mechanics, the argument checks, LogitLens's methods and logit_lens_torch on a tiny CPU model."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import lensref as LR
from tests import util
from var_amd import abi, hip

R_, L_ = 3, 7
_M = {}


def _case(V):
    z, zf, gt = LR.rows(V, R_, L_, V)
    g = gt.view(-1).numpy()
    valid = (g >= 0) & (g < V)
    return z, zf, gt, g, valid


@pytest.mark.parametrize('V', [4096, 1000, 4099, 5000])
def test_host_twin_against_float64(V):
    z, zf, gt, g, valid = _case(V)
    nll, ent, kl, pred, rank = (o.view(-1).numpy() for o in LR.run_host(z, zf, gt, R_, L_, V))
    zn, zfn = z.numpy(), zf.numpy()
    n64, e64, k64, p64, r64 = LR.lens_defs(zn, zfn, np.where(valid, g, 0))
    # integers: exactly the definitions; pred is torch.argmax on every row, the out-of-range ones included
    assert np.array_equal(pred, z.argmax(-1).numpy()) and np.array_equal(pred[valid], p64[valid])
    assert np.array_equal(rank[valid], r64[valid]) and (rank[~valid] == -1).all() and np.isnan(nll[~valid]).all()
    assert (pred[2], rank[2], pred[3], rank[3], pred[6], rank[6], pred[LR.NAN_ROW]) == (5, 1, 9, 0, 0, 1, 33)
    assert rank[4] == int((z[4] > 0.125).sum()) + 1
    # nll: the project's bar of the row pass, on the rows whose reference is finite (the NaN row follows varhip_token_eval_f32: pinned on the GPU)
    fin = valid & np.isfinite(n64)
    ok, worst = LR.kernel_bar_ok(-nll[fin], -n64[fin], zn[fin])
    print(f'V={V}: nll max |diff| {worst:.3e}')
    assert ok and fin.sum() >= R_ * L_ - 5
    inf = valid & np.isinf(n64)                                                  # a token under a -inf logit
    assert np.array_equal(nll[inf].astype(np.float64), n64[inf])
    # entropy and kl: the derived bar; NaN and +inf exactly where the definitions have them (a token outside [0, V) does not touch them)
    for name, got, ref in (('entropy', ent, e64), ('kl', kl, k64)):
        ok, worst, bar = LR.bars_ok(got, ref, zn, zfn)
        print(f'V={V}: {name} max |diff| {worst:.3e}, smallest bar {bar:.3e}')
        assert ok, (name, worst, bar)
    assert kl[LR.KL_ZERO] == 0.0 and not np.signbit(kl[LR.KL_ZERO])
    assert np.isfinite(kl[LR.KL_FINITE]) and kl[LR.KL_FINITE] > 0 and kl[LR.KL_INF] == np.inf
    assert np.isnan(kl[LR.KL_NAN]) and np.isfinite(ent[LR.KL_NAN]) and np.isnan(kl[LR.NAN_ROW]) and np.isnan(ent[LR.NAN_ROW])
    assert (ent[np.isfinite(ent)] >= 0).all() and (ent[np.isfinite(ent)] <= np.log(V) * (1 + 1e-6)).all()


@pytest.mark.parametrize('V', [4096, 4099])
def test_the_bars_catch_a_dropped_element(V):
    """the planted fault: the same sums without the row's last element, on a copy of the reference"""
    z, zf, gt, g, valid = _case(V)
    _, e64, k64, _, _ = LR.lens_defs(z.numpy(), zf.numpy(), np.where(valid, g, 0))
    _, e_bad, k_bad, _, _ = LR.lens_defs(z.numpy(), zf.numpy(), np.where(valid, g, 0), drop_last=True)
    for name, bad, ref in (('entropy', e_bad, e64), ('kl', k_bad, k64)):
        ok, worst, bar = LR.bars_ok(bad, ref, z.numpy(), zf.numpy())
        print(f'V={V}: {name} with the last element dropped: max |diff| {worst:.3e}, smallest bar {bar:.3e}')
        assert not ok


@pytest.mark.parametrize('V', [4096, 1000, 4099])
def test_twin_bits_do_not_depend_on_alignment(V):
    z, zf, gt, _, _ = _case(V)
    want = LR.run_host(z, zf, gt, R_, L_, V)
    za, zfa = torch.empty(z.numel() + 8), torch.empty(zf.numel() + 8)
    off = [(4 - (t.data_ptr() % 16) // 4) % 4 + 1 for t in (za, zfa)]              # 4 bytes past a 16-byte boundary
    z1, zf1 = za[off[0]:off[0] + z.numel()].view_as(z), zfa[off[1]:off[1] + zf.numel()].view_as(zf)
    z1.copy_(z); zf1.copy_(zf)
    assert z1.data_ptr() % 16 == 4 and zf1.data_ptr() % 16 == 4
    got = LR.run_host(z1, zf1, gt, R_, L_, V)
    for a, b in zip(want, got):
        assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)
    same = LR.run_host(z, z, gt, R_, L_, V)                                      # one pointer: kl = +0.0 on every row without a NaN
    k = same[2].view(-1)
    assert np.isnan(k[LR.NAN_ROW].item()) and torch.equal(torch.cat((k[:LR.NAN_ROW], k[LR.NAN_ROW + 1:])).view(torch.int32), torch.zeros(R_ * L_ - 1, dtype=torch.int32))
    assert torch.equal(same[1].view(torch.int32), want[1].view(torch.int32))


def test_refused_sizes_write_nothing():
    V = 1000
    z, zf, gt, _, _ = _case(V)
    outs = lambda: [torch.full((R_, L_), LR.SENT_F), torch.full((R_, L_), LR.SENT_F), torch.full((R_, L_), LR.SENT_F),
                    torch.full((R_, L_), LR.SENT_I, dtype=torch.int64), torch.full((R_, L_), LR.SENT_I, dtype=torch.int32)]
    good = dict(ld_gt=L_, R=R_, l=L_, V=V, ld_out=L_)
    for bad in (dict(R=0), dict(l=0), dict(V=0), dict(ld_gt=L_ - 1), dict(ld_out=L_ - 1), dict(null=0), dict(null=1), dict(null=2), dict(null=5)):
        a = dict(good, **{k: v for k, v in bad.items() if k != 'null'})
        o = outs()
        ops = [z, zf, gt] + o
        if 'null' in bad:
            ops[bad['null']] = None
        rc = hip.lib().host['token_lens_host_f32'](*[None if t is None else t.data_ptr() for t in ops[:3]], a['ld_gt'], a['R'], a['l'], a['V'],
                                                   *[None if t is None else t.data_ptr() for t in ops[3:]], a['ld_out'])
        assert rc == abi.EINVAL, bad
        for t, ref in zip(o, outs()):
            assert torch.equal(t, ref), bad


# ---- the public call on a tiny CPU model: the PyTorch route ------------------------------------------------------------------------------------
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
        _M['m'] = (var, gt, lab, var.logit_lens(gt, lab))
    return _M['m']


def test_torch_route_on_a_tiny_model():
    from var_amd.models.var import LogitLens
    var, gt, lab, r = _model()
    D, N, L, V = var.depth, 3, var.L, var.V
    assert 2 <= D <= 4 and isinstance(r, LogitLens) and r.layers == tuple(range(D)) and r.patch_nums == tuple(var.patch_nums)
    for t, dt in ((r.nll, torch.float32), (r.entropy, torch.float32), (r.kl, torch.float32), (r.pred, torch.int64), (r.rank, torch.int32)):
        assert t.shape == (N, D, L) and t.dtype == dt
    x = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    with torch.no_grad():
        z = var._forward_torch(lab, x)
    want = -torch.log_softmax(z.double(), -1).gather(-1, gt.unsqueeze(-1)).squeeze(-1)
    err = float((r.nll[:, -1].double() - want).abs().max())
    print(f'last layer nll vs -log_softmax(forward logits): max |diff| {err:.3e}')
    assert err <= 2.0 ** -24 * float(want.abs().max())                            # one rounding to float32
    assert torch.equal(r.pred[:, -1], z.argmax(-1))
    assert torch.equal(r.kl[:, -1], torch.zeros(N, L)) and bool((r.kl >= 0).all()) and bool((r.kl[:, 0] > 0).all())
    assert bool((r.entropy >= 0).all()) and bool((r.entropy <= float(np.log(V))).all())
    for bi in (1, 0):                                                             # (the same batching: PyTorch's CPU GEMMs are not batch-invariant)
        one = var.logit_lens(gt, lab, layers=(bi,))
        for k in ('nll', 'entropy', 'kl', 'pred', 'rank'):
            assert torch.equal(getattr(one, k)[:, 0], getattr(r, k)[:, bi]), (bi, k)
        assert one.layers == (bi,)
    two = var.logit_lens(gt, lab, max_rows=2)                                     # two passes: the same values up to the GEMMs' rounding
    assert float((two.nll - r.nll).abs().max()) <= 1e-4 and two.nll.shape == r.nll.shape
    assert float((var.logit_lens(gt[:1], 1).nll - r.nll[:1]).abs().max()) <= 1e-4           # an int label


def test_argument_refusals():
    var, gt, lab, _ = _model()
    D = var.depth
    for kw in (dict(layers=(D,)), dict(layers=(-1,)), dict(layers=(1, 0)), dict(layers=(0, 0)), dict(layers=()), dict(layers=(0.5,)), dict(max_rows=0)):
        with pytest.raises(ValueError):
            var.logit_lens(gt, lab, **kw)
    for bad_gt, bad_lab in ((gt[:, :-1], lab), (gt.view(-1), lab), (gt, lab[:2]), (gt, torch.tensor([1, 2, var.num_classes + 1])), (gt, torch.tensor([1, -1, 0]))):
        with pytest.raises(ValueError):
            var.logit_lens(bad_gt, bad_lab)
    bad = gt.clone(); bad[0, 0] = var.V
    with pytest.raises(ValueError):
        var.logit_lens(bad, lab)


def test_methods_on_a_hand_made_result():
    from var_amd.models.var import LogitLens
    # one image, layers (0, 2, 5), patch_nums (1, 2): L = 5
    pred = torch.tensor([[[7, 1, 3, 4, 9],
                          [7, 2, 8, 4, 0],
                          [7, 2, 3, 4, 5]]])
    rank = torch.tensor([[[0, 3, 0, 1, 2], [0, 0, 5, 0, 0], [0, 0, 0, 0, 1]]], dtype=torch.int32)
    nll = torch.arange(15, dtype=torch.float32).view(1, 3, 5)
    r = LogitLens((0, 2, 5), nll, nll * 2, nll * 0.5, pred, rank, (1, 2))
    assert r.agree().tolist() == [[[True, False, True, True, False], [True, True, False, True, False], [True] * 5]]
    assert r.settle_depth().tolist() == [[0, 2, 5, 0, 5]]
    assert r.acc().tolist() == [[1.0, 0.25], [1.0, 0.75], [1.0, 0.75]]
    ps = r.per_scale()
    assert ps['nll'].dtype == torch.float64 and ps['nll'].tolist() == [[0.0, 2.5], [5.0, 7.5], [10.0, 12.5]]
    assert ps['entropy'].tolist() == [[0.0, 5.0], [10.0, 15.0], [20.0, 25.0]] and ps['kl'].tolist() == [[0.0, 1.25], [2.5, 3.75], [5.0, 6.25]]
    assert ps['agree'].tolist() == [[1.0, 0.5], [1.0, 0.5], [1.0, 1.0]] and torch.equal(ps['acc'], r.acc())
