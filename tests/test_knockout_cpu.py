"""VAR.attention_knockout without a GPU: the yardstick of the GPU kernel tests proven on the CPU (the oracle's attn_cached_f32 on the gathered
cache against the float64 masked reference of tests/knockoutcases.py, a planted off-by-one in the gather caught, the deck's coverage recomputed),
and the public call on a tiny CPU model through attention_knockout_torch: refusals, the clean row, causality, the identities between edges,
entry order, and AttentionKnockout's methods."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import knockoutcases as KC
from tests import util

CASES = KC.cases()
FIELDS = ('nll', 'entropy', 'kl', 'pred', 'rank')
_M = {}


def _oracle():
    util.ensure_oracle_built()
    from oracle import var_oracle
    return var_oracle.lib()


def _twin(L, q, kc, vc, n):
    """the oracle's attn_cached_f32 for one (row, head): l queries [l][64] over a cache of exactly n keys"""
    from oracle.var_oracle import _p
    out = np.full(q.shape, np.nan, np.float32)
    q, kc, vc = (np.ascontiguousarray(a, dtype=np.float32) for a in (q, kc, vc))
    assert L['attn_cached_f32'](_p(q), _p(kc), _p(vc), _p(out), 1, q.shape[0], 1, n, kc.shape[0]) == 0
    return out


def test_the_deck_covers_what_it_claims():
    assert KC.coverage(CASES) == KC.COVERAGE
    for c in CASES:
        assert c['H'] == 2 and c['B2'] <= 3 and c['l'] <= c['curL'] < c['Lmax'] and 1 <= c['S1'] <= 16
        b = KC.build(c)
        assert np.isnan(b.k[:, :, c['curL']:]).all() and np.isnan(b.v[:, :, c['curL']:]).all()
        for bb in range(c['B2']):
            for h in range(c['H']):
                vis = KC.visible(c['ends'], c['masks'][bb][h])
                assert np.isfinite(b.k[bb, h, :c['curL']][vis]).all() and np.isnan(b.k[bb, h, :c['curL']][~vis]).all()
                assert np.isfinite(b.v[bb, h, :c['curL']][vis]).all() and np.isnan(b.v[bb, h, :c['curL']][~vis]).all()


@pytest.mark.parametrize('c', CASES, ids=[c['name'] for c in CASES])
def test_gather_then_the_oracle_is_within_the_float64_bar(c):
    L, b = _oracle(), KC.build(c)
    worst = 0.0
    for bb in range(c['B2']):
        for h in range(c['H']):
            mask = c['masks'][bb][h]
            vis = KC.visible(c['ends'], mask)
            q = KC.q_of(b, bb, h)
            ref, bar = KC.masked_reference(q, b.k[bb, h], b.v[bb, h], vis)
            kc, vc, n = KC.gather(mask, c['ends'], b.k[bb, h], b.v[bb, h])
            assert n == int(vis.sum()) == KC.n_visible(c, bb, h)
            if n == 0:
                assert not ref.any() and not bar.any()
                continue
            assert np.isfinite(kc).all() and np.isfinite(vc).all()
            got = _twin(L, q, kc, vc, n).astype(np.float64)
            assert np.isfinite(got).all()
            ratio = float((np.abs(got - ref) / bar).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (bb, h, ratio)
    print(f"{c['name']}: max |oracle(gathered) - masked float64| / bar = {worst:.3f}")


def test_a_planted_off_by_one_in_the_gather_is_caught():
    """every visible scale behind the cache's first taken one row further on: on every (row, head) where that moves a finite row the result
    leaves the bar by a wide margin (where the shifted row is a hidden scale's NaN, the result is NaN)"""
    L = _oracle()
    caught = 0
    for c in CASES[:6]:
        b = KC.build(c)
        for bb in range(c['B2']):
            for h in range(c['H']):
                mask = c['masks'][bb][h]
                vis = KC.visible(c['ends'], mask)
                if not vis[1:].any():
                    continue
                q = KC.q_of(b, bb, h)
                ref, bar = KC.masked_reference(q, b.k[bb, h], b.v[bb, h], vis)
                kc, vc, n = KC.gather(mask, c['ends'], b.k[bb, h], b.v[bb, h], shift=1)
                got = _twin(L, q, kc, vc, n).astype(np.float64)
                with np.errstate(invalid='ignore'):
                    off = np.abs(got - ref) / bar
                assert np.isnan(off).any() or float(off.max()) > 100.0, (c['name'], bb, h, float(np.nanmax(off)))
                caught += 1
    assert caught >= 15


# ---- the public call on a tiny CPU model: the PyTorch route ------------------------------------------------------------------------------------
EDGES = ((1, 0), (2, 1), (3, 3), (4, 2), ((4, 0), (4, 1)), (3, 1, 1), (2, 0, 0, 1), ((3, 1, 0), (3, 1, 1)))


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


def _full():
    if 'r' not in _M:
        var, gt, lab = _model()
        _M['r'] = var.attention_knockout(gt, lab, EDGES)
    return _M['r']


def _same(a, i, b, j, what, tokens=slice(None)):
    for k in FIELDS:
        assert torch.equal(getattr(a, k)[:, i, tokens], getattr(b, k)[:, j, tokens]), f'{what}: {k}'


def test_result_and_the_clean_row_is_evaluate():
    from var_amd.models import args as A
    from var_amd.models.var import AttentionKnockout, attention_knockout_torch
    var, gt, lab = _model()
    assert var.depth == 2 and var.num_heads == 2 and tuple(var.patch_nums) == (1, 2, 3, 4, 5)
    r = _full()
    N, P, L, S = 2, len(EDGES), var.L, 5
    assert isinstance(r, AttentionKnockout) and r.layers == (0, 1) and r.heads == (0, 1) and r.patch_nums == (1, 2, 3, 4, 5)
    assert r.edges[0] == ((1, 0, (0, 1), (0, 1)),) and r.edges[5] == ((3, 1, (1,), (0, 1)),) and r.edges[6] == ((2, 0, (0,), (1,)),)
    for k, dt in zip(FIELDS, (torch.float32, torch.float32, torch.float32, torch.int64, torch.int32)):
        assert getattr(r, k).shape == (N, P + 1, L) and getattr(r, k).dtype == dt
    # the clean row: the logits of the model's own forward pass, bit for bit (an image at a time: the route's rows are passes of their own),
    # so pred and rank are evaluate's exactly and nll is the float64 log-softmax of evaluate's logits
    seen = {}
    cuts = A.knockout_masks(r.edges[:1], var.num_heads)
    attention_knockout_torch(var, gt, lab, cuts, _tap=lambda n, j, z: seen.__setitem__((n, j), z))
    for i in range(N):
        x = var.vae_proxy[0].quantize.idxBl_to_var_input([gt[i:i + 1, b:e] for b, e in var.begin_ends])
        with torch.no_grad():
            z = var._forward_torch(lab[i:i + 1], x)[0].float()
        assert torch.equal(seen[(i, 0)], z), 'the clean row is not the forward pass'
        assert not torch.equal(seen[(i, 1)], z)
        ev = var.evaluate(gt[i:i + 1], lab[i:i + 1])
        assert torch.equal(r.pred[i, 0], ev.pred_BL[0]) and torch.equal(r.rank[i, 0], ev.rank_BL[0])
        want = -torch.log_softmax(z.double(), -1).gather(-1, gt[i].unsqueeze(-1)).squeeze(-1)
        assert torch.equal(r.nll[i, 0], want.float())
        assert float((r.nll[i, 0] - ev.nll_BL[0]).abs().max()) <= 2e-6              # (evaluate's CPU route takes the log-softmax in fp32)
    assert torch.equal(r.kl[:, 0], torch.zeros(N, L)) and not bool(torch.signbit(r.kl[:, 0]).any())
    assert bool(torch.isfinite(r.nll).all()) and bool((r.entropy >= 0).all()) and bool((r.kl[:, 1:] >= 0).all())
    # the methods
    assert torch.equal(r.effect(), r.nll[:, 1:] - r.nll[:, :1])
    ps = r.per_scale()
    assert ps['effect'].shape == (P, S) and ps['effect'].dtype == torch.float64 and ps['kl'].shape == (P, S)
    b3, e3 = var.begin_ends[3]
    assert abs(float(ps['effect'][2, 3]) - float(r.effect()[:, 2, b3:e3].double().mean())) <= 1e-12
    mq, ma = r.edge_matrix(), r.edge_matrix(at='all')
    assert mq.shape == (S, S) and mq.dtype == torch.float64
    assert int((~torch.isnan(mq)).sum()) == 6 and bool(torch.isnan(mq[4, 0])) and torch.equal(torch.isnan(mq), torch.isnan(ma))
    b4 = var.begin_ends[4][0]
    assert abs(float(mq[4, 2]) - float(r.effect()[:, 3, b4:].double().mean())) <= 1e-12
    assert abs(float(mq[3, 3]) - float(r.effect()[:, 2, b3:e3].double().mean())) <= 1e-12
    assert abs(float(ma[3, 3]) - float(r.effect()[:, 2, b3:].double().mean())) <= 1e-12
    assert abs(float(mq[3, 1]) - float(r.effect()[:, 5, b3:e3].double().mean())) <= 1e-12           # (a per-layer edge counts as a single edge)
    with pytest.raises(ValueError, match='at must be'):
        r.edge_matrix(at='key')


def test_default_sweep():
    var, gt, lab = _model()
    full = var.attention_knockout(gt[:1], 1)
    want = [(q, k) for q in range(5) for k in range(q)] + [(q, q) for q in range(1, 5)]
    assert [g[0][:2] for g in full.edges] == want and all(len(g) == 1 for g in full.edges) and len(want) == 14
    assert len([(q, k) for q in range(10) for k in range(q)] + [(q, q) for q in range(1, 10)]) == 54
    assert not bool(torch.isnan(full.edge_matrix())[torch.tril(torch.ones(5, 5, dtype=torch.bool))][1:].any()) and bool(torch.isnan(full.edge_matrix()[0, 0]))
    r = _full()
    for j, i in ((want.index((1, 0)), 0), (want.index((2, 1)), 1), (want.index((3, 3)), 2), (want.index((4, 2)), 3)):
        for k in FIELDS:
            assert torch.equal(getattr(full, k)[0, j + 1], getattr(r, k)[0, i + 1]), (j, k)


def test_causality_and_the_cut_does_something():
    """the tokens of the scales below q of an edge (q, k) are the clean row's, exactly; some token of scale q is not"""
    var = _model()[0]
    r = _full()
    for j, group in enumerate(r.edges):
        q0 = min(e[0] for e in group)
        b, e = var.begin_ends[q0]
        _same(r, j + 1, r, 0, f'{EDGES[j]}: the scales below {q0}', slice(0, b))
        assert not torch.equal(r.nll[:, j + 1, b:e], r.nll[:, 0, b:e]), f'{EDGES[j]}: no token of scale {q0} changed'
        assert bool((r.kl[:, j + 1, b:e] > 0).any())


def test_all_layers_is_the_tuple_of_its_per_layer_edges():
    var, gt, lab = _model()
    r = _full()
    both = var.attention_knockout(gt, lab, [((2, 1, 0), (2, 1, 1)), ((2, 1, 0, 0), (2, 1, 0, 1), (2, 1, 1, 0), (2, 1, 1, 1)), (2, 1)], layers=(0, 1))
    for j in range(3):
        _same(both, j + 1, r, 2, f'(2, 1) against its per-layer / per-head edges, form {j}')
    one = var.attention_knockout(gt, lab, [(3, 1)], layers=(1,))
    _same(one, 1, r, 6, '(3, 1) with layers=(1,) against (3, 1, 1)')
    _same(r, 8, r, 0, 'both layers of (3, 1) written out: the scales below 3', slice(0, var.begin_ends[3][0]))
    h1 = var.attention_knockout(gt, lab, [(2, 0, 0)], heads=(1,))
    _same(h1, 1, r, 7, '(2, 0, 0) with heads=(1,) against (2, 0, 0, 1)')
    whole = var.attention_knockout(gt, lab, [(3, 1)])
    _same(whole, 1, r, 8, '(3, 1) over all layers against the tuple of its per-layer edges')
    assert not torch.equal(one.nll[:, 1], whole.nll[:, 1])                                # ... and one layer is not both


def test_entry_order_and_packing_change_nothing():
    var, gt, lab = _model()
    r = _full()
    perm = [5, 2, 7, 0, 4, 1, 6, 3]
    other = var.attention_knockout(gt, lab, [EDGES[j] for j in perm], max_rows=3)
    _same(other, 0, r, 0, 'the clean row')
    for i, j in enumerate(perm):
        _same(other, i + 1, r, j + 1, f'permuted: {EDGES[j]}')


def test_argument_refusals():
    var, gt, lab = _model()
    bad_edges = [(), 'edge', 3, ((0, 0),), ((1, 2),), ((5, 0),), ((-1, 0),), ((1, -1),), ((1.0, 0),), ((True, 0),), ((2,),), ((2, 1, 0, 0, 0),), ((2, 1, 2),),
                 ((2, 1, 0, 2),), ((2, 1, -1),), ((2, 1, 0, -1),), ((2, 1, 0.0),), ((),), (((2, 1), (2, 1)),), (((2, 1), (2, 1, 0)),), (((2, 1, 1, 0), (2, 1)),),
                 (((1, 0), (1, 1)),), (((2, 0), (2, 1), (2, 2)),), (((2, 0, 1, 0), (2, 1, 1, 0), (2, 2, 1)),), (((3, 1), 'x'),), ({'q': 1},)]
    for e in bad_edges:
        with pytest.raises(ValueError, match='edges'):
            var.attention_knockout(gt, lab, e)
    with pytest.raises(ValueError, match=r'\(0, 0\).*without a visible key'):
        var.attention_knockout(gt, lab, [(1, 0), (0, 0)])
    with pytest.raises(ValueError, match='duplicate'):
        var.attention_knockout(gt, lab, [((4, 2), (4, 2))])
    for kw in (dict(layers=()), dict(layers=(2,)), dict(layers=(1, 0)), dict(layers=(0, 0)), dict(layers=0.5), dict(heads=()), dict(heads=(2,)),
               dict(heads=(1, 0)), dict(heads=(-1,)), dict(heads=1.5), dict(max_rows=1), dict(max_rows=2.0), dict(max_rows=None)):
        with pytest.raises(ValueError):
            var.attention_knockout(gt, lab, EDGES[:2], **kw)
    for bad_gt, bad_lab in ((gt[:, :-1], lab), (gt.view(-1), lab), (gt, lab[:1]), (gt, torch.tensor([1, var.num_classes + 1])), (gt, torch.tensor([-1, 0])),
                            (gt.float(), lab)):
        with pytest.raises(ValueError):
            var.attention_knockout(bad_gt, bad_lab, EDGES[:2])
    bad = gt.clone(); bad[0, 0] = var.V
    with pytest.raises(ValueError):
        var.attention_knockout(bad, lab, EDGES[:2])
    touched = []

    class Spy(torch.Tensor):                                   # a refused edge is refused before the tokens are read
        @classmethod
        def __torch_function__(cls, func, types, args=(), kwargs=None):
            if func.__name__ in ('aminmax', 'to'):
                touched.append(func.__name__)
            return super().__torch_function__(func, types, args, kwargs or {})
    with pytest.raises(ValueError, match='edges'):
        var.attention_knockout(gt.as_subclass(Spy), lab, [(0, 0)])
    assert not touched
    assert var.attention_knockout(gt, lab, EDGES[:1], max_rows=2).nll.shape == (2, 2, var.L)
