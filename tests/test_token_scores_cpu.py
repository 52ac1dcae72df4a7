"""VAR.token_scores on CPU (the PyTorch branch): the fork's smooth_bayesian, fast_neighbor_bayesian and l2_dist scores (eval_prob.py:37-92,
389-393; var_analysis.py:252-258) against an independent float64 restatement, on the d2 fixture model and on the reference's own logits, the
identities between the modes, and the argument checks."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

from models import build_vae_var
from var_amd.detinit import fill_module_
from var_amd.models.var import code_distance_rows

_M = {}


def fixture_model(golden_dir):
    """the d2 model of tests/golden/encode_t_pn12345.npz on CPU, its tokens and the reference's teacher-forced logits"""
    if 'm' not in _M:
        z = np.load(f'{golden_dir}/encode_t_pn12345.npz')
        meta = json.loads(str(z['meta']))
        with contextlib.redirect_stdout(io.StringIO()):
            vae, var = build_vae_var(device='cpu', patch_nums=tuple(meta['patch_nums']), depth=meta['depth'], ch=meta['ch'])
        fill_module_(var, meta['depth'], 0, 'var.'); fill_module_(vae, meta['depth'], 0, 'vae.')
        var.eval(); vae.eval(); var.cond_drop_rate = 0.0
        gt = torch.from_numpy(np.concatenate([z[f'idx_s{si}'] for si in range(len(meta['patch_nums']))], 1).astype(np.int64))
        _M['m'] = (vae, var, meta, gt, torch.from_numpy(z['logits']))
    return _M['m']


def restate(z, gt, score, par, dist):
    """float64 restatement: z (R, l, V) logits, gt (l,) tokens, dist (V, V) or None -> (R, l) float64.  Order: z descending, ties by
    ascending index (a stable argsort of -z)."""
    z = np.asarray(z, dtype=np.float64)
    R, l, V = z.shape
    out = np.empty((R, l))
    for r in range(R):
        for t in range(l):
            x = z[r, t]
            g = int(gt[t])
            lse = x.max() + math.log(np.exp(x - x.max()).sum())
            lp = x - lse
            p = np.exp(lp)
            if score == 'neighbor_max':
                out[r, t] = lp[dist[g] <= par].max()
                continue
            d = None if dist is None else dist[g]
            if score == 'expected_distance' and par is None:
                out[r, t] = -(p * d).sum()
                continue
            order = np.argsort(-x, kind='stable')
            if score == 'expected_distance':
                T = order[:par]
                out[r, t] = -(p[T] * d[T]).sum() / p[T].sum()
            else:
                rank = int(np.nonzero(order == g)[0][0])
                lo = rank - rank % par
                hi = min(lo + par, V)
                out[r, t] = math.log(p[order[lo:hi]].sum() / (hi - lo) + 1e-10)
    return out


def table(var):
    cb = var.vae_proxy[0].quantize.embedding.weight.detach().float()
    return code_distance_rows(cb, torch.arange(cb.shape[0])).double().numpy()


MODES = [('group_smoothed', dict(group=50), 50), ('group_smoothed', dict(group=7), 7), ('neighbor_max', None, None),
         ('expected_distance', dict(), None), ('expected_distance', dict(top_k=20), 20)]


def _kw(var, dist, score, kw, par):
    if score == 'neighbor_max':
        thr = float(np.median(dist[dist > 0]) * 0.8)       # a few percent of the codes are neighbours
        return dict(threshold=thr), thr
    return kw, par


def test_distance_rows_are_the_direct_form(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    cb = var.vae_proxy[0].quantize.embedding.weight.detach().double()
    rows = torch.tensor([0, 5, 4095, 77])
    want = (cb[rows].unsqueeze(1) - cb.unsqueeze(0)).pow(2).sum(-1).sqrt()
    got = code_distance_rows(cb.float(), rows).double()
    assert float(((got - want).abs() / (want + 1e-30)).max()) <= 4e-6
    assert bool((got[torch.arange(4), rows] == 0).all())


@pytest.mark.parametrize('score,kw,par', MODES)
def test_matches_float64_restatement(golden_dir, score, kw, par):
    """the PyTorch branch on the d2 fixture model (two images, three classes, with and without guidance) against the float64 restatement of
    its own logits (forward per image, the guided combine as in var_analysis.py:333-344)"""
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    dist = table(var)
    kw, par = _kw(var, dist, score, kw, par)
    classes = [3, meta['labels'][0], 1000]
    x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    pns = meta['patch_nums']
    for cfg in (0.0, 1.5):
        got = var.token_scores(gt, classes, score, cfg=cfg, **kw)
        assert got.shape == (2, 3, var.L) and got.dtype == torch.float32
        t = cfg * torch.tensor([si / (len(pns) - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)]).view(1, -1, 1)
        for i in range(2):
            with torch.no_grad():
                z = var(torch.tensor(classes), x[i:i + 1].expand(3, -1, -1))
                if cfg > 0:
                    z = (1 + t) * z - t * var(torch.tensor([var.num_classes]), x[i:i + 1])
            want = restate(z, gt[i], score, par, dist)
            err = np.abs(got[i].double().numpy() - want) / (1 + np.abs(want))
            assert err.max() <= 2e-6, f'{score} cfg={cfg} image {i}: relative error {err.max():.3e}'


@pytest.mark.parametrize('score,kw,par', MODES)
def test_matches_reference_logits(golden_dir, score, kw, par):
    """the fixture's own labels, against the float64 restatement of the reference's logits (the bound of test_likelihood_cpu)"""
    vae, var, meta, gt, ref_logits = fixture_model(golden_dir)
    dist = table(var)
    kw, par = _kw(var, dist, score, kw, par)
    got = var.token_scores(gt, torch.tensor(meta['labels']).view(-1, 1), score, **kw)
    for i in range(2):
        want = restate(ref_logits[i:i + 1], gt[i], score, par, dist)
        err = float(np.abs(got[i].double().numpy() - want).max())
        assert err <= 7e-4, f'{score} image {i}: max |diff| {err:.3e} against the reference logits'


def test_identities(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    classes = [3, 17, 1000]
    V = var.V
    lp = var.token_log_likelihood(gt, classes, cfg=1.0)
    assert torch.equal(var.token_scores(gt, classes, 'log_prob', cfg=1.0), lp)
    # group = 1 is the plain score with the fork's 1e-10; a group of the whole codebook is uniform
    g1 = var.token_scores(gt, classes, 'group_smoothed', cfg=1.0, group=1)
    assert torch.allclose(g1, torch.log(lp.exp() + 1e-10), atol=2e-6, rtol=0)
    for G in (V, V + 13):
        gv = var.token_scores(gt, classes, 'group_smoothed', cfg=1.0, group=G)
        assert torch.allclose(gv, torch.full_like(gv, math.log(1 / V + 1e-10)), atol=2e-6, rtol=0)
    # threshold 0 on a codebook of distinct codes keeps gt alone; a threshold above every distance takes the best code
    cb = var.vae_proxy[0].quantize.embedding.weight.detach()
    assert torch.unique(cb, dim=0).shape[0] == V
    assert torch.equal(var.token_scores(gt, classes, 'neighbor_max', cfg=1.0, threshold=0.0), lp)
    big = float(table(var).max()) * 2 + 1                  # (an infinite threshold is refused)
    x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    with torch.no_grad():
        z = torch.stack([var(torch.tensor(classes), x[i:i + 1].expand(3, -1, -1)) for i in range(2)])
    nm = var.token_scores(gt, classes, 'neighbor_max', threshold=big)
    assert torch.allclose(nm, z.log_softmax(-1).amax(-1), atol=1e-6, rtol=0)
    # top_k = V is the full sum; top_k = 1 is minus the distance to the argmax (first index on ties)
    full = var.token_scores(gt, classes, 'expected_distance')
    assert torch.allclose(var.token_scores(gt, classes, 'expected_distance', top_k=V), full, rtol=1e-5, atol=0)
    t1 = var.token_scores(gt, classes, 'expected_distance', top_k=1)
    am = z.argmax(-1)
    dist = torch.from_numpy(table(var)).float()
    want = -dist[gt.unsqueeze(1).expand(-1, 3, -1), am]
    assert torch.allclose(t1, want, rtol=3e-7, atol=0)            # (p d / p: two roundings)


def test_argument_checks(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    ok = [1, 2]
    bad = [
        dict(score='bayesian'),                                                  # unknown score
        dict(score='log_prob', group=5),                                         # parameters of other modes
        dict(score='log_prob', threshold=1.0),
        dict(score='group_smoothed', top_k=3),
        dict(score='group_smoothed', threshold=1.0),
        dict(score='neighbor_max', threshold=1.0, group=2),
        dict(score='expected_distance', threshold=1.0),
        dict(score='expected_distance', group=4),
        dict(score='group_smoothed', group=0),                                   # group >= 1
        dict(score='group_smoothed', group=-3),
        dict(score='group_smoothed', group=2.5),
        dict(score='neighbor_max'),                                              # threshold: required, finite, >= 0
        dict(score='neighbor_max', threshold=-0.1),
        dict(score='neighbor_max', threshold=float('inf')),
        dict(score='neighbor_max', threshold=float('nan')),
        dict(score='expected_distance', top_k=0),                                # top_k in [1, V]
        dict(score='expected_distance', top_k=var.V + 1),
        dict(score='group_smoothed', cfg=-1.0),                                  # the token_log_likelihood checks apply
        dict(score='group_smoothed', max_rows=0),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            var.token_scores(gt, ok, **kw)
    with pytest.raises(ValueError):
        var.token_scores(torch.where(gt == gt[0, 3], var.V, gt), ok, 'group_smoothed')
    # the boundaries themselves are accepted
    for kw in (dict(group=1), dict(score='expected_distance', top_k=1), dict(score='expected_distance', top_k=var.V),
               dict(score='neighbor_max', threshold=0.0)):
        kw = dict(dict(score='group_smoothed'), **kw)
        assert torch.isfinite(var.token_scores(gt, ok, **kw)).all()
