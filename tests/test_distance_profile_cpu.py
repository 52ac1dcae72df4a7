"""VAR.distance_profile on CPU (the PyTorch branch): distance_profile_torch against the independent float64 restatement of
tests/distprofref.py on the d2 fixture model and on the reference's own logits, the fork's curve (var_analysis.py:694-732: the per-bin mean
of the flattened (distance, probability) pairs) computed the long way, the arithmetic of DistanceProfile, the argument checks and the routing."""
import math

import numpy as np
import pytest
import torch

from tests import distprofref as ref
from tests.test_token_scores_cpu import fixture_model          # (one d2 fixture model for both files)
from var_amd.models.var import DistanceProfile, code_distance_rows, distance_profile_torch

_T = {}


def table(var, gt):
    """the fp32 direct-form distance table of the fixture's codebook (V, V) with the rows of the fixture's tokens filled in (the others are
    never read), computed once"""
    if 't' not in _T:
        cb = var.vae_proxy[0].quantize.embedding.weight.detach().float()
        rows = torch.unique(gt)
        t = np.full((cb.shape[0], cb.shape[0]), np.nan, np.float32)
        t[rows.numpy()] = code_distance_rows(cb, rows).numpy()
        _T['t'] = t
    return _T['t']


def edges_for(dist, n=100):
    return np.linspace(0, float(np.nanmax(dist)), n).astype(np.float32)


def test_reference_logits_against_the_restatement(golden_dir):
    """distance_profile_torch on the reference's own teacher-forced logits, per image and scale: counts equal, mass within the bar"""
    vae, var, meta, gt, ref_logits = fixture_model(golden_dir)
    dist = table(var, gt)
    for edges, min_prob in ((edges_for(dist), 0.0), (np.array([0.0, 1.0, 2.5, np.inf], np.float32), 0.0), (edges_for(dist, 8), 1e-10)):
        for i in range(2):
            assert ref.clear_of_threshold(ref_logits[i].numpy(), gt[i].numpy(), min_prob) or min_prob == 0.0
            for b, e in var.begin_ends:
                z = ref_logits[i:i + 1, b:e]
                c, m = distance_profile_torch(z, gt[i, b:e], torch.from_numpy(dist[gt[i, b:e].numpy()]), torch.from_numpy(edges), min_prob)
                assert c.dtype == torch.int64 and m.dtype == torch.int64 and c.shape == (1, len(edges) - 1)
                wc, wm = ref.profile(z.numpy()[None], gt[i:i + 1, b:e].numpy(), dist, edges, min_prob)
                ok, msg = ref.mass_ok(m.numpy(), c.numpy(), wc[0], wm[0])
                assert ok, f'image {i} tokens {b}:{e} min_prob {min_prob}: {msg}'


@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_model_against_the_restatement(golden_dir, cfg):
    """var.distance_profile on the d2 fixture model (two images, three classes) against the restatement of its own logits: the same forward
    calls as the route under test makes (all three class rows in one batch), so both sides see the same fp32 z"""
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    dist = table(var, gt)
    edges = edges_for(dist)
    classes = [3, meta['labels'][0], 1000]
    r = var.distance_profile(gt, classes, edges, cfg=cfg)
    S, B = len(var.patch_nums), len(edges) - 1
    assert isinstance(r, DistanceProfile) and r.count_NKSB.shape == (2, 3, S, B) and r.mass_q_NKSB.shape == (2, 3, S, B)
    assert r.count_NKSB.dtype == torch.int64 and r.mass_q_NKSB.dtype == torch.int64 and r.mass_NKSB.dtype == torch.float64
    assert r.patch_nums == tuple(var.patch_nums) and r.min_prob == 0.0 and torch.equal(r.edges, torch.from_numpy(edges))
    assert torch.equal(var.distance_profile(gt, classes, edges, cfg=cfg, max_rows=2).count_NKSB, r.count_NKSB)      # (min_prob 0: d alone decides)
    x = vae.quantize.idxBl_to_var_input([gt[:, b:e] for b, e in var.begin_ends])
    pns = meta['patch_nums']
    t = cfg * torch.tensor([si / (len(pns) - 1) for si, pn in enumerate(pns) for _ in range(pn * pn)]).view(1, -1, 1)
    for i in range(2):
        with torch.no_grad():
            z = var(torch.tensor(classes), x[i:i + 1].expand(3, -1, -1))
            if cfg > 0:
                z = (1 + t) * z - t * var(torch.tensor([var.num_classes]), x[i:i + 1])
        for si, (b, e) in enumerate(var.begin_ends):
            wc, wm = ref.profile(z[None, :, b:e].numpy(), gt[i:i + 1, b:e].numpy(), dist, edges)
            ok, msg = ref.mass_ok(r.mass_q_NKSB[i, :, si].numpy(), r.count_NKSB[i, :, si].numpy(), wc[0], wm[0])
            assert ok, f'cfg {cfg} image {i} scale {si}: {msg}'
            # every pair lands somewhere (the last edge is the table's maximum: only pairs at that distance are dropped)
            assert int(r.count_NKSB[i, 0, si].sum()) >= (e - b) * var.V - (e - b) * 2


def test_the_forks_curve_the_long_way(golden_dir):
    """var_analysis.py:694-732: flatten the (distance, probability) pairs of a scale, cut at probs > 1e-10, bins = linspace(0, max_dist, 100),
    the mean probability per bin with boolean masks: the restatement's mass / count is that curve"""
    vae, var, meta, gt, ref_logits = fixture_model(golden_dir)
    dist = table(var, gt)
    b, e = var.begin_ends[-1]
    p = ref.row_probs(ref_logits[0, b:e].numpy())
    d = dist[gt[0, b:e].numpy()]
    flat_d, flat_p = d.reshape(-1), p.reshape(-1)
    keep = flat_p > np.float64(np.float32(1e-10))
    flat_d, flat_p = flat_d[keep], flat_p[keep]
    bins = np.linspace(0, min(float(flat_d.max()), 30), 100).astype(np.float32)
    want = np.array([flat_p[(flat_d >= bins[i]) & (flat_d < bins[i + 1])].mean() if ((flat_d >= bins[i]) & (flat_d < bins[i + 1])).any() else np.nan
                     for i in range(len(bins) - 1)])
    c, m = ref.profile(ref_logits[None, 0:1, b:e].numpy(), gt[0:1, b:e].numpy(), dist, bins, 1e-10)
    with np.errstate(invalid='ignore', divide='ignore'):
        got = m[0, 0] / c[0, 0]
    assert np.array_equal(np.isnan(got), np.isnan(want)) and not np.isnan(want).all()
    fin = ~np.isnan(want)
    assert np.allclose(got[fin], want[fin], rtol=1e-12, atol=0)
    # ... and DistanceProfile.mean_prob of the PyTorch route gives it within the mass bar over the count
    cc, mm = distance_profile_torch(ref_logits[0:1, b:e], gt[0, b:e], torch.from_numpy(d), torch.from_numpy(bins), 1e-10)
    prof = DistanceProfile(cc.view(1, 1, 1, -1), mm.view(1, 1, 1, -1), torch.from_numpy(bins), 1e-10, (var.patch_nums[-1],))
    mp = prof.mean_prob()[0, 0, 0].numpy()
    assert np.array_equal(cc.numpy()[0], c[0, 0]) and np.array_equal(np.isnan(mp), np.isnan(want))
    assert (np.abs(mp[fin] - want[fin]) <= ref.REL * want[fin] + 1 / ref.Q).all()


def test_distance_profile_arithmetic():
    count = torch.tensor([[[[2, 0, 4]]], [[[6, 0, 0]]]])                     # (N=2, K=1, S=1, B=3)
    mass_q = torch.tensor([[[[1 << 47, 0, 1 << 48]]], [[[3 << 47, 0, 0]]]])
    edges = torch.tensor([0.0, 1.0, 3.0, math.inf])
    r = DistanceProfile(count, mass_q, edges, 0.25, (4,))
    assert r.mass_NKSB.dtype == torch.float64 and r.mass_NKSB.reshape(-1).tolist() == [0.5, 0.0, 1.0, 1.5, 0.0, 0.0]
    mp = r.mean_prob()
    assert mp.shape == (2, 1, 1, 3) and mp.dtype == torch.float64
    assert mp[0, 0, 0, 0] == 0.25 and math.isnan(mp[0, 0, 0, 1]) and mp[0, 0, 0, 2] == 0.25
    assert mp[1, 0, 0, 0] == 0.25 and math.isnan(mp[1, 0, 0, 1]) and math.isnan(mp[1, 0, 0, 2])
    mo = r.mean_prob(over_images=True)
    assert mo.shape == (1, 1, 3) and mo[0, 0, 0] == 2.0 / 8 and math.isnan(mo[0, 0, 1]) and mo[0, 0, 2] == 0.25
    assert r.centers().tolist() == [0.5, 2.0, math.inf] and r.centers().dtype == torch.float64
    assert r.min_prob == 0.25 and r.patch_nums == (4,) and 'bins=3' in repr(r)


def test_argument_checks(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    ok_e = [0.0, 1.0, 2.0]
    nan = float('nan')
    for bad in ([0.0], [], [[0.0, 1.0]], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [-0.5, 1.0], [0.0, nan], [nan, 1.0], list(range(258)),
                [0.0, 1.0, 1.0 + 1e-9],                                       # equal once rounded to fp32
                [math.inf, math.inf], 'edges'):
        with pytest.raises(ValueError):
            var.distance_profile(gt, [1, 2], bad)
    for mp in (-1e-9, 1.0, 1.5, nan, math.inf, 1.0 - 1e-12, True, '0.1', None):   # (1 - 1e-12 is 1 in fp32)
        with pytest.raises(ValueError):
            var.distance_profile(gt, [1, 2], ok_e, min_prob=mp)
    for kw in (dict(cfg=-1.0), dict(cfg=nan), dict(max_rows=0), dict(cfg=1.0, max_rows=1)):          # the token_scores checks apply
        with pytest.raises(ValueError):
            var.distance_profile(gt, [1, 2], ok_e, **kw)
    with pytest.raises(ValueError):
        var.distance_profile(torch.where(gt == gt[0, 3], var.V, gt), [1, 2], ok_e)
    with pytest.raises(ValueError):
        var.distance_profile(gt, [1, 1001], ok_e)
    # the boundaries themselves are accepted: one bin, 256 bins, a last edge of +inf, a tensor of edges, min_prob just below 1
    g1 = gt[:1]
    for e in ([0.0, math.inf], np.linspace(0, 40, 257), torch.tensor([0.5, 1.0]), (0, 1, 2)):
        r = var.distance_profile(g1, [1], e)
        assert r.count_NKSB.shape[-1] == len(e) - 1
    full = var.distance_profile(g1, [1], [0.0, math.inf])
    assert full.count_NKSB[0, 0, :, 0].tolist() == [pn * pn * var.V for pn in var.patch_nums]
    assert int(var.distance_profile(g1, [1], [0.0, math.inf], min_prob=0.999).count_NKSB.sum()) == 0


def test_routes_to_torch_on_cpu_and_in_train_mode(golden_dir, monkeypatch):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    from var_amd.models import var as var_mod
    calls = []
    real = var_mod.distance_profile_torch
    monkeypatch.setattr(var_mod, 'distance_profile_torch', lambda *a: (calls.append(a[0].shape), real(*a))[1])
    monkeypatch.setattr(type(var), 'engine', lambda self: pytest.fail('the CPU route must not build the HIP engine'))
    assert not var._scoring_on_hip(gt)
    r = var.distance_profile(gt[:1], [1, 2, 3], [0.0, 5.0, math.inf], max_rows=2)
    S = len(var.patch_nums)
    assert len(calls) == 2 * S and calls[0] == (2, 1, var.V) and calls[1] == (1, 1, var.V), 'max_rows class rows at a time, scale by scale'
    assert r.count_NKSB.device.type == 'cpu' and r.count_NKSB.shape == (1, 3, S, 2)
