"""VAR.evaluate on CPU (the PyTorch route): the trainer's validation metrics (reference trainer.py:54-84, :126-156) against the reference's own
logits, the per-token definitions on planted logits, the arithmetic of EvalResult and the argument checks."""
import numpy as np
import pytest
import torch

from tests import evalref

_M = {}


def model(golden_dir):
    if 'm' not in _M:
        _M['m'] = evalref.fixture_model(golden_dir, 'cpu')
    return _M['m']


def test_matches_reference_logits(golden_dir):
    vae, var = model(golden_dir)
    var.cond_drop_rate = 0.1                        # ignored: labels are used as given
    evalref.check_against_reference_fixture(var, golden_dir, 'cpu')


def planted(V, L):
    """(3, L, V) logits and (3, L) tokens with the corner cases at known rows"""
    g = torch.Generator().manual_seed(5)
    z = torch.randn(3, L, V, generator=g) * 3
    gt = torch.randint(0, V, (3, L), generator=g)
    z[0, 0, :] -= 50; z[0, 0, 17] = 9.0; gt[0, 0] = 17                          # gt is the only maximum: pred = gt, rank 0
    z[0, 1, 5] = z[0, 1, 9] = 30.0; gt[0, 1] = 9                                 # tie at the maximum, gt the higher index: pred 5, rank 1
    z[0, 2, 5] = z[0, 2, 9] = 30.0; gt[0, 2] = 5                                 # ... gt the lower index: pred 5, rank 0
    z[1, 3, 100] = z[1, 3, 200] = z[1, 3, 300] = 0.125; gt[1, 3] = 200           # gt tied with a lower and a higher index, below the maximum
    z[1, 4, 0] = 0.0; z[1, 4, 1] = -0.0; z[1, 4, 2:] = -1.0; gt[1, 4] = 1        # +0 == -0: pred 0, rank 1
    z[2, 5, 7] = float('nan'); z[2, 5, 100] = float('nan'); gt[2, 5] = 3          # a NaN row: pred 7, nll NaN, NaN compares false
    z[2, L - 1, V - 1] = 40.0; gt[2, L - 1] = V - 1                              # the last code of the last token
    return z, gt


def test_definitions_on_planted_logits(golden_dir, monkeypatch):
    vae, var = model(golden_dir)
    V, L, pns = var.V, var.L, var.patch_nums
    z, gt = planted(V, L)
    monkeypatch.setattr(var, '_forward_torch', lambda lab, x: z[:lab.shape[0]].clone())
    r = var.evaluate(gt, [1, 2, 3])
    nll, smooth, pred, rank = evalref.token_defs(z.numpy(), gt.numpy())
    assert (pred[0, 0], rank[0, 0], pred[0, 1], rank[0, 1], pred[0, 2], rank[0, 2]) == (17, 0, 5, 1, 5, 0)
    assert (pred[1, 4], rank[1, 4], pred[2, 5], pred[2, L - 1], rank[2, L - 1]) == (0, 1, 7, V - 1, 0)
    assert rank[1, 3] == int((z[1, 3] > 0.125).sum()) + 1
    assert np.array_equal(r.pred_BL.numpy(), pred) and np.array_equal(r.rank_BL.numpy(), rank)
    assert bool(torch.isnan(r.nll_BL[2, 5])) and int(torch.isnan(r.nll_BL).sum()) == 1
    ok = ~np.isnan(nll)
    assert np.abs(r.nll_BL.double().numpy() - nll)[ok].max() <= 1e-5
    be = var.begin_ends
    assert r.correct_S.tolist() == [int((rank[:, b:e] == 0).sum()) for b, e in be]
    assert r.tokens_S.tolist() == [3 * pn * pn for pn in pns]
    assert np.array_equal(r.pred_hist_V.numpy(), np.bincount(pred.reshape(-1), minlength=V))
    for k in (1, 2, 5, V):
        assert r.topk_correct_S(k).tolist() == [int((rank[:, b:e] < k).sum()) for b, e in be], k
    assert r.topk_correct_S(1).tolist() == r.correct_S.tolist() and r.topk_correct_S(V).tolist() == r.tokens_S.tolist()
    # trainer.py:140-143 and :149-155 on the same predictions
    p = torch.from_numpy(pred).view(-1).bincount(minlength=V).float()
    p /= p.sum()
    assert abs(r.z_voc_usage - (p > 0.001 / V).float().mean().item() * 100) < 1e-9
    ps = r.per_scale()
    assert list(ps) == [f'{n}_{16 * pn}' for pn in pns for n in ('acc', 'L')]
    for (b, e), pn in zip(be, pns):
        assert abs(ps[f'acc_{16 * pn}'] - (pred[:, b:e] == gt.numpy()[:, b:e]).mean() * 100) < 1e-9
        want = nll[:, b:e].mean()
        assert (np.isnan(want) and np.isnan(ps[f'L_{16 * pn}'])) or abs(ps[f'L_{16 * pn}'] - want) <= 1e-5
    assert abs(r.acc_mean - 100 * (rank == 0).mean()) < 1e-9 and abs(r.acc_tail - 100 * (rank[:, be[-1][0]:] == 0).mean()) < 1e-9
    # the smoothed objective on the NaN-free images: torch's own label-smoothed cross entropy in float64
    rs = var.evaluate(gt[:2], [1, 2], label_smooth=0.1)
    want = float(torch.nn.functional.cross_entropy(z[:2].double().view(-1, V), gt[:2].reshape(-1), label_smoothing=0.1))
    assert abs(rs.loss - want) <= 1e-5 * abs(want), (rs.loss, want)
    assert abs(float(rs.smooth_S.sum()) - smooth[:2].sum()) <= 1e-5 * np.abs(smooth[:2]).sum()


def test_result_arithmetic(golden_dir):
    vae, var = model(golden_dir)
    g = torch.Generator().manual_seed(11)
    gt = torch.randint(0, var.V, (4, var.L), generator=g)
    lab = torch.tensor([3, 1000, 17, 980])
    whole = var.evaluate(gt, lab, label_smooth=0.1, max_rows=2)                 # (the same two-image forward passes as the halves)
    a, b = var.evaluate(gt[:2], lab[:2], label_smooth=0.1), var.evaluate(gt[2:], lab[2:], label_smooth=0.1)
    s = a + b
    assert s.images == 4 and s.label_smooth == 0.1 and s.patch_nums == whole.patch_nums
    for name in ('correct_S', 'tokens_S', 'pred_hist_V', 'nll_BL', 'pred_BL', 'rank_BL'):
        assert torch.equal(getattr(s, name), getattr(whole, name)), name
    for name in ('nll_S', 'smooth_S'):
        x, y = getattr(s, name), getattr(whole, name)
        assert float(((x - y).abs() / y.abs()).max()) <= 1e-12, name
    assert abs(s.L_mean - whole.L_mean) <= 1e-12 * whole.L_mean and abs(s.loss - whole.loss) <= 1e-12 * abs(whole.loss)
    assert int(s.pred_hist_V.sum()) == 4 * var.L
    # one four-image forward pass instead: the CPU GEMMs of 4 and 2 rows may round differently, so within the project's bar for this model
    # (evalref.BAR) on the values and exact on what does not depend on them
    four = var.evaluate(gt, lab, label_smooth=0.1, max_rows=4)
    assert torch.equal(four.tokens_S, s.tokens_S) and four.images == 4 and int(four.pred_hist_V.sum()) == 4 * var.L
    assert float((four.nll_BL - s.nll_BL).abs().max()) <= evalref.BAR and abs(four.L_mean - s.L_mean) <= evalref.BAR
    assert abs(four.loss - s.loss) <= evalref.BAR
    with pytest.raises(ValueError):
        a + var.evaluate(gt[2:], lab[2:], label_smooth=0.2)
    with pytest.raises(TypeError):
        a + 1


def test_argument_checks_and_token_spellings(golden_dir):
    vae, var = model(golden_dir)
    meta, gt, _ = evalref.fixture(golden_dir)
    ok = torch.tensor(meta['labels'])
    per_scale = [gt[:, b:e] for b, e in var.begin_ends]
    bad = [
        dict(gt_tokens=gt[:, :-1], label_B=ok),                                 # token shape
        dict(gt_tokens=gt[0], label_B=ok),
        dict(gt_tokens=gt.float(), label_B=ok),
        dict(gt_tokens=per_scale[:-1], label_B=ok),                             # the per-scale list
        dict(gt_tokens=per_scale[:-1] + [per_scale[-1][:, :-1]], label_B=ok),
        dict(gt_tokens=per_scale[:-1] + [per_scale[-1][:1]], label_B=ok),
        dict(gt_tokens=torch.where(gt == gt[0, 3], -1, gt), label_B=ok),        # token range
        dict(gt_tokens=torch.where(gt == gt[1, 7], var.V, gt), label_B=ok),
        dict(gt_tokens=gt, label_B=torch.tensor([1, -1])),                      # label range
        dict(gt_tokens=gt, label_B=torch.tensor([1, var.num_classes + 1])),
        dict(gt_tokens=gt, label_B=torch.tensor([1, 2, 3])),                    # (N,)
        dict(gt_tokens=gt, label_B=torch.tensor([[1], [2]])),
        dict(gt_tokens=gt, label_B=torch.tensor([1.0, 2.0])),
        dict(gt_tokens=gt, label_B=ok, label_smooth=-0.1),                      # label_smooth in [0, 1), finite
        dict(gt_tokens=gt, label_B=ok, label_smooth=1.0),
        dict(gt_tokens=gt, label_B=ok, label_smooth=float('nan')),
        dict(gt_tokens=gt, label_B=ok, label_smooth=float('inf')),
        dict(gt_tokens=gt, label_B=ok, max_rows=0),                             # max_rows
        dict(gt_tokens=gt, label_B=ok, max_rows=1.5),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            var.evaluate(**kw)
    with pytest.raises(TypeError):
        var.evaluate(gt, ok, 0.1)                                               # label_smooth and max_rows are keyword-only
    a = var.evaluate(gt, ok)
    b = var.evaluate(per_scale, meta['labels'], max_rows=2)
    c = var.evaluate(gt.tolist(), ok.to(torch.int32))
    for name in ('nll_S', 'smooth_S', 'correct_S', 'tokens_S', 'pred_hist_V', 'nll_BL', 'pred_BL', 'rank_BL'):
        assert torch.equal(getattr(a, name), getattr(b, name)) and torch.equal(getattr(a, name), getattr(c, name)), name
    # the boundaries themselves are accepted
    r = var.evaluate(torch.where(gt == gt[0, 3], var.V - 1, gt), [0, var.num_classes], label_smooth=0.999, max_rows=1)
    assert bool(torch.isfinite(r.nll_BL).all())


def test_progressive_stage_covers_its_scales_only(golden_dir):
    """prog_si >= 0 (the PyTorch route): the result holds the scales 0 .. prog_si, as trainer.py:150 stops there"""
    vae, var = model(golden_dir)
    meta, gt, _ = evalref.fixture(golden_dir)
    full = var.evaluate(gt, meta['labels'])
    var.prog_si = 2
    try:
        r = var.evaluate(gt, meta['labels'])
    finally:
        var.prog_si = -1
    ed = var.begin_ends[2][1]
    assert r.patch_nums == var.patch_nums[:3] and r.nll_BL.shape == (2, ed) and r.tokens_S.tolist() == full.tokens_S[:3].tolist()
    assert float((r.nll_BL - full.nll_BL[:, :ed]).abs().max()) <= 1e-5          # the block-causal mask: a prefix does not see the later scales
    assert list(r.per_scale()) == list(full.per_scale())[:6]
