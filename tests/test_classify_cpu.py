"""VAR.classify on CPU (the PyTorch branch: token_scores in full, then the pruning rule) against the rule stated independently in numpy on
token_scores' own output: predictions, float64 running totals (np.add.accumulate, bitwise), depths, the NaN pattern of pruned candidates,
and the argument checks."""
import numpy as np
import pytest
import torch

from tests.test_likelihood_cpu import fixture_model

MODES = [('log_prob', {}), ('group_smoothed', dict(group=7)), ('neighbor_max', dict(threshold=0.5)), ('expected_distance', dict(top_k=9))]


def rule_key(total, pos):
    """the classification rule as a sort key: higher total first, NaN below everything, ties by lower position"""
    return (1, 0.0, pos) if np.isnan(total) else (0, -total, pos)


def expect(tokens, ends, schedule):
    """the rule applied to full (N, K, L) scores -> pred, total, depth, masked tokens (numpy)"""
    N, K, L = tokens.shape
    cum = np.add.accumulate(tokens.astype(np.float64), axis=-1)
    depth = np.full((N, K), len(ends) - 1, dtype=np.int64)
    pred = np.zeros(N, dtype=np.int64)
    for n in range(N):
        alive = list(range(K))
        for s, m in sorted(schedule.items()):
            ranked = sorted(alive, key=lambda c: rule_key(cum[n, c, ends[s] - 1], c))
            for c in ranked[m:]:
                depth[n, c] = s
            alive = sorted(ranked[:m])
        pred[n] = min(alive, key=lambda c: rule_key(cum[n, c, L - 1], c))
    end = np.asarray(ends)[depth]
    total = np.array([[cum[n, c, end[n, c] - 1] for c in range(K)] for n in range(N)])
    masked = tokens.copy()
    masked[np.arange(L)[None, None, :] >= end[..., None]] = np.nan
    return pred, total, depth, masked


def same(a, b):
    """bitwise equality of float arrays, NaN positions included"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize('score,kw', MODES)
@pytest.mark.parametrize('cfg', [0.0, 1.5])
def test_no_pruning_is_the_rule_on_token_scores(golden_dir, score, kw, cfg):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    var.cond_drop_rate = 0.0
    classes = [3, 980, 1000, 3, 17]
    full = var.token_scores(gt, classes, score, cfg=cfg, **kw).numpy()
    ends = [e for _, e in var.begin_ends]
    pred, total, depth, masked = expect(full, ends, {})
    for keep in (None, {}):
        r = var.classify(gt, classes, score, cfg=cfg, keep=keep, **kw)
        assert r.pred.dtype == torch.int64 and r.total.dtype == torch.float64 and r.depth.dtype == torch.int64 and r.tokens.dtype == torch.float32
        assert np.array_equal(r.pred.numpy(), pred)
        assert same(r.total.numpy(), total), 'totals differ from the sequential float64 sum'
        assert bool((r.depth == len(var.patch_nums) - 1).all())
        assert same(r.tokens.numpy(), full)
    # the totals are the token-ordered sums themselves
    assert same(total, np.add.accumulate(full.astype(np.float64), axis=-1)[..., -1])


@pytest.mark.parametrize('score,kw', MODES[:2])
def test_pruning_schedule(golden_dir, score, kw):
    """K = 9 with duplicate labels (bit-identical totals: the lower position survives a boundary that splits them), two boundaries, and one
    boundary that drops nothing"""
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    var.cond_drop_rate = 0.0
    classes = torch.tensor([[5, 5, 200, 7, 999, 5, 31, 1000, 64], [12, 400, 12, 12, 3, 88, 0, 1, 2]])
    ends = [e for _, e in var.begin_ends]
    for cfg in (0.0, 1.5):
        full = var.token_scores(gt, classes, score, cfg=cfg, max_rows=4, **kw).numpy()     # (CPU GEMMs round by row count)
        for keep in ({1: 4, 3: 2}, {0: 1}, {2: 9}, {0: 6, 1: 6, 2: 3}):
            pred, total, depth, masked = expect(full, ends, keep)
            r = var.classify(gt, classes, score, cfg=cfg, max_rows=4, keep=keep, **kw)
            assert np.array_equal(r.pred.numpy(), pred), (cfg, keep)
            assert np.array_equal(r.depth.numpy(), depth), (cfg, keep)
            assert same(r.total.numpy(), total), (cfg, keep)
            assert same(r.tokens.numpy(), masked), (cfg, keep)
            assert bool(((r.depth == len(ends) - 1).sum(-1) == min([9] + list(keep.values()))).all()), (cfg, keep)
    # one class three times: bit-identical totals at every scale, so the lowest positions survive and win
    r = var.classify(gt, [7, 7, 7], score, keep={0: 2}, **kw)
    assert r.pred.tolist() == [0, 0] and r.depth.tolist() == [[len(ends) - 1, len(ends) - 1, 0]] * 2
    assert same(r.total[:, 0].numpy(), r.total[:, 1].numpy())


def test_argument_checks(golden_dir):
    vae, var, meta, gt, _ = fixture_model(golden_dir)
    S = len(var.patch_nums)
    ok = [1, 2, 3]
    for keep in ({S - 1: 1}, {0: 0}, {0: True}, {True: 1}, {0: 1.0}, {1.0: 1}, {-1: 1}, {S: 2}, {0: -2}, [(0, 1)], {'0': 1}):
        with pytest.raises(ValueError):
            var.classify(gt, ok, keep=keep)
    bad = [
        dict(gt_tokens=gt[:, :-1], label=ok), dict(gt_tokens=gt.float(), label=ok), dict(gt_tokens=torch.where(gt == gt[0, 3], -1, gt), label=ok),
        dict(gt_tokens=gt, label=[1, -1]), dict(gt_tokens=gt, label=[1, var.num_classes + 1]), dict(gt_tokens=gt, label=torch.zeros(0, dtype=torch.int64)),
        dict(gt_tokens=gt, label=torch.zeros(3, 2, dtype=torch.int64)), dict(gt_tokens=gt, label=[1.0, 2.0]),
        dict(gt_tokens=gt, label=ok, cfg=-0.5), dict(gt_tokens=gt, label=ok, cfg=float('nan')), dict(gt_tokens=gt, label=ok, max_rows=0),
        dict(gt_tokens=gt, label=ok, cfg=1.0, max_rows=1),
        dict(gt_tokens=gt, label=ok, score='nope'), dict(gt_tokens=gt, label=ok, group=5), dict(gt_tokens=gt, label=ok, score='group_smoothed', group=0),
        dict(gt_tokens=gt, label=ok, score='neighbor_max'), dict(gt_tokens=gt, label=ok, score='neighbor_max', threshold=-1.0),
        dict(gt_tokens=gt, label=ok, score='expected_distance', top_k=var.V + 1), dict(gt_tokens=gt, label=ok, score='log_prob', top_k=3),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            var.classify(**kw)
    # the boundaries of keep themselves are accepted
    r = var.classify(gt, ok, keep={0: 1, S - 2: 1000})
    assert r.pred.shape == (2,) and r.depth.shape == (2, 3) and r.tokens.shape == (2, 3, var.L)
